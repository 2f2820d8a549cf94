/*
 * position_searcher.cpp — AgxPositionSearcher and agx_position_searcher_* of the C ABI (include/agx.h): the whole search on boards
 * (k_load_positions / k_harvest_positions of engine.hip, launched through engine_launch.hpp, around the engine's own stages).
 */
#include "engine_host.hpp"
#include "sample_v201.hpp"

#include <cstring>
#include <mutex>
#include <string>

using namespace agx;
using namespace agx_host;

struct AgxPositionSearcher
{
		AgxEngine *engine = nullptr;
		int slots = 0, device = -1;
		std::mutex mutex;
		PositionJob job;      // the job in flight (device addresses); cursor / finished / slot_* are the searcher's own
		int *state = nullptr;      // device: cursor, finished, slot_position[slots], slot_steps[slots]
		int *poll_host = nullptr;  // pinned: two finished counts on their way back (search), then slot_position[slots] (slots)
		hipEvent_t poll_event[2] = { nullptr, nullptr };
		int job_n = 0;             // positions of the job in flight, 0 = none
		int job_finished = 0;      // ... of which known to be finished
		unsigned long long device_bytes = 0;
		// the calls of one searcher share its pool: a call on another stream than the previous one is ordered behind it on the device
		hipEvent_t done = nullptr;
		hipStream_t last_stream = nullptr;
		bool launched = false;
};

namespace
{
	int searcher_enter(AgxPositionSearcher *ps, hipStream_t stream, const char *what)
	{ // (under the searcher's mutex) the calling thread's device, and the order behind the previous call's stream
		int current = -1;
		AGX_HIP_CHECK(hipGetDevice(&current));
		AGX_REQUIRE(current == ps->device, AGX_ERR_STATE, "%s: the searcher lives on device %d, the calling thread's current device is %d", what, ps->device, current);
		if (ps->launched && ps->last_stream != stream)
			AGX_HIP_CHECK(hipStreamWaitEvent(stream, ps->done, 0));
		return AGX_OK;
	}
	int searcher_leave(AgxPositionSearcher *ps, hipStream_t stream, int status)
	{
		const hipError_t launched = hipGetLastError();
		AGX_HIP_CHECK(hipEventRecord(ps->done, stream));
		ps->launched = true;
		ps->last_stream = stream;
		AGX_HIP_CHECK(launched);
		return status;
	}
	/* one staged call: under the searcher's mutex, behind the previous call's stream, `run(stream)`, then the mark the next call waits for */
	template<typename Run>
	int searcher_call(AgxPositionSearcher *ps, void *stream, const char *what, Run run)
	{
		AGX_REQUIRE(ps != nullptr, AGX_ERR_INVALID, "%s: null searcher", what);
		hipStream_t s = static_cast<hipStream_t>(stream);
		std::lock_guard<std::mutex> lock(ps->mutex);
		const int st = searcher_enter(ps, s, what);
		return (st != AGX_OK) ? st : searcher_leave(ps, s, run(s));
	}
	EngineDev searcher_dev(const AgxPositionSearcher *ps)
	{ // the pool as one group (agx_engine_*_group(e, 0, 1)); the engine's own record keeps what set_max_simulations / set_batch_size changed
		EngineDev d = ps->engine->dev;
		d.g0 = 0;
		d.nn_counter = 16;
		d.yield_counter = 32;
		d.grp_first = 0;
		d.grp_count = d.n_games;
		return d;
	}
	int searcher_default_steps(const AgxPositionSearcher *ps)
	{ // agx.h: agx_position_searcher_begin
		const EngineDev &d = ps->engine->dev;
		const long long steps = (static_cast<long long>(d.max_sims) + 2) * (2 * d.batch + 1) + ARENA_CLASSES;
		return static_cast<int>(std::min<long long>(steps, 0x7FFFFFF0));
	}
	/* (under the mutex) is the job in flight finished?  Asks the device when the host does not know yet: waits for the previous call's stream only */
	int searcher_job_open(AgxPositionSearcher *ps, bool *open)
	{
		*open = false;
		if (ps->job_n == 0 || ps->job_finished >= ps->job_n)
			return AGX_OK;
		if (ps->launched)
			AGX_HIP_CHECK(hipEventSynchronize(ps->done));
		int finished = 0;
		AGX_HIP_CHECK(hipMemcpy(&finished, ps->job.finished, sizeof(int), hipMemcpyDeviceToHost));
		ps->job_finished = finished;
		*open = finished < ps->job_n;
		return AGX_OK;
	}
	int searcher_begin_locked(AgxPositionSearcher *ps, int n, const uint8_t *d_boards, const uint8_t *d_signs, const int32_t *d_serials,
			const AgxPositionSearchOutputs *out, const AgxPositionSampleSink *sink, int max_pv, int max_steps, hipStream_t stream)
	{
		bool open = false;
		const int st = searcher_job_open(ps, &open);
		if (st != AGX_OK)
			return st;
		AGX_REQUIRE(!open, AGX_ERR_STATE, "agx_position_searcher_begin: the previous job has finished %d of its %d positions", ps->job_finished, ps->job_n);
		const int entered = searcher_enter(ps, stream, "agx_position_searcher_begin");
		if (entered != AGX_OK)
			return entered;
		ps->job.boards = d_boards;
		ps->job.signs = d_signs;
		ps->job.serials = d_serials;
		ps->job.n = n;
		ps->job.max_pv = max_pv;
		ps->job.max_steps = (max_steps > 0) ? max_steps : searcher_default_steps(ps);
		ps->job.out = *out;
		std::memset(&ps->job.sink, 0, sizeof(ps->job.sink));
		if (sink != nullptr && sink->d_bytes != nullptr && sink->d_sizes != nullptr)
			ps->job.sink = *sink;
		ps->job_n = n;
		ps->job_finished = 0;
		const EngineDev d = searcher_dev(ps);
		agx_eng::positions_reset(ps->job, stream);
		agx_eng::load_positions(d, ps->slots, ps->job, stream);
		return searcher_leave(ps, stream, AGX_OK);
	}
	int searcher_begin_checks(AgxPositionSearcher *ps, int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxPositionSearchOutputs *out, int max_pv, const char *what)
	{
		AGX_REQUIRE(ps != nullptr && out != nullptr, AGX_ERR_INVALID, "%s: null argument", what);
		AGX_REQUIRE(n >= 0, AGX_ERR_INVALID, "%s: %d positions", what, n);
		AGX_REQUIRE(max_pv >= 0 && max_pv <= MAXHW, AGX_ERR_INVALID, "%s: max_pv %d outside [0, %d]", what, max_pv, MAXHW);
		AGX_REQUIRE(n == 0 || (d_boards != nullptr && d_signs != nullptr), AGX_ERR_INVALID, "%s: null boards or signs", what);
		return AGX_OK;
	}
	int searcher_sink_checks(const AgxPositionSearcher *ps, const AgxPositionSampleSink *sink, const char *what)
	{ // (after searcher_begin_checks) a sample never outgrows its stride: 16 bytes and at most one entry per cell
		if (sink == nullptr || sink->d_bytes == nullptr || sink->d_sizes == nullptr)
			return AGX_OK;
		const int needed = agx::v201::HEADER_BYTES + agx::v201::ENTRY_BYTES * ps->engine->dev.hw;
		AGX_REQUIRE(sink->stride >= needed && sink->stride % 4 == 0, AGX_ERR_INVALID, "%s: a sample stride of %d bytes (at least %d and a multiple of 4 expected)", what,
				sink->stride, needed);
		return AGX_OK;
	}
	int searcher_harvest_locked(AgxPositionSearcher *ps, hipStream_t stream)
	{ // harvest -> arena service -> load: ordered by the launch order on one stream, as the stages behind k_advance are
		const EngineDev d = searcher_dev(ps);
		agx_eng::harvest_positions(d, ps->slots, ps->job, stream);
		agx_eng::arena_service(d, ps->slots, 0, stream);
		agx_eng::arena_copy(d, ps->slots, stream); // (its last part per game commits)
		agx_eng::load_positions(d, ps->slots, ps->job, stream);
		return AGX_OK;
	}
}

int agx::position_searcher_describe(AgxPositionSearcher *ps, int *rules, int *board_size, int *slots)
{
	AGX_REQUIRE(ps != nullptr, AGX_ERR_INVALID, "position searcher: null searcher");
	*rules = ps->engine->dev.rules;
	*board_size = ps->engine->dev.n;
	*slots = ps->slots;
	return AGX_OK;
}

extern "C" {

int agx_position_searcher_create(const AgxEngineConfig *cfg, AgxPositionSearcher **out)
{
	AGX_REQUIRE(cfg != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_position_searcher_create: null argument");
	*out = nullptr;
	AGX_REQUIRE(!cfg->match_mode, AGX_ERR_UNSUPPORTED, "agx_position_searcher_create: match_mode pools play matches, they search no positions");
	AGX_REQUIRE(cfg->search_threads <= 1 && cfg->search_buffers <= 1, AGX_ERR_UNSUPPORTED,
			"agx_position_searcher_create: search_threads > 1 / search_buffers > 1 make the pool one tree; the searcher needs a tree per slot");
	AgxEngineConfig own = *cfg;
	own.record_format = 0; // nothing is played: no move records, no samples, no finished games
	own.record_capacity = 1;
	own.record_edge_capacity = 1;
	own.record_sample_capacity = 4;
	own.game_end_capacity = 1;
	AgxEngine *engine = nullptr;
	const int created = agx_engine_create(&own, &engine);
	if (created != AGX_OK)
		return created;
	AgxPositionSearcher *ps = new AgxPositionSearcher();
	ps->engine = engine;
	ps->slots = cfg->n_games;
	std::memset(&ps->job, 0, sizeof(ps->job));
	const size_t words = 2 + 2 * static_cast<size_t>(ps->slots);
	int status = AGX_OK;
	if (hipGetDevice(&ps->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&ps->state), words * sizeof(int)) != hipSuccess
			|| hipHostMalloc(reinterpret_cast<void**>(&ps->poll_host), (2 + static_cast<size_t>(ps->slots)) * sizeof(int)) != hipSuccess
			|| hipEventCreateWithFlags(&ps->done, hipEventDisableTiming) != hipSuccess
			|| hipEventCreateWithFlags(&ps->poll_event[0], hipEventDisableTiming) != hipSuccess
			|| hipEventCreateWithFlags(&ps->poll_event[1], hipEventDisableTiming) != hipSuccess)
	{
		(void) hipGetLastError();
		agx::set_error("agx_position_searcher_create: allocating the slot records failed");
		status = AGX_ERR_HIP;
	}
	if (status == AGX_OK)
	{
		ps->job.cursor = ps->state;
		ps->job.finished = ps->state + 1;
		ps->job.slot_position = ps->state + 2;
		ps->job.slot_steps = ps->state + 2 + ps->slots;
		ps->device_bytes = engine->mem.device_bytes + words * sizeof(int);
		agx_eng::positions_init(engine->dev, ps->slots, ps->job, nullptr);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
		{
			(void) hipGetLastError();
			agx::set_error("agx_position_searcher_create: the launch that idles the slots failed");
			status = AGX_ERR_HIP;
		}
		engine->begun = true; // (the staged calls are the engine's own; its slots take positions where a pool takes openings)
	}
	if (status != AGX_OK)
	{
		const std::string message = agx_last_error();
		agx_position_searcher_destroy(ps);
		agx::set_error("%s", message.c_str());
		return status;
	}
	*out = ps;
	return AGX_OK;
}

int agx_position_searcher_destroy(AgxPositionSearcher *ps)
{
	if (ps == nullptr)
		return AGX_OK;
	if (ps->launched)
		(void) hipEventSynchronize(ps->done);
	if (ps->state != nullptr)
		(void) hipFree(ps->state);
	if (ps->poll_host != nullptr)
		(void) hipHostFree(ps->poll_host);
	for (hipEvent_t ev : { ps->done, ps->poll_event[0], ps->poll_event[1] })
		if (ev != nullptr)
			(void) hipEventDestroy(ev);
	(void) agx_engine_destroy(ps->engine);
	delete ps;
	return AGX_OK;
}

int agx_position_searcher_info(const AgxPositionSearcher *ps, int *slots, uint64_t *device_bytes)
{
	AGX_REQUIRE(ps != nullptr, AGX_ERR_INVALID, "agx_position_searcher_info: null searcher");
	if (slots != nullptr)
		*slots = ps->slots;
	if (device_bytes != nullptr)
		*device_bytes = ps->device_bytes;
	return AGX_OK;
}

int agx_position_searcher_engine(AgxPositionSearcher *ps, AgxEngine **out)
{
	AGX_REQUIRE(ps != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_position_searcher_engine: null argument");
	*out = ps->engine;
	return AGX_OK;
}

int agx_position_searcher_begin(AgxPositionSearcher *ps, int n, const uint8_t *d_boards, const uint8_t *d_signs, const int32_t *d_serials,
		const AgxPositionSearchOutputs *out, int max_pv, int max_steps, void *stream)
{
	return agx_position_searcher_begin_ex(ps, n, d_boards, d_signs, d_serials, out, nullptr, max_pv, max_steps, stream);
}

int agx_position_searcher_begin_ex(AgxPositionSearcher *ps, int n, const uint8_t *d_boards, const uint8_t *d_signs, const int32_t *d_serials,
		const AgxPositionSearchOutputs *out, const AgxPositionSampleSink *sink, int max_pv, int max_steps, void *stream)
{
	int st = searcher_begin_checks(ps, n, d_boards, d_signs, out, max_pv, "agx_position_searcher_begin");
	if (st == AGX_OK)
		st = searcher_sink_checks(ps, sink, "agx_position_searcher_begin");
	if (st != AGX_OK || n == 0)
		return st;
	std::lock_guard<std::mutex> lock(ps->mutex);
	return searcher_begin_locked(ps, n, d_boards, d_signs, d_serials, out, sink, max_pv, max_steps, static_cast<hipStream_t>(stream));
}

int agx_position_searcher_select_solve(AgxPositionSearcher *ps, void *stream)
{
	return searcher_call(ps, stream, "agx_position_searcher_select_solve", [&](hipStream_t) { return agx_engine_select_solve_group(ps->engine, 0, 1, stream); });
}

int agx_position_searcher_buffers(AgxPositionSearcher *ps, AgxEngineBuffers *out)
{
	AGX_REQUIRE(ps != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_position_searcher_buffers: null argument");
	return agx_engine_buffers(ps->engine, out);
}

int agx_position_searcher_evaluate(AgxPositionSearcher *ps, AgxNet *net, void *stream)
{
	AGX_REQUIRE(ps != nullptr && net != nullptr, AGX_ERR_INVALID, "agx_position_searcher_evaluate: null argument");
	return searcher_call(ps, stream, "agx_position_searcher_evaluate", [&](hipStream_t) { return agx_engine_evaluate_group(ps->engine, net, 0, 1, stream); });
}

int agx_position_searcher_expand(AgxPositionSearcher *ps, void *stream)
{ // (the harvest stage services the arenas)
	return searcher_call(ps, stream, "agx_position_searcher_expand", [&](hipStream_t) { return expand_stage(ps->engine, 0, 1, stream, false); });
}

int agx_position_searcher_harvest(AgxPositionSearcher *ps, void *stream)
{
	return searcher_call(ps, stream, "agx_position_searcher_harvest", [&](hipStream_t s) { return searcher_harvest_locked(ps, s); });
}

int agx_position_searcher_slots(AgxPositionSearcher *ps, void *stream, int *h_position_of_slot)
{
	AGX_REQUIRE(ps != nullptr && h_position_of_slot != nullptr, AGX_ERR_INVALID, "agx_position_searcher_slots: null argument");
	std::lock_guard<std::mutex> lock(ps->mutex);
	hipStream_t s = static_cast<hipStream_t>(stream);
	const int st = searcher_enter(ps, s, "agx_position_searcher_slots");
	if (st != AGX_OK)
		return st;
	AGX_HIP_CHECK(hipMemcpyAsync(ps->poll_host + 2, ps->job.slot_position, ps->slots * sizeof(int), hipMemcpyDeviceToHost, s));
	AGX_HIP_CHECK(hipStreamSynchronize(s));
	std::memcpy(h_position_of_slot, ps->poll_host + 2, ps->slots * sizeof(int));
	return AGX_OK;
}

int agx_position_searcher_finished(AgxPositionSearcher *ps, void *stream, int *count)
{
	AGX_REQUIRE(ps != nullptr && count != nullptr, AGX_ERR_INVALID, "agx_position_searcher_finished: null argument");
	std::lock_guard<std::mutex> lock(ps->mutex);
	hipStream_t s = static_cast<hipStream_t>(stream);
	const int st = searcher_enter(ps, s, "agx_position_searcher_finished");
	if (st != AGX_OK)
		return st;
	if (ps->job_n == 0)
	{
		*count = 0;
		return AGX_OK;
	}
	AGX_HIP_CHECK(hipMemcpyAsync(ps->poll_host, ps->job.finished, sizeof(int), hipMemcpyDeviceToHost, s));
	AGX_HIP_CHECK(hipStreamSynchronize(s));
	ps->job_finished = ps->poll_host[0];
	*count = ps->job_finished;
	return AGX_OK;
}

int agx_position_searcher_search(AgxPositionSearcher *ps, AgxNet *net, int n, const uint8_t *d_boards, const uint8_t *d_signs, const int32_t *d_serials,
		const AgxPositionSearchOutputs *out, int max_pv, int max_steps, void *stream_)
{
	return agx_position_searcher_search_ex(ps, net, n, d_boards, d_signs, d_serials, out, nullptr, max_pv, max_steps, stream_);
}

int agx_position_searcher_search_ex(AgxPositionSearcher *ps, AgxNet *net, int n, const uint8_t *d_boards, const uint8_t *d_signs, const int32_t *d_serials,
		const AgxPositionSearchOutputs *out, const AgxPositionSampleSink *sink, int max_pv, int max_steps, void *stream_)
{
	int checked = searcher_begin_checks(ps, n, d_boards, d_signs, out, max_pv, "agx_position_searcher_search");
	if (checked == AGX_OK)
		checked = searcher_sink_checks(ps, sink, "agx_position_searcher_search");
	if (checked != AGX_OK)
		return checked;
	AGX_REQUIRE(net != nullptr, AGX_ERR_INVALID, "agx_position_searcher_search: null network");
	if (n == 0)
		return AGX_OK;
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	std::lock_guard<std::mutex> lock(ps->mutex);
	int st = searcher_begin_locked(ps, n, d_boards, d_signs, d_serials, out, sink, max_pv, max_steps, stream);
	if (st != AGX_OK)
		return st;
	// every position finishes within max_steps steps of its load, a slot loads a new one in the step that finishes the old one: the slots work
	// through the list in at most ceil(n / slots) rounds of max_steps steps
	const long long rounds = (static_cast<long long>(n) + ps->slots - 1) / ps->slots;
	const long long step_bound = rounds * ps->job.max_steps + 1;
	constexpr int POLL_EVERY = 4; // steps between two reads of the finished counter; the read of the previous poll is awaited, so POLL_EVERY steps stay queued
	int polls = 0;
	bool all_finished = false;
	for (long long step = 0; !all_finished && step < step_bound + 2 * POLL_EVERY; step++)
	{
		st = agx_engine_select_solve_group(ps->engine, 0, 1, stream_);
		if (st == AGX_OK)
			st = agx_engine_evaluate_group(ps->engine, net, 0, 1, stream_);
		if (st == AGX_OK)
			st = expand_stage(ps->engine, 0, 1, stream_, false);
		if (st == AGX_OK)
			st = searcher_harvest_locked(ps, stream);
		if (st != AGX_OK)
			break;
		if ((step + 1) % POLL_EVERY != 0)
			continue;
		const int slot = polls & 1;
		if (hipMemcpyAsync(ps->poll_host + slot, ps->job.finished, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess
				|| hipEventRecord(ps->poll_event[slot], stream) != hipSuccess)
		{
			agx::set_error("agx_position_searcher_search: queuing a read of the finished counter failed: %s", hipGetErrorString(hipGetLastError()));
			st = AGX_ERR_HIP;
			break;
		}
		polls++;
		if (polls >= 2)
		{ // the poll before this one: its steps were queued POLL_EVERY steps ago
			st = agx_event_synchronize(ps->poll_event[slot ^ 1]);
			if (st != AGX_OK)
				break;
			ps->job_finished = ps->poll_host[slot ^ 1];
			all_finished = ps->job_finished >= n;
		}
	}
	(void) searcher_leave(ps, stream, AGX_OK);
	const hipError_t drained = hipStreamSynchronize(stream);
	if (st != AGX_OK)
		return st;
	AGX_HIP_CHECK(drained);
	int finished = 0;
	AGX_HIP_CHECK(hipMemcpy(&finished, ps->job.finished, sizeof(int), hipMemcpyDeviceToHost));
	ps->job_finished = finished;
	AGX_REQUIRE(finished >= n, AGX_ERR_STATE, "agx_position_searcher_search: %d of %d positions finished within the step bound", finished, n);
	return AGX_OK;
}

} /* extern "C" */
