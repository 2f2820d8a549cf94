/*
 * position_solver.cpp — AgxPositionSolver and agx_position_solver_* of the C ABI (include/agx.h): the threat solver on boards
 * (k_solve_positions in engine.hip, launched through engine_launch.hpp).
 */
#include "engine_host.hpp"
#include "tables_host.hpp"

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

using namespace agx;
using namespace agx_host;

struct AgxPositionSolver
{
		int rules = 0, n = 0, capacity = 0, waves = 0;
		int device = -1;
		std::mutex mutex;
		EngineDev dev; // only what solve_task reads: tables, limits, the per-wave areas, a task and a game record per wave
		DeviceAllocations mem; // (mem.bytes_per_wave: a wave's table, spill areas and records)
		AgxSolvedPositions workspace; // [capacity] outputs of agx_position_evaluator_evaluate_solved the caller did not ask for
		// the waves of two launches share the per-wave areas: a call on another stream than the previous one is ordered behind it on the device
		hipEvent_t done = nullptr;
		hipStream_t last_stream = nullptr;
		bool launched = false;
};

int agx::position_solver_describe(AgxPositionSolver *ps, int *rules, int *board_size, int *capacity, AgxSolvedPositions *workspace)
{
	AGX_REQUIRE(ps != nullptr, AGX_ERR_INVALID, "null position solver");
	*rules = ps->rules;
	*board_size = ps->n;
	*capacity = ps->capacity;
	*workspace = ps->workspace;
	return AGX_OK;
}
int agx::position_solver_mark(AgxPositionSolver *ps, hipStream_t stream)
{
	std::lock_guard<std::mutex> lock(ps->mutex);
	AGX_HIP_CHECK(hipEventRecord(ps->done, stream));
	ps->launched = true;
	ps->last_stream = stream;
	return AGX_OK;
}

extern "C" {

int agx_position_solver_create(int rules, int board_size, int capacity, int max_positions, uint64_t table_entries, uint64_t zobrist_seed, AgxPositionSolver **out)
{
	AGX_REQUIRE(out != nullptr, AGX_ERR_INVALID, "agx_position_solver_create: null argument");
	*out = nullptr;
	AGX_REQUIRE(rules >= 0 && rules <= AGX_CARO6, AGX_ERR_INVALID, "agx_position_solver_create: unknown rules %d", rules);
	AGX_REQUIRE(board_size >= 5 && board_size <= MAXN, AGX_ERR_UNSUPPORTED, "agx_position_solver_create: board size %d not in [5, %d]", board_size, MAXN);
	AGX_REQUIRE(capacity > 0 && capacity <= (1 << 20), AGX_ERR_INVALID, "agx_position_solver_create: capacity %d", capacity);
	AGX_REQUIRE(max_positions >= 1 && max_positions <= 1000, AGX_ERR_UNSUPPORTED, "agx_position_solver_create: max_positions must be in [1, 1000]");
	AGX_REQUIRE(table_entries <= (1ull << 32), AGX_ERR_INVALID, "agx_position_solver_create: %llu table entries per wave (at most 2^32)",
			static_cast<unsigned long long>(table_entries));
	AgxPositionSolver *ps = new AgxPositionSolver();
	ps->rules = rules;
	ps->n = board_size;
	ps->capacity = capacity;
	std::memset(&ps->workspace, 0, sizeof(ps->workspace));
	EngineDev &d = ps->dev;
	std::memset(&d, 0, sizeof(d));
	int status = AGX_OK, cus = 0;
	if (hipGetDevice(&ps->device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ps->device) != hipSuccess)
	{
		(void) hipGetLastError();
		agx::set_error("agx_position_solver_create: no HIP device");
		status = AGX_ERR_HIP;
	}
	// one wave per SIMD: k_solve_positions is compiled like k_solve, for the fastest single wave (uncapped registers), and every wave brings
	// a table and spill areas of its own
	ps->waves = std::min(capacity, 4 * std::max(1, cus));
	if (const char *cap = std::getenv("AGX_POSSOLVE_MAX_WAVES"))
		if (std::atoi(cap) > 0)
			ps->waves = std::min(ps->waves, std::atoi(cap));
	d.rules = rules;
	d.n = board_size;
	d.hw = board_size * board_size;
	d.draw_after = d.hw;
	d.n_games = ps->waves;
	d.batch = d.batch_limit = 1;
	d.tss_max_nodes = max_positions;
	d.tss_max_depth = 100;
	d.solve_time_ticks = 0ull;
	d.zobrist_seed = zobrist_seed;
	const size_t buckets = round_pow2(std::max<size_t>(table_entries, 4)) / 4;
	d.tt_bucket_mask = buckets - 1;
	d.act_cap = d.hw * (d.hw + 1) / 2 + 64;
	d.tt_mod = ps->waves;
	const size_t W = ps->waves, hw = d.hw, C = capacity;
	HostTables tables;
	build_host_tables(rules, tables);
	std::vector<uint8_t> packed(4096); // cross type | circle type << 4 (dev_solver.hpp: threat_lookup)
	for (int i = 0; i < 4096; i++)
		packed[i] = static_cast<uint8_t>((tables.threat[2 * i] & 15u) | ((tables.threat[2 * i + 1] & 15u) << 4));
	ps->mem.waves = ps->waves;
	ps->mem.who = "agx_position_solver_create: ";
#define AGX_TRY(expr) if (status == AGX_OK) status = (expr)
	AGX_TRY(ps->mem.alloc(&d.tt, W * buckets * 8, true));
	AGX_TRY(ps->mem.alloc(&d.act, W * d.act_cap, true));
	AGX_TRY(ps->mem.alloc(&d.list_spill, W * 20 * static_cast<size_t>(MAXHW), true));
	AGX_TRY(ps->mem.alloc(&d.frame_spill, W * MAX_FRAMES, true));
	AGX_TRY(ps->mem.alloc(&d.snap_spill, W * (hw + 2) * 64, true)); // one undo-snapshot level per stone on the board, whatever the rules
	AGX_TRY(ps->mem.alloc(&d.tasks, W, true));
	AGX_TRY(ps->mem.alloc(&d.games, W, true));
	AGX_TRY(ps->mem.alloc(&d.nn_features, W * hw, true)); // solve_task encodes the network input of its task on the way
	AGX_TRY(ps->mem.upload(&d.t_pattern, tables.pattern));
	AGX_TRY(ps->mem.upload(&d.t_ho3, tables.half_open_three));
	AGX_TRY(ps->mem.upload(&d.t_threat, tables.threat));
	AGX_TRY(ps->mem.upload(&d.t_threat_packed, packed));
	AGX_TRY(ps->mem.upload(&d.t_defense, tables.defense));
	AGX_TRY(ps->mem.alloc(&ps->workspace.score, C));
	AGX_TRY(ps->mem.alloc(&ps->workspace.n_actions, C));
	AGX_TRY(ps->mem.alloc(&ps->workspace.moves, C * hw));
	AGX_TRY(ps->mem.alloc(&ps->workspace.move_scores, C * hw));
	AGX_TRY(ps->mem.alloc(&ps->workspace.status, C));
#undef AGX_TRY
	if (status == AGX_OK && (ps->mem.memset(d.games, 0, W * sizeof(GameState)) != AGX_OK || ps->mem.memset(d.tasks, 0, W * sizeof(DTask)) != AGX_OK
			|| hipEventCreateWithFlags(&ps->done, hipEventDisableTiming) != hipSuccess))
	{
		agx::set_error("agx_position_solver_create: clearing the per-wave records failed");
		status = AGX_ERR_HIP;
	}
	if (status != AGX_OK)
	{ // one way out for every failure: what was allocated is freed, *out stays null
		const std::string message = agx_last_error();
		agx_position_solver_destroy(ps);
		agx::set_error("%s", message.c_str());
		return status;
	}
	*out = ps;
	return AGX_OK;
}

int agx_position_solver_destroy(AgxPositionSolver *ps)
{
	if (ps == nullptr)
		return AGX_OK;
	if (ps->launched)
		(void) hipEventSynchronize(ps->done);
	ps->mem.free_all();
	if (ps->done != nullptr)
		(void) hipEventDestroy(ps->done);
	delete ps;
	return AGX_OK;
}

int agx_position_solver_info(const AgxPositionSolver *ps, int *waves, uint64_t *bytes_per_wave, uint64_t *device_bytes)
{
	AGX_REQUIRE(ps != nullptr, AGX_ERR_INVALID, "agx_position_solver_info: null solver");
	if (waves != nullptr)
		*waves = ps->waves;
	if (bytes_per_wave != nullptr)
		*bytes_per_wave = ps->mem.bytes_per_wave;
	if (device_bytes != nullptr)
		*device_bytes = ps->mem.device_bytes;
	return AGX_OK;
}

int agx_position_solver_solve(AgxPositionSolver *ps, int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxSolvedPositions *out, void *stream_)
{
	AGX_REQUIRE(ps != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_position_solver_solve: null argument");
	AGX_REQUIRE(n >= 0 && n <= ps->capacity, AGX_ERR_INVALID, "agx_position_solver_solve: %d positions, the solver was created for %d", n, ps->capacity);
	if (n == 0)
		return AGX_OK;
	AGX_REQUIRE(d_boards != nullptr && d_signs != nullptr, AGX_ERR_INVALID, "agx_position_solver_solve: null boards or signs");
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	std::lock_guard<std::mutex> lock(ps->mutex);
	int current = -1;
	AGX_HIP_CHECK(hipGetDevice(&current));
	AGX_REQUIRE(current == ps->device, AGX_ERR_STATE, "agx_position_solver_solve: the solver lives on device %d, the calling thread's current device is %d", ps->device, current);
	if (ps->launched && ps->last_stream != stream)
		AGX_HIP_CHECK(hipStreamWaitEvent(stream, ps->done, 0));
	SolvePositionsArgs A;
	A.boards = d_boards;
	A.signs = d_signs;
	A.n = n;
	A.out = *out;
	agx_eng::solve_positions(ps->dev, std::min(n, ps->waves), A, stream);
	const hipError_t launched = hipGetLastError();
	AGX_HIP_CHECK(hipEventRecord(ps->done, stream));
	ps->launched = true;
	ps->last_stream = stream;
	AGX_HIP_CHECK(launched);
	return AGX_OK;
}

} /* extern "C" */
