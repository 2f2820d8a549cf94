/*
 * engine_host.hpp — the host side of the engine, shared by engine_host.cpp (AgxEngine and agx_engine_*), position_solver.cpp and
 * position_searcher.cpp: the engine object, the owner of its device allocations, the timer around a launch and the prologue of a stage.
 * No kernel is in reach of these files: they launch through engine_launch.hpp (engine.hip).
 */
#ifndef AGX_ENGINE_HOST_HPP_
#define AGX_ENGINE_HOST_HPP_

#include "agx_internal.hpp"
#include "engine_types.hpp"
#include "engine_launch.hpp"

#include <algorithm>
#include <vector>

namespace agx_host
{
	using namespace agx;

	/* What an object holds on the device: the pointers, their sum, and — for the position solver — the share of one wave.  sizing_only: nothing
	 * touches a device, alloc only adds up and every other member does nothing (agx_engine_estimate_device_bytes). */
	struct DeviceAllocations
	{
			std::vector<void*> pointers;
			unsigned long long device_bytes = 0; // sum of the allocations' sizes
			unsigned long long bytes_per_wave = 0; // ... of those made per_wave, divided by `waves`
			int waves = 0;
			bool sizing_only = false;
			const char *who = ""; // in front of an error text: "" or "agx_..._create: "

			template<typename T>
			int alloc(T **ptr, size_t count, bool per_wave = false)
			{
				const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
				void *p = nullptr;
				if (!sizing_only)
				{
					const hipError_t err = hipMalloc(&p, bytes);
					if (err != hipSuccess)
					{
						(void) hipGetLastError(); // the failure must not stay behind as the "last error" of this thread's later, successful calls
						agx::set_error("%shipMalloc of %zu bytes failed: %s", who, count * sizeof(T), hipGetErrorString(err));
						return AGX_ERR_HIP;
					}
					pointers.push_back(p);
				}
				device_bytes += bytes;
				if (per_wave)
					bytes_per_wave += bytes / static_cast<size_t>(waves);
				*ptr = static_cast<T*>(p);
				return AGX_OK;
			}
			template<typename T>
			int upload(const T **ptr, const std::vector<T> &src)
			{
				T *p = nullptr;
				const int st = alloc(&p, src.size());
				*ptr = p;
				return (st != AGX_OK) ? st : copy_in(p, src.data(), src.size() * sizeof(T));
			}
			int memset(void *p, int value, size_t bytes)
			{
				return sizing_only ? AGX_OK : checked("hipMemset", hipMemset(p, value, bytes));
			}
			int copy_in(void *dst, const void *src, size_t bytes)
			{
				return sizing_only ? AGX_OK : checked("hipMemcpy", hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
			}
			void free_all()
			{
				for (void *p : pointers)
					(void) hipFree(p);
				pointers.clear();
			}
		private:
			int checked(const char *call, hipError_t err)
			{
				if (err == hipSuccess)
					return AGX_OK;
				agx::set_error("%s%s failed: %s", who, call, hipGetErrorString(err));
				return AGX_ERR_HIP;
			}
	};

	inline size_t round_pow2(size_t x)
	{
		size_t r = 1;
		while (r < x)
			r <<= 1;
		return r;
	}
}

struct AgxEngine
{
		AgxEngineConfig cfg;
		agx::EngineDev dev;
		agx_host::DeviceAllocations mem; // mem.device_bytes: agx_engine_device_bytes; mem.sizing_only: agx_engine_estimate_device_bytes
		std::vector<agx::GameState> idle_games; // the pool before agx_engine_begin: every game idle, in its class-0 arena bundle
		std::vector<unsigned long long> debug_solve_nodes; // solver nodes per position of the last agx_debug_solve
		agx::ArenaHeap idle_heap;
		std::vector<uint64_t> zobrist; // [2*hw][2]
		bool begun = false;
		// Search::select and the threat solver of a game in one launch (k_solve<.., FUSED>); AGX_FUSE_SELECT=0 keeps them as two launches
		// (separate k_select / k_solve times in agx_engine_kernel_timing and in profiles)
		bool fuse_select = true;
		uint8_t *board_staging = nullptr; // agx_engine_set_board: the caller's board on its way to the device
		uint16_t *moves_staging = nullptr; // agx_engine_restore_game: the saved move list on its way to the device
		int *summary_dev = nullptr, *summary_host = nullptr; // agx_engine_root_summary: four words on their way back (device, pinned host)
		long long *match_sum_dev = nullptr, *match_sum_host = nullptr; // agx_engine_match_summary: its four sums, the same way
		// agx_engine_match_track_pairs: the pair log (head, shadows, entries: one allocation) and the pinned words its head comes back in;
		// pair_log.head == nullptr: no tracking, no launch
		agx::PairLogDev pair_log;
		size_t pair_log_bytes = 0;
		long long *pair_head_host = nullptr;
		// match pools: what each player searches with (agx_engine_set_player_search; both start as the pool's configuration).  dev's own
		// fields stay the pool's: has_q and tss_max_nodes there are what the pool was ALLOCATED for, the upper bounds of a player's
		agx::PlayerSearchDev player[2];
		// agx_engine_node_info / agx_engine_principal_variation: the paths on their way to the device and the answers on their way back, one
		// staging buffer each side (grown on demand)
		uint8_t *query_dev = nullptr, *query_host = nullptr;
		size_t query_bytes = 0;
		// AgxEngineConfig.speculative_solver: select + solver as one persistent launch with the leaves of a batch solved in parallel (k_search_spec)
		bool speculative = false;
		bool external_moves = false; // agx_engine_set_board has been called: the caller makes the moves, no advance stage services the arenas
		int spec_waves = 0; // waves of that launch over the whole pool
		// optional per-kernel timing (agx_engine_kernel_timing): HIP events on the launch stream around every kernel of a step
		bool timing = false;
		std::vector<hipEvent_t> events;   // groups of (before, after) per kernel launch
		std::vector<int> event_kernel;    // kernel id of each pair: 0 select, 1 solve, 2 expand, 3 advance
		std::vector<hipEvent_t> free_events;
};

namespace agx_host
{
	inline hipEvent_t timing_event(AgxEngine *e)
	{
		hipEvent_t ev = nullptr;
		if (!e->free_events.empty())
		{
			ev = e->free_events.back();
			e->free_events.pop_back();
		}
		else
			(void) hipEventCreate(&ev);
		return ev;
	}
	struct KernelTimer
	{ // records an event pair around one kernel launch when timing is enabled
			AgxEngine *e;
			hipStream_t s;
			hipEvent_t a = nullptr;
			KernelTimer(AgxEngine *engine, hipStream_t stream, int kernel) :
					e(engine), s(stream)
			{
				if (e->timing)
				{
					a = timing_event(e);
					(void) hipEventRecord(a, s);
					e->event_kernel.push_back(kernel);
				}
			}
			~KernelTimer()
			{
				if (e->timing)
				{
					hipEvent_t b = timing_event(e);
					(void) hipEventRecord(b, s);
					e->events.push_back(a);
					e->events.push_back(b);
				}
			}
	};

	/* What a stage launches with: the launch's own copy of the engine's record, narrowed to its games, and the stream */
	struct Stage
	{
			EngineDev d;
			int count = 0; // games from d.g0
			hipStream_t s = nullptr;
	};
	/* the prologue of a group stage `name`: the engine exists and has begun, games [d.g0, d.g0 + count) of group `group` out of `n_groups`
	 * equal parts of the pool (a match pool: that player's settings), the stream */
	int group_stage(AgxEngine *e, const char *name, int group, int n_groups, void *stream, Stage &st);
	/* Search::generateEdges + expand + backup for every game of the group (agx_engine_expand_group; the position searcher's expand stage) */
	int expand_stage(AgxEngine *e, int group, int n_groups, void *stream, bool with_arena_service);
}

#endif
