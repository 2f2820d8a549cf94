/*
 * engine_launch.hpp — the launch layer of engine.hip: one plain function per kernel of the engine (or per instantiation family), for the host
 * files that own the objects and the C ABI (engine_host.cpp, position_solver.cpp, position_searcher.cpp).  A launcher enqueues its kernel on
 * `s` with the grid the kernel is written for and does nothing else: no checks, no object, no error query (the caller asks hipGetLastError
 * once per entry point).  The kernels take EngineDev by value, so what a launcher is given is what the launch reads.
 */
#ifndef AGX_ENGINE_LAUNCH_HPP_
#define AGX_ENGINE_LAUNCH_HPP_

#include <hip/hip_runtime.h>

#include "engine_types.hpp"

namespace agx_eng
{
	using agx::EngineDev;

	/* k_search_spec of these rules and board size: the one-wave workgroups a compute unit keeps resident (asked of the runtime, 12 if it will not say) */
	int spec_resident_waves_per_cu(int rules, int n);
	/* select + speculative solve + scheduleToNN of `count` games from d.g0 as one persistent launch of d.spec_waves waves (MERGED when d.match_merged) */
	void search_spec(const EngineDev &d, int count, hipStream_t s);

	void begin(const EngineDev &d, hipStream_t s);                                  // every game of the pool
	void assign_openings(const EngineDev &d, int count, hipStream_t s);
	void match_restart(const EngineDev &d, int pairs, hipStream_t s);
	void reset_spec(int *nn_counter, int *nn_second, int *spec_counters, int *done_counter, hipStream_t s);
	void solve(const EngineDev &d, int count, bool with_select, hipStream_t s);     // k_solve<.., FUSED = with_select>, one wave per game from d.g0
	void reset_counter(int *counter, int *second, hipStream_t s);
	void select(const EngineDev &d, int waves, hipStream_t s);

	void expand_merged(const EngineDev &d, hipStream_t s);                          // a match pool's launch over both players' trees
	void advance_merged(const EngineDev &d, hipStream_t s);
	void match_pair_log(const EngineDev &d, const agx::PairLogDev &log, hipStream_t s);
	void arena_service(const EngineDev &d, int count, int assign_count, hipStream_t s);
	void arena_copy(const EngineDev &d, int trees, hipStream_t s);                  // CLEAR_PARTS workgroups per tree
	void clear_tables(const EngineDev &d, int games, int restart, hipStream_t s);   // CLEAR_PARTS workgroups per game
	void expand(const EngineDev &d, int waves, hipStream_t s);
	void advance(const EngineDev &d, int trees, hipStream_t s);
	void restart(const EngineDev &d, int games, hipStream_t s);

	void cancel_pending(const EngineDev &d, int waves, hipStream_t s);
	void set_board(const EngineDev &d, int g, const uint8_t *board, int sign_to_move, int force_remove_root, hipStream_t s);
	void restore_game(const EngineDev &d, int g, const uint16_t *moves, int count, int opening_id, int nn_queued, hipStream_t s);
	void root_summary(const EngineDev &d, int g, int *out, hipStream_t s);
	void node_info(const EngineDev &d, int n_paths, int tree, const uint16_t *moves, const int *offsets, AgxNodeView *out_nodes, AgxEdgeView *out_edges,
			int edges_per_path, hipStream_t s);
	void principal_variation(const EngineDev &d, int tree, const uint16_t *moves, int n_moves, int max_length, int *out_length, uint16_t *out_pv,
			AgxEdgeView *out_edges, AgxNodeView *out_nodes, hipStream_t s);
	void match_summary(const EngineDev &d, long long *out, hipStream_t s);

	void debug_load_tasks(const EngineDev &d, const uint8_t *boards, const int *signs, int count, hipStream_t s);
	void debug_pattern_state(const EngineDev &d, int count, const uint8_t *boards, const int *signs, const uint16_t *moves, int n_moves, uint8_t *ptypes,
			uint8_t *threats, int16_t *lists, int lists_stride, hipStream_t s);

	void solve_positions(const EngineDev &d, int waves, const agx::SolvePositionsArgs &args, hipStream_t s);
	void positions_reset(const agx::PositionJob &job, hipStream_t s);
	void load_positions(const EngineDev &d, int slots, const agx::PositionJob &job, hipStream_t s);
	void harvest_positions(const EngineDev &d, int slots, const agx::PositionJob &job, hipStream_t s);
	void positions_init(const EngineDev &d, int slots, const agx::PositionJob &job, hipStream_t s);
}

#endif
