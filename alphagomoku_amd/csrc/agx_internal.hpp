/*
 * agx_internal.hpp — shared helpers of the HIP/C++ implementation behind include/agx.h.
 */
#ifndef AGX_INTERNAL_HPP_
#define AGX_INTERNAL_HPP_

#include <hip/hip_runtime.h>
#include <string>
#include <cstdio>
#include <cstdarg>

#include "../../include/agx.h"

namespace agx
{
	void set_error(const char *fmt, ...);

	struct HipError
	{
			hipError_t code;
	};

	/* net_score.hip: one launch of one workgroup on `stream` that adds the n records of d_scores into *d_total in sample order (the ordered
	 * reduction behind agx_net_score_outputs); checks hipGetLastError, so a caller's launch just before it is covered too */
	int add_sample_scores(int n, AgxSampleScore *d_scores, AgxNetScore *d_total, hipStream_t stream);

	/* position_solver.cpp, for agx_position_evaluator_evaluate_solved (position_eval.hip): what a position solver was created for and its device
	 * workspace [capacity] (score, n_actions, moves, move_scores, status; the other members null) ... */
	int position_solver_describe(AgxPositionSolver *solver, int *rules, int *board_size, int *capacity, AgxSolvedPositions *workspace);
	/* ... and "the work enqueued on `stream` so far still reads the solver's workspace": the solver's next call on another stream waits for it */
	int position_solver_mark(AgxPositionSolver *solver, hipStream_t stream);
	/* position_searcher.cpp, for agx_dataset_reanalyse (training_batch.hip): what a position searcher was created for */
	int position_searcher_describe(AgxPositionSearcher *ps, int *rules, int *board_size, int *slots);
}

#define AGX_HIP_CHECK(expr)                                                                         \
	do {                                                                                            \
		hipError_t _e = (expr);                                                                     \
		if (_e != hipSuccess) {                                                                     \
			agx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
			return AGX_ERR_HIP;                                                                     \
		}                                                                                           \
	} while (0)

#define AGX_REQUIRE(cond, code, ...)                                                                \
	do {                                                                                            \
		if (!(cond)) {                                                                              \
			agx::set_error(__VA_ARGS__);                                                            \
			return (code);                                                                          \
		}                                                                                           \
	} while (0)

#endif /* AGX_INTERNAL_HPP_ */
