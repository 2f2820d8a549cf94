/*
 * position_eval.hip — boards to policy, value and best moves on the device (agx.h: agx_position_evaluator_*).
 *
 * What it stands for: the primary entry point of the reference's network, AGNetwork::packInputData(index, board, signToMove)
 * (AGNetwork.hpp:60: PatternCalculator::setBoard + NNInputFeatures::encode on the host, one position after the other), for the callers
 * that hold a board and no search: the analysis front end, SupervisedLearning::validate, a network-only player, opening balancing.
 * Averaging over several symmetries and the top-k picks are this project's own (the reference's NNEvaluator draws ONE random symmetry per
 * position and has no top-k on this path); DESIGN 3.9 gives the formulas.
 *
 * MI355X mapping: two kernels around the tower, one wavefront per unit of work, nothing shared between waves, no atomics.
 *   k_encode_positions   one wave per (position, symmetry) ROW: the board gathered through symmetry_source() into LDS, then the solver's
 *                        own solver_set_board / solver_encode_features / solver_encode_forbidden on it (dev_solver.hpp, as
 *                        k_training_batch drives them: an EngineDev that carries only tables, per-wave threat-list tails and — renju —
 *                        18 undo-snapshot levels in HBM), the feature words to row p * S + j.
 *   k_combine_positions  one wave per POSITION behind the tower: the S rows of a position are added cell by cell through the inverse
 *                        symmetry map (built once per wave in LDS), masked, optionally renormalised, and the top_k legal cells picked.
 *   k_combine_solved_positions  the same behind the threat solver (agx_position_evaluator_evaluate_solved; the solve itself is
 *                        k_solve_positions in engine.hip): the solver's action list is the move set, a proven position gets its score's value.
 * Every sum has a fixed order (ascending symmetry; cell order for the renormalisation), so the outputs are a pure function of the
 * tower's rows: tests/position_eval_ref.py (position_solve_ref.py behind the solver) restates the combine step in numpy float32 and the comparison is on the bits.
 * Like training_batch.hip the file is built with -ffp-contract=off and correctly rounded float32 division.
 */
#include "agx_internal.hpp"
#include "dev_solver.hpp"
#include "symmetry.hpp"
#include "tables_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace agx
{
	namespace
	{
		constexpr int PE_SNAP_LEVELS = 18; // renju_is_forbidden nests at most 16 stones (dev_solver.hpp: fstack)
		constexpr int PE_MAX_WAVES = 2048; // workgroups of a launch (one wave each); more rows / positions stride.  Sizes the per-wave spill areas
		constexpr int PE_MAX_TOP_K = 8;

		struct EncodeArgs
		{
				const uint8_t *boards;  // [n][hw] 0 empty, 1 cross, 2 circle
				const uint8_t *signs;   // [n] 1 cross, 2 circle
				int n, mask, S;
				uint32_t *features;     // [n * S][hw]
				int *status;            // [n], zeroed on the stream before the launch; may be null
				uint16_t *list_spill;   // [waves][20][SH::HW]
				uint64_t *snap_spill;   // [waves][PE_SNAP_LEVELS][64], null unless renju
		};

		/* the j-th set bit of mask (j < popcount(mask)) */
		__host__ __device__ __forceinline__ int symmetry_of_rank(int mask, int j)
		{
			int s = 0;
			for (int bit = 0; bit < 8; bit++)
				if ((mask >> bit) & 1)
				{
					if (j == 0)
						s = bit;
					j--;
				}
			return s;
		}

		template<int N>
		__global__ __launch_bounds__(64) void k_encode_positions(EngineDev E, EncodeArgs A)
		{
			using namespace dev;
			typedef SolverSharedT<N> SH;
			__shared__ SH sh;
			__shared__ uint8_t board[N * N]; // the position under the row's symmetry
			__shared__ uint32_t feat[N * N];
			const int lane = threadIdx.x;
			const int n = E.n, hw = E.hw;
			const int rows = A.n * A.S;
			solver_load_threat_table(sh, E, lane);

			for (int row = blockIdx.x; row < rows; row += gridDim.x)
			{
				const int p = row / A.S;
				const int s = symmetry_of_rank(A.mask, row % A.S);
				const uint8_t *src = A.boards + static_cast<size_t>(p) * hw;
				const int sign_to_move = A.signs[p];
				bool bad = false;
				for (int i = lane; i < hw; i += 64)
				{
					int sr, sc;
					symmetry_source(s, n, i / n, i % n, sr, sc);
					const uint8_t v = src[sr * n + sc];
					bad |= (v > 2);
					board[i] = v;
				}
				uint32_t *out = A.features + static_cast<size_t>(row) * hw;
				if (__ballot(bad) != 0ull || (sign_to_move != 1 && sign_to_move != 2))
				{ // not a position: nothing of it reaches the solver (whose tables are indexed by cell values)
					for (int i = lane; i < hw; i += 64)
						out[i] = 0u;
					if (lane == 0 && A.status != nullptr)
						A.status[p] = AGX_POSEVAL_STATUS_BAD_INPUT; // (every row of the position writes the same word)
					wave_sync();
					continue;
				}
				wave_sync();
				if (lane == 0)
				{ // (before solver_set_board: a threat list longer than its LDS capacity continues in the spill area)
					sh.error = 0;
					sh.spill_lists = A.list_spill + static_cast<size_t>(blockIdx.x) * 20 * SH::HW;
					sh.spill_frames = nullptr;
				}
				wave_sync();
				solver_set_board(sh, E, board, sign_to_move, lane);
				if (lane == 0)
				{ // snapshot level `stones on the board` is slot 0 of this wave's area
					const uintptr_t area = reinterpret_cast<uintptr_t>(A.snap_spill) + static_cast<uintptr_t>(blockIdx.x) * PE_SNAP_LEVELS * 64 * sizeof(u64);
					sh.snap = (A.snap_spill == nullptr) ? nullptr : reinterpret_cast<u64*>(area - static_cast<uintptr_t>(sh.depth) * 64 * sizeof(u64));
				}
				wave_sync();
				solver_encode_features(sh, E, feat, lane);
				wave_sync();
				solver_encode_forbidden(sh, E, feat, lane); // renju, cross to move: bit 6 on the fouls (wave_sync inside)
				wave_sync();
				for (int i = lane; i < hw; i += 64)
					out[i] = feat[i];
				// renju_is_forbidden gives up (its probe stones left on the board) when 3x3 forks nest 16 deep: the row's words are not to be trusted
				if (lane == 0 && sh.error != 0 && A.status != nullptr)
					A.status[p] = AGX_POSEVAL_STATUS_FOUL_PROBE;
				wave_sync(); // the next row reuses the LDS arrays
			}
		}

		struct CombineArgs
		{
				int n, mask, S, flags, top_k;
				const uint8_t *boards;         // [n][hw]
				const uint32_t *features;      // [n * S][hw]; read only with AGX_POSEVAL_MASK_FORBIDDEN (row p * S is then the identity's)
				const float *policy_rows;      // [n * S][hw]
				const float *value_rows;       // [n * S][3]
				const float *q_rows;           // [n * S][hw][2] or null
				const int *status_in;          // [n] or null
				float *policy, *value, *action_values; // [n][hw], [n][3], [n][hw][2]; each may be null
				int *top_cells;                // [n][top_k] or null
				float *top_probs;              // [n][top_k] or null
				int *status;                   // [n] or null
		};

		/* (k_combine_solved_positions below repeats the sums, the ordered renormalising sum and the top-k rounds of this kernel: a change to
		 * an order or a tie-break here is a change there, and in tests/position_eval_ref.py / position_solve_ref.py) */
		template<int N>
		__global__ __launch_bounds__(64) void k_combine_positions(CombineArgs A)
		{
			constexpr int HW = N * N, CHUNKS = (HW + 63) / 64;
			// image[j][c]: where cell c of the untransformed board lies in the row of the j-th symmetry.  2-byte entries, row-major: the 64
			// lanes of a read take 64 consecutive cells of one row, i.e. 32 consecutive dwords, every bank once (two lanes share a dword)
			__shared__ uint16_t image[8][HW];
			const int lane = threadIdx.x;
			const int S = A.S;
			for (int j = 0; j < S; j++)
			{
				const int s = symmetry_of_rank(A.mask, j);
				for (int i = lane; i < HW; i += 64)
				{ // the row's cell i shows the board's cell (sr, sc): the inverse of symmetry_source
					int sr, sc;
					symmetry_source(s, N, i / N, i % N, sr, sc);
					image[j][sr * N + sc] = static_cast<uint16_t>(i);
				}
			}
			__syncthreads();
			const float inv_s = 1.0f / static_cast<float>(S);

			for (int p = blockIdx.x; p < A.n; p += gridDim.x)
			{
				const int st = (A.status_in != nullptr) ? A.status_in[p] : 0;
				const bool bad = (st & AGX_POSEVAL_STATUS_BAD_INPUT) != 0;
				const size_t row0 = static_cast<size_t>(p) * S;
				if (lane == 0 && A.status != nullptr)
					A.status[p] = st;
				if (lane < 3 && A.value != nullptr)
				{
					float sum = 0.0f;
					for (int j = 0; j < S; j++)
						sum += A.value_rows[(row0 + j) * 3 + lane];
					A.value[static_cast<size_t>(p) * 3 + lane] = bad ? 0.0f : sum * inv_s;
				}
				float prob[CHUNKS];
				uint32_t legal = 0; // bit ch: cell ch * 64 + lane may be picked
				float total = 0.0f;
#pragma unroll
				for (int ch = 0; ch < CHUNKS; ch++)
				{
					const int cell = ch * 64 + lane;
					const bool inside = cell < HW;
					float sum = 0.0f, win = 0.0f, draw = 0.0f;
					bool free_cell = false;
					if (inside && !bad)
					{
						for (int j = 0; j < S; j++)
						{
							const size_t at = (row0 + j) * HW + image[j][cell];
							sum += A.policy_rows[at];
							if (A.q_rows != nullptr && A.action_values != nullptr)
							{
								win += A.q_rows[at * 2 + 0];
								draw += A.q_rows[at * 2 + 1];
							}
						}
						sum *= inv_s;
						free_cell = (A.boards[static_cast<size_t>(p) * HW + cell] == 0);
						if (free_cell && (A.flags & AGX_POSEVAL_MASK_FORBIDDEN) != 0)
							free_cell = ((A.features[row0 * HW + cell] >> 6) & 1u) == 0u;
						if (!free_cell)
							sum = 0.0f;
					}
					if (inside && A.action_values != nullptr)
					{
						float *q = A.action_values + (static_cast<size_t>(p) * HW + cell) * 2;
						q[0] = win * inv_s;
						q[1] = draw * inv_s;
					}
					prob[ch] = sum;
					legal |= free_cell ? (1u << ch) : 0u;
					if ((A.flags & AGX_POSEVAL_RENORMALISE) != 0)
					{ // total += prob[cell], in cell order; + 0.0f changes nothing
						unsigned long long nonzero = __ballot(sum != 0.0f);
						while (nonzero != 0ull)
						{
							const int from = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(nonzero)) - 1);
							nonzero &= nonzero - 1ull;
							total += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sum), from));
						}
					}
				}
				if ((A.flags & AGX_POSEVAL_RENORMALISE) != 0 && total != 0.0f)
				{
					const float scale = 1.0f / total;
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
						prob[ch] *= scale;
				}
				if (A.policy != nullptr)
				{
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
						if (ch * 64 + lane < HW)
							A.policy[static_cast<size_t>(p) * HW + ch * 64 + lane] = prob[ch];
				}
				// top_k rounds of an argmax over (value, lowest cell index) among the legal cells not picked yet; a NaN orders as -inf
				for (int k = 0; k < A.top_k; k++)
				{
					float best = -INFINITY;
					int at = 0x7FFFFFFF; // "no cell": loses against every cell
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
					{
						const float key = (prob[ch] != prob[ch]) ? -INFINITY : prob[ch];
						if (((legal >> ch) & 1u) != 0u && (key > best || at == 0x7FFFFFFF))
						{
							best = key;
							at = ch * 64 + lane;
						}
					}
#pragma unroll
					for (int off = 1; off < 64; off <<= 1)
					{
						const float ov = __shfl_xor(best, off, 64);
						const int oi = __shfl_xor(at, off, 64);
						if (oi != 0x7FFFFFFF && (at == 0x7FFFFFFF || ov > best || (ov == best && oi < at)))
						{
							best = ov;
							at = oi;
						}
					}
					const size_t slot = static_cast<size_t>(p) * A.top_k + k;
					if (at == 0x7FFFFFFF)
					{ // fewer legal cells than top_k
						if (lane == 0 && A.top_cells != nullptr)
							A.top_cells[slot] = -1;
						if (lane == 0 && A.top_probs != nullptr)
							A.top_probs[slot] = 0.0f;
						continue;
					}
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
						if (ch * 64 + lane == at)
						{ // the winner's own lane
							if (A.top_cells != nullptr)
								A.top_cells[slot] = at;
							if (A.top_probs != nullptr)
								A.top_probs[slot] = prob[ch];
							legal &= ~(1u << ch);
						}
				}
			}
		}
		struct SolvedArgs
		{ // what agx_position_solver_solve wrote for the batch
				const uint16_t *score;       // [n]
				const int *n_actions;        // [n]
				const uint16_t *moves;       // [n][hw]
				const uint16_t *move_scores; // [n][hw]
				const int *status;           // [n]
		};

		/* k_combine_positions behind the solver (agx_position_evaluator_evaluate_solved): the same sums in the same orders, then the solver's
		 * action list as the move set — an unproven position keeps the network's policy on the list only, a proven one gets its score's value
		 * and 1.0f / k on the k best actions.  A kernel of its own: k_combine_positions stays as it is. */
		template<int N>
		__global__ __launch_bounds__(64) void k_combine_solved_positions(CombineArgs A, SolvedArgs V)
		{
			constexpr int HW = N * N, CHUNKS = (HW + 63) / 64;
			__shared__ uint16_t image[8][HW]; // as in k_combine_positions
			__shared__ uint8_t listed[HW];    // 0: not in the action list, 1: in it, 2: in it with the list's best score
			const int lane = threadIdx.x;
			const int S = A.S;
			for (int j = 0; j < S; j++)
			{
				const int s = symmetry_of_rank(A.mask, j);
				for (int i = lane; i < HW; i += 64)
				{
					int sr, sc;
					symmetry_source(s, N, i / N, i % N, sr, sc);
					image[j][sr * N + sc] = static_cast<uint16_t>(i);
				}
			}
			__syncthreads();
			const float inv_s = 1.0f / static_cast<float>(S);

			for (int p = blockIdx.x; p < A.n; p += gridDim.x)
			{
				const int st_eval = (A.status_in != nullptr) ? A.status_in[p] : 0, st_solver = V.status[p];
				const bool bad = (st_eval & AGX_POSEVAL_STATUS_BAD_INPUT) != 0 || st_solver == AGX_POSSOLVE_STATUS_BAD_INPUT;
				const size_t row0 = static_cast<size_t>(p) * S;
				const uint32_t score = V.score[p];
				const int pv = (score >> 13) & 3;
				const bool proven = !bad && pv != 2 && score != 0u && score != 0xFFFFu; // Score::isProven
				const int count = bad ? 0 : min(V.n_actions[p], HW);
				uint32_t best = 0;
				for (int i = lane; i < count; i += 64)
					best = max(best, static_cast<uint32_t>(V.move_scores[static_cast<size_t>(p) * HW + i]));
#pragma unroll
				for (int off = 1; off < 64; off <<= 1)
					best = max(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), off, 64)));
				__syncthreads(); // the previous position's marks have been read
				for (int i = lane; i < HW; i += 64)
					listed[i] = 0;
				__syncthreads();
				int n_best = 0;
				for (int i = lane; i < count; i += 64)
				{
					const uint32_t m = V.moves[static_cast<size_t>(p) * HW + i];
					const int cell = static_cast<int>((m >> 2) & 127u) * N + static_cast<int>((m >> 9) & 127u);
					const bool is_best = V.move_scores[static_cast<size_t>(p) * HW + i] == best;
					if (cell < HW)
					{
						listed[cell] = is_best ? 2 : 1;
						n_best += is_best ? 1 : 0;
					}
				}
#pragma unroll
				for (int off = 1; off < 64; off <<= 1)
					n_best += __shfl_xor(n_best, off, 64);
				__syncthreads();
				const float share = (n_best > 0) ? 1.0f / static_cast<float>(n_best) : 0.0f;
				if (lane == 0 && A.status != nullptr)
					A.status[p] = max(st_eval, st_solver);
				if (lane < 3 && A.value != nullptr)
				{
					float sum = 0.0f;
					for (int j = 0; j < S; j++)
						sum += A.value_rows[(row0 + j) * 3 + lane];
					const float of_score = (pv == ((lane == 0) ? 3 : ((lane == 1) ? 1 : 0))) ? 1.0f : 0.0f;
					A.value[static_cast<size_t>(p) * 3 + lane] = bad ? 0.0f : (proven ? of_score : sum * inv_s);
				}
				float prob[CHUNKS];
				uint32_t legal = 0; // bit ch: cell ch * 64 + lane may be picked
				float total = 0.0f;
#pragma unroll
				for (int ch = 0; ch < CHUNKS; ch++)
				{
					const int cell = ch * 64 + lane;
					const bool inside = cell < HW;
					float sum = 0.0f, win = 0.0f, draw = 0.0f;
					bool free_cell = false;
					if (inside && !bad)
					{
						for (int j = 0; j < S; j++)
						{
							const size_t at = (row0 + j) * HW + image[j][cell];
							sum += A.policy_rows[at];
							if (A.q_rows != nullptr && A.action_values != nullptr)
							{
								win += A.q_rows[at * 2 + 0];
								draw += A.q_rows[at * 2 + 1];
							}
						}
						sum *= inv_s;
						free_cell = (A.boards[static_cast<size_t>(p) * HW + cell] == 0);
						if (free_cell && (A.flags & AGX_POSEVAL_MASK_FORBIDDEN) != 0)
							free_cell = ((A.features[row0 * HW + cell] >> 6) & 1u) == 0u;
						const int mark = listed[cell];
						if (!free_cell || mark == 0)
							sum = 0.0f;
						if (proven)
							sum = (mark == 2) ? share : 0.0f;
						free_cell = free_cell && mark != 0;
					}
					if (inside && A.action_values != nullptr)
					{
						float *q = A.action_values + (static_cast<size_t>(p) * HW + cell) * 2;
						q[0] = win * inv_s;
						q[1] = draw * inv_s;
					}
					prob[ch] = sum;
					legal |= free_cell ? (1u << ch) : 0u;
					if ((A.flags & AGX_POSEVAL_RENORMALISE) != 0 && !proven)
					{ // total += prob[cell], in cell order; + 0.0f changes nothing
						unsigned long long nonzero = __ballot(sum != 0.0f);
						while (nonzero != 0ull)
						{
							const int from = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(nonzero)) - 1);
							nonzero &= nonzero - 1ull;
							total += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sum), from));
						}
					}
				}
				if ((A.flags & AGX_POSEVAL_RENORMALISE) != 0 && !proven && total != 0.0f)
				{
					const float scale = 1.0f / total;
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
						prob[ch] *= scale;
				}
				if (A.policy != nullptr)
				{
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
						if (ch * 64 + lane < HW)
							A.policy[static_cast<size_t>(p) * HW + ch * 64 + lane] = prob[ch];
				}
				// the top_k rounds of k_combine_positions
				for (int k = 0; k < A.top_k; k++)
				{
					float best_p = -INFINITY;
					int at = 0x7FFFFFFF; // "no cell": loses against every cell
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
					{
						const float key = (prob[ch] != prob[ch]) ? -INFINITY : prob[ch];
						if (((legal >> ch) & 1u) != 0u && (key > best_p || at == 0x7FFFFFFF))
						{
							best_p = key;
							at = ch * 64 + lane;
						}
					}
#pragma unroll
					for (int off = 1; off < 64; off <<= 1)
					{
						const float ov = __shfl_xor(best_p, off, 64);
						const int oi = __shfl_xor(at, off, 64);
						if (oi != 0x7FFFFFFF && (at == 0x7FFFFFFF || ov > best_p || (ov == best_p && oi < at)))
						{
							best_p = ov;
							at = oi;
						}
					}
					const size_t slot = static_cast<size_t>(p) * A.top_k + k;
					if (at == 0x7FFFFFFF)
					{ // fewer legal cells than top_k
						if (lane == 0 && A.top_cells != nullptr)
							A.top_cells[slot] = -1;
						if (lane == 0 && A.top_probs != nullptr)
							A.top_probs[slot] = 0.0f;
						continue;
					}
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
						if (ch * 64 + lane == at)
						{ // the winner's own lane
							if (A.top_cells != nullptr)
								A.top_cells[slot] = at;
							if (A.top_probs != nullptr)
								A.top_probs[slot] = prob[ch];
							legal &= ~(1u << ch);
						}
				}
			}
		}
	}
}

struct AgxPositionEvaluator
{
		int rules = 0, n = 0, capacity = 0;
		int device = -1;
		std::mutex mutex;
		uint8_t *d_pattern = nullptr, *d_threat_packed = nullptr;
		uint16_t *d_list_spill = nullptr;
		uint64_t *d_snap_spill = nullptr;
		// workspace of evaluate: capacity x 8 rows
		uint32_t *d_features = nullptr;
		float *d_policy = nullptr, *d_value = nullptr, *d_q = nullptr;
		int *d_status = nullptr; // [capacity]
		// the waves of two launches share the spill areas and the workspace: a call on another stream than the previous one is ordered
		// behind it on the device (no host wait)
		hipEvent_t done = nullptr;
		hipStream_t last_stream = nullptr;
		bool launched = false;
};

namespace
{
	int popcount8(int mask)
	{
		int c = 0;
		for (int b = 0; b < 8; b++)
			c += (mask >> b) & 1;
		return c;
	}
	int order_behind_previous(AgxPositionEvaluator *pe, hipStream_t stream)
	{
		int current = -1;
		AGX_HIP_CHECK(hipGetDevice(&current));
		AGX_REQUIRE(current == pe->device, AGX_ERR_STATE, "agx_position_evaluator: the evaluator lives on device %d, the calling thread's current device is %d", pe->device,
				current);
		if (pe->launched && pe->last_stream != stream)
			AGX_HIP_CHECK(hipStreamWaitEvent(stream, pe->done, 0));
		return AGX_OK;
	}
	int mark_launched(AgxPositionEvaluator *pe, hipStream_t stream)
	{
		AGX_HIP_CHECK(hipEventRecord(pe->done, stream));
		pe->launched = true;
		pe->last_stream = stream;
		return AGX_OK;
	}
	int launch_encode(AgxPositionEvaluator *pe, int n, const uint8_t *d_boards, const uint8_t *d_signs, int mask, uint32_t *d_features, int *d_status, hipStream_t stream)
	{
		agx::EngineDev E;
		std::memset(&E, 0, sizeof(E));
		E.rules = pe->rules;
		E.n = pe->n;
		E.hw = pe->n * pe->n;
		E.t_pattern = pe->d_pattern;
		E.t_threat_packed = pe->d_threat_packed;
		agx::EncodeArgs A;
		A.boards = d_boards;
		A.signs = d_signs;
		A.n = n;
		A.mask = mask;
		A.S = popcount8(mask);
		A.features = d_features;
		A.status = d_status;
		A.list_spill = pe->d_list_spill;
		A.snap_spill = pe->d_snap_spill;
		if (d_status != nullptr)
			AGX_HIP_CHECK(hipMemsetAsync(d_status, 0, sizeof(int) * n, stream));
		const int waves = std::min(n * A.S, agx::PE_MAX_WAVES);
		if (pe->n == 15)
			hipLaunchKernelGGL(agx::k_encode_positions<15>, dim3(waves), dim3(64), 0, stream, E, A);
		else
			hipLaunchKernelGGL(agx::k_encode_positions<agx::MAXN>, dim3(waves), dim3(64), 0, stream, E, A);
		AGX_HIP_CHECK(hipGetLastError());
		return AGX_OK;
	}
	int launch_combine(AgxPositionEvaluator *pe, int n, const uint8_t *d_boards, int mask, int flags, int top_k, const uint32_t *d_features, const float *d_policy_rows,
			const float *d_value_rows, const float *d_q_rows, const int *d_status_in, const AgxPositionOutputs *out, hipStream_t stream,
			const agx::SolvedArgs *solved = nullptr)
	{
		agx::CombineArgs A;
		A.n = n;
		A.mask = mask;
		A.S = popcount8(mask);
		A.flags = flags;
		A.top_k = top_k;
		A.boards = d_boards;
		A.features = d_features;
		A.policy_rows = d_policy_rows;
		A.value_rows = d_value_rows;
		A.q_rows = d_q_rows;
		A.status_in = d_status_in;
		A.policy = out->policy;
		A.value = out->value;
		A.action_values = out->action_values;
		A.top_cells = out->top_cells;
		A.top_probs = out->top_probs;
		A.status = out->status;
		const int waves = std::min(n, agx::PE_MAX_WAVES);
		if (solved != nullptr)
		{
			if (pe->n == 15)
				hipLaunchKernelGGL(agx::k_combine_solved_positions<15>, dim3(waves), dim3(64), 0, stream, A, *solved);
			else
				hipLaunchKernelGGL(agx::k_combine_solved_positions<agx::MAXN>, dim3(waves), dim3(64), 0, stream, A, *solved);
		}
		else if (pe->n == 15)
			hipLaunchKernelGGL(agx::k_combine_positions<15>, dim3(waves), dim3(64), 0, stream, A);
		else
			hipLaunchKernelGGL(agx::k_combine_positions<agx::MAXN>, dim3(waves), dim3(64), 0, stream, A);
		AGX_HIP_CHECK(hipGetLastError());
		return AGX_OK;
	}
	/* what encode, combine and evaluate refuse alike */
	int check_batch(const AgxPositionEvaluator *pe, const char *who, int n, int mask)
	{
		AGX_REQUIRE(n >= 0 && n <= pe->capacity, AGX_ERR_INVALID, "%s: %d positions, the evaluator was created for %d", who, n, pe->capacity);
		AGX_REQUIRE(mask >= 1 && mask <= 0xFF, AGX_ERR_INVALID, "%s: symmetry mask 0x%x (bits 0..7, at least one)", who, mask);
		return AGX_OK;
	}
	int check_combine(const char *who, int mask, int flags, int top_k)
	{
		AGX_REQUIRE((flags & ~(AGX_POSEVAL_MASK_FORBIDDEN | AGX_POSEVAL_RENORMALISE)) == 0, AGX_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
		AGX_REQUIRE(top_k >= 0 && top_k <= agx::PE_MAX_TOP_K, AGX_ERR_INVALID, "%s: top_k %d (0..%d)", who, top_k, agx::PE_MAX_TOP_K);
		AGX_REQUIRE((flags & AGX_POSEVAL_MASK_FORBIDDEN) == 0 || (mask & 1) != 0, AGX_ERR_UNSUPPORTED,
				"%s: AGX_POSEVAL_MASK_FORBIDDEN reads the forbidden bits of the identity's row, which symmetry mask 0x%x leaves out", who, mask);
		return AGX_OK;
	}
}

extern "C" {

int agx_position_evaluator_create(int rules, int board_size, int capacity, AgxPositionEvaluator **out)
{
	AGX_REQUIRE(out != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_create: null argument");
	*out = nullptr;
	AGX_REQUIRE(rules >= 0 && rules <= AGX_CARO6, AGX_ERR_INVALID, "agx_position_evaluator_create: invalid rules %d", rules);
	AGX_REQUIRE(board_size == 15 || board_size == agx::MAXN, AGX_ERR_UNSUPPORTED, "agx_position_evaluator_create: boards of 15x15 and %dx%d only (got %d)", agx::MAXN,
			agx::MAXN, board_size);
	AGX_REQUIRE(capacity > 0 && capacity <= (1 << 20), AGX_ERR_INVALID, "agx_position_evaluator_create: capacity %d", capacity);
	AgxPositionEvaluator *pe = new AgxPositionEvaluator();
	pe->rules = rules;
	pe->n = board_size;
	pe->capacity = capacity;
	int st = AGX_OK;
	if (hipGetDevice(&pe->device) != hipSuccess)
	{
		agx::set_error("agx_position_evaluator_create: hipGetDevice failed");
		st = AGX_ERR_HIP;
	}
	agx::HostTables tables;
	agx::build_host_tables(rules, tables);
	std::vector<uint8_t> packed(4096); // cross type | circle type << 4 (dev_solver.hpp: threat_lookup)
	for (int i = 0; i < 4096; i++)
		packed[i] = static_cast<uint8_t>((tables.threat[2 * i] & 15u) | ((tables.threat[2 * i + 1] & 15u) << 4));
	const size_t hw = static_cast<size_t>(board_size) * board_size, rows = static_cast<size_t>(capacity) * 8;
	const auto alloc = [&](void **p, size_t bytes)
	{
		if (st == AGX_OK && hipMalloc(p, bytes) != hipSuccess)
		{
			agx::set_error("agx_position_evaluator_create: hipMalloc of %zu bytes failed", bytes);
			st = AGX_ERR_HIP;
		}
	};
	alloc(reinterpret_cast<void**>(&pe->d_pattern), tables.pattern.size());
	alloc(reinterpret_cast<void**>(&pe->d_threat_packed), packed.size());
	alloc(reinterpret_cast<void**>(&pe->d_list_spill), static_cast<size_t>(agx::PE_MAX_WAVES) * 20 * hw * sizeof(uint16_t));
	if (rules == AGX_RENJU)
		alloc(reinterpret_cast<void**>(&pe->d_snap_spill), static_cast<size_t>(agx::PE_MAX_WAVES) * agx::PE_SNAP_LEVELS * 64 * sizeof(uint64_t));
	alloc(reinterpret_cast<void**>(&pe->d_features), rows * hw * sizeof(uint32_t));
	alloc(reinterpret_cast<void**>(&pe->d_policy), rows * hw * sizeof(float));
	alloc(reinterpret_cast<void**>(&pe->d_value), rows * 3 * sizeof(float));
	alloc(reinterpret_cast<void**>(&pe->d_q), rows * hw * 2 * sizeof(float));
	alloc(reinterpret_cast<void**>(&pe->d_status), static_cast<size_t>(capacity) * sizeof(int));
	if (st == AGX_OK && (hipMemcpy(pe->d_pattern, tables.pattern.data(), tables.pattern.size(), hipMemcpyHostToDevice) != hipSuccess
			|| hipMemcpy(pe->d_threat_packed, packed.data(), packed.size(), hipMemcpyHostToDevice) != hipSuccess
			|| hipEventCreateWithFlags(&pe->done, hipEventDisableTiming) != hipSuccess))
	{
		agx::set_error("agx_position_evaluator_create: uploading the tables failed");
		st = AGX_ERR_HIP;
	}
	if (st != AGX_OK)
	{ // one way out for every failure: what was allocated is freed, *out stays null
		const std::string message = agx_last_error();
		agx_position_evaluator_destroy(pe);
		agx::set_error("%s", message.c_str());
		return st;
	}
	*out = pe;
	return AGX_OK;
}

int agx_position_evaluator_destroy(AgxPositionEvaluator *pe)
{
	if (pe == nullptr)
		return AGX_OK;
	if (pe->launched)
		(void) hipEventSynchronize(pe->done);
	for (void *p : { static_cast<void*>(pe->d_pattern), static_cast<void*>(pe->d_threat_packed), static_cast<void*>(pe->d_list_spill), static_cast<void*>(pe->d_snap_spill),
			static_cast<void*>(pe->d_features), static_cast<void*>(pe->d_policy), static_cast<void*>(pe->d_value), static_cast<void*>(pe->d_q), static_cast<void*>(pe->d_status) })
		if (p != nullptr)
			(void) hipFree(p);
	if (pe->done != nullptr)
		(void) hipEventDestroy(pe->done);
	delete pe;
	return AGX_OK;
}

int agx_position_evaluator_encode(AgxPositionEvaluator *pe, int n, const uint8_t *d_boards, const uint8_t *d_signs, int symmetry_mask, uint32_t *d_features, int *d_status,
		void *stream_)
{
	AGX_REQUIRE(pe != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_encode: null evaluator");
	int st = check_batch(pe, "agx_position_evaluator_encode", n, symmetry_mask);
	if (st != AGX_OK || n == 0)
		return st;
	AGX_REQUIRE(d_boards != nullptr && d_signs != nullptr && d_features != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_encode: null argument (only d_status is optional)");
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	std::lock_guard<std::mutex> lock(pe->mutex);
	st = order_behind_previous(pe, stream);
	if (st != AGX_OK)
		return st;
	st = launch_encode(pe, n, d_boards, d_signs, symmetry_mask, d_features, d_status, stream);
	const int marked = mark_launched(pe, stream); // (also behind a failure: the status memset may be enqueued)
	return (st != AGX_OK) ? st : marked;
}

int agx_position_evaluator_combine(AgxPositionEvaluator *pe, int n, const uint8_t *d_boards, int symmetry_mask, int flags, int top_k, const uint32_t *d_features,
		const float *d_policy_rows, const float *d_value_rows, const float *d_action_value_rows, const int *d_status_in, const AgxPositionOutputs *out, void *stream_)
{
	AGX_REQUIRE(pe != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_combine: null argument");
	int st = check_batch(pe, "agx_position_evaluator_combine", n, symmetry_mask);
	if (st == AGX_OK)
		st = check_combine("agx_position_evaluator_combine", symmetry_mask, flags, top_k);
	if (st != AGX_OK || n == 0)
		return st;
	AGX_REQUIRE(d_boards != nullptr && d_policy_rows != nullptr && d_value_rows != nullptr, AGX_ERR_INVALID,
			"agx_position_evaluator_combine: the boards, the policy rows and the value rows are needed");
	AGX_REQUIRE((flags & AGX_POSEVAL_MASK_FORBIDDEN) == 0 || d_features != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_combine: AGX_POSEVAL_MASK_FORBIDDEN needs the feature rows");
	AGX_REQUIRE(out->action_values == nullptr || d_action_value_rows != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_combine: action values asked for without their rows");
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	std::lock_guard<std::mutex> lock(pe->mutex);
	st = order_behind_previous(pe, stream);
	if (st != AGX_OK)
		return st;
	st = launch_combine(pe, n, d_boards, symmetry_mask, flags, top_k, d_features, d_policy_rows, d_value_rows, d_action_value_rows, d_status_in, out, stream);
	const int marked = mark_launched(pe, stream); // (also behind a failure: the status memset may be enqueued)
	return (st != AGX_OK) ? st : marked;
}

int agx_position_evaluator_evaluate(AgxPositionEvaluator *pe, AgxNet *net, int n, const uint8_t *d_boards, const uint8_t *d_signs, int symmetry_mask, int flags, int top_k,
		const AgxPositionOutputs *out, void *stream_)
{
	AGX_REQUIRE(pe != nullptr && net != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_evaluate: null argument");
	int st = check_batch(pe, "agx_position_evaluator_evaluate", n, symmetry_mask);
	if (st == AGX_OK)
		st = check_combine("agx_position_evaluator_evaluate", symmetry_mask, flags, top_k);
	if (st != AGX_OK)
		return st;
	AgxNetDesc desc;
	st = agx_net_description(net, &desc);
	if (st != AGX_OK)
		return st;
	AGX_REQUIRE(desc.rows == pe->n && desc.cols == pe->n, AGX_ERR_INVALID, "agx_position_evaluator_evaluate: the network's board is %dx%d, the evaluator's %dx%d", desc.rows,
			desc.cols, pe->n, pe->n);
	AGX_REQUIRE(out->action_values == nullptr || desc.action_values != 0, AGX_ERR_INVALID,
			"agx_position_evaluator_evaluate: action values asked of a network without that head ('pv')");
	if (n == 0)
		return AGX_OK;
	AGX_REQUIRE(d_boards != nullptr && d_signs != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_evaluate: null boards or signs");
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	const int rows = n * popcount8(symmetry_mask);
	const bool with_q = (out->action_values != nullptr);
	std::lock_guard<std::mutex> lock(pe->mutex);
	st = order_behind_previous(pe, stream);
	if (st != AGX_OK)
		return st;
	st = launch_encode(pe, n, d_boards, d_signs, symmetry_mask, pe->d_features, pe->d_status, stream);
	if (st == AGX_OK)
		st = with_q ? agx_nn_forward_pvq(net, pe->d_features, rows, pe->d_policy, pe->d_value, pe->d_q, stream) :
				agx_nn_forward(net, pe->d_features, rows, pe->d_policy, pe->d_value, stream);
	if (st == AGX_OK)
		st = launch_combine(pe, n, d_boards, symmetry_mask, flags, top_k, pe->d_features, pe->d_policy, pe->d_value, with_q ? pe->d_q : nullptr, pe->d_status, out, stream);
	// also behind a launch that failed half way: whatever was enqueued still uses the spill areas and the workspace
	const int marked = mark_launched(pe, stream);
	return (st != AGX_OK) ? st : marked;
}

int agx_position_evaluator_evaluate_solved(AgxPositionEvaluator *pe, AgxPositionSolver *solver, AgxNet *net, int n, const uint8_t *d_boards, const uint8_t *d_signs,
		int symmetry_mask, int flags, int top_k, const AgxPositionOutputs *out, const AgxSolvedPositions *solved_out, void *stream_)
{
	AGX_REQUIRE(pe != nullptr && solver != nullptr && net != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_evaluate_solved: null argument");
	int st = check_batch(pe, "agx_position_evaluator_evaluate_solved", n, symmetry_mask);
	if (st == AGX_OK)
		st = check_combine("agx_position_evaluator_evaluate_solved", symmetry_mask, flags, top_k);
	if (st != AGX_OK)
		return st;
	int solver_rules = 0, solver_n = 0, solver_capacity = 0;
	AgxSolvedPositions use;
	st = agx::position_solver_describe(solver, &solver_rules, &solver_n, &solver_capacity, &use);
	if (st != AGX_OK)
		return st;
	AGX_REQUIRE(solver_rules == pe->rules && solver_n == pe->n, AGX_ERR_INVALID,
			"agx_position_evaluator_evaluate_solved: the solver was created for rules %d on %dx%d, the evaluator for rules %d on %dx%d", solver_rules, solver_n, solver_n, pe->rules,
			pe->n, pe->n);
	AGX_REQUIRE(n <= solver_capacity, AGX_ERR_INVALID, "agx_position_evaluator_evaluate_solved: %d positions, the solver was created for %d", n, solver_capacity);
	AgxNetDesc desc;
	st = agx_net_description(net, &desc);
	if (st != AGX_OK)
		return st;
	AGX_REQUIRE(desc.rows == pe->n && desc.cols == pe->n, AGX_ERR_INVALID, "agx_position_evaluator_evaluate_solved: the network's board is %dx%d, the evaluator's %dx%d", desc.rows,
			desc.cols, pe->n, pe->n);
	AGX_REQUIRE(out->action_values == nullptr || desc.action_values != 0, AGX_ERR_INVALID,
			"agx_position_evaluator_evaluate_solved: action values asked of a network without that head ('pv')");
	if (n == 0)
		return AGX_OK;
	AGX_REQUIRE(d_boards != nullptr && d_signs != nullptr, AGX_ERR_INVALID, "agx_position_evaluator_evaluate_solved: null boards or signs");
	if (solved_out != nullptr)
	{ // the combine launch reads five of the solver's outputs: the caller's arrays where given, the solver's workspace otherwise
		use.score = (solved_out->score != nullptr) ? solved_out->score : use.score;
		use.n_actions = (solved_out->n_actions != nullptr) ? solved_out->n_actions : use.n_actions;
		use.moves = (solved_out->moves != nullptr) ? solved_out->moves : use.moves;
		use.move_scores = (solved_out->move_scores != nullptr) ? solved_out->move_scores : use.move_scores;
		use.status = (solved_out->status != nullptr) ? solved_out->status : use.status;
		use.flags = solved_out->flags;
		use.nodes = solved_out->nodes;
		use.value = solved_out->value;
	}
	agx::SolvedArgs V;
	V.score = use.score;
	V.n_actions = use.n_actions;
	V.moves = use.moves;
	V.move_scores = use.move_scores;
	V.status = use.status;
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	const int rows = n * popcount8(symmetry_mask);
	const bool with_q = (out->action_values != nullptr);
	std::lock_guard<std::mutex> lock(pe->mutex);
	st = order_behind_previous(pe, stream);
	if (st != AGX_OK)
		return st;
	st = agx_position_solver_solve(solver, n, d_boards, d_signs, &use, stream);
	if (st != AGX_OK)
		return st; // (the solver has marked its own launch; nothing of the evaluator's is enqueued)
	st = launch_encode(pe, n, d_boards, d_signs, symmetry_mask, pe->d_features, pe->d_status, stream);
	if (st == AGX_OK)
		st = with_q ? agx_nn_forward_pvq(net, pe->d_features, rows, pe->d_policy, pe->d_value, pe->d_q, stream) :
				agx_nn_forward(net, pe->d_features, rows, pe->d_policy, pe->d_value, stream);
	if (st == AGX_OK)
		st = launch_combine(pe, n, d_boards, symmetry_mask, flags, top_k, pe->d_features, pe->d_policy, pe->d_value, with_q ? pe->d_q : nullptr, pe->d_status, out, stream, &V);
	// also behind a launch that failed half way: whatever was enqueued still uses the workspaces of both
	const int marked = mark_launched(pe, stream);
	const int marked_solver = agx::position_solver_mark(solver, stream);
	return (st != AGX_OK) ? st : ((marked != AGX_OK) ? marked : marked_solver);
}

} /* extern "C" */
