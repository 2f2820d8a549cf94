/*
 * training_batch.hip — format-201 games to network tensors on the device: the consumer of the self-play record sink.
 *
 * What it replaces (all host code in the reference, one thread, sample by sample): the dataset reader behind
 * include/alphagomoku/dataset/torch_api.h (src/dataset/torch_api.cpp: load_dataset_fragment, get_dataset_size, get_tensor_shapes,
 * load_batch :185-279), i.e. per sample GameDataStorage::getSample (GameDataStorage.cpp:134-147: board from the game's moves),
 * SearchDataStorage_v201::storeTo (SearchDataStorage.cpp:375-409), apply_symmetry_in_place on the board and every per-cell array,
 * PatternCalculator::setBoard + NNInputFeatures::encode, and the targets.
 *
 * MI355X mapping: ONE WAVEFRONT PER SAMPLE, one launch per batch.  The games' bytes live in HBM (uploaded once per fragment); the host
 * resolves each (fragment, game, sample, augmentation) against its per-game index into a 32-byte record (where the sample and the
 * game's moves start, move count, outcome).  A wave
 *   1. scatters the first move_number moves into a board in LDS, and — 64 entries at a time, a wave prefix sum over their
 *      location_delta bytes — the index of every entry into a per-cell map in LDS (2 bytes per cell; the 6-byte entries themselves are
 *      decoded later, from L2, by the lane that owns the cell);
 *   2. gathers the board through symmetry_source() and runs the solver's own solver_set_board / solver_encode_features /
 *      solver_encode_forbidden on it (dev_solver.hpp: the pattern state in LDS, ~10 KB at 15x15), features into LDS;
 *   3. walks the cells of the TRANSFORMED board 64 at a time: entry through the map at the cell's source, dequantised as storeTo does,
 *      action values written, the policy addend kept in a register; the float32 policy sum is formed in cell order, one addend after
 *      the other — addends that are exactly +0 are skipped (x + 0 == x), the others are read lane by lane out of a ballot —, and the
 *      policy is written as addend * (1.0f / sum);
 *   4. expands the feature words into the 0 / 1 input planes (float32 or half), coalesced.
 * There is no engine behind the kernel: it gets an EngineDev that carries only what those three solver functions read (rules, board,
 * pattern and threat tables).  Of the solver's HBM spill areas it needs two per wave: the threat-list tails, and — renju, cross to
 * move, where the foul probes place and remove stones — 18 undo-snapshot levels (a probe nests at most 16 stones; sh.snap is biased
 * by the number of stones on the board so that level `stones` is slot 0).
 *
 * The build uses -ffp-contract=off and correctly rounded float32 division: every output is bit-identical to a float32 restatement
 * on the CPU (tests/training_batch_ref.py).
 *
 * Stage 3 has three compile-time variants (TARGETS_*): the two visit-count policies as they always were; the same plus
 * action_values_weight (visits / sum of visits, the weight of the reference's action-value loss); and the targets of SamplerValues
 * (dataset/Sampler.cpp:138-214, the reference's default sampler), which go through logf and expf: that policy is within 1 ulp-level
 * differences of a float32 restatement (tests/training_targets_ref.py), everything else is bit-identical to it.
 *
 * Differences from the reference, on purpose:
 *  - torch_api.cpp:274-277 never advances action_values_target inside its batch loop: it writes every sample's action values over
 *    sample 0's.  Here sample b's action values go to index b.
 *  - a sample whose policy addends are all zero (no visits, nothing proven) gives 0 * (1 / 0) = NaN there and here; the NaN's sign
 *    and payload are the hardware's.
 *  - BaseSampler's random choices (std::random_shuffle, randInt) are not part of this file: the caller names the samples.
 */
#include "agx_internal.hpp"
#include "dev_solver.hpp"
#include "sample_v201.hpp"
#include "symmetry.hpp"
#include "tables_host.hpp"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace agx
{
	namespace
	{
		struct BatchRecord
		{ // one sample of a batch, resolved by the host
				const uint8_t *blob;  // the fragment's games (device)
				uint32_t sample_off;  // the sample's 16-byte header inside the blob
				uint32_t moves_off;   // the game's first u16 move inside the blob
				int32_t n_moves;
				int32_t outcome;      // GameOutcome: 1 draw, 2 cross won, 3 circle won
				int32_t augmentation;
				int32_t pad;
		};
		static_assert(sizeof(BatchRecord) == 32, "batch record layout");

		constexpr int SNAP_LEVELS = 18; // renju_is_forbidden nests at most 16 stones (dev_solver.hpp: fstack)

		struct BatchArgs
		{
				const BatchRecord *records;
				int n;
				int fp16, visits_mode;
				void *input;            // may be null
				uint32_t *features;     // may be null
				float *policy, *value, *moves_left, *action_values;
				uint16_t *list_spill;   // [waves][20][SH::HW]
				uint64_t *snap_spill;   // [waves][SNAP_LEVELS][64], null unless renju
				int *error;             // pinned host word: batch index + 1 of a sample whose foul probe gave up (see the end of the sample loop)
				float *weight;          // action_values_weight; null in TARGETS_PLAIN, may be null in TARGETS_VALUES
		};

		/* the compile-time variants of stage 3.  TARGETS_PLAIN is the kernel as it was before the other two existed: the two visit-count
		 * policies, no weight output.  A launch picks the variant from the flags and the weight pointer, so a call that asks for neither
		 * runs the code it always ran. */
		enum
		{
			TARGETS_PLAIN = 0,    // visit-count policy (torch_api.cpp / SamplerVisits)
			TARGETS_WEIGHTED = 1, // ... plus action_values_weight
			TARGETS_VALUES = 2    // SamplerValues (Sampler.cpp:138-214), action_values_weight when its pointer is set
		};

		__device__ __forceinline__ uint32_t load_u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8); }
		__device__ __forceinline__ uint32_t load_u32(const uint8_t *p) { return load_u16(p) | (load_u16(p + 2) << 16); }
		/* inclusive prefix sum over the 64 lanes */
		__device__ __forceinline__ int wave_scan64_add(int v, int lane)
		{
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
			{
				const int t = __shfl_up(v, off, 64);
				v += (lane >= off) ? t : 0;
			}
			return v;
		}

		__device__ __forceinline__ int wave_sum_int(int v)
		{
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
				v += __shfl_xor(v, off, 64);
			return v;
		}
		__device__ __forceinline__ float wave_max_float(float v)
		{
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
				v = fmaxf(v, __shfl_xor(v, off, 64));
			return v;
		}
		/* the float of lane `src` (the same in every lane) */
		__device__ __forceinline__ float lane_float(float v, int src)
		{
			return v201::bits_float(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v201::float_bits(v)), src)));
		}
		/* Value::getExpectation */
		__device__ __forceinline__ float expectation(float win, float draw) { return win + 0.5f * draw; }
		/* the count both samplers leave in TrainingDataPack::visit_count (Sampler.cpp:112,161): a proven move has at least one visit */
		__device__ __forceinline__ int fixed_up_visits(bool empty, uint32_t score, int visits)
		{
			return (empty && dev::s_proven(score)) ? max(1, visits) : visits;
		}
		/* fill_action_values_mask (SupervisedLearning.cpp:55-61): count * (1 / sum of the counts); all zero when the sum is */
		template<int CHUNKS>
		__device__ __forceinline__ void write_weights(float *out, const int (&counts)[CHUNKS], int hw, int lane)
		{
			int total = 0;
#pragma unroll
			for (int ch = 0; ch < CHUNKS; ch++)
				total += counts[ch];
			total = __builtin_amdgcn_readfirstlane(wave_sum_int(total));
			const float inv = (total == 0) ? 0.0f : 1.0f / static_cast<float>(total);
#pragma unroll
			for (int ch = 0; ch < CHUNKS; ch++)
			{
				const int cell = ch * 64 + lane;
				if (cell < hw)
					out[cell] = (total == 0) ? 0.0f : static_cast<float>(counts[ch]) * inv;
			}
		}

		/* Stage 3 of TARGETS_VALUES: SamplerValues::prepare_training_data (Sampler.cpp:138-214) on sample b, in float32, one operation after
		 * the other.  Every sequential float sum of the reference is formed one addend after the other (a ballot of the lanes that
		 * contribute, then readlane in lane order), over the cells of the TRANSFORMED board where the reference, which samples before it
		 * applies the symmetry, runs over the untransformed one: a difference of float32 rounding only.  The sums of storeTo run in entry
		 * order, as there. */
		template<int N>
		struct ValuesTemp
		{ // per cell of the transformed board, between the loops of values_targets (LDS of the TARGETS_VALUES variant only)
				float prior[N * N];
				float q[N * N];      // the cell's Q, then its logit, then its exponential
				int count[N * N];    // fixed_up_visits
				uint8_t flag[N * N]; // 1 empty, 2 visited or proven
		};
		template<int N>
		__device__ __forceinline__ void values_targets(const BatchArgs &A, ValuesTemp<N> &T, int b, const uint8_t *sample, float value_scale, float visit_scale, int count,
				int s, int n, int hw, const uint8_t *board, const uint16_t *entry_of, int lane)
		{
			using namespace dev;
			const float policy_scale = v201::ScaleFormat::decode(load_u16(sample + 2));
			const uint32_t minimax_score = load_u16(sample + 6);

			// minimax value: storeTo's running sums over the entries (SearchDataStorage.cpp:377-406)
			float win_rate = 0.0f, draw_rate = 0.0f;
			int sum_visits = 0;
			for (int base = 0; base < count; base += 64)
			{
				const int k = base + lane;
				float v = 0.0f, wv = 0.0f, dv = 0.0f;
				if (k < count)
				{
					const uint8_t *q = sample + v201::HEADER_BYTES + v201::ENTRY_BYTES * k;
					v = v201::VisitFormat::decode(q[1]) * visit_scale + 0.5f;
					float w = v201::PriorFormat::decode(q[4]) * value_scale;
					float d = v201::PriorFormat::decode(q[5]) * value_scale;
					const float total = w + d; // get_valid_value
					if (total > 1.0f)
					{
						w /= total;
						d /= total;
					}
					wv = w * v;
					dv = d * v;
				}
				const int here = __builtin_amdgcn_readfirstlane(min(64, count - base));
				for (int j = 0; j < here; j++)
				{
					const int src = __builtin_amdgcn_readfirstlane(j);
					sum_visits = static_cast<int>(static_cast<float>(sum_visits) + lane_float(v, src)); // int sum_visits += float visits
					win_rate += lane_float(wv, src);
					draw_rate += lane_float(dv, src);
				}
			}
			float mm_win, mm_draw;
			if (sum_visits == 0)
				s_to_value(minimax_score, mm_win, mm_draw);
			else
			{
				mm_win = win_rate / static_cast<float>(sum_visits);
				mm_draw = draw_rate / static_cast<float>(sum_visits);
				const float total = mm_win + mm_draw;
				if (total > 1.0f)
				{
					mm_win /= total;
					mm_draw /= total;
				}
			}
			if (s_proven(minimax_score)) // get_value(minimax_value, minimax_score)
				s_to_value(minimax_score, mm_win, mm_draw);
			const float minimax_V = expectation(mm_win, mm_draw);

			// first loop (:152-165): the cells that have a visit or a proven score.  What the later loops need of a cell waits in LDS; a lane
			// reads back only what it wrote itself (cells lane, lane + 64, ...), so nothing has to be synchronised
			float sum_PxQ = 0.0f, sum_P = 0.0f;
			int unvisited = 0, count_sum = 0;
			for (int base = 0; base < hw; base += 64)
			{
				const int cell = base + lane;
				const bool inside = cell < hw;
				int visits = 0;
				float win = 0.0f, draw = 0.0f, p = 0.0f;
				uint32_t score = s_unknown(0); // SearchDataPack::clear
				if (inside)
				{
					int sr, sc;
					symmetry_source(s, n, cell / n, cell % n, sr, sc);
					const int e = entry_of[sr * n + sc];
					if (e != 0)
					{ // storeTo
						const uint8_t *q = sample + v201::HEADER_BYTES + v201::ENTRY_BYTES * (e - 1);
						visits = static_cast<int>(v201::VisitFormat::decode(q[1]) * visit_scale + 0.5f);
						p = v201::PriorFormat::decode(q[2]) * policy_scale;
						win = v201::PriorFormat::decode(q[4]) * value_scale;
						draw = v201::PriorFormat::decode(q[5]) * value_scale;
						const float total = win + draw;
						if (total > 1.0f)
						{
							win /= total;
							draw /= total;
						}
						score = v201::score_from_code(q[3]);
					}
				}
				const bool empty = inside && board[cell] == 0;
				const bool counted = empty && (visits > 0 || s_proven(score));
				const float distance = static_cast<float>(s_distance(score));
				float Q;
				switch (s_pv(score))
				{ // the Q of the second loop (:180-195); the raw action value where nothing is proven
					case 0: Q = -1.0f / (1.0f + distance); break;
					case 1: Q = 0.5f; break; // Value::draw().getExpectation()
					case 3: Q = 1.0f + 2.0f / (1.0f + distance); break;
					default: Q = expectation(win, draw); break;
				}
				if (s_proven(score)) // get_value(action_value, score)
					s_to_value(score, win, draw);
				const int fixed = inside ? fixed_up_visits(empty, score, visits) : 0;
				count_sum += fixed;
				if (inside)
				{
					T.prior[cell] = p;
					T.q[cell] = Q;
					T.count[cell] = fixed;
					T.flag[cell] = static_cast<uint8_t>((empty ? 1 : 0) | (counted ? 2 : 0));
					// the cleared pack (0, 0) wherever the second loop writes nothing
					const float w = counted ? win : 0.0f, d = counted ? draw : 0.0f;
					float *av = A.action_values + (static_cast<size_t>(b) * hw + cell) * 3;
					av[0] = w;
					av[1] = d;
					av[2] = 1.0f - (w + d); // Value::loss_rate
				}
				const float pxq = p * expectation(win, draw);
				u64 todo = __ballot(counted);
				unvisited += __popcll(__ballot(empty && !counted));
				while (todo != 0ull)
				{
					const int src = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(todo)) - 1);
					todo &= todo - 1ull;
					sum_PxQ += lane_float(pxq, src);
					sum_P += lane_float(p, src);
				}
			}
			sum_PxQ = sum_P * sum_PxQ + (1.0f - sum_P) * minimax_V;

			// second loop (:170-201): the logits and their maximum.  Without an unvisited cell the default P is never used (and not formed)
			const float spread = (unvisited > 0) ? (1.0f - sum_P) / static_cast<float>(unvisited) : 0.0f;
			const float default_P = (0.0f < spread) ? spread : 0.0f; // std::max(0.0f, ...)
			float max_value = -FLT_MAX;
			for (int cell = lane; cell < hw; cell += 64)
				if (T.flag[cell] & 1)
				{
					const bool counted = (T.flag[cell] & 2) != 0;
					const float logit = 50.0f * (counted ? T.q[cell] : sum_PxQ) + logf(FLT_EPSILON + (counted ? T.prior[cell] : default_P));
					T.q[cell] = logit;
					max_value = fmaxf(max_value, logit);
				}
			max_value = wave_max_float(max_value);

			// normalisation (:203-213)
			float sum_policy = 0.0f;
			for (int base = 0; base < hw; base += 64)
			{
				const int cell = base + lane;
				const bool empty = cell < hw && (T.flag[cell] & 1) != 0;
				float e = 0.0f;
				if (empty)
				{
					const float shifted = T.q[cell] - max_value;
					e = expf((-20.0f < shifted) ? shifted : -20.0f); // std::max(-20.0f, ...)
					T.q[cell] = e;
				}
				u64 todo = __ballot(empty);
				while (todo != 0ull)
				{
					const int src = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(todo)) - 1);
					todo &= todo - 1ull;
					sum_policy += lane_float(e, src);
				}
			}
			for (int cell = lane; cell < hw; cell += 64)
				A.policy[static_cast<size_t>(b) * hw + cell] = (T.flag[cell] & 1) ? T.q[cell] / sum_policy : 0.0f;
			if (A.weight != nullptr)
			{ // fill_action_values_mask, as write_weights forms it
				const int total = __builtin_amdgcn_readfirstlane(wave_sum_int(count_sum));
				const float inv = (total == 0) ? 0.0f : 1.0f / static_cast<float>(total);
				for (int cell = lane; cell < hw; cell += 64)
					A.weight[static_cast<size_t>(b) * hw + cell] = (total == 0) ? 0.0f : static_cast<float>(T.count[cell]) * inv;
			}
		}

		template<int N, int TARGETS>
		__global__ __launch_bounds__(64) void k_training_batch(EngineDev E, BatchArgs A)
		{
			using namespace dev;
			typedef SolverSharedT<N> SH;
			constexpr int CHUNKS = (N * N + 63) / 64;
			__shared__ SH sh;
			__shared__ uint8_t src_board[N * N];  // the position as the game's moves give it
			__shared__ uint8_t board[N * N];      // ... under the sample's symmetry
			__shared__ uint16_t entry_of[N * N];  // entry index + 1 per cell of the UNtransformed board, 0 = no entry
			__shared__ uint32_t feat[N * N];
			const int lane = threadIdx.x;
			const int n = E.n, hw = E.hw;
			solver_load_threat_table(sh, E, lane);

			for (int b = blockIdx.x; b < A.n; b += gridDim.x)
			{
				const BatchRecord rec = A.records[b];
				const uint8_t *sample = rec.blob + rec.sample_off;
				const uint8_t *moves = rec.blob + rec.moves_off;
				const float value_scale = v201::ScaleFormat::decode(load_u16(sample + 0));
				const float visit_scale = v201::ScaleFormat::decode(load_u16(sample + 4));
				const int move_number = static_cast<int>(load_u16(sample + 8));
				const int count = static_cast<int>(load_u32(sample + 12));
				const int sign_to_move = static_cast<int>(load_u16(moves + 2 * move_number) & 3u);
				const int s = rec.augmentation;

				// ---- 1. board and entry map, in the game's own orientation ----
				for (int i = lane; i < hw; i += 64)
				{
					src_board[i] = 0;
					entry_of[i] = 0;
				}
				wave_sync();
				for (int k = lane; k < move_number; k += 64)
				{ // Board::putMove of moves 0 .. move_number - 1 (the host has checked that they lie on the board)
					const uint32_t mv = load_u16(moves + 2 * k);
					const int cell = static_cast<int>((mv >> 2) & 127u) * n + static_cast<int>((mv >> 9) & 127u);
					if (cell < hw)
						src_board[cell] = static_cast<uint8_t>(mv & 3u);
				}
				int carry = 0; // storeTo's current_idx after the entries before this chunk
				for (int base = 0; base < count; base += 64)
				{
					const int k = base + lane;
					const int delta = (k < count) ? sample[v201::HEADER_BYTES + v201::ENTRY_BYTES * k] : 0;
					const int at = carry + wave_scan64_add(delta, lane);
					if (k < count && at < hw)
						entry_of[at] = static_cast<uint16_t>(k + 1);
					carry = __shfl(at, 63, 64);
				}
				wave_sync();

				// ---- 2. the transformed board, its pattern state and its features ----
				for (int i = lane; i < hw; i += 64)
				{
					int sr, sc;
					symmetry_source(s, n, i / n, i % n, sr, sc);
					board[i] = src_board[sr * n + sc];
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
					const uintptr_t area = reinterpret_cast<uintptr_t>(A.snap_spill) + static_cast<uintptr_t>(blockIdx.x) * SNAP_LEVELS * 64 * sizeof(u64);
					sh.snap = (A.snap_spill == nullptr) ? nullptr : reinterpret_cast<u64*>(area - static_cast<uintptr_t>(sh.depth) * 64 * sizeof(u64));
				}
				wave_sync();
				solver_encode_features(sh, E, feat, lane);
				wave_sync();
				solver_encode_forbidden(sh, E, feat, lane); // renju, cross to move: bit 6 on the fouls (wave_sync inside)
				wave_sync();

				// ---- 3. targets, cell by cell of the transformed board ----
				if constexpr (TARGETS == TARGETS_VALUES)
				{
					__shared__ ValuesTemp<N> temp;
					values_targets<N>(A, temp, b, sample, value_scale, visit_scale, count, s, n, hw, board, entry_of, lane);
				}
				else
				{
					float addend[CHUNKS];
					int counts[CHUNKS]; // (TARGETS_WEIGHTED only)
					float sum = 0.0f;
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
					{
						const int cell = ch * 64 + lane;
						const bool inside = cell < hw;
						int visits = 0;
						float win = 0.0f, draw = 0.0f;
						uint32_t score = s_unknown(0); // SearchDataPack::clear
						if (inside)
						{
							int sr, sc;
							symmetry_source(s, n, cell / n, cell % n, sr, sc);
							const int e = entry_of[sr * n + sc];
							if (e != 0)
							{ // storeTo (SearchDataStorage.cpp:375-409)
								const uint8_t *q = sample + v201::HEADER_BYTES + v201::ENTRY_BYTES * (e - 1);
								visits = static_cast<int>(v201::VisitFormat::decode(q[1]) * visit_scale + 0.5f);
								win = v201::PriorFormat::decode(q[4]) * value_scale;
								draw = v201::PriorFormat::decode(q[5]) * value_scale;
								const float total = win + draw; // get_valid_value (:52-61)
								if (total > 1.0f)
								{
									win /= total;
									draw /= total;
								}
								score = v201::score_from_code(q[3]);
							}
						}
						if constexpr (TARGETS == TARGETS_WEIGHTED)
							counts[ch] = inside ? fixed_up_visits(board[cell] == 0, score, visits) : 0;
						if (s_proven(score))
							s_to_value(score, win, draw);
						float p;
						switch (s_pv(score))
						{ // torch_api.cpp:252-267 / Sampler.cpp:117-130
							case 0: p = 1.0e-6f; break;
							case 1: p = static_cast<float>(A.visits_mode ? visits : max(1, visits)); break;
							case 3: p = 1.0e+6f; break;
							default: p = static_cast<float>(visits); break;
						}
						p = inside ? p : 0.0f;
						addend[ch] = p;
						if (inside)
						{
							float *av = A.action_values + (static_cast<size_t>(b) * hw + cell) * 3;
							av[0] = win;
							av[1] = draw;
							av[2] = 1.0f - (win + draw); // Value::loss_rate
						}
						u64 nonzero = __ballot(p != 0.0f); // policy_sum += policy_target[i], in cell order; + 0.0f changes nothing
						while (nonzero != 0ull)
						{
							const int src = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(nonzero)) - 1);
							nonzero &= nonzero - 1ull;
							sum += v201::bits_float(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v201::float_bits(p)), src)));
						}
					}
					const float scale = 1.0f / sum;
#pragma unroll
					for (int ch = 0; ch < CHUNKS; ch++)
					{
						const int cell = ch * 64 + lane;
						if (cell < hw)
							A.policy[static_cast<size_t>(b) * hw + cell] = addend[ch] * scale;
					}
					if constexpr (TARGETS == TARGETS_WEIGHTED)
						write_weights<CHUNKS>(A.weight + static_cast<size_t>(b) * hw, counts, hw, lane);
				}
				if (lane == 0)
				{ // convertOutcome(game_outcome, sign to move) (Value.cpp:16-29), moves_left (GameDataStorage.cpp:141)
					const bool won = (rec.outcome == 2 && sign_to_move == 1) || (rec.outcome == 3 && sign_to_move == 2);
					const bool drawn = (rec.outcome != 2 && rec.outcome != 3);
					const float w = won ? 1.0f : 0.0f, d = drawn ? 1.0f : 0.0f;
					A.value[static_cast<size_t>(b) * 3 + 0] = w;
					A.value[static_cast<size_t>(b) * 3 + 1] = d;
					A.value[static_cast<size_t>(b) * 3 + 2] = 1.0f - (w + d);
					A.moves_left[b] = static_cast<float>(rec.n_moves - move_number);
				}

				// ---- 4. the network input ----
				if (A.features != nullptr)
					for (int i = lane; i < hw; i += 64)
						A.features[static_cast<size_t>(b) * hw + i] = feat[i];
				if (A.input != nullptr)
				{
					const int planes = hw * 32;
					if (A.fp16)
					{
						__half *out = static_cast<__half*>(A.input) + static_cast<size_t>(b) * planes;
						for (int i = lane; i < planes; i += 64)
							out[i] = __ushort_as_half(((feat[i >> 5] >> (i & 31)) & 1u) ? static_cast<unsigned short>(0x3C00u) : static_cast<unsigned short>(0u));
					}
					else
					{
						float *out = static_cast<float*>(A.input) + static_cast<size_t>(b) * planes;
						for (int i = lane; i < planes; i += 64)
							out[i] = ((feat[i >> 5] >> (i & 31)) & 1u) ? 1.0f : 0.0f;
					}
				}
				// renju_is_forbidden gives up (ERR_FRAMES, its probe stones left on the board) when 3x3 forks nest 16 deep: the sample's features
				// are then not to be trusted.  The host reports it: the host-pointer form at once, the device form at the next call.
				if (lane == 0 && sh.error != 0)
					*A.error = b + 1;
				wave_sync(); // the next sample reuses the LDS arrays
			}
		}

		/* The positions of the samples as the position searcher takes them (agx_dataset_positions): stage 1 of k_training_batch without
		 * the entry map — one wavefront per sample scatters the game's first move_number moves into a board in LDS and writes it out
		 * whole, and the colour of move move_number as the side to move (the rule of k_training_batch; the host has checked that the
		 * moves lie on the board and that move_number is below the game's move count). */
		__global__ __launch_bounds__(64) void k_dataset_positions(const BatchRecord *records, int count, int n, int hw, uint8_t *boards, uint8_t *signs)
		{
			using namespace dev;
			__shared__ uint8_t board[MAXHW];
			const int lane = threadIdx.x;
			for (int b = blockIdx.x; b < count; b += gridDim.x)
			{
				const BatchRecord rec = records[b];
				const uint8_t *sample = rec.blob + rec.sample_off;
				const uint8_t *moves = rec.blob + rec.moves_off;
				const int move_number = min(static_cast<int>(load_u16(sample + 8)), rec.n_moves - 1);
				for (int i = lane; i < hw; i += 64)
					board[i] = 0;
				wave_sync();
				for (int k = lane; k < move_number; k += 64)
				{ // Board::putMove of moves 0 .. move_number - 1
					const uint32_t mv = load_u16(moves + 2 * k);
					const int cell = static_cast<int>((mv >> 2) & 127u) * n + static_cast<int>((mv >> 9) & 127u);
					if (cell < hw)
						board[cell] = static_cast<uint8_t>(mv & 3u);
				}
				wave_sync();
				for (int i = lane; i < hw; i += 64)
					boards[static_cast<size_t>(b) * hw + i] = board[i];
				if (lane == 0)
					signs[b] = static_cast<uint8_t>(load_u16(moves + 2 * move_number) & 3u);
				wave_sync(); // the next sample reuses the board
			}
		}
	}
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */
namespace
{
	using agx::BatchRecord;
	using agx::BatchArgs;

	constexpr int MAX_WAVES = 2048; // workgroups of a launch (one wave each); larger batches stride.  Sizes the per-wave spill areas
	constexpr int RING = 4;         // batches whose records may be in flight before a call waits for the oldest one's

	struct GameIndex
	{
			std::vector<uint32_t> sample_off; // header of every sample, inside the fragment's blob
			uint32_t moves_off = 0;
			int n_moves = 0, outcome = 0;
	};
	struct Fragment
	{
			std::vector<uint8_t> blob; // the games' GameDataStorage bytes, one after the other
			std::vector<GameIndex> games;
			AgxGameBufferStats stats { };
			uint8_t *d_blob = nullptr; // uploaded at the first batch that uses the fragment
	};
	struct RecordSlot
	{
			BatchRecord *h = nullptr, *d = nullptr;
			int capacity = 0;
			hipEvent_t done = nullptr; // recorded behind the launch that read the slot
			bool in_flight = false;
	};

	/* appends one game to the fragment after checking everything the kernel relies on; returns an empty string or what is wrong */
	std::string index_game(Fragment &f, const uint8_t *g, size_t size, int rows, int cols)
	{
		using namespace agx::v201;
		const int hw = rows * cols;
		if (size < 20)
			return "is truncated (" + std::to_string(size) + " bytes)";
		if (f.blob.size() + size > 0xFFFFFFF0ull)
			return "does not fit: a fragment holds less than 4 GiB";
		const size_t base = f.blob.size();
		GameIndex gi;
		uint32_t n_samples = 0, n_moves = 0;
		std::memcpy(&n_samples, g, 4);
		if (n_samples == 0)
			return "holds no samples (GameGenerator only hands over games that do)";
		size_t at = 4;
		std::vector<int> move_numbers;
		for (uint32_t k = 0; k < n_samples; k++)
		{
			if (size - at < static_cast<size_t>(HEADER_BYTES))
				return "is truncated in sample " + std::to_string(k);
			uint16_t move_number;
			uint32_t count;
			std::memcpy(&move_number, g + at + 8, 2);
			std::memcpy(&count, g + at + 12, 4);
			if (count > static_cast<uint32_t>(hw) || size - at - HEADER_BYTES < static_cast<size_t>(ENTRY_BYTES) * count)
				return "is truncated in sample " + std::to_string(k) + " (" + std::to_string(count) + " entries)";
			int cell = 0;
			for (uint32_t e = 0; e < count; e++)
			{
				const int delta = g[at + HEADER_BYTES + ENTRY_BYTES * e];
				cell += delta;
				if (cell >= hw || (e > 0 && delta == 0))
					return "has an entry outside the board or twice on one cell in sample " + std::to_string(k);
			}
			gi.sample_off.push_back(static_cast<uint32_t>(base + at));
			move_numbers.push_back(move_number);
			at += HEADER_BYTES + static_cast<size_t>(ENTRY_BYTES) * count;
		}
		if (size - at < 4)
			return "is truncated before its moves";
		std::memcpy(&n_moves, g + at, 4);
		at += 4;
		if (n_moves > static_cast<uint32_t>(hw) || size - at != 2 * static_cast<size_t>(n_moves) + 12)
			return "has " + std::to_string(size) + " bytes where its layout needs " + std::to_string(at + 2 * static_cast<size_t>(n_moves) + 12);
		gi.moves_off = static_cast<uint32_t>(base + at);
		gi.n_moves = static_cast<int>(n_moves);
		std::vector<uint8_t> taken(hw, 0);
		for (uint32_t k = 0; k < n_moves; k++)
		{
			uint16_t mv;
			std::memcpy(&mv, g + at + 2 * k, 2);
			const int sign = mv & 3, r = (mv >> 2) & 127, c = (mv >> 9) & 127;
			if ((sign != 1 && sign != 2) || r >= rows || c >= cols || taken[r * cols + c])
				return "has a move outside the board, without a colour or on a taken cell (move " + std::to_string(k) + ")";
			taken[r * cols + c] = 1;
		}
		at += 2 * static_cast<size_t>(n_moves);
		int tail[3];
		std::memcpy(tail, g + at, 12);
		if (tail[1] != rows || tail[2] != cols)
			return "is " + std::to_string(tail[1]) + "x" + std::to_string(tail[2]) + ", the dataset " + std::to_string(rows) + "x" + std::to_string(cols);
		if (tail[0] < 0 || tail[0] > 3)
			return "has no valid outcome";
		for (size_t k = 0; k < move_numbers.size(); k++) // GameDataStorage::getSample: played_moves.at(move_number)
			if (move_numbers[k] >= gi.n_moves)
				return "has sample " + std::to_string(k) + " at move " + std::to_string(move_numbers[k]) + " of " + std::to_string(gi.n_moves);
		gi.outcome = tail[0];
		f.blob.insert(f.blob.end(), g, g + size);
		f.stats.games++;
		f.stats.samples += static_cast<int>(n_samples);
		f.stats.game_length += gi.n_moves;
		f.stats.cross_win += (gi.outcome == 2);
		f.stats.draws += (gi.outcome == 1);
		f.stats.circle_win += (gi.outcome == 3);
		f.games.push_back(std::move(gi));
		return std::string();
	}
}

struct AgxDataset
{
		int rules = 0, rows = 0, cols = 0;
		mutable std::mutex mutex;
		std::mutex host_mutex; // held over a whole agx_dataset_load_batch_host: the calls share one staging area and one stream
		std::map<int, std::unique_ptr<Fragment>> fragments;
		// device side, created at the first load_batch (every piece on its own: a call that fails half way leaves what it got to the next
		// call and to destroy)
		bool device_ready = false;
		bool tables_uploaded = false;
		int device = -1;        // the HIP device of the first load_batch: everything the dataset owns lives there
		int *h_error = nullptr; // pinned, written by the kernel: batch index + 1 of a sample whose renju foul probe gave up
		uint8_t *d_pattern = nullptr, *d_threat_packed = nullptr;
		uint16_t *d_list_spill = nullptr;
		uint64_t *d_snap_spill = nullptr;
		RecordSlot slots[RING];
		std::vector<BatchRecord*> retired_host, retired_device; // record buffers a larger batch has replaced: freed with the dataset
		int next_slot = 0;
		bool launched = false;
		hipStream_t last_stream = nullptr;
		hipEvent_t last_done = nullptr; // the slot event behind the latest launch
		// staging of the host-pointer form
		hipStream_t host_stream = nullptr;
		void *d_stage = nullptr;
		size_t stage_bytes = 0;
};

namespace
{
	int tile_hw(const AgxDataset *d) { return (d->rows <= 15) ? 225 : agx::MAXHW; } // SolverSharedT<N>::HW of the kernel that serves this board

	int wait_for_batches(AgxDataset *d)
	{ // every launch that may still read a fragment or a record slot
		for (RecordSlot &s : d->slots)
			if (s.in_flight)
			{
				AGX_HIP_CHECK(hipEventSynchronize(s.done));
				s.in_flight = false;
			}
		return AGX_OK;
	}
	int prepare_device(AgxDataset *d)
	{
		int current = -1;
		AGX_HIP_CHECK(hipGetDevice(&current));
		if (d->device < 0)
			d->device = current;
		AGX_REQUIRE(current == d->device, AGX_ERR_STATE, "agx_dataset_load_batch: the dataset lives on device %d, the calling thread's current device is %d", d->device,
				current);
		if (d->device_ready)
			return AGX_OK;
		if (!d->tables_uploaded)
		{
			agx::HostTables tables;
			agx::build_host_tables(d->rules, tables);
			std::vector<uint8_t> packed(4096); // cross type | circle type << 4 (dev_solver.hpp: threat_lookup)
			for (int i = 0; i < 4096; i++)
				packed[i] = static_cast<uint8_t>((tables.threat[2 * i] & 15u) | ((tables.threat[2 * i + 1] & 15u) << 4));
			if (d->d_pattern == nullptr)
				AGX_HIP_CHECK(hipMalloc(&d->d_pattern, tables.pattern.size()));
			AGX_HIP_CHECK(hipMemcpy(d->d_pattern, tables.pattern.data(), tables.pattern.size(), hipMemcpyHostToDevice));
			if (d->d_threat_packed == nullptr)
				AGX_HIP_CHECK(hipMalloc(&d->d_threat_packed, packed.size()));
			AGX_HIP_CHECK(hipMemcpy(d->d_threat_packed, packed.data(), packed.size(), hipMemcpyHostToDevice));
			d->tables_uploaded = true;
		}
		if (d->d_list_spill == nullptr)
			AGX_HIP_CHECK(hipMalloc(&d->d_list_spill, static_cast<size_t>(MAX_WAVES) * 20 * tile_hw(d) * sizeof(uint16_t)));
		if (d->rules == AGX_RENJU && d->d_snap_spill == nullptr)
			AGX_HIP_CHECK(hipMalloc(&d->d_snap_spill, static_cast<size_t>(MAX_WAVES) * agx::SNAP_LEVELS * 64 * sizeof(uint64_t)));
		if (d->h_error == nullptr)
		{
			AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&d->h_error), sizeof(int), hipHostMallocDefault));
			*d->h_error = 0;
		}
		for (RecordSlot &s : d->slots)
			if (s.done == nullptr)
				AGX_HIP_CHECK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
		d->device_ready = true;
		return AGX_OK;
	}
	int resolve(const AgxDataset *d, int n, const AgxDatasetSample *samples, std::vector<Fragment*> *used)
	{ // every index of the batch, before anything touches the device
		for (int b = 0; b < n; b++)
		{
			const AgxDatasetSample &s = samples[b];
			auto it = d->fragments.find(s.fragment);
			AGX_REQUIRE(it != d->fragments.end(), AGX_ERR_INVALID, "agx_dataset_load_batch: sample %d names fragment %d, which is not loaded", b, s.fragment);
			const Fragment &f = *it->second;
			AGX_REQUIRE(s.game >= 0 && s.game < static_cast<int>(f.games.size()), AGX_ERR_INVALID, "agx_dataset_load_batch: sample %d names game %d of fragment %d (%zu games)", b,
					s.game, s.fragment, f.games.size());
			AGX_REQUIRE(s.sample >= 0 && s.sample < static_cast<int>(f.games[s.game].sample_off.size()), AGX_ERR_INVALID,
					"agx_dataset_load_batch: sample %d names sample %d of a game with %zu", b, s.sample, f.games[s.game].sample_off.size());
			AGX_REQUIRE(s.augmentation >= 0 && s.augmentation < 8, AGX_ERR_INVALID, "agx_dataset_load_batch: sample %d names augmentation %d (0..7)", b, s.augmentation);
			if (used != nullptr && std::find(used->begin(), used->end(), it->second.get()) == used->end())
				used->push_back(it->second.get());
		}
		return AGX_OK;
	}
	/* The record ring of the batch launches (agx_dataset_load_batch_ex, agx_dataset_positions), under the dataset's mutex.  take_record_slot:
	 * the fragments the batch uses go to the device (once per fragment: a blocking copy out of pageable memory), the next slot of the ring is
	 * free again once the launch that read it RING batches ago has finished — the only thing a call ever waits for. */
	int take_record_slot(AgxDataset *d, const std::vector<Fragment*> &used, RecordSlot **out)
	{
		for (Fragment *f : used)
			if (f->d_blob == nullptr)
			{
				AGX_HIP_CHECK(hipMalloc(&f->d_blob, std::max<size_t>(f->blob.size(), 1)));
				AGX_HIP_CHECK(hipMemcpy(f->d_blob, f->blob.data(), f->blob.size(), hipMemcpyHostToDevice));
			}
		RecordSlot &slot = d->slots[d->next_slot];
		d->next_slot = (d->next_slot + 1) % RING;
		if (slot.in_flight)
		{
			AGX_HIP_CHECK(hipEventSynchronize(slot.done));
			slot.in_flight = false;
		}
		*out = &slot;
		return AGX_OK;
	}
	/* ... the samples resolved into the slot's pinned records and sent behind `stream` ... */
	int send_records(AgxDataset *d, RecordSlot &slot, int n, const AgxDatasetSample *h_samples, hipStream_t stream)
	{
		if (slot.capacity < n)
		{ // a larger batch than this slot has seen: new buffers (an allocation, which the runtime may serialise with the device's work); the
		  // old ones are not freed here, which would synchronise the device, but with the dataset
			if (slot.h != nullptr)
				d->retired_host.push_back(slot.h);
			if (slot.d != nullptr)
				d->retired_device.push_back(slot.d);
			slot.h = nullptr;
			slot.d = nullptr;
			slot.capacity = 0;
			const int capacity = std::max(n, 1024);
			AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&slot.h), sizeof(BatchRecord) * capacity, hipHostMallocDefault));
			AGX_HIP_CHECK(hipMalloc(&slot.d, sizeof(BatchRecord) * capacity));
			slot.capacity = capacity;
		}
		for (int b = 0; b < n; b++)
		{
			const AgxDatasetSample &s = h_samples[b];
			const Fragment &f = *d->fragments.find(s.fragment)->second;
			const GameIndex &g = f.games[s.game];
			BatchRecord &r = slot.h[b];
			r.blob = f.d_blob;
			r.sample_off = g.sample_off[s.sample];
			r.moves_off = g.moves_off;
			r.n_moves = g.n_moves;
			r.outcome = g.outcome;
			r.augmentation = s.augmentation;
			r.pad = 0;
		}
		// the waves of two launches share the spill areas: launches on one stream follow each other anyway, a launch on ANOTHER stream
		// is ordered behind the previous one on the device (no host wait)
		if (d->launched && d->last_stream != stream)
			AGX_HIP_CHECK(hipStreamWaitEvent(stream, d->last_done, 0));
		AGX_HIP_CHECK(hipMemcpyAsync(slot.d, slot.h, sizeof(BatchRecord) * n, hipMemcpyHostToDevice, stream));
		return AGX_OK;
	}
	/* ... and the launch that reads them is on its way */
	int mark_launched(AgxDataset *d, RecordSlot &slot, hipStream_t stream)
	{
		AGX_HIP_CHECK(hipGetLastError());
		AGX_HIP_CHECK(hipEventRecord(slot.done, stream));
		slot.in_flight = true;
		d->launched = true;
		d->last_stream = stream;
		d->last_done = slot.done;
		return AGX_OK;
	}
	void fill_shape(AgxTensorShape *t, std::initializer_list<int> dims)
	{
		if (t == nullptr)
			return;
		t->rank = static_cast<int>(dims.size());
		for (int i = 0; i < 4; i++)
			t->dim[i] = (i < t->rank) ? dims.begin()[i] : 0;
	}
	int add_fragment(AgxDataset *d, int fragment, const AgxGameBuffer *buffer, const char *who)
	{ // (the dataset's mutex is held)
		int rules = 0, rows = 0, cols = 0;
		int st = agx_game_buffer_config(buffer, &rules, &rows, &cols, nullptr);
		if (st != AGX_OK)
			return st;
		AGX_REQUIRE(rows == d->rows && cols == d->cols, AGX_ERR_INVALID, "%s: the games are %dx%d, the dataset %dx%d", who, rows, cols, d->rows, d->cols);
		AGX_REQUIRE(rules == d->rules, AGX_ERR_INVALID, "%s: the games were played under other rules (%d) than the dataset's (%d)", who, rules, d->rules);
		AgxGameBufferStats stats;
		st = agx_game_buffer_stats(buffer, &stats);
		if (st != AGX_OK)
			return st;
		std::unique_ptr<Fragment> f(new Fragment());
		std::vector<uint8_t> bytes;
		for (int i = 0; i < stats.games; i++)
		{
			size_t size = 0;
			st = agx_game_buffer_game(buffer, i, nullptr, 0, &size);
			if (st != AGX_OK)
				return st;
			bytes.resize(size);
			st = agx_game_buffer_game(buffer, i, bytes.data(), bytes.size(), &size);
			if (st != AGX_OK)
				return st;
			const std::string wrong = index_game(*f, bytes.data(), size, d->rows, d->cols);
			AGX_REQUIRE(wrong.empty(), AGX_ERR_INVALID, "%s: game %d %s", who, i, wrong.c_str());
		}
		d->fragments[fragment] = std::move(f);
		return AGX_OK;
	}
}

extern "C" {

int agx_dataset_create(int rules, int rows, int cols, AgxDataset **out)
{
	AGX_REQUIRE(out != nullptr, AGX_ERR_INVALID, "agx_dataset_create: null argument");
	AGX_REQUIRE(rules >= 0 && rules <= AGX_CARO6, AGX_ERR_INVALID, "agx_dataset_create: invalid rules %d", rules);
	AGX_REQUIRE(rows == cols && rows >= 5 && rows <= agx::MAXN, AGX_ERR_UNSUPPORTED, "agx_dataset_create: square boards from 5x5 to %dx%d only (got %dx%d)", agx::MAXN,
			agx::MAXN, rows, cols);
	AgxDataset *d = new AgxDataset();
	d->rules = rules;
	d->rows = rows;
	d->cols = cols;
	*out = d;
	return AGX_OK;
}
int agx_dataset_destroy(AgxDataset *d)
{
	if (d == nullptr)
		return AGX_OK;
	// whatever a (possibly failed) load_batch left behind; a dataset that never reached a device makes no HIP call here
	(void) wait_for_batches(d);
	if (d->host_stream != nullptr)
		(void) hipStreamSynchronize(d->host_stream);
	for (auto &kv : d->fragments)
		if (kv.second->d_blob != nullptr)
			(void) hipFree(kv.second->d_blob);
	for (RecordSlot &s : d->slots)
	{
		if (s.h != nullptr)
			(void) hipHostFree(s.h);
		if (s.d != nullptr)
			(void) hipFree(s.d);
		if (s.done != nullptr)
			(void) hipEventDestroy(s.done);
	}
	for (void *p : { static_cast<void*>(d->d_pattern), static_cast<void*>(d->d_threat_packed), static_cast<void*>(d->d_list_spill), static_cast<void*>(d->d_snap_spill),
			d->d_stage })
		if (p != nullptr)
			(void) hipFree(p);
	for (BatchRecord *p : d->retired_host)
		(void) hipHostFree(p);
	for (BatchRecord *p : d->retired_device)
		(void) hipFree(p);
	if (d->h_error != nullptr)
		(void) hipHostFree(d->h_error);
	if (d->host_stream != nullptr)
		(void) hipStreamDestroy(d->host_stream);
	delete d;
	return AGX_OK;
}
int agx_dataset_add_fragment_buffer(AgxDataset *d, int fragment, const AgxGameBuffer *buffer)
{
	AGX_REQUIRE(d != nullptr && buffer != nullptr, AGX_ERR_INVALID, "agx_dataset_add_fragment_buffer: null argument");
	std::lock_guard<std::mutex> lock(d->mutex);
	AGX_REQUIRE(fragment >= 0 && d->fragments.count(fragment) == 0, AGX_ERR_INVALID, "agx_dataset_add_fragment_buffer: fragment %d is negative or already loaded", fragment);
	return add_fragment(d, fragment, buffer, "agx_dataset_add_fragment_buffer");
}
int agx_dataset_add_fragment_file(AgxDataset *d, int fragment, const char *path)
{
	AGX_REQUIRE(d != nullptr && path != nullptr, AGX_ERR_INVALID, "agx_dataset_add_fragment_file: null argument");
	std::lock_guard<std::mutex> lock(d->mutex);
	AGX_REQUIRE(fragment >= 0 && d->fragments.count(fragment) == 0, AGX_ERR_INVALID, "agx_dataset_add_fragment_file: fragment %d is negative or already loaded", fragment);
	AgxGameBuffer *buffer = nullptr;
	int st = agx_game_buffer_create(d->rules, d->rows, d->cols, 0, &buffer);
	if (st != AGX_OK)
		return st;
	st = agx_game_buffer_load(buffer, path); // refuses other rules, another board and broken layouts with its own message
	if (st == AGX_OK)
		st = add_fragment(d, fragment, buffer, "agx_dataset_add_fragment_file");
	agx_game_buffer_destroy(buffer);
	return st;
}
int agx_dataset_unload_fragment(AgxDataset *d, int fragment)
{
	AGX_REQUIRE(d != nullptr, AGX_ERR_INVALID, "agx_dataset_unload_fragment: null dataset");
	std::lock_guard<std::mutex> lock(d->mutex);
	auto it = d->fragments.find(fragment);
	AGX_REQUIRE(it != d->fragments.end(), AGX_ERR_INVALID, "agx_dataset_unload_fragment: fragment %d is not loaded", fragment);
	if (it->second->d_blob != nullptr)
	{
		const int st = wait_for_batches(d);
		if (st != AGX_OK)
			return st;
		AGX_HIP_CHECK(hipFree(it->second->d_blob));
	}
	d->fragments.erase(it);
	return AGX_OK;
}
int agx_dataset_games(const AgxDataset *d, int *games)
{
	AGX_REQUIRE(d != nullptr && games != nullptr, AGX_ERR_INVALID, "agx_dataset_games: null argument");
	std::lock_guard<std::mutex> lock(d->mutex);
	*games = 0;
	for (const auto &kv : d->fragments)
		*games += static_cast<int>(kv.second->games.size());
	return AGX_OK;
}
int agx_dataset_sizes(const AgxDataset *d, int *h_sizes, int capacity_games)
{
	AGX_REQUIRE(d != nullptr && h_sizes != nullptr, AGX_ERR_INVALID, "agx_dataset_sizes: null argument");
	std::lock_guard<std::mutex> lock(d->mutex);
	int idx = 0;
	for (const auto &kv : d->fragments)
		for (size_t j = 0; j < kv.second->games.size(); j++, idx++)
		{
			AGX_REQUIRE(idx < capacity_games, AGX_ERR_INVALID, "agx_dataset_sizes: more than %d games", capacity_games);
			h_sizes[4 * idx + 0] = kv.first;
			h_sizes[4 * idx + 1] = static_cast<int>(j);
			h_sizes[4 * idx + 2] = static_cast<int>(kv.second->games[j].sample_off.size());
			h_sizes[4 * idx + 3] = 8; // number_of_available_symmetries of a square board
		}
	return AGX_OK;
}
int agx_dataset_stats(const AgxDataset *d, AgxGameBufferStats *out)
{
	AGX_REQUIRE(d != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_dataset_stats: null argument");
	std::lock_guard<std::mutex> lock(d->mutex);
	std::memset(out, 0, sizeof(*out));
	for (const auto &kv : d->fragments)
	{
		const AgxGameBufferStats &s = kv.second->stats;
		out->games += s.games;
		out->samples += s.samples;
		out->cross_win += s.cross_win;
		out->draws += s.draws;
		out->circle_win += s.circle_win;
		out->game_length += s.game_length;
	}
	return AGX_OK;
}
int agx_dataset_tensor_shapes(const AgxDataset *d, int n, AgxTensorShape *input, AgxTensorShape *features, AgxTensorShape *policy_target, AgxTensorShape *value_target,
		AgxTensorShape *moves_left_target, AgxTensorShape *action_values_target)
{
	AGX_REQUIRE(d != nullptr && n >= 0, AGX_ERR_INVALID, "agx_dataset_tensor_shapes: null dataset or negative batch");
	fill_shape(input, { n, d->rows, d->cols, 32 });
	fill_shape(features, { n, d->rows * d->cols });
	fill_shape(policy_target, { n, d->rows, d->cols });
	fill_shape(value_target, { n, 3 });
	fill_shape(moves_left_target, { n, 1 });
	fill_shape(action_values_target, { n, d->rows, d->cols, 3 });
	return AGX_OK;
}

int agx_dataset_load_batch(AgxDataset *d, int n, const AgxDatasetSample *h_samples, void *d_input, uint32_t *d_features, float *d_policy, float *d_value,
		float *d_moves_left, float *d_action_values, int flags, void *stream_)
{
	const AgxBatchTensors tensors = { d_input, d_features, d_policy, d_value, d_moves_left, d_action_values, nullptr };
	return agx_dataset_load_batch_ex(d, n, h_samples, &tensors, flags, stream_);
}

int agx_dataset_load_batch_ex(AgxDataset *d, int n, const AgxDatasetSample *h_samples, const AgxBatchTensors *tensors, int flags, void *stream_)
{
	AGX_REQUIRE(d != nullptr && tensors != nullptr && n >= 0 && (h_samples != nullptr || n == 0), AGX_ERR_INVALID, "agx_dataset_load_batch: null argument or negative batch");
	AGX_REQUIRE(tensors->policy != nullptr && tensors->value != nullptr && tensors->moves_left != nullptr && tensors->action_values != nullptr, AGX_ERR_INVALID,
			"agx_dataset_load_batch: a target tensor is null (only input, features and action_values_weight are optional)");
	AGX_REQUIRE((flags & ~(AGX_BATCH_INPUT_FP16 | AGX_BATCH_POLICY_VISITS | AGX_BATCH_POLICY_VALUES)) == 0, AGX_ERR_INVALID, "agx_dataset_load_batch: unknown flags 0x%x", flags);
	AGX_REQUIRE((flags & AGX_BATCH_POLICY_VISITS) == 0 || (flags & AGX_BATCH_POLICY_VALUES) == 0, AGX_ERR_INVALID,
			"agx_dataset_load_batch: AGX_BATCH_POLICY_VISITS and AGX_BATCH_POLICY_VALUES name two different policy targets");
	std::lock_guard<std::mutex> lock(d->mutex);
	std::vector<Fragment*> used;
	int st = resolve(d, n, h_samples, &used);
	if (st != AGX_OK || n == 0)
		return st;
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	st = prepare_device(d);
	if (st != AGX_OK)
		return st;
	RecordSlot *taken = nullptr;
	st = take_record_slot(d, used, &taken);
	if (st != AGX_OK)
		return st;
	RecordSlot &slot = *taken;
	if (*d->h_error != 0)
	{ // left by a sample of an earlier batch (the kernel's note on ERR_FRAMES)
		const int b = *d->h_error - 1;
		*d->h_error = 0;
		AGX_REQUIRE(false, AGX_ERR_STATE, "agx_dataset_load_batch: sample %d of an earlier batch nests renju 3x3 forks deeper than the foul test follows: its features are invalid", b);
	}
	st = send_records(d, slot, n, h_samples, stream);
	if (st != AGX_OK)
		return st;
	agx::EngineDev E;
	std::memset(&E, 0, sizeof(E));
	E.rules = d->rules;
	E.n = d->rows;
	E.hw = d->rows * d->cols;
	E.t_pattern = d->d_pattern;
	E.t_threat_packed = d->d_threat_packed;
	BatchArgs A;
	A.records = slot.d;
	A.n = n;
	A.fp16 = (flags & AGX_BATCH_INPUT_FP16) ? 1 : 0;
	A.visits_mode = (flags & AGX_BATCH_POLICY_VISITS) ? 1 : 0;
	A.input = tensors->input;
	A.features = tensors->features;
	A.policy = tensors->policy;
	A.value = tensors->value;
	A.moves_left = tensors->moves_left;
	A.action_values = tensors->action_values;
	A.weight = tensors->action_values_weight;
	A.list_spill = d->d_list_spill;
	A.snap_spill = d->d_snap_spill;
	AGX_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&A.error), d->h_error, 0));
	const int waves = std::min(n, MAX_WAVES);
	const int targets = (flags & AGX_BATCH_POLICY_VALUES) ? agx::TARGETS_VALUES : (A.weight != nullptr ? agx::TARGETS_WEIGHTED : agx::TARGETS_PLAIN);
	const bool small = (d->rows <= 15);
	switch (targets)
	{
		case agx::TARGETS_VALUES:
			if (small)
				hipLaunchKernelGGL((agx::k_training_batch<15, agx::TARGETS_VALUES>), dim3(waves), dim3(64), 0, stream, E, A);
			else
				hipLaunchKernelGGL((agx::k_training_batch<agx::MAXN, agx::TARGETS_VALUES>), dim3(waves), dim3(64), 0, stream, E, A);
			break;
		case agx::TARGETS_WEIGHTED:
			if (small)
				hipLaunchKernelGGL((agx::k_training_batch<15, agx::TARGETS_WEIGHTED>), dim3(waves), dim3(64), 0, stream, E, A);
			else
				hipLaunchKernelGGL((agx::k_training_batch<agx::MAXN, agx::TARGETS_WEIGHTED>), dim3(waves), dim3(64), 0, stream, E, A);
			break;
		default:
			if (small)
				hipLaunchKernelGGL((agx::k_training_batch<15, agx::TARGETS_PLAIN>), dim3(waves), dim3(64), 0, stream, E, A);
			else
				hipLaunchKernelGGL((agx::k_training_batch<agx::MAXN, agx::TARGETS_PLAIN>), dim3(waves), dim3(64), 0, stream, E, A);
			break;
	}
	return mark_launched(d, slot, stream);
}

int agx_dataset_load_batch_host(AgxDataset *d, int n, const AgxDatasetSample *h_samples, void *h_input, uint32_t *h_features, float *h_policy, float *h_value,
		float *h_moves_left, float *h_action_values, int flags)
{
	const AgxBatchTensors tensors = { h_input, h_features, h_policy, h_value, h_moves_left, h_action_values, nullptr };
	return agx_dataset_load_batch_host_ex(d, n, h_samples, &tensors, flags);
}

int agx_dataset_load_batch_host_ex(AgxDataset *d, int n, const AgxDatasetSample *h_samples, const AgxBatchTensors *tensors, int flags)
{
	AGX_REQUIRE(d != nullptr && tensors != nullptr && n >= 0 && (h_samples != nullptr || n == 0), AGX_ERR_INVALID, "agx_dataset_load_batch_host: null argument or negative batch");
	void *h_input = tensors->input;
	uint32_t *h_features = tensors->features;
	float *h_weight = tensors->action_values_weight;
	AGX_REQUIRE(tensors->policy != nullptr && tensors->value != nullptr && tensors->moves_left != nullptr && tensors->action_values != nullptr, AGX_ERR_INVALID,
			"agx_dataset_load_batch_host: a target tensor is null (only input, features and action_values_weight are optional)");
	AGX_REQUIRE((flags & ~(AGX_BATCH_INPUT_FP16 | AGX_BATCH_POLICY_VISITS | AGX_BATCH_POLICY_VALUES)) == 0, AGX_ERR_INVALID, "agx_dataset_load_batch_host: unknown flags 0x%x", flags);
	AGX_REQUIRE((flags & AGX_BATCH_POLICY_VISITS) == 0 || (flags & AGX_BATCH_POLICY_VALUES) == 0, AGX_ERR_INVALID,
			"agx_dataset_load_batch_host: AGX_BATCH_POLICY_VISITS and AGX_BATCH_POLICY_VALUES name two different policy targets");
	if (n == 0)
		return AGX_OK;
	constexpr int OUTPUTS = 7;
	const size_t hw = static_cast<size_t>(d->rows) * d->cols, N = static_cast<size_t>(n);
	const size_t bytes[OUTPUTS] = { h_input ? N * hw * 32 * ((flags & AGX_BATCH_INPUT_FP16) ? 2 : 4) : 0, h_features ? N * hw * 4 : 0, N * hw * 4, N * 3 * 4, N * 4,
			N * hw * 3 * 4, h_weight ? N * hw * 4 : 0 };
	void *host[OUTPUTS] = { h_input, h_features, tensors->policy, tensors->value, tensors->moves_left, tensors->action_values, h_weight };
	size_t offset[OUTPUTS], total = 0;
	for (int i = 0; i < OUTPUTS; i++)
	{
		offset[i] = total;
		total += (bytes[i] + 255) / 256 * 256;
	}
	uint8_t *stage = nullptr;
	hipStream_t stream = nullptr;
	std::lock_guard<std::mutex> whole_call(d->host_mutex); // one staging area, one stream: host-pointer calls run one after the other
	{
		std::lock_guard<std::mutex> lock(d->mutex);
		const int valid = resolve(d, n, h_samples, nullptr); // an index out of range is refused before the device is touched
		if (valid != AGX_OK)
			return valid;
		if (d->host_stream == nullptr)
			AGX_HIP_CHECK(hipStreamCreateWithFlags(&d->host_stream, hipStreamNonBlocking));
		if (d->stage_bytes < total)
		{
			AGX_HIP_CHECK(hipStreamSynchronize(d->host_stream));
			if (d->d_stage != nullptr)
				AGX_HIP_CHECK(hipFree(d->d_stage));
			d->d_stage = nullptr;
			d->stage_bytes = 0;
			AGX_HIP_CHECK(hipMalloc(&d->d_stage, total));
			d->stage_bytes = total;
		}
		stage = static_cast<uint8_t*>(d->d_stage);
		stream = d->host_stream;
	}
	const AgxBatchTensors staged = { h_input ? stage + offset[0] : nullptr, h_features ? reinterpret_cast<uint32_t*>(stage + offset[1]) : nullptr,
			reinterpret_cast<float*>(stage + offset[2]), reinterpret_cast<float*>(stage + offset[3]), reinterpret_cast<float*>(stage + offset[4]),
			reinterpret_cast<float*>(stage + offset[5]), h_weight ? reinterpret_cast<float*>(stage + offset[6]) : nullptr };
	const int st = agx_dataset_load_batch_ex(d, n, h_samples, &staged, flags, stream);
	if (st != AGX_OK)
		return st;
	for (int i = 0; i < OUTPUTS; i++)
		if (bytes[i] != 0)
			AGX_HIP_CHECK(hipMemcpyAsync(host[i], stage + offset[i], bytes[i], hipMemcpyDeviceToHost, stream));
	AGX_HIP_CHECK(hipStreamSynchronize(stream));
	{
		std::lock_guard<std::mutex> lock(d->mutex);
		const int failed = *d->h_error;
		*d->h_error = 0;
		AGX_REQUIRE(failed == 0, AGX_ERR_STATE, "agx_dataset_load_batch_host: a sample (index %d of this or an earlier batch) nests renju 3x3 forks deeper than the foul test follows: its features are invalid",
				failed - 1);
	}
	return AGX_OK;
}

int agx_dataset_positions(AgxDataset *d, int n, const AgxDatasetSample *h_samples, uint8_t *d_boards, uint8_t *d_signs, void *stream_)
{
	AGX_REQUIRE(d != nullptr && n >= 0 && (h_samples != nullptr || n == 0), AGX_ERR_INVALID, "agx_dataset_positions: null argument or a negative count");
	AGX_REQUIRE(n == 0 || (d_boards != nullptr && d_signs != nullptr), AGX_ERR_INVALID, "agx_dataset_positions: null boards or signs");
	std::lock_guard<std::mutex> lock(d->mutex);
	std::vector<Fragment*> used;
	std::vector<AgxDatasetSample> plain(h_samples, h_samples + n);
	for (AgxDatasetSample &s : plain)
		s.augmentation = 0; // (ignored: a position has no orientation of its own)
	int st = resolve(d, n, plain.data(), &used);
	if (st != AGX_OK || n == 0)
		return st;
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	st = prepare_device(d);
	if (st != AGX_OK)
		return st;
	RecordSlot *slot = nullptr;
	st = take_record_slot(d, used, &slot);
	if (st == AGX_OK)
		st = send_records(d, *slot, n, plain.data(), stream);
	if (st != AGX_OK)
		return st;
	hipLaunchKernelGGL(agx::k_dataset_positions, dim3(std::min(n, MAX_WAVES)), dim3(64), 0, stream, slot->d, n, d->rows, d->rows * d->cols, d_boards, d_signs);
	return mark_launched(d, *slot, stream);
}

namespace
{
	struct ReanalyseScratch
	{ // what one pass allocates, freed on every way out
			uint8_t *d_bytes = nullptr;  // boards | signs | sample bytes
			int32_t *d_words = nullptr;  // serials | sizes | status | info
			uint8_t *h_bytes = nullptr;  // pinned: sample bytes
			int32_t *h_words = nullptr;  // pinned: serials | sizes | status | info
			~ReanalyseScratch()
			{
				if (d_bytes != nullptr)
					(void) hipFree(d_bytes);
				if (d_words != nullptr)
					(void) hipFree(d_words);
				if (h_bytes != nullptr)
					(void) hipHostFree(h_bytes);
				if (h_words != nullptr)
					(void) hipHostFree(h_words);
			}
	};
}

int agx_dataset_reanalyse(AgxDataset *d, int fragment, AgxPositionSearcher *searcher, AgxNet *net, AgxGameBuffer *out, const AgxReanalyseOptions *options,
		AgxReanalyseStats *stats, void *stream_)
{
	const char *who = "agx_dataset_reanalyse";
	AGX_REQUIRE(d != nullptr && searcher != nullptr && net != nullptr && out != nullptr, AGX_ERR_INVALID, "%s: null argument", who);
	const AgxReanalyseOptions opt = (options != nullptr) ? *options : AgxReanalyseOptions { 0, 0, 0 };
	AGX_REQUIRE(opt.chunk >= 0, AGX_ERR_INVALID, "%s: a chunk of %d positions", who, opt.chunk);
	int s_rules = 0, s_size = 0, s_slots = 0, o_rules = 0, o_rows = 0, o_cols = 0;
	int st = agx::position_searcher_describe(searcher, &s_rules, &s_size, &s_slots);
	if (st == AGX_OK)
		st = agx_game_buffer_config(out, &o_rules, &o_rows, &o_cols, nullptr);
	if (st != AGX_OK)
		return st;
	AGX_REQUIRE(s_rules == d->rules && s_size == d->rows && s_size == d->cols, AGX_ERR_INVALID, "%s: the searcher plays rules %d on %dx%d, the dataset rules %d on %dx%d", who,
			s_rules, s_size, s_size, d->rules, d->rows, d->cols);
	AGX_REQUIRE(o_rules == d->rules && o_rows == d->rows && o_cols == d->cols, AGX_ERR_INVALID, "%s: the output buffer holds rules %d on %dx%d, the dataset rules %d on %dx%d", who,
			o_rules, o_rows, o_cols, d->rules, d->rows, d->cols);
	// the work list: the samples of the fragment in (game, sample) order
	std::vector<AgxDatasetSample> list;
	std::vector<int> game_samples;
	{
		std::lock_guard<std::mutex> lock(d->mutex);
		auto it = d->fragments.find(fragment);
		AGX_REQUIRE(it != d->fragments.end(), AGX_ERR_INVALID, "%s: fragment %d is not loaded", who, fragment);
		const Fragment &f = *it->second;
		for (size_t g = 0; g < f.games.size(); g++)
		{
			game_samples.push_back(static_cast<int>(f.games[g].sample_off.size()));
			for (size_t k = 0; k < f.games[g].sample_off.size(); k++)
				list.push_back(AgxDatasetSample { fragment, static_cast<int>(g), static_cast<int>(k), 0 });
		}
	}
	AgxReanalyseStats total;
	std::memset(&total, 0, sizeof(total));
	if (stats != nullptr)
		*stats = total;
	if (list.empty())
		return AGX_OK;
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	const size_t hw = static_cast<size_t>(d->rows) * d->cols;
	const size_t stride = (agx::v201::HEADER_BYTES + agx::v201::ENTRY_BYTES * hw + 3) / 4 * 4;
	const size_t chunk = std::min<size_t>(list.size(), (opt.chunk > 0) ? opt.chunk : 16384);
	const size_t signs_at = chunk * hw, bytes_at = (signs_at + chunk + 255) / 256 * 256;
	ReanalyseScratch m;
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m.d_bytes), bytes_at + chunk * stride));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m.d_words), chunk * 7 * sizeof(int32_t)));
	AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m.h_bytes), chunk * stride, hipHostMallocDefault));
	AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&m.h_words), chunk * 7 * sizeof(int32_t), hipHostMallocDefault));
	AgxPositionSearchOutputs outputs;
	std::memset(&outputs, 0, sizeof(outputs));
	outputs.status = m.d_words + 2 * chunk;
	outputs.info = m.d_words + 3 * chunk;
	const AgxPositionSampleSink sink = { m.d_bytes + bytes_at, static_cast<int>(stride), m.d_words + chunk };
	// the game whose samples are coming in (the list is in game order: one game is open at a time)
	size_t game = 0;
	std::vector<std::vector<uint8_t>> fresh;
	std::vector<const uint8_t*> pointers;
	std::vector<int32_t> sizes;
	for (size_t j0 = 0; j0 < list.size(); j0 += chunk)
	{
		const int count = static_cast<int>(std::min(chunk, list.size() - j0));
		st = agx_dataset_positions(d, count, list.data() + j0, m.d_bytes, m.d_bytes + signs_at, stream_);
		if (st != AGX_OK)
			return st;
		for (int i = 0; i < count; i++)
			m.h_words[i] = static_cast<int32_t>(static_cast<uint32_t>(opt.serial_base) + static_cast<uint32_t>(j0 + i));
		AGX_HIP_CHECK(hipMemcpyAsync(m.d_words, m.h_words, count * sizeof(int32_t), hipMemcpyHostToDevice, stream));
		st = agx_position_searcher_search_ex(searcher, net, count, m.d_bytes, m.d_bytes + signs_at, m.d_words, &outputs, &sink, 0, opt.max_steps, stream_);
		if (st != AGX_OK)
			return st;
		// sizes | status | info in one copy, then the used part of every sample's stride in one more
		AGX_HIP_CHECK(hipMemcpyAsync(m.h_words + chunk, m.d_words + chunk, chunk * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
		AGX_HIP_CHECK(hipStreamSynchronize(stream));
		const int32_t *h_sizes = m.h_words + chunk, *h_status = m.h_words + 2 * chunk, *h_info = m.h_words + 3 * chunk;
		size_t used = 0;
		for (int i = 0; i < count; i++)
		{
			AGX_REQUIRE(h_sizes[i] >= 0 && static_cast<size_t>(h_sizes[i]) <= stride && h_status[i] >= 0 && h_status[i] <= 3, AGX_ERR_STATE,
					"%s: position %zu came back with %d bytes and status %d", who, j0 + i, h_sizes[i], h_status[i]);
			if (h_status[i] == 0)
				used = std::max(used, static_cast<size_t>(h_sizes[i]));
		}
		if (used > 0)
		{
			AGX_HIP_CHECK(hipMemcpy2DAsync(m.h_bytes, stride, sink.d_bytes, stride, used, count, hipMemcpyDeviceToHost, stream));
			AGX_HIP_CHECK(hipStreamSynchronize(stream));
		}
		for (int i = 0; i < count; i++)
		{
			const bool replace = (h_status[i] == 0 && h_sizes[i] > 0); // a truncated search is no training target
			total.samples++;
			total.status[h_status[i]]++;
			total.steps += h_info[4 * i + 2];
			(replace ? total.replaced : total.kept)++;
			fresh.emplace_back();
			if (replace)
				fresh.back().assign(m.h_bytes + i * stride, m.h_bytes + i * stride + h_sizes[i]);
			if (static_cast<int>(fresh.size()) < game_samples[game])
				continue;
			pointers.clear();
			sizes.clear();
			for (const std::vector<uint8_t> &s : fresh)
			{
				pointers.push_back(s.data());
				sizes.push_back(static_cast<int32_t>(s.size()));
			}
			{
				std::lock_guard<std::mutex> lock(d->mutex);
				auto it = d->fragments.find(fragment);
				AGX_REQUIRE(it != d->fragments.end() && game < it->second->games.size() && static_cast<int>(it->second->games[game].sample_off.size()) == game_samples[game],
						AGX_ERR_STATE, "%s: fragment %d was unloaded or replaced during the pass", who, fragment);
				const GameIndex &g = it->second->games[game];
				const size_t begin = g.sample_off[0] - 4, end = g.moves_off + 2 * static_cast<size_t>(g.n_moves) + 12;
				st = agx_game_buffer_add_reanalysed(out, it->second->blob.data() + begin, end - begin, game_samples[game], pointers.data(), sizes.data());
			}
			if (st != AGX_OK)
				return st;
			total.games++;
			fresh.clear();
			game++;
		}
	}
	if (stats != nullptr)
		*stats = total;
	return AGX_OK;
}

} /* extern "C" */
