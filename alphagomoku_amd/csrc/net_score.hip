/*
 * net_score.hip — a network scored against saved games on the device: cross-entropy losses and top-k accuracy (agx.h: agx_net_score_*).
 *
 * What it replaces: the validation pass of the reference's training loop (SupervisedLearning::validate: AGNetwork::getLoss and
 * getAccuracy, src/networks/NetworkDataPack.cpp:321-345, over host copies of the outputs and the targets).  getAccuracy is followed line
 * by line; the loss formulas are this project's own (MinML's loss code is not in the reference tree) and are defined in agx.h.
 *
 * MI355X mapping: ONE WAVEFRONT PER SAMPLE, like k_training_batch.  A lane owns the cells lane, lane + 64, ...: at most 7 of the 400 cells
 * of a 20x20 board, kept in registers.  A lane adds its float32 terms up in float64 in cell order, the 64 partial sums meet in a butterfly
 * of 6 exchanges: a fixed tree per sample, whatever the grid.  An argmax is a butterfly on (value, lowest index).  The samples' records
 * are then added in SAMPLE ORDER, one after the other, by one lane of a single workgroup: the only summation order that gives the same
 * bits when a set of samples is scored in one call or in several chained ones.  No atomics.
 */
#include "agx_internal.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace agx
{
	namespace
	{
		constexpr int SCORE_MAX_HW = 400;
		constexpr int SCORE_CHUNKS = (SCORE_MAX_HW + 63) / 64;
		constexpr int SCORE_MAX_WAVES = 4096; // workgroups of a launch (one wave each); larger batches stride
		constexpr int FUSED_WAVES = 16;      // waves of the one-workgroup form

		struct ScoreArgs
		{
				int hw, n;
				const float *policy, *value, *action_values;                      // outputs: [n][hw], [n][3], [n][hw][2] or null
				const float *policy_target, *value_target, *action_values_target; // targets: [n][hw], [n][3], [n][hw][3] or null
				AgxSampleScore *scores;                                           // [n] (null in the one-workgroup form)
				AgxNetScore *total;
				const float *q_weight;                                            // [n][hw] or null: agx_net_score_outputs_weighted
		};

		/* float32 term, as defined in agx.h: the product is rounded to float32 (the file is compiled with -ffp-contract=off) */
		__device__ __forceinline__ float ce_term(float t, float p)
		{
			return -(t * logf(fmaxf(p, FLT_MIN)));
		}
		__device__ __forceinline__ double wave_sum(double v)
		{
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
				v += __shfl_xor(v, off, 64);
			return v;
		}
		/* std::max_element over the whole board: the largest value, of equal ones the lowest index.  Every lane gets the result. */
		__device__ __forceinline__ int wave_first_max(const float (&v)[SCORE_CHUNKS], int hw, int lane)
		{
			float best = -INFINITY;
			int at = 0x7FFFFFFF; // "no cell": loses against every cell, also one that holds -inf
#pragma unroll
			for (int ch = 0; ch < SCORE_CHUNKS; ch++)
			{
				const int cell = ch * 64 + lane;
				if (cell < hw && (v[ch] > best || at == 0x7FFFFFFF))
				{
					best = v[ch];
					at = cell;
				}
			}
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
			{
				const float ov = __shfl_xor(best, off, 64);
				const int oi = __shfl_xor(at, off, 64);
				if (ov > best || (ov == best && oi < at))
				{
					best = ov;
					at = oi;
				}
			}
			return at;
		}
		/* max_element compares with <, which is false for a NaN on either side: a NaN on cell 0 stays the maximum, a NaN elsewhere never
		 * becomes it.  The same with ordered values: */
		__device__ __forceinline__ float ordered(float v, int cell)
		{
			return (v != v) ? ((cell == 0) ? INFINITY : -INFINITY) : v;
		}

		/* the record of sample b, complete in every lane of the wave */
		__device__ __forceinline__ AgxSampleScore score_sample(const ScoreArgs &A, int b, int lane)
		{
			const int hw = A.hw;
			const float *p = A.policy + static_cast<size_t>(b) * hw;
			const float *t = A.policy_target + static_cast<size_t>(b) * hw;
			const bool with_q = (A.action_values != nullptr);
			float out[SCORE_CHUNKS], target[SCORE_CHUNKS];
			double policy_sum = 0.0, q_sum = 0.0;
			int cells = 0;
#pragma unroll
			for (int ch = 0; ch < SCORE_CHUNKS; ch++)
			{
				const int cell = ch * 64 + lane;
				out[ch] = 0.0f;
				target[ch] = 0.0f;
				if (cell < hw)
				{
					const float pv = p[cell], tv = t[cell];
					out[ch] = ordered(pv, cell);
					target[ch] = ordered(tv, cell);
					if (tv > 0.0f)
						policy_sum += static_cast<double>(ce_term(tv, pv));
					if (A.q_weight != nullptr)
					{ // (needs action values: the host has checked)
						const float w = A.q_weight[static_cast<size_t>(b) * hw + cell];
						if (w > 0.0f)
						{
							const float *q = A.action_values + (static_cast<size_t>(b) * hw + cell) * 2;
							const float *qt = A.action_values_target + (static_cast<size_t>(b) * hw + cell) * 3;
							const float win = q[0], draw = q[1];
							double ce = 0.0;
							ce += static_cast<double>(ce_term(qt[0], win));
							ce += static_cast<double>(ce_term(qt[1], draw));
							ce += static_cast<double>(ce_term(qt[2], 1.0f - win - draw)); // Value::loss_rate
							q_sum += static_cast<double>(w) * ce;
							cells++;
						}
					}
					else if (tv > 0.0f)
					{
						if (with_q)
						{
							const float *q = A.action_values + (static_cast<size_t>(b) * hw + cell) * 2;
							const float *qt = A.action_values_target + (static_cast<size_t>(b) * hw + cell) * 3;
							const float win = q[0], draw = q[1];
							q_sum += static_cast<double>(ce_term(qt[0], win));
							q_sum += static_cast<double>(ce_term(qt[1], draw));
							q_sum += static_cast<double>(ce_term(qt[2], 1.0f - win - draw)); // Value::loss_rate
							cells++;
						}
					}
				}
			}
			AgxSampleScore r;
			r.policy_ce = wave_sum(policy_sum);
			r.q_ce = wave_sum(q_sum);
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
				cells += __shfl_xor(cells, off, 64);
			r.q_cells = cells;
			double value_sum = 0.0;
			for (int c = 0; c < 3; c++)
			{
				const float tv = A.value_target[static_cast<size_t>(b) * 3 + c];
				if (tv > 0.0f)
					value_sum += static_cast<double>(ce_term(tv, A.value[static_cast<size_t>(b) * 3 + c]));
			}
			r.value_ce = value_sum;
			// getAccuracy (NetworkDataPack.cpp:333-341) with top_k = 4
			const int correct = wave_first_max(target, hw, lane);
			for (int m = 0; m < 4; m++)
				r.topk_hit[m] = 0;
			for (int l = 0; l < 4; l++)
			{
				const int best = wave_first_max(out, hw, lane);
				if (best == correct)
					for (int m = l; m < 4; m++)
						r.topk_hit[m] += 1;
#pragma unroll
				for (int ch = 0; ch < SCORE_CHUNKS; ch++)
					if (ch * 64 + lane == best)
						out[ch] = 0.0f;
			}
			r.reserved = 0;
			return r;
		}
		__device__ __forceinline__ void add_record(AgxNetScore &acc, const AgxSampleScore &s)
		{
			acc.samples += 1;
			acc.policy_ce += s.policy_ce;
			acc.value_ce += s.value_ce;
			acc.q_ce += s.q_ce;
			acc.q_cells += s.q_cells;
			for (int m = 0; m < 4; m++)
				acc.topk_hit[m] += s.topk_hit[m];
		}

		__global__ __launch_bounds__(64) void k_score_batch(ScoreArgs A)
		{
			const int lane = threadIdx.x;
			for (int b = blockIdx.x; b < A.n; b += gridDim.x)
			{
				const AgxSampleScore r = score_sample(A, b, lane);
				if (lane == 0)
					A.scores[b] = r;
			}
		}
		/* one workgroup, one wave: 64 records at a time into LDS, lane 0 adds them in sample order */
		__global__ __launch_bounds__(64) void k_score_reduce(ScoreArgs A)
		{
			__shared__ AgxSampleScore stage[64];
			const int lane = threadIdx.x;
			AgxNetScore acc = *A.total;
			for (int base = 0; base < A.n; base += 64)
			{
				const int count = min(64, A.n - base);
				if (lane < count)
					stage[lane] = A.scores[base + lane];
				__syncthreads();
				if (lane == 0)
					for (int k = 0; k < count; k++)
						add_record(acc, stage[k]);
				__syncthreads();
			}
			if (lane == 0)
				*A.total = acc;
		}
		/* both in one workgroup, for callers that keep no per-sample records: 16 waves score 16 samples, thread 0 adds them in sample order */
		__global__ __launch_bounds__(64 * FUSED_WAVES) void k_score_batch_total(ScoreArgs A)
		{
			__shared__ AgxSampleScore stage[FUSED_WAVES];
			const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
			AgxNetScore acc;
			if (threadIdx.x == 0)
				acc = *A.total;
			for (int base = 0; base < A.n; base += FUSED_WAVES)
			{
				const int count = min(FUSED_WAVES, A.n - base);
				if (wave < count)
				{
					const AgxSampleScore r = score_sample(A, base + wave, lane);
					if (lane == 0)
						stage[wave] = r;
				}
				__syncthreads();
				if (threadIdx.x == 0)
					for (int k = 0; k < count; k++)
						add_record(acc, stage[k]);
				__syncthreads();
			}
			if (threadIdx.x == 0)
				*A.total = acc;
		}

		struct Scratch
		{ // device memory of one agx_net_score_dataset call
				void *p = nullptr;
				~Scratch()
				{
					if (p != nullptr)
						(void) hipFree(p);
				}
		};
	}

	/* agx_internal.hpp: k_score_reduce for the other files that write per-sample records (head_loss.hip) */
	int add_sample_scores(int n, AgxSampleScore *d_scores, AgxNetScore *d_total, hipStream_t stream)
	{
		ScoreArgs A { };
		A.n = n;
		A.scores = d_scores;
		A.total = d_total;
		hipLaunchKernelGGL(k_score_reduce, dim3(1), dim3(64), 0, stream, A);
		AGX_HIP_CHECK(hipGetLastError());
		return AGX_OK;
	}
}

extern "C" {

int agx_net_score_clear(AgxNetScore *d_total, void *stream)
{
	AGX_REQUIRE(d_total != nullptr, AGX_ERR_INVALID, "agx_net_score_clear: null argument");
	AGX_HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof(AgxNetScore), static_cast<hipStream_t>(stream)));
	return AGX_OK;
}

int agx_net_score_outputs(int rows, int cols, int n, const float *d_policy, const float *d_value, const float *d_action_values, const float *d_policy_target,
		const float *d_value_target, const float *d_action_values_target, AgxSampleScore *d_sample_scores, AgxNetScore *d_total, void *stream_)
{
	return agx_net_score_outputs_weighted(rows, cols, n, d_policy, d_value, d_action_values, d_policy_target, d_value_target, d_action_values_target, nullptr,
			d_sample_scores, d_total, stream_);
}

int agx_net_score_outputs_weighted(int rows, int cols, int n, const float *d_policy, const float *d_value, const float *d_action_values, const float *d_policy_target,
		const float *d_value_target, const float *d_action_values_target, const float *d_q_weight, AgxSampleScore *d_sample_scores, AgxNetScore *d_total, void *stream_)
{
	static_assert(sizeof(AgxSampleScore) == 48 && sizeof(AgxNetScore) == 72, "score record layouts");
	AGX_REQUIRE(rows >= 5 && rows <= 20 && cols >= 5 && cols <= 20, AGX_ERR_INVALID, "agx_net_score_outputs: boards from 5x5 to 20x20 (got %dx%d)", rows, cols);
	AGX_REQUIRE(n > 0, AGX_ERR_INVALID, "agx_net_score_outputs: %d samples", n);
	AGX_REQUIRE(d_policy != nullptr && d_value != nullptr && d_policy_target != nullptr && d_value_target != nullptr && d_total != nullptr, AGX_ERR_INVALID,
			"agx_net_score_outputs: null argument (only the two action-value tensors and d_sample_scores are optional)");
	AGX_REQUIRE((d_action_values == nullptr) == (d_action_values_target == nullptr), AGX_ERR_INVALID,
			"agx_net_score_outputs: action values need both the outputs and the targets");
	AGX_REQUIRE(d_q_weight == nullptr || d_action_values != nullptr, AGX_ERR_INVALID, "agx_net_score_outputs_weighted: a weight without action values");
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	agx::ScoreArgs A;
	A.hw = rows * cols;
	A.n = n;
	A.policy = d_policy;
	A.value = d_value;
	A.action_values = d_action_values;
	A.policy_target = d_policy_target;
	A.value_target = d_value_target;
	A.action_values_target = d_action_values_target;
	A.scores = d_sample_scores;
	A.total = d_total;
	A.q_weight = d_q_weight;
	if (d_sample_scores == nullptr)
		hipLaunchKernelGGL(agx::k_score_batch_total, dim3(1), dim3(64 * agx::FUSED_WAVES), 0, stream, A);
	else
	{
		hipLaunchKernelGGL(agx::k_score_batch, dim3(std::min(n, agx::SCORE_MAX_WAVES)), dim3(64), 0, stream, A);
		hipLaunchKernelGGL(agx::k_score_reduce, dim3(1), dim3(64), 0, stream, A);
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}

int agx_net_score_dataset(AgxNet *net, AgxDataset *dataset, int n, const AgxDatasetSample *h_samples, int chunk, AgxNetScore *h_out, void *stream_)
{
	return agx_net_score_dataset_ex(net, dataset, n, h_samples, chunk, 0, 0, h_out, stream_);
}

int agx_net_score_dataset_ex(AgxNet *net, AgxDataset *dataset, int n, const AgxDatasetSample *h_samples, int chunk, int batch_flags, int q_weighted, AgxNetScore *h_out,
		void *stream_)
{
	AGX_REQUIRE(net != nullptr && dataset != nullptr && h_samples != nullptr && h_out != nullptr, AGX_ERR_INVALID, "agx_net_score_dataset: null argument");
	AGX_REQUIRE(n > 0 && chunk >= 0, AGX_ERR_INVALID, "agx_net_score_dataset: %d samples in chunks of %d", n, chunk);
	AGX_REQUIRE((batch_flags & ~(AGX_BATCH_POLICY_VISITS | AGX_BATCH_POLICY_VALUES)) == 0, AGX_ERR_INVALID,
			"agx_net_score_dataset_ex: batch flags 0x%x (only the two policy flags: the path reads feature words)", batch_flags);
	AgxNetDesc desc;
	int st = agx_net_description(net, &desc);
	if (st != AGX_OK)
		return st;
	AgxTensorShape board;
	st = agx_dataset_tensor_shapes(dataset, 1, nullptr, nullptr, &board, nullptr, nullptr, nullptr);
	if (st != AGX_OK)
		return st;
	AGX_REQUIRE(board.dim[1] == desc.rows && board.dim[2] == desc.cols, AGX_ERR_INVALID, "agx_net_score_dataset: the dataset's games are %dx%d, the network's board %dx%d",
			board.dim[1], board.dim[2], desc.rows, desc.cols);
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	const size_t hw = static_cast<size_t>(desc.rows) * desc.cols, C = static_cast<size_t>(std::min(chunk == 0 ? 1024 : chunk, n));
	const bool with_q = (desc.action_values != 0), weighted = with_q && (q_weighted != 0);
	// features, policy / value / moves-left / action-value targets, the network's policy / value / action values, the records, the total,
	// the action-value weights
	constexpr int AREAS = 11;
	const size_t bytes[AREAS] = { C * hw * 4, C * hw * 4, C * 3 * 4, C * 4, C * hw * 3 * 4, C * hw * 4, C * 3 * 4, with_q ? C * hw * 2 * 4 : 0, C * sizeof(AgxSampleScore),
			sizeof(AgxNetScore), weighted ? C * hw * 4 : 0 };
	size_t offset[AREAS], total = 0;
	for (int i = 0; i < AREAS; i++)
	{
		offset[i] = total;
		total += (bytes[i] + 255) / 256 * 256;
	}
	agx::Scratch scratch;
	AGX_HIP_CHECK(hipMalloc(&scratch.p, total));
	uint8_t *base = static_cast<uint8_t*>(scratch.p);
	const auto at = [&](int i) { return reinterpret_cast<float*>(base + offset[i]); };
	AgxNetScore *d_total = reinterpret_cast<AgxNetScore*>(base + offset[9]);
	st = agx_net_score_clear(d_total, stream);
	for (int first = 0; first < n && st == AGX_OK; first += static_cast<int>(C))
	{
		const int count = std::min(static_cast<int>(C), n - first);
		const AgxBatchTensors tensors = { nullptr, reinterpret_cast<uint32_t*>(at(0)), at(1), at(2), at(3), at(4), weighted ? at(10) : nullptr };
		st = agx_dataset_load_batch_ex(dataset, count, h_samples + first, &tensors, batch_flags, stream);
		if (st == AGX_OK)
			st = with_q ? agx_nn_forward_pvq(net, reinterpret_cast<const uint32_t*>(at(0)), count, at(5), at(6), at(7), stream) :
					agx_nn_forward(net, reinterpret_cast<const uint32_t*>(at(0)), count, at(5), at(6), stream);
		if (st == AGX_OK)
			st = agx_net_score_outputs_weighted(desc.rows, desc.cols, count, at(5), at(6), with_q ? at(7) : nullptr, at(1), at(2), with_q ? at(4) : nullptr,
					weighted ? at(10) : nullptr, reinterpret_cast<AgxSampleScore*>(base + offset[8]), d_total, stream);
	}
	if (st != AGX_OK)
	{ // whatever was enqueued still uses the scratch
		(void) hipStreamSynchronize(stream);
		return st;
	}
	AGX_HIP_CHECK(hipMemcpyAsync(h_out, d_total, sizeof(AgxNetScore), hipMemcpyDeviceToHost, stream));
	AGX_HIP_CHECK(hipStreamSynchronize(stream));
	return AGX_OK;
}

} /* extern "C" */
