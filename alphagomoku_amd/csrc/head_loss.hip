/*
 * head_loss.hip — the training loss of the three heads and its gradients with respect to the logits, on the device (agx.h: agx_head_loss_grad).
 *
 * What it replaces: the loss layer at the end of the reference's training graph (graph.setOptimizer / train in src/networks/networks.cpp and
 * SupervisedLearning).  MinML's loss code is not in the reference tree, so the formulas are this project's own and are defined in agx.h: the
 * cross-entropy of net_score.hip in its log-sum-exp form, on logits instead of probabilities.  The convolutions' backward pass and the optimiser
 * stay with PyTorch; this file hands it dL/dlogits.
 *
 * MI355X mapping: ONE WAVEFRONT PER SAMPLE, like k_score_batch.  A lane owns the cells lane, lane + 64, ...: at most 7 of the 400 cells of a
 * 20x20 board, logits, targets and exponentials kept in registers.  A lane adds its float32 terms up in float64 in cell order, the 64 partial
 * sums meet in a butterfly of 6 exchanges: a fixed tree per sample, whatever the grid.  The per-cell softmax over the 3 action-value classes
 * needs no exchange at all.  The samples' records are added in sample order by net_score.hip's one-workgroup reduction.  No atomics.
 */
#include "agx_internal.hpp"

#include <algorithm>
#include <cmath>

namespace agx
{
	namespace
	{
		constexpr int LOSS_MAX_HW = 400;
		constexpr int LOSS_CHUNKS = (LOSS_MAX_HW + 63) / 64;
		constexpr int LOSS_MAX_WAVES = 4096; // workgroups of a launch (one wave each); larger batches stride

		struct HeadLossArgs
		{
				int hw, n;
				const float *policy, *value, *q;                      // logits: [n][hw], [n][3], [n][hw][3] or null
				const float *policy_target, *value_target, *q_target; // targets: [n][hw], [n][3], [n][hw][3] or null
				float policy_scale, value_scale, q_scale;
				float *policy_grad, *value_grad, *q_grad;             // like the logits; all null: losses only
				AgxSampleScore *scores;                               // [n]
				const float *q_weight;                                // [n][hw]: k_head_loss<true> only
		};

		__device__ __forceinline__ double wave_sum(double v)
		{
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
				v += __shfl_xor(v, off, 64);
			return v;
		}
		__device__ __forceinline__ float wave_max(float v)
		{
#pragma unroll
			for (int off = 1; off < 64; off <<= 1)
				v = fmaxf(v, __shfl_xor(v, off, 64));
			return v;
		}
		/* a target that counts: the positive ones.  Everything else — zeros, negative values, NaN filler — is selected away, never multiplied */
		__device__ __forceinline__ float counted(float t)
		{
			return (t > 0.0f) ? t : 0.0f;
		}
		/* softmax cross-entropy over 3 logits held by one lane: adds the float32 terms t * (lse - z) of the positive targets to `loss`
		 * in class order and, with `grad`, writes scale * (p * T - t) for the 3 classes */
		__device__ __forceinline__ void three_way(const float *z, const float *t, float scale, double &loss, float *grad)
		{
			const float z0 = z[0], z1 = z[1], z2 = z[2];
			const float t0 = counted(t[0]), t1 = counted(t[1]), t2 = counted(t[2]);
			const float m = fmaxf(fmaxf(z0, z1), z2);
			const float e0 = expf(z0 - m), e1 = expf(z1 - m), e2 = expf(z2 - m);
			const double S = static_cast<double>(e0) + static_cast<double>(e1) + static_cast<double>(e2);
			const float Sf = static_cast<float>(S);
			const float lse = m + logf(Sf);
			if (t0 > 0.0f)
				loss += static_cast<double>(t0 * (lse - z0));
			if (t1 > 0.0f)
				loss += static_cast<double>(t1 * (lse - z1));
			if (t2 > 0.0f)
				loss += static_cast<double>(t2 * (lse - z2));
			if (grad != nullptr)
			{
				const float T = static_cast<float>(static_cast<double>(t0) + static_cast<double>(t1) + static_cast<double>(t2));
				grad[0] = scale * ((e0 / Sf) * T - t0);
				grad[1] = scale * ((e1 / Sf) * T - t1);
				grad[2] = scale * ((e2 / Sf) * T - t2);
			}
		}

		/* WEIGHTED: the action-value cells that count are those with A.q_weight > 0 (agx.h: agx_head_loss_grad_weighted) */
		template<bool WEIGHTED>
		__global__ __launch_bounds__(64) void k_head_loss(HeadLossArgs A)
		{
			const int lane = threadIdx.x;
			const int hw = A.hw;
			const bool with_q = (A.q != nullptr), with_grad = (A.policy_grad != nullptr);
			for (int b = blockIdx.x; b < A.n; b += gridDim.x)
			{
				const size_t row = static_cast<size_t>(b) * hw;
				const float *zp = A.policy + row;
				const float *tp = A.policy_target + row;
				float z[LOSS_CHUNKS], t[LOSS_CHUNKS], e[LOSS_CHUNKS];
				float m = -INFINITY;
#pragma unroll
				for (int ch = 0; ch < LOSS_CHUNKS; ch++)
				{
					const int cell = ch * 64 + lane;
					z[ch] = 0.0f;
					t[ch] = 0.0f;
					if (cell < hw)
					{
						z[ch] = zp[cell];
						t[ch] = counted(tp[cell]);
						m = fmaxf(m, z[ch]);
					}
				}
				m = wave_max(m);
				double exp_sum = 0.0, target_sum = 0.0;
#pragma unroll
				for (int ch = 0; ch < LOSS_CHUNKS; ch++)
				{
					e[ch] = 0.0f;
					if (ch * 64 + lane < hw)
					{
						e[ch] = expf(z[ch] - m);
						exp_sum += static_cast<double>(e[ch]);
						target_sum += static_cast<double>(t[ch]);
					}
				}
				const float Sf = static_cast<float>(wave_sum(exp_sum));
				const float T = static_cast<float>(wave_sum(target_sum));
				const float lse = m + logf(Sf);
				double policy_sum = 0.0, q_sum = 0.0;
				int cells = 0;
#pragma unroll
				for (int ch = 0; ch < LOSS_CHUNKS; ch++)
				{
					const int cell = ch * 64 + lane;
					if (cell < hw)
					{
						const bool edge = (t[ch] > 0.0f);
						if (edge)
							policy_sum += static_cast<double>(t[ch] * (lse - z[ch]));
						if (with_grad)
							A.policy_grad[row + cell] = A.policy_scale * ((e[ch] / Sf) * T - t[ch]);
						if (with_q)
						{
							const size_t at = (row + cell) * 3;
							float w = 0.0f;
							if constexpr (WEIGHTED)
								w = A.q_weight[row + cell];
							if (WEIGHTED ? (w > 0.0f) : edge)
							{
								if constexpr (WEIGHTED)
								{
									double ce = 0.0;
									three_way(A.q + at, A.q_target + at, A.q_scale * w, ce, with_grad ? A.q_grad + at : nullptr);
									q_sum += static_cast<double>(w) * ce;
								}
								else
									three_way(A.q + at, A.q_target + at, A.q_scale, q_sum, with_grad ? A.q_grad + at : nullptr);
								cells++;
							}
							else if (with_grad)
							{ // the cell does not count (no edge; weighted: no weight): its action-value target is filler and is not even read
								A.q_grad[at] = 0.0f;
								A.q_grad[at + 1] = 0.0f;
								A.q_grad[at + 2] = 0.0f;
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
				if (lane == 0)
				{
					double value_sum = 0.0;
					float grad[3];
					three_way(A.value + static_cast<size_t>(b) * 3, A.value_target + static_cast<size_t>(b) * 3, A.value_scale, value_sum, with_grad ? grad : nullptr);
					if (with_grad)
						for (int c = 0; c < 3; c++)
							A.value_grad[static_cast<size_t>(b) * 3 + c] = grad[c];
					r.value_ce = value_sum;
					for (int k = 0; k < 4; k++)
						r.topk_hit[k] = 0;
					r.reserved = 0;
					A.scores[b] = r;
				}
			}
		}
	}
}

extern "C" {

int agx_head_loss_grad(int rows, int cols, int n, const float *d_policy_logits, const float *d_value_logits, const float *d_q_logits, const float *d_policy_target,
		const float *d_value_target, const float *d_q_target, float policy_scale, float value_scale, float q_scale, float *d_policy_grad, float *d_value_grad,
		float *d_q_grad, AgxSampleScore *d_sample_scores, AgxNetScore *d_total, void *stream_)
{
	return agx_head_loss_grad_weighted(rows, cols, n, d_policy_logits, d_value_logits, d_q_logits, d_policy_target, d_value_target, d_q_target, nullptr, policy_scale,
			value_scale, q_scale, d_policy_grad, d_value_grad, d_q_grad, d_sample_scores, d_total, stream_);
}

int agx_head_loss_grad_weighted(int rows, int cols, int n, const float *d_policy_logits, const float *d_value_logits, const float *d_q_logits,
		const float *d_policy_target, const float *d_value_target, const float *d_q_target, const float *d_q_weight, float policy_scale, float value_scale, float q_scale,
		float *d_policy_grad, float *d_value_grad, float *d_q_grad, AgxSampleScore *d_sample_scores, AgxNetScore *d_total, void *stream_)
{
	AGX_REQUIRE(rows >= 5 && rows <= 20 && cols >= 5 && cols <= 20, AGX_ERR_INVALID, "agx_head_loss_grad: boards from 5x5 to 20x20 (got %dx%d)", rows, cols);
	AGX_REQUIRE(n > 0, AGX_ERR_INVALID, "agx_head_loss_grad: %d samples", n);
	AGX_REQUIRE(d_policy_logits != nullptr && d_value_logits != nullptr && d_policy_target != nullptr && d_value_target != nullptr && d_sample_scores != nullptr
			&& d_total != nullptr, AGX_ERR_INVALID, "agx_head_loss_grad: null argument (only the action-value tensors and the three gradients are optional)");
	AGX_REQUIRE((d_q_logits == nullptr) == (d_q_target == nullptr), AGX_ERR_INVALID, "agx_head_loss_grad: action values need both the logits and the targets");
	AGX_REQUIRE(d_q_weight == nullptr || d_q_logits != nullptr, AGX_ERR_INVALID, "agx_head_loss_grad_weighted: a weight without action values");
	const bool with_grad = (d_policy_grad != nullptr || d_value_grad != nullptr || d_q_grad != nullptr);
	AGX_REQUIRE(!with_grad || (d_policy_grad != nullptr && d_value_grad != nullptr && (d_q_grad != nullptr) == (d_q_logits != nullptr)), AGX_ERR_INVALID,
			"agx_head_loss_grad: gradients are written for every head that has logits, or for none");
	hipStream_t stream = static_cast<hipStream_t>(stream_);
	agx::HeadLossArgs A;
	A.hw = rows * cols;
	A.n = n;
	A.policy = d_policy_logits;
	A.value = d_value_logits;
	A.q = d_q_logits;
	A.policy_target = d_policy_target;
	A.value_target = d_value_target;
	A.q_target = d_q_target;
	A.policy_scale = policy_scale;
	A.value_scale = value_scale;
	A.q_scale = q_scale;
	A.policy_grad = d_policy_grad;
	A.value_grad = d_value_grad;
	A.q_grad = d_q_grad;
	A.scores = d_sample_scores;
	A.q_weight = d_q_weight;
	if (d_q_weight != nullptr)
		hipLaunchKernelGGL(agx::k_head_loss<true>, dim3(std::min(n, agx::LOSS_MAX_WAVES)), dim3(64), 0, stream, A);
	else
		hipLaunchKernelGGL(agx::k_head_loss<false>, dim3(std::min(n, agx::LOSS_MAX_WAVES)), dim3(64), 0, stream, A);
	return agx::add_sample_scores(n, d_sample_scores, d_total, stream);
}

} /* extern "C" */
