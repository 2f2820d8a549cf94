/*
 * nn_device.hpp — the device code that the network kernel files share: nn_forward.hip (the 15x15 and 20x20 towers, the value head's
 * dense layers, the residual towers' host side), nn_any_board.hip (the run-time-shaped towers, residual and bottleneck blocks) and, for the
 * types and mfma_settle() / own(), nn_convnext.hip; nn_layered.hip (the layered towers) takes the types, the helpers and value_head_kernel.  The vector types, the launch record NetParams, the small
 * helpers of the layers (LDS barrier, MFMA settle, fp16 + fp32 add, carried bias values, workgroup reductions) and the pieces both towers run word for
 * word: the unpacking of a feature byte, the staging of the heads' 1x1 weights, the action-values softmax, the value head's dense kernel.  The functions are in the unnamed
 * namespace and forced inline: each .hip file gets its own copy, exactly as if the text stood there.  The types are in agx_nn: NetParams
 * crosses from one file to the other (agx_any::launch), and a function over a type of the unnamed namespace cannot be linked.
 */
#ifndef AGX_NN_DEVICE_HPP_
#define AGX_NN_DEVICE_HPP_

#include <hip/hip_runtime.h>
#include <cstdint>

namespace agx_nn
{
	typedef _Float16 half_t;
	typedef _Float16 half8 __attribute__((ext_vector_type(8)));
	typedef _Float16 half4 __attribute__((ext_vector_type(4)));
	typedef _Float16 half2 __attribute__((ext_vector_type(2)));
	typedef float floatx4 __attribute__((ext_vector_type(4)));

	/* One launch, filled by agx_res::launch() (nn_forward.hip) and passed by value to the tower kernel that runs — a fixed-shape one or the
	 * run-time-shaped one.  The value head's dense fields (wv2, bv2, wv3, bv3) are read by the host only, for value_head_kernel's launch: they
	 * stay in the record so that the towers' kernel-argument offsets do not move. */
	struct NetParams
	{
			const half8 *w_in;      // packed conv5x5 fragments
			const half8 *w_tower;   // packed 3x3 fragments: 2*blocks layers, then the policy conv
			const float *bias;      // [1 + 2*blocks + 1][F]
			const float *wp2;       // [F]
			const float *wv1;       // [F][4]
			const half_t *wv2;      // value-head dense weights in MFMA A-fragment order [KPAD/32][D/16][lane][8] (value_head_kernel)
			half_t *vhead_x;        // [batch][KPAD]: the value head's conv1x1 output of every board of the launch, input of value_head_kernel
			const float *bv2;       // [D]
			const float *wv3;       // [D][3]
			float bp2;
			float bv1[4];
			float bv3[3];
			int blocks;
			int batch;
			const int *slot_list; // optional: batch element i is slot slot_list[i]
			const int *count_ptr; // optional: batch size read on the device
			const float *wq2;     // [F][4] action-values head 1x1 weights (3 outputs, padded), null without the head
			float bq2[3];
			float *q;             // action values out: float[slots][HW][2] = (win, draw) per cell, null = head not evaluated
			half4 *skip;          // single-plane variants only: residual inputs in accumulator layout, [workgroup][wave][MT][NTW][lane]
	};
}

namespace
{
	using namespace agx_nn;

	/* A workgroup barrier for hand-offs through LDS only: orders (and waits for) this wave's LDS accesses, not its global stores in flight.
	 * __syncthreads() is s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier: in the single-plane kernels every wave reaches the layer barrier right
	 * behind the 2 * NTW global stores of its residual values (read back only by the same lane, a layer later) and would sit there for a
	 * store round trip, twice per residual block. */
	__device__ __forceinline__ void lds_barrier()
	{
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
		__builtin_amdgcn_s_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
	}

	/* A lane index as this use's own value: per-lane addresses made from lane indices the compiler can see are kernel-wide constants to it, computed
	 * once in front of the board loop for every tile of every layer and kept in scratch (hundreds of registers) */
	__device__ __forceinline__ int own(int v)
	{
		asm volatile("" : "+v"(v));
		return v;
	}

	/* Behind a tile loop and in front of the first VALU read of its accumulators.  A wave with fewer tiles than the accumulator
	 * array leaves the loop by a branch straight behind its last MFMA; measured on MI355X with 64 filters on an 8x8 board (one tile per wave), the
	 * epilogue then read the last two registers of the MFMA issued last before they were written: the wait states between an MFMA and a VALU read
	 * of its result are software's to keep, and on that path the pad was one state.  16 states, then every accumulator as an operand of an (empty)
	 * statement behind them, so that no read is scheduled in front of the pad. */
	template<int N>
	__device__ __forceinline__ void mfma_settle(floatx4 (&acc)[N])
	{
		asm volatile("s_nop 15");
#pragma unroll
		for (int n = 0; n < N; n++)
			asm volatile("" : "+v"(acc[n]));
	}
	template<int M, int N>
	__device__ __forceinline__ void mfma_settle(floatx4 (&acc)[M][N])
	{
		asm volatile("s_nop 15");
#pragma unroll
		for (int i = 0; i < M; i++)
#pragma unroll
			for (int n = 0; n < N; n++)
				asm volatile("" : "+v"(acc[i][n]));
	}

	/* (float) one half of a packed pair + addend as ONE instruction: v_fma_mix_f32 widens the fp16 operand itself (h * 1.0 + b rounds once,
	 * exactly like the conversion followed by the add) */
	__device__ __forceinline__ float half_plus_float_lo(uint32_t packed_halves, float addend)
	{
		float d;
		asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(packed_halves), "v"(addend));
		return d;
	}
	__device__ __forceinline__ float half_plus_float_hi(uint32_t packed_halves, float addend)
	{
		float d;
		asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(packed_halves), "v"(addend));
		return d;
	}

	/* A layer's bias values, requested by the layer in front of it behind its k-loop: requested at the layer's own top — straight behind the
	 * layer barrier — every wave of the workgroup waits out an L2 round trip there, per channel tile, with nothing to hide it (the
	 * accumulators start from the bias).  Carried across the epilogue and the barrier only, where the k-loop's weight registers are free. */
	template<int MT>
	struct BiasCarry
	{
			floatx4 b[MT];
	};

	/* maximum / sum over the 8 waves of a workgroup; `red` is [8] floats of LDS.  The partials are combined in a fixed order. */
	__device__ __forceinline__ float block_reduce_max(float v, float *red, int tid)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
			v = fmaxf(v, __shfl_xor(v, o));
		__syncthreads();
		if ((tid & 63) == 0)
			red[tid >> 6] = v;
		__syncthreads();
		return fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
	}
	__device__ __forceinline__ float block_reduce_sum(float v, float *red, int tid)
	{
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
			v += __shfl_xor(v, o);
		__syncthreads();
		if ((tid & 63) == 0)
			red[tid >> 6] = v;
		__syncthreads();
		return ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
	}

	/* ml::unpackInput (AGNetwork.cpp:249-258) for one byte of a cell's feature word: bit j -> channel j as the half 0.0 or 1.0, eight halves */
	__device__ __forceinline__ uint4 unpack_feature_byte(uint32_t bits)
	{
		uint4 v;
		v.x = ((bits & 1u) ? 0x3C00u : 0u) | ((bits & 2u) ? 0x3C000000u : 0u);
		v.y = ((bits & 4u) ? 0x3C00u : 0u) | ((bits & 8u) ? 0x3C000000u : 0u);
		v.z = ((bits & 16u) ? 0x3C00u : 0u) | ((bits & 32u) ? 0x3C000000u : 0u);
		v.w = ((bits & 64u) ? 0x3C00u : 0u) | ((bits & 128u) ? 0x3C000000u : 0u);
		return v;
	}

	/* The heads' 1x1 weights into LDS, once per kernel: the F x 4 value-head conv1x1 (wv1 is [F][4] fp32) as MFMA A fragments
	 * s_wv1f [F / 32][64] — lane l = unit (l & 15) (4 real, 12 zero), inputs kc * 32 + 8 * (l >> 4) .. + 7 —, the policy head's s_wp2 [F] and,
	 * with the action-values head, s_wq2 [F][4].  (The three pointers, not the launch record: handed the record by reference the 20x20 and the
	 * action-values towers came out with other register allocations.) */
	template<int F, int THREADS, bool QHEAD>
	__device__ __forceinline__ void stage_head_weights(const float *wv1, const float *wp2, const float *wq2, int tid, half8 *s_wv1f, float *s_wp2, float *s_wq2)
	{
		for (int i = tid; i < (F / 32) * 64; i += THREADS)
		{
			const int kc = i / 64, l = i % 64, unit = l & 15;
			half8 f;
#pragma unroll
			for (int j = 0; j < 8; j++)
				f[j] = static_cast<half_t>((unit < 4) ? wv1[(kc * 32 + 8 * (l >> 4) + j) * 4 + unit] : 0.0f);
			s_wv1f[i] = f;
		}
		for (int i = tid; i < F; i += THREADS)
			s_wp2[i] = wp2[i];
		if (QHEAD)
			for (int i = tid; i < F * 4; i += THREADS)
				s_wq2[i] = wq2[i];
	}

	/* softmax over the three logits (win, draw, loss) of the action-values head (blocks.cpp:119-127): win and draw, the two that are stored */
	__device__ __forceinline__ float2 softmax3_win_draw(float z0, float z1, float z2)
	{
		const float m = fmaxf(z0, fmaxf(z1, z2));
		const float e0 = __expf(z0 - m), e1 = __expf(z1 - m), e2 = __expf(z2 - m);
		const float inv = 1.0f / (e0 + e1 + e2);
		return make_float2(e0 * inv, e1 * inv);
	}

	/* bias + (float) residual, four values of a lane: the packed halves of `residual` widened and added to `bias` */
	__device__ __forceinline__ floatx4 bias_plus_residual(uint2 residual, floatx4 bias)
	{
		floatx4 v;
		v[0] = half_plus_float_lo(residual.x, bias[0]);
		v[1] = half_plus_float_hi(residual.x, bias[1]);
		v[2] = half_plus_float_lo(residual.y, bias[2]);
		v[3] = half_plus_float_hi(residual.y, bias[3]);
		return v;
	}

	/* a cell's policy logit from the channel groups' partial sums `ppart` [CG][PS], added in a fixed order */
	template<int CG, int PS>
	__device__ __forceinline__ float sum_partial_logits(const float *ppart, int idx)
	{
		static_assert(CG == 8 || CG == 4 || CG == 2, "channel groups");
		if constexpr (CG == 8)
			return ((ppart[idx] + ppart[PS + idx]) + (ppart[2 * PS + idx] + ppart[3 * PS + idx]))
					+ ((ppart[4 * PS + idx] + ppart[5 * PS + idx]) + (ppart[6 * PS + idx] + ppart[7 * PS + idx]));
		else if constexpr (CG == 4)
			return (ppart[idx] + ppart[PS + idx]) + (ppart[2 * PS + idx] + ppart[3 * PS + idx]);
		else
			return ppart[idx] + ppart[PS + idx];
	}

	/*
	 * Value head behind the tower, for every board of a launch: hidden = ReLU(W2^T x + b2) (4 HW -> D), out = softmax(W3^T hidden + b3)
	 * (createValueHead, blocks.cpp:108-118).  One workgroup = 16 boards (one MFMA position tile) x all D hidden units: wave w owns the
	 * 16-unit tiles w * D/64 .. and walks K in 32-input steps (weights pre-packed in A-fragment order: pack_value_dense, nn_pack.hpp; the
	 * boards' inputs are rows of kpad halves: value_kpad()).  3.1 GFLOP for a whole self-play batch — microseconds.  The one kernel behind every
	 * tower — the fixed-shape ones, the run-time-shaped one and the layered one (nn_layered.hip): the input length is an argument.
	 */
	template<int D>
	__global__ __launch_bounds__(256) void value_head_kernel(const half_t *__restrict__ x, const half8 *__restrict__ w2, const float *__restrict__ b2,
			const float *__restrict__ w3, float b30, float b31, float b32, const int *__restrict__ slot_list, const int *__restrict__ count_ptr, int batch_cap,
			int kpad, float *__restrict__ value)
	{
		constexpr int MTW = D / 64; // 16-unit tiles per wave
		__shared__ float hid[16][D + 1];
		const int batch = (count_ptr != nullptr) ? min(*count_ptr, batch_cap) : batch_cap;
		const int b0 = blockIdx.x * 16;
		if (b0 >= batch)
			return;
		const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q4 = lane >> 4;
		const int board = min(b0 + r, batch - 1); // the tail tile repeats the last board (never stored)
		floatx4 acc[MTW];
#pragma unroll
		for (int i = 0; i < MTW; i++)
			acc[i] = floatx4 { 0.0f, 0.0f, 0.0f, 0.0f };
		const half8 *xb = reinterpret_cast<const half8*>(x + static_cast<size_t>(board) * kpad) + q4;
		const half8 *wp = w2 + (wave * MTW) * 64 + lane;
		const int ksteps = kpad / 32;
		for (int kc = 0; kc < ksteps; kc++)
		{
			const half8 bfrag = xb[kc * 4];
#pragma unroll
			for (int i = 0; i < MTW; i++)
				acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wp[(kc * (D / 16) + i) * 64], bfrag, acc[i], 0, 0, 0);
		}
		// lane holds hidden units 4 * q4 .. + 3 of tile i for board r
#pragma unroll
		for (int i = 0; i < MTW; i++)
		{
			const int u = (wave * MTW + i) * 16 + 4 * q4;
#pragma unroll
			for (int e = 0; e < 4; e++)
				hid[r][u + e] = fmaxf(acc[i][e] + b2[u + e], 0.0f);
		}
		__syncthreads();
		// 16 boards x 3 outputs: threads 0 .. 47 each reduce one (board, output) pair in a fixed order
		__shared__ float logits[16][3];
		if (tid < 48)
		{
			const int bb = tid / 3, o = tid % 3;
			float sacc = 0.0f;
			for (int j = 0; j < D; j++)
				sacc += hid[bb][j] * w3[j * 3 + o];
			logits[bb][o] = sacc + ((o == 0) ? b30 : ((o == 1) ? b31 : b32));
		}
		__syncthreads();
		if (tid < 16 && b0 + tid < batch)
		{
			const int bi = b0 + tid;
			const int slot = (slot_list != nullptr) ? slot_list[bi] : bi;
			const float z0 = logits[tid][0], z1 = logits[tid][1], z2 = logits[tid][2];
			const float m = fmaxf(z0, fmaxf(z1, z2));
			const float e0 = __expf(z0 - m), e1 = __expf(z1 - m), e2 = __expf(z2 - m);
			const float inv = 1.0f / (e0 + e1 + e2);
			value[static_cast<size_t>(slot) * 3 + 0] = e0 * inv;
			value[static_cast<size_t>(slot) * 3 + 1] = e1 * inv;
			value[static_cast<size_t>(slot) * 3 + 2] = e2 * inv;
		}
	}
}

#endif /* AGX_NN_DEVICE_HPP_ */
