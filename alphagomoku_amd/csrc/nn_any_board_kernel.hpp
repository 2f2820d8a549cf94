/*
 * nn_any_board_kernel.hpp — the policy/value towers for any board with 5 <= rows, cols <= 20 (rows and cols independent), gfx950 (CDNA4): the residual
 * networks (ResnetPV / PVraw / PVQ) and the bottleneck networks (BottleneckPV / BottleneckPVraw / BottleneckPVQ, networks.cpp:170-361 of the
 * reference) in ONE kernel frame with the block as the only seam.
 *
 * nn_forward.hip carries a kernel per board (15x15, 20x20) with the shape as a template parameter.  This file is the general one: the board
 * shape is a kernel ARGUMENT (struct Shape), compile-time are the filter count, the block kind and the head / input variants: twelve instantiations.
 * The kernel template is this ONE text; its instantiations are made in two translation units, one per block kind (nn_any_board.hip: RESIDUAL and
 * agx_any::launch(); nn_any_board_bottleneck.hip: BOTTLENECK).  In one module hipcc gives the six bottleneck instantiations another instruction
 * order — the same optimised IR but for the place of one hoisted address — that is 0.4 - 0.8 % slower on 15x15 (profiles/nn_one_frame.txt); alone
 * in their module they are, instruction for instruction, what they were as a file of their own.
 *
 *   - Persistent grid, optional slot list with the count read on the device.  One workgroup (8 waves) carries a board through the whole network in
 *     ONE activation plane in LDS, computed in place: a layer's outputs stay in accumulators until every wave has read the plane.  The plane is
 *     sized for the largest board (20x20: 477 positions), so every shape fits.
 *   - Row stride S = cols + 1, one spare row above and below, the spare column / rows / the last tile's overhang kept at zero: a 3x3 tap is
 *     the offset dy * S + dx in the flattened position index.  Tiles are 16 consecutive positions; NT = ceil(rows * S / 16) of them.
 *   - The wave layout follows the OUTPUT width M of a layer (Lay<M>): M / 32 channel groups of two 16-channel tiles, 8 / (M / 32) position groups,
 *     the tiles dealt to the position groups in runs of ceil(NT / PG).  M = 128: 4 x 2 (14 accumulator tiles per wave), 64: 2 x 4 (7), 32: 1 x 8 (4);
 *     the accumulators are sized for 20x20, tiles a shape does not have are skipped by wave-uniform branches.
 *   - The k-loop is tap-major with the activation fragments of all tiles of a wave read per (tap, 32-channel chunk): a tile is 16 positions = a
 *     whole period of the XOR chunk swizzle, so every LDS address is one per-lane base per tap + an immediate.  Nothing in the loop divides: the
 *     only run-time divisions by S (cell of a position: the on-board mask, the input conv's plane index) are a multiply and a shift (Shape::magic).
 *   - The blocks.  RESIDUAL: x = relu(x + W2 * relu(W1 * x + b1) + b2), both 3x3, F -> F.  BOTTLENECK (createBottleneckBlock_v3, blocks.cpp:84-97):
 *         y = relu(W1 . x + b1)   1x1, F -> F/2        y = relu(W2 * y + b2)   3x3, F/2 -> F/2        x = relu(x + W3 * y + b3)   3x3, F/2 -> F
 *     The half-width activations keep the full-width position stride and use the first F/2 channels of a position (chunks 0 .. F/16 - 1 before
 *     the swizzle): the halo positions of the 3x3 taps are never written and stay the zeros they are, the stale upper channels are never read.
 *   - The block input x waits in a per-workgroup global scratch, in the accumulator layout of the full-width layers, written and read by the same
 *     lane: written by the input block / a block's last convolution, requested by the layer in front of the last one behind its k-loop, added to
 *     the bias when the last one's accumulators start.
 *   - mfma_settle() (nn_device.hpp) stands behind every tile loop.
 *   - Every reduction order is fixed by the shape alone: results do not depend on grid, batch, slot list or launch width.
 *
 * Numerics: fp16 weights for everything that feeds the matrix cores, fp32 accumulation from the bias (+ the residual), one rounding to fp16
 * per stored activation behind the ReLU, the last 1x1 of policy / q and all biases in fp32, q's hidden activation tanh rounded to fp16.
 * The value head's dense layers run in value_head_kernel (nn_device.hpp) behind the tower (agx_res::launch, nn_forward.hip), K = 4 * rows * cols padded to 32.
 * The types, the launch record and the helpers shared with nn_forward.hip are in nn_device.hpp.
 *
 * Slower per FLOP than the two specialised kernels (DESIGN.md 3.1 has the measured ratios): no row- or column-stationary reuse of
 * activation fragments, one fragment read per (tap, tile) for two MFMAs.
 */
#ifndef AGX_NN_ANY_BOARD_KERNEL_HPP_
#define AGX_NN_ANY_BOARD_KERNEL_HPP_

#include "nn_device.hpp"
#include "nn_any_board.hpp"

#include <cmath>

namespace
{
	using agx_any::RESIDUAL;
	using agx_any::BOTTLENECK;

	struct Shape
	{
			int rows, cols;
			int S;        // row stride in positions: cols + 1
			int NT;       // 16-position tiles of the output: ceil(rows * S / 16)
			int ntw;      // tiles per position group of a full-width layer: ceil(NT / Lay<F>::PG)
			int ntw_h;    // of a half-width layer: ceil(NT / Lay<F / 2>::PG) (read by the bottleneck instantiations only)
			int HW;
			int kpad;     // value-head dense input length (agx_res::Net::kpad()): 4 HW rounded up to 32
			int plane16;  // 16-byte units of the activation plane: (1 + S + NT * 16 + S + 2) positions
			int S5;       // row stride of the padded input plane: S + 4
			int npos5;    // its positions: (rows + 4) * S5 + 4
			int magic;    // position / S == (position * magic) >> 16 for every position of a plane (65536 / S + 1: exact below 65536 / S)
	};

	constexpr int NT_MAX = (agx_any::MAX_SIDE * (agx_any::MAX_SIDE + 1) + 15) / 16; // 27

	/* the activation plane of a network with F filters */
	template<int F>
	struct Cfg
	{
			static_assert(F == 64 || F == 128, "filters");
			static constexpr int CH = F / 8;                        // 16-byte chunks per position
			static constexpr int PPR_SHIFT = (F == 128) ? 0 : 1;    // log2 of the positions per 256-byte bank row
			static constexpr int KC = F / 32;
			static constexpr int NPOS_MAX = 1 + (agx_any::MAX_SIDE + 1) + NT_MAX * 16 + (agx_any::MAX_SIDE + 1) + 2; // 477
			static constexpr int POS_BYTES = F * 2;
			static constexpr int PLANE_MAX = NPOS_MAX * POS_BYTES;
			static constexpr int NPOS5_MAX = (agx_any::MAX_SIDE + 4) * (agx_any::MAX_SIDE + 5) + 4;
			static_assert(NPOS5_MAX * 64 <= PLANE_MAX, "the padded input plane of every shape lies inside the plane area");
			static constexpr int PS = NT_MAX * 16;                  // stride of the heads' partial-sum rows
			static constexpr int THREADS = 512;
			// plane + value conv1x1 fragments [KC][64] half8 + reduction scratch + wp2 [F] + wq2 [F][4] + policy partial sums [F / 32][PS] + q sums [3][PS]
			static constexpr int LDS_BYTES = PLANE_MAX + KC * 64 * 16 + (8 + 8) * 4 + F * 4 + F * 16 + (F / 32) * PS * 4 + 3 * PS * 4;
			static_assert(LDS_BYTES <= 163840, "does not fit in LDS");
			__device__ static __forceinline__ int offset(int index, int chunk)
			{ // byte offset of a 16-byte chunk of stored position `index` (= position + 1): XOR-swizzled inside the position's bank row
				return index * POS_BYTES + ((chunk ^ ((index >> PPR_SHIFT) & (CH - 1))) * 16);
			}
	};

	/* the wave layout of a layer with M output channels: CG channel groups x PG position groups of the 8 waves, two 16-channel tiles per wave */
	template<int M>
	struct Lay
	{
			static_assert(M == 32 || M == 64 || M == 128, "output channels");
			static constexpr int CG = M / 32;
			static constexpr int CG_SHIFT = (M == 128) ? 2 : ((M == 64) ? 1 : 0);
			static constexpr int PG = 8 / CG;
			static constexpr int MT = 2;
			static constexpr int MTILES = M / 16;
			static constexpr int NTW = (NT_MAX + PG - 1) / PG;      // accumulator tiles of a wave (the largest board's): 14, 7, 4
	};
	template<int F>
	constexpr int SKIP_PER_WG = 8 * Lay<F>::MT * Lay<F>::NTW * 64; // half4 elements of residual scratch per workgroup
	static_assert(Lay<128>::NTW >= Lay<64>::NTW && Lay<64>::NTW >= Lay<32>::NTW,
			"the residual scratch is sized by the full-width layout: only full-width layers save to it, with either block kind");

	/* What the block kind decides beside the block itself, both for the rate alone (profiles/nn_one_frame.txt).  The depth of the weight ring of
	 * a 3x3 k-loop over K input channels; and whether a layer makes the per-lane part of its addresses its own (own(), nn_device.hpp), where the
	 * residual instantiations otherwise keep them as kernel-wide constants in scratch. */
	template<int BLOCK, int K>
	constexpr int RING = (BLOCK == BOTTLENECK) ? 3 : ((K == 128) ? 4 : 2);
	template<int BLOCK>
	constexpr bool OWN = (BLOCK == RESIDUAL);

	/* what a wave owns in a layer: channels [mg * 32, mg * 32 + 32) of tiles n0 .. n0 + count - 1 (wave-uniform, in scalar registers) */
	struct WaveTiles
	{
			int mg, n0, count;
	};
	template<int M>
	__device__ __forceinline__ WaveTiles wave_tiles(const Shape &sh, int ntw, int wave)
	{
		typedef Lay<M> L;
		WaveTiles w;
		w.mg = __builtin_amdgcn_readfirstlane(wave & (L::CG - 1));
		const int first = __builtin_amdgcn_readfirstlane((wave >> L::CG_SHIFT) * ntw);
		const int left = sh.NT - first;
		w.count = (left < 0) ? 0 : ((left < ntw) ? left : ntw);
		w.n0 = (w.count > 0) ? first : 0; // (a wave without tiles computes nothing; its addresses stay inside the plane)
		return w;
	}
	__device__ __forceinline__ int div_stride(const Shape &sh, int position)
	{
		return (position * sh.magic) >> 16;
	}
	/* bit n = this lane's cell of the wave's tile n is on the board */
	__device__ __forceinline__ uint32_t on_board_bits(const Shape &sh, const WaveTiles &wt, int lane)
	{
		uint32_t bits = 0;
		for (int n = 0; n < wt.count; n++)
		{
			const int pos = sh.S + (wt.n0 + n) * 16 + (lane & 15);
			const int y1 = div_stride(sh, pos); // y + 1
			if (pos - y1 * sh.S < sh.cols && y1 - 1 < sh.rows)
				bits |= 1u << n;
		}
		return bits;
	}

	typedef BiasCarry<2> Bias2;
	template<int M>
	__device__ __forceinline__ void request_bias(const float *__restrict__ bias, const WaveTiles &wt, int lane, Bias2 &carry)
	{
#pragma unroll
		for (int i = 0; i < 2; i++)
			carry.b[i] = *reinterpret_cast<const floatx4*>(bias + (wt.mg * 2 + i) * 16 + 4 * (lane >> 4));
	}
	template<int M>
	__device__ __forceinline__ void start_from_bias(const Bias2 &bias, floatx4 (&acc)[2][Lay<M>::NTW])
	{
#pragma unroll
		for (int i = 0; i < 2; i++)
#pragma unroll
			for (int n = 0; n < Lay<M>::NTW; n++)
				acc[i][n] = bias.b[i];
	}
	template<int F>
	struct SkipCarry
	{ // the block input in the accumulator layout of a full-width layer, requested by the layer in front of the block's last one behind its k-loop
			uint2 v[2][Lay<F>::NTW];
	};

	typedef __attribute__((address_space(1))) half4 global_half4;
	template<int F>
	__device__ __forceinline__ global_half4* lane_skip(half4 *skip, int wave, int lane)
	{ // this lane's part of the workgroup's residual scratch [wave][MT][NTW][lane]: scalar base + lane offset (+ immediates)
		return (global_half4*) (skip + __builtin_amdgcn_readfirstlane(wave * Lay<F>::MT * Lay<F>::NTW * 64)) + lane;
	}

	/* the same for one layer: with OWN_ADDR the lane's part of the address is made again, the layer's own; without, the kernel-wide pointer serves */
	template<int F, bool OWN_ADDR>
	__device__ __forceinline__ global_half4* layer_skip(global_half4 *my_skip, half4 *skip, int wave, int lane)
	{
		return OWN_ADDR ? lane_skip<F>(skip, wave, own(lane)) : my_skip;
	}

	/* one k-step (32 input channels of one tap) for all tiles of a wave: activation fragments in groups of at most 8 tiles, two MFMAs each */
	template<int F, int NTW>
	__device__ __forceinline__ void mac_step(const char *chunk_ptr, const half8 (&a)[2], const WaveTiles &wt, floatx4 (&acc)[2][NTW])
	{
		constexpr int TILE_BYTES = 16 * Cfg<F>::POS_BYTES; // a tile further on: whole bank rows, the same swizzle
		constexpr int BG = 8;
#pragma unroll
		for (int g0 = 0; g0 < NTW; g0 += BG)
		{
			if (g0 < wt.count)
			{
				half8 b[BG];
#pragma unroll
				for (int n = 0; n < BG; n++)
					if (g0 + n < NTW)
						b[n] = *reinterpret_cast<const half8*>(chunk_ptr + ((g0 + n < wt.count) ? (g0 + n) : 0) * TILE_BYTES);
				__builtin_amdgcn_iglp_opt(0);
#pragma unroll
				for (int n = 0; n < BG; n++)
					if (g0 + n < NTW && g0 + n < wt.count)
					{
#pragma unroll
						for (int i = 0; i < 2; i++)
							acc[i][g0 + n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[n], acc[i][g0 + n], 0, 0, 0);
					}
			}
		}
	}

	/*
	 * acc += the convolution of the first K channels of the plane (F filters: position stride and swizzle) to M channels, TAPS = 9 (3x3,
	 * tap-major) or 1 (1x1): TAPS * K / 32 k-steps.  3x3: the weight fragments of a k-step are requested RING - 1 steps ahead through a ring
	 * (3 * K / 32 steps per tap row, a multiple of RING: the ring index is static in the unrolled row).  1x1: all K / 32 steps' fragments are
	 * requested at the top.
	 */
	template<int F, int K, int M, int TAPS, int RING = 1>
	__device__ __forceinline__ void conv_mac(const char *src, const half8 *__restrict__ wpk, const Shape &sh, const WaveTiles &wt, int lane,
			floatx4 (&acc)[2][Lay<M>::NTW])
	{
		typedef Cfg<F> C;
		typedef Lay<M> L;
		static_assert(TAPS == 9 || TAPS == 1, "3x3 or 1x1");
		static_assert(K % 32 == 0 && K <= F, "input channels");
		constexpr int KC = K / 32;
		const int r = lane & 15;
		const int q4 = lane >> 4;
		const half8 *wp = wpk + (wt.mg * L::MT) * 64 + lane;
		const int centre = 1 + sh.S + wt.n0 * 16 + r; // stored index of this lane's position in the wave's first tile
		if constexpr (TAPS == 1)
		{
			half8 a[KC][2];
#pragma unroll
			for (int kc = 0; kc < KC; kc++)
#pragma unroll
				for (int i = 0; i < 2; i++)
					a[kc][i] = wp[(kc * L::MTILES + i) * 64];
			const int swz0 = (centre >> C::PPR_SHIFT) & (C::CH - 1);
			const char *src0 = src + centre * C::POS_BYTES;
#pragma unroll
			for (int kc = 0; kc < KC; kc++)
				mac_step<F, L::NTW>(src0 + (((kc * 4 + q4) ^ swz0) * 16), a[kc], wt, acc);
		}
		else
		{
			constexpr int STEPS = 9 * KC, ROW = 3 * KC;
			static_assert(RING >= 2 && ROW % RING == 0, "static ring index inside the unrolled tap row");
			half8 a_ring[RING][2];
#pragma unroll
			for (int u = 0; u < RING - 1; u++)
#pragma unroll
				for (int i = 0; i < 2; i++)
					a_ring[u][i] = wp[(u * L::MTILES + i) * 64];
#pragma unroll 1
			for (int dyi = 0; dyi < 3; dyi++)
			{
				const int row_index = centre + (dyi - 1) * sh.S;
#pragma unroll
				for (int dxi = 0; dxi < 3; dxi++)
				{
					const int index0 = row_index + (dxi - 1);
					const int swz0 = (index0 >> C::PPR_SHIFT) & (C::CH - 1);
					const char *src0 = src + index0 * C::POS_BYTES;
#pragma unroll
					for (int kc = 0; kc < KC; kc++)
					{
						const int s = dxi * KC + kc; // step inside the tap row (compile-time in the unrolled body)
						// (past the layer's end the requests wrap to its own first fragments instead of branching around the fetch)
						const int step = dyi * ROW + s + RING - 1;
						const int ahead = (step < STEPS) ? step : (step - STEPS);
#pragma unroll
						for (int i = 0; i < 2; i++)
							a_ring[(s + RING - 1) % RING][i] = wp[(ahead * L::MTILES + i) * 64];
						mac_step<F, L::NTW>(src0 + (((kc * 4 + q4) ^ swz0) * 16), a_ring[s % RING], wt, acc);
					}
				}
			}
		}
		mfma_settle(acc);
	}

	/*
	 * The epilogue of a block layer with M output channels: ReLU, one rounding to fp16, cells that are not on the board — the spare column, the
	 * last tile's overhang — masked to zero; with SAVE the values are also the next block's input (scratch); behind the barrier (every wave has
	 * consumed the plane) the first M channels of the wave's positions are overwritten.  `fetch` (the layer in front of the block's last one): the
	 * block input is requested for the last layer while the accumulators are dead, in flight through the barrier and the plane write.
	 */
	template<int F, int M, bool SAVE, bool OWN_ADDR>
	__device__ __forceinline__ void store_relu(char *plane, floatx4 (&acc)[2][Lay<M>::NTW], const Shape &sh, const WaveTiles &wt, int lane, uint32_t valid_bits,
			global_half4 *my_skip, SkipCarry<F> *fetch, const WaveTiles *fetch_tiles)
	{
		typedef Cfg<F> C;
		typedef Lay<M> L;
		const int r = lane & 15;
		const int q4 = lane >> 4;
		uint2 out[2][L::NTW];
#pragma unroll
		for (int i = 0; i < 2; i++)
		{
#pragma unroll
			for (int n = 0; n < L::NTW; n++)
			{
				const floatx4 v = acc[i][n];
				half2 lo { static_cast<half_t>(v[0]), static_cast<half_t>(v[1]) }, hi { static_cast<half_t>(v[2]), static_cast<half_t>(v[3]) };
				const half2 zero2 { static_cast<half_t>(0.0f), static_cast<half_t>(0.0f) };
				lo = __builtin_elementwise_max(lo, zero2); // (ReLU after the conversion on packed halves: rounding is monotonic)
				hi = __builtin_elementwise_max(hi, zero2);
				const uint32_t keep = ((valid_bits >> n) & 1u) ? 0xFFFFFFFFu : 0u;
				const uint2 packed { __builtin_bit_cast(uint32_t, lo) & keep, __builtin_bit_cast(uint32_t, hi) & keep };
				out[i][n] = packed;
				if (SAVE && n < wt.count)
					my_skip[(i * L::NTW + n) * 64] = __builtin_bit_cast(half4, packed);
			}
		}
		if (fetch != nullptr)
		{
#pragma unroll
			for (int i = 0; i < 2; i++)
#pragma unroll
				for (int n = 0; n < Lay<F>::NTW; n++)
					fetch->v[i][n] = (n < fetch_tiles->count) ? __builtin_bit_cast(uint2, my_skip[(i * Lay<F>::NTW + n) * 64]) : uint2 { 0u, 0u };
		}
		lds_barrier(); // every wave has consumed the plane: it can be overwritten now
		const int index0 = 1 + sh.S + wt.n0 * 16 + (OWN_ADDR ? own(r) : r);
#pragma unroll
		for (int i = 0; i < 2; i++)
		{
			const int ch = (wt.mg * 2 + i) * 16 + 4 * q4;
			char *out0 = plane + C::offset(index0, ch / 8) + (ch % 8) * 2; // (a tile further on: 16 positions, the same swizzle)
#pragma unroll
			for (int n = 0; n < L::NTW; n++)
				if (n < wt.count)
					*reinterpret_cast<uint2*>(out0 + n * 16 * C::POS_BYTES) = out[i][n];
		}
	}

	/*
	 * A head's 3x3 convolution F -> F over the plane, folded with its 1x1 convolution.
	 * QHEAD false: policy conv + ReLU and the 1x1 F -> 1: per-channel-group partial logits into `ppart` [CG][PS].
	 * QHEAD true: action-values conv + tanh and the 1x1 F -> 3: `ppart` is [3][PS], the channel groups add their partial sums one after the
	 * other (a fixed order: results do not depend on wave timing).  The bias is added behind the k-loop; `next_bias` is requested for the layer
	 * behind this one.
	 * (The head epilogues, the policy softmax and the value head's conv1x1 stand here a second time next to nn_forward.hip's on purpose: written
	 *  once over a tile map, each of them moved the register allocation of the fixed-shape kernels — DESIGN.md 3.1.)
	 */
	template<int F, bool QHEAD, int RING>
	__device__ __forceinline__ void head_layer(const char *plane, const half8 *__restrict__ wpk, Bias2 &bias_carry, const float *__restrict__ next_bias,
			const float *__restrict__ wp2, float *ppart, const Shape &sh, const WaveTiles &wt, int lane)
	{
		typedef Cfg<F> C;
		typedef Lay<F> L;
		const int r = lane & 15;
		const int q4 = lane >> 4;
		floatx4 acc[2][L::NTW];
#pragma unroll
		for (int i = 0; i < 2; i++)
#pragma unroll
			for (int n = 0; n < L::NTW; n++)
				acc[i][n] = floatx4 { 0.0f, 0.0f, 0.0f, 0.0f };
		conv_mac<F, F, F, 9, RING>(plane, wpk, sh, wt, lane, acc);
		const Bias2 bias_now = bias_carry;
		if (next_bias != nullptr)
			request_bias<F>(next_bias, wt, lane, bias_carry);
		const int tile0 = wt.n0 * 16; // position (stride S, 0 = cell (0, 0)) of lane 0's cell in the wave's first tile
		if (QHEAD)
		{
			float part[3][L::NTW];
#pragma unroll
			for (int o = 0; o < 3; o++)
#pragma unroll
				for (int n = 0; n < L::NTW; n++)
					part[o][n] = 0.0f;
#pragma unroll
			for (int i = 0; i < 2; i++)
			{
				const int ch = (wt.mg * 2 + i) * 16 + 4 * q4;
				const floatx4 bv = bias_now.b[i];
#pragma unroll
				for (int n = 0; n < L::NTW; n++)
					if (n < wt.count)
					{
						const floatx4 v = acc[i][n] + bv;
#pragma unroll
						for (int j = 0; j < 4; j++)
						{
							const float t = static_cast<float>(static_cast<half_t>(tanhf(v[j]))); // fp16 like a stored plane
							const floatx4 w = *reinterpret_cast<const floatx4*>(wp2 + (ch + j) * 4);
							part[0][n] += t * w[0];
							part[1][n] += t * w[1];
							part[2][n] += t * w[2];
						}
					}
			}
#pragma unroll
			for (int o = 0; o < 3; o++)
#pragma unroll
				for (int n = 0; n < L::NTW; n++)
				{
					part[o][n] += __shfl_xor(part[o][n], 16);
					part[o][n] += __shfl_xor(part[o][n], 32);
				}
			for (int group = 0; group < L::CG; group++)
			{
				if (wt.mg == group && q4 == 0)
				{
#pragma unroll
					for (int o = 0; o < 3; o++)
#pragma unroll
						for (int n = 0; n < L::NTW; n++)
							if (n < wt.count)
							{
								float *dst = ppart + o * C::PS + tile0 + n * 16 + r;
								*dst = (group == 0) ? part[o][n] : (*dst + part[o][n]);
							}
				}
				__syncthreads();
			}
			return;
		}
		float part[L::NTW];
#pragma unroll
		for (int n = 0; n < L::NTW; n++)
			part[n] = 0.0f;
#pragma unroll
		for (int i = 0; i < 2; i++)
		{
			const int ch = (wt.mg * 2 + i) * 16 + 4 * q4;
			const floatx4 bv = bias_now.b[i];
			const floatx4 wv = *reinterpret_cast<const floatx4*>(wp2 + ch);
#pragma unroll
			for (int n = 0; n < L::NTW; n++)
			{
				const floatx4 v = acc[i][n] + bv;
				// the ReLU output rounded to fp16 before the 1x1 conv, like a stored plane
				part[n] += static_cast<float>(static_cast<half_t>(fmaxf(v[0], 0.0f))) * wv[0];
				part[n] += static_cast<float>(static_cast<half_t>(fmaxf(v[1], 0.0f))) * wv[1];
				part[n] += static_cast<float>(static_cast<half_t>(fmaxf(v[2], 0.0f))) * wv[2];
				part[n] += static_cast<float>(static_cast<half_t>(fmaxf(v[3], 0.0f))) * wv[3];
			}
		}
#pragma unroll
		for (int n = 0; n < L::NTW; n++)
		{
			float s = part[n];
			s += __shfl_xor(s, 16);
			s += __shfl_xor(s, 32);
			if (q4 == 0 && n < wt.count)
				ppart[wt.mg * C::PS + tile0 + n * 16 + r] = s;
		}
	}

	/*
	 * Input block: 5x5 convolution of the bit-unpacked padded input plane `in5` (stride S5; 32 channels: 64 bytes per position,
	 * chunk-swizzled by (index >> 2) & 3; RAW: 8 channels, 16 bytes per position, one k-step = four horizontal taps) + bias + ReLU.
	 * `in5` aliases the plane: the plane is cleared and written behind a barrier; the outputs are also the first block's input (scratch).
	 */
	template<int F, bool RAW, bool OWN_ADDR>
	__device__ __forceinline__ void conv5x5_input(char *plane, const half8 *__restrict__ wpk, const float *__restrict__ bias, global_half4 *my_skip, const Shape &sh,
			const WaveTiles &wt, int wave, int lane, uint32_t valid_bits)
	{
		typedef Cfg<F> C;
		typedef Lay<F> L;
		const int r = OWN_ADDR ? own(lane & 15) : (lane & 15);
		const int q4 = lane >> 4;
		const char *in5 = plane;
		floatx4 acc[2][L::NTW];
#pragma unroll
		for (int i = 0; i < 2; i++)
#pragma unroll
			for (int n = 0; n < L::NTW; n++)
				acc[i][n] = floatx4 { 0.0f, 0.0f, 0.0f, 0.0f };
		// padded-plane index of the (dy = 0, dx = 0) input cell of this lane's position in every tile: with position p = (y + 1) S + x,
		// (y + 2) S5 + (x + 2) = p + S + 4 y + 10
		int q0[L::NTW];
#pragma unroll
		for (int n = 0; n < L::NTW; n++)
		{
			const int pos = sh.S + (wt.n0 + n) * 16 + r;
			q0[n] = pos + sh.S + 4 * (div_stride(sh, pos) - 1) + 10 + (RAW ? q4 : 0);
		}
		constexpr int TAPS = RAW ? 10 : 25; // RAW: k-step t = 2 * dy + column group (dx 0-3, dx 4 + three zero-weight taps)
		const half8 *wp = wpk + (wt.mg * 2) * 64 + lane;
		half8 a_next[2];
#pragma unroll
		for (int i = 0; i < 2; i++)
			a_next[i] = wp[i * 64];
		int dy = -2, step = 0; // t = dy-major; `step` = the tap's column (RAW: column group) inside the row
#pragma unroll 1
		for (int t = 0; t < TAPS; t++)
		{
			const int off = dy * sh.S5 + (RAW ? (4 * step - 2) : (step - 2));
			half8 a[2];
#pragma unroll
			for (int i = 0; i < 2; i++)
				a[i] = a_next[i];
			const int tn = (t + 1 < TAPS) ? (t + 1) : 0;
#pragma unroll
			for (int i = 0; i < 2; i++)
				a_next[i] = wp[(tn * L::MTILES + i) * 64];
#pragma unroll
			for (int n = 0; n < L::NTW; n++)
				if (n < wt.count)
				{
					int q = q0[n] + off;
					q = (q < 0) ? 0 : ((q >= sh.npos5) ? (sh.npos5 - 1) : q); // only dummy positions (and RAW's zero-weight taps) can fall outside
					const half8 b = RAW ? *reinterpret_cast<const half8*>(in5 + q * 16)
							: *reinterpret_cast<const half8*>(in5 + (q * 4 + (q4 ^ ((q >> 2) & 3))) * 16);
#pragma unroll
					for (int i = 0; i < 2; i++)
						acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b, acc[i][n], 0, 0, 0);
				}
			if (++step == (RAW ? 2 : 5))
			{
				step = 0;
				dy++;
			}
		}
		mfma_settle(acc);
		__syncthreads();
		const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
		for (int i = wave * 64 + lane; i < sh.plane16; i += C::THREADS)
			reinterpret_cast<uint4*>(plane)[i] = zero4;
		__syncthreads();
		const int index0 = 1 + sh.S + wt.n0 * 16 + r;
#pragma unroll
		for (int i = 0; i < 2; i++)
		{
			const int ch = (wt.mg * 2 + i) * 16 + 4 * q4;
			const floatx4 bv = *reinterpret_cast<const floatx4*>(bias + ch);
			char *out0 = plane + C::offset(index0, ch / 8) + (ch % 8) * 2;
#pragma unroll
			for (int n = 0; n < L::NTW; n++)
				if (n < wt.count)
				{
					const bool valid = (valid_bits >> n) & 1u;
					const floatx4 v = acc[i][n] + bv;
					half4 o;
					o[0] = static_cast<half_t>(valid ? fmaxf(v[0], 0.0f) : 0.0f);
					o[1] = static_cast<half_t>(valid ? fmaxf(v[1], 0.0f) : 0.0f);
					o[2] = static_cast<half_t>(valid ? fmaxf(v[2], 0.0f) : 0.0f);
					o[3] = static_cast<half_t>(valid ? fmaxf(v[3], 0.0f) : 0.0f);
					*reinterpret_cast<half4*>(out0 + n * 16 * C::POS_BYTES) = o;
					my_skip[(i * L::NTW + n) * 64] = o;
				}
		}
	}

	/* the policy of board `b` from the channel groups' partial logits: bias, softmax over the rows * cols real cells (one per thread) */
	template<int F>
	__device__ __forceinline__ void policy_softmax(const float *ppart, float *red, float bp2, const Shape &sh, int tid, int cell_pos, float *policy, int b)
	{
		float logit = -3.0e38f;
		if (tid < sh.HW)
			logit = bp2 + sum_partial_logits<Lay<F>::CG, Cfg<F>::PS>(ppart, cell_pos);
		const float m = block_reduce_max(logit, red, tid);
		const float e = (tid < sh.HW) ? __expf(logit - m) : 0.0f;
		const float sum = block_reduce_sum(e, red, tid);
		if (tid < sh.HW)
			policy[static_cast<size_t>(b) * sh.HW + tid] = e / sum;
	}

	/* the action values of board `b` from the summed logits `qpart` [3][PS]: bias, softmax over the 3 per cell, (win, draw) stored */
	template<int F>
	__device__ __forceinline__ void q_output(const float *qpart, const NetParams &p, const Shape &sh, int tid, int cell_pos, int b)
	{
		typedef Cfg<F> C;
		if (tid < sh.HW)
		{
			const float z0 = p.bq2[0] + qpart[cell_pos], z1 = p.bq2[1] + qpart[C::PS + cell_pos], z2 = p.bq2[2] + qpart[2 * C::PS + cell_pos];
			const float2 win_draw = softmax3_win_draw(z0, z1, z2);
			float *out = p.q + (static_cast<size_t>(b) * sh.HW + tid) * 2;
			out[0] = win_draw.x;
			out[1] = win_draw.y;
		}
	}

	template<int F, int BLOCK, bool QHEAD, bool RAW>
	__global__ __launch_bounds__(512) void nn_any_board_kernel(NetParams p, Shape sh, const uint32_t *__restrict__ features, float *__restrict__ policy)
	{
		typedef Cfg<F> C;
		constexpr int FH = F / 2;
		constexpr bool OWN_ADDR = OWN<BLOCK>;
		__shared__ __attribute__((aligned(16))) char lds[C::LDS_BYTES];
		char *plane = lds;
		half8 *s_wv1f = reinterpret_cast<half8*>(lds + C::PLANE_MAX);     // [KC][64]: A fragments of the value head's conv1x1 (4 real units of 16)
		float *red = reinterpret_cast<float*>(s_wv1f + C::KC * 64);       // [8] wave partials (+ 8 spare)
		float *s_wp2 = red + 16;                                          // [F] policy-head 1x1 weights
		float *s_wq2 = s_wp2 + F;                                         // [F][4] action-values head 1x1 weights
		float *ppart = s_wq2 + F * 4;                                     // [CG][PS] policy partial logits
		float *qpart = ppart + Lay<F>::CG * C::PS;                        // [3][PS] action-value logits

		const int tid = threadIdx.x;
		const int wave = tid >> 6;
		const int lane = tid & 63;
		// half8 elements of the packed layers: a 3x3 F -> F (a head's conv, a residual block's two), a bottleneck block's W1 (1 tap, F -> F/2),
		// W2 (F/2 -> F/2) and W3 (F/2 -> F); floats of a block's biases
		constexpr int HEAD_H8 = 9 * (F / 32) * (F / 16) * 64;
		constexpr int W1_H8 = (F / 32) * (FH / 16) * 64, W2_H8 = 9 * (FH / 32) * (FH / 16) * 64, W3_H8 = 9 * (FH / 32) * (F / 16) * 64;
		constexpr int BLOCK_H8 = (BLOCK == BOTTLENECK) ? (W1_H8 + W2_H8 + W3_H8) : 2 * HEAD_H8, BLOCK_BIAS = 2 * F;
		const WaveTiles wf = wave_tiles<F>(sh, sh.ntw, wave);     // full-width layers
		const WaveTiles wh = wave_tiles<FH>(sh, sh.ntw_h, wave);  // half-width layers (bottleneck blocks; dead code in the residual instantiations)
		half4 *skip = p.skip + static_cast<size_t>(blockIdx.x) * SKIP_PER_WG<F>;
		global_half4 *my_skip = lane_skip<F>(skip, wave, lane);

		stage_head_weights<F, C::THREADS, QHEAD>(p.wv1, p.wp2, p.wq2, tid, s_wv1f, s_wp2, s_wq2);

		// once per kernel: this thread's cell (one feature word / one policy output per thread) and this lane's on-board masks of the wave's tiles
		const int cell_y = (tid < sh.HW) ? tid / sh.cols : 0, cell_x = (tid < sh.HW) ? tid - cell_y * sh.cols : 0;
		const int cell_q5 = (cell_y + 2) * sh.S5 + (cell_x + 2);   // in the padded input plane
		const int cell_pos = cell_y * sh.S + cell_x;               // position (stride S)
		const uint32_t valid_f = on_board_bits(sh, wf, lane), valid_h = (BLOCK == BOTTLENECK) ? on_board_bits(sh, wh, lane) : 0u;

		const int batch = (p.count_ptr != nullptr) ? min(*p.count_ptr, p.batch) : p.batch;
		uint32_t next_word = 0; // this thread's feature word of the board about to be staged
		if (static_cast<int>(blockIdx.x) < batch && tid < sh.HW)
			next_word = features[static_cast<size_t>((p.slot_list != nullptr) ? p.slot_list[blockIdx.x] : static_cast<int>(blockIdx.x)) * sh.HW + tid];
		const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
		for (int bi = blockIdx.x; bi < batch; bi += gridDim.x)
		{
			const int b = (p.slot_list != nullptr) ? p.slot_list[bi] : bi;
			// ---- stage the bit-unpacked input into the padded plane ----
			__syncthreads();
			for (int i = tid; i < sh.npos5 * (RAW ? 1 : 4); i += C::THREADS)
				reinterpret_cast<uint4*>(plane)[i] = zero4;
			__syncthreads();
			if (tid < sh.HW)
			{
				const uint32_t word = next_word;
				const int q = cell_q5;
#pragma unroll
				for (int k = 0; k < (RAW ? 1 : 4); k++)
				{
					const uint32_t bits = (word >> (8 * k)) & 255u;
					const uint4 v = unpack_feature_byte(bits);
					if (RAW) // the low byte of the word, 16 bytes per position
						*reinterpret_cast<uint4*>(plane + q * 16) = v;
					else
						*reinterpret_cast<uint4*>(plane + (q * 4 + (k ^ ((q >> 2) & 3))) * 16) = v;
				}
			}
			__syncthreads();
			conv5x5_input<F, RAW, OWN_ADDR>(plane, p.w_in, p.bias, layer_skip<F, OWN_ADDR>(my_skip, skip, wave, lane), sh, wf, wave, lane, valid_f);
			Bias2 bias_carry; // the next layer's bias values in that layer's wave layout: requested behind the k-loop of the layer in front of it
			if (BLOCK == BOTTLENECK && p.blocks > 0)
				request_bias<FH>(p.bias + F, wh, lane, bias_carry);
			else
				request_bias<F>(p.bias + F, wf, lane, bias_carry);
			__syncthreads();

			// ---- the blocks ----
			for (int blk = 0; blk < p.blocks; blk++)
			{
				const half8 *w1 = p.w_tower + static_cast<size_t>(blk) * BLOCK_H8, *w2 = w1 + W1_H8, *w3 = w2 + W2_H8; // (w2, w3: bottleneck)
				const float *b1 = p.bias + F + blk * BLOCK_BIAS; // this block's biases, then the next block's (or the policy conv's)
				SkipCarry<F> x;
				if constexpr (BLOCK == RESIDUAL)
				{ // b1 [F], b2 [F]
					{ // 3x3, F -> F
						floatx4 acc[2][Lay<F>::NTW];
						start_from_bias<F>(bias_carry, acc);
						conv_mac<F, F, F, 9, RING<BLOCK, F>>(plane, w1, sh, wf, lane, acc);
						request_bias<F>(b1 + F, wf, lane, bias_carry);
						store_relu<F, F, false, OWN_ADDR>(plane, acc, sh, wf, lane, valid_f, layer_skip<F, OWN_ADDR>(my_skip, skip, wave, lane), &x, &wf);
					}
					lds_barrier();
					{ // 3x3, F -> F, + x
						floatx4 acc[2][Lay<F>::NTW];
#pragma unroll
						for (int i = 0; i < 2; i++)
#pragma unroll
							for (int n = 0; n < Lay<F>::NTW; n++)
								acc[i][n] = bias_plus_residual(x.v[i][n], bias_carry.b[i]);
						conv_mac<F, F, F, 9, RING<BLOCK, F>>(plane, w1 + HEAD_H8, sh, wf, lane, acc);
						request_bias<F>(b1 + 2 * F, wf, lane, bias_carry);
						store_relu<F, F, true, OWN_ADDR>(plane, acc, sh, wf, lane, valid_f, layer_skip<F, OWN_ADDR>(my_skip, skip, wave, lane), nullptr, nullptr);
					}
					lds_barrier();
				}
				else
				{ // b1 [F/2], b2 [F/2], b3 [F]
					{ // 1x1, F -> F/2
						floatx4 acc[2][Lay<FH>::NTW];
						start_from_bias<FH>(bias_carry, acc);
						conv_mac<F, F, FH, 1>(plane, w1, sh, wh, lane, acc);
						request_bias<FH>(b1 + FH, wh, lane, bias_carry);
						store_relu<F, FH, false, OWN_ADDR>(plane, acc, sh, wh, lane, valid_h, my_skip, nullptr, nullptr);
					}
					lds_barrier();
					{ // 3x3, F/2 -> F/2
						floatx4 acc[2][Lay<FH>::NTW];
						start_from_bias<FH>(bias_carry, acc);
						conv_mac<F, FH, FH, 9, RING<BLOCK, FH>>(plane, w2, sh, wh, lane, acc);
						request_bias<F>(b1 + F, wf, lane, bias_carry);
						store_relu<F, FH, false, OWN_ADDR>(plane, acc, sh, wh, lane, valid_h, my_skip, &x, &wf);
					}
					lds_barrier();
					{ // 3x3, F/2 -> F, + x
						floatx4 acc[2][Lay<F>::NTW];
#pragma unroll
						for (int i = 0; i < 2; i++)
#pragma unroll
							for (int n = 0; n < Lay<F>::NTW; n++)
								acc[i][n] = bias_plus_residual(x.v[i][n], bias_carry.b[i]);
						conv_mac<F, FH, F, 9, RING<BLOCK, FH>>(plane, w3, sh, wf, lane, acc);
						if (blk + 1 < p.blocks)
							request_bias<FH>(b1 + 2 * F, wh, lane, bias_carry);
						else
							request_bias<F>(b1 + 2 * F, wf, lane, bias_carry);
						store_relu<F, F, true, OWN_ADDR>(plane, acc, sh, wf, lane, valid_f, layer_skip<F, OWN_ADDR>(my_skip, skip, wave, lane), nullptr, nullptr);
					}
					lds_barrier();
				}
			}
			const half8 *w_heads = p.w_tower + static_cast<size_t>(p.blocks) * BLOCK_H8;
			const float *b_heads = p.bias + F + p.blocks * BLOCK_BIAS;

			// ---- value head, stage 1: conv1x1 F -> 4 + ReLU as one 16 x 16 MFMA tile per 16 positions (4 of the 16 units are real), the tiles dealt
			//      round-robin to the waves; the dense layers run in value_head_kernel (nn_device.hpp) for all boards of the launch ----
			{
				const int r = lane & 15, q4 = lane >> 4;
				for (int n = wave; n < sh.NT; n += C::THREADS / 64)
				{
					floatx4 v[1][1] = { { floatx4 { p.bv1[0], p.bv1[1], p.bv1[2], p.bv1[3] } } };
					const int index0 = 1 + sh.S + n * 16 + r;
#pragma unroll
					for (int kc = 0; kc < C::KC; kc++)
					{
						const half8 bfrag = *reinterpret_cast<const half8*>(plane + C::offset(index0, kc * 4 + q4));
						v[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(s_wv1f[kc * 64 + lane], bfrag, v[0][0], 0, 0, 0);
					}
					mfma_settle(v);
					// lanes with q4 == 0 hold outputs 0 .. 3 of position r of tile n
					const int pos = sh.S + n * 16 + r;
					const int y1 = div_stride(sh, pos);
					const int x = pos - y1 * sh.S, y = y1 - 1;
					if (q4 == 0 && x < sh.cols && y < sh.rows)
					{
						half4 o;
						o[0] = static_cast<half_t>(fmaxf(v[0][0][0], 0.0f));
						o[1] = static_cast<half_t>(fmaxf(v[0][0][1], 0.0f));
						o[2] = static_cast<half_t>(fmaxf(v[0][0][2], 0.0f));
						o[3] = static_cast<half_t>(fmaxf(v[0][0][3], 0.0f));
						*reinterpret_cast<half4*>(p.vhead_x + static_cast<size_t>(bi) * sh.kpad + (y * sh.cols + x) * 4) = o;
					}
				}
			}
			// ---- policy head: conv3x3 + ReLU folded with the conv1x1 F -> 1 ----
			head_layer<F, false, RING<BLOCK, F>>(plane, w_heads, bias_carry, QHEAD ? b_heads + F : nullptr, s_wp2, ppart, sh, wf, lane);
			__syncthreads();
			// the next board's input: requested here, consumed by the staging at the top
			if (bi + static_cast<int>(gridDim.x) < batch && tid < sh.HW)
			{
				const int nb = bi + static_cast<int>(gridDim.x);
				next_word = features[static_cast<size_t>((p.slot_list != nullptr) ? p.slot_list[nb] : nb) * sh.HW + tid];
			}
			policy_softmax<F>(ppart, red, p.bp2, sh, tid, cell_pos, policy, b);
			// ---- action-values head: conv3x3 + tanh, conv1x1 F -> 3 + bias, softmax over the 3 per cell ----
			if (QHEAD)
			{
				__syncthreads(); // the policy head is done with the partial-sum buffers
				head_layer<F, true, RING<BLOCK, F>>(plane, w_heads + HEAD_H8, bias_carry, nullptr, s_wq2, qpart, sh, wf, lane);
				q_output<F>(qpart, p, sh, tid, cell_pos, b);
			}
		}
	}

	Shape make_shape(int rows, int cols, int filters, int kpad)
	{
		const int pg = 8 / (filters / 32), pg_h = 8 / (filters / 64); // Lay<F>::PG, Lay<F / 2>::PG
		Shape sh;
		sh.rows = rows;
		sh.cols = cols;
		sh.S = cols + 1;
		sh.NT = (rows * sh.S + 15) / 16;
		sh.ntw = (sh.NT + pg - 1) / pg;
		sh.ntw_h = (sh.NT + pg_h - 1) / pg_h;
		sh.HW = rows * cols;
		sh.kpad = kpad;
		sh.plane16 = (1 + sh.S + sh.NT * 16 + sh.S + 2) * (filters * 2) / 16;
		sh.S5 = sh.S + 4;
		sh.npos5 = (rows + 4) * sh.S5 + 4;
		sh.magic = 65536 / sh.S + 1;
		return sh;
	}

	/* the six instantiations of one block kind, launched for a record that agx_any::launch() has checked */
	template<int BLOCK>
	int launch_block(const NetParams &p, int rows, int cols, int filters, bool raw, int grid, int kpad, const uint32_t *d_features, float *d_policy, hipStream_t stream)
	{
		const bool qhead = (p.q != nullptr);
		const dim3 g(grid), t(512);
		const Shape sh = make_shape(rows, cols, filters, kpad);
#define AGX_ANY_TOWER(FF, QH, RW) hipLaunchKernelGGL((nn_any_board_kernel<FF, BLOCK, QH, RW>), g, t, 0, stream, p, sh, d_features, d_policy)
#define AGX_ANY_HEADS(FF) do { if (qhead) AGX_ANY_TOWER(FF, true, false); else if (raw) AGX_ANY_TOWER(FF, false, true); else AGX_ANY_TOWER(FF, false, false); } while (0)
		if (filters == 128)
			AGX_ANY_HEADS(128);
		else
			AGX_ANY_HEADS(64);
#undef AGX_ANY_HEADS
#undef AGX_ANY_TOWER
		AGX_HIP_CHECK(hipGetLastError());
		return AGX_OK;
	}
}

namespace agx_any
{
	/* launch_block<BOTTLENECK> (nn_any_board_bottleneck.hip), called by launch() */
	int launch_bottleneck(const agx_nn::NetParams &p, int rows, int cols, int filters, bool raw, int grid, int kpad, const uint32_t *d_features, float *d_policy,
			hipStream_t stream);
}

#endif /* AGX_NN_ANY_BOARD_KERNEL_HPP_ */
