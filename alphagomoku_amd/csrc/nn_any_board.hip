/*
 * nn_any_board.hip — the policy/value tower for any board with 5 <= rows, cols <= 20 (rows and cols independent), gfx950 (CDNA4).
 *
 * nn_forward.hip carries a kernel per board (15x15, 20x20) with the shape as a template parameter: row tiles, column tiles, two planes
 * or one.  This file is the general one: the board shape is a kernel ARGUMENT (struct Shape), only what the MFMA tiling needs is
 * compile-time — the filter count and the head / input variants — so every shape runs one of six instantiations.
 *
 *   - One workgroup (8 waves) carries a board through the whole tower in ONE activation plane in LDS, computed in place: a layer's
 *     outputs stay in accumulators until every wave has read the plane (the path Geometry<64, 20, 20> takes in nn_forward.hip).
 *     The plane is sized for the largest board (20x20: 477 positions), so every shape fits.
 *   - Row stride S = cols + 1, one spare row above and below, the spare column / rows / the last tile's overhang kept at zero: a 3x3 tap is
 *     the offset dy * S + dx in the flattened position index.  Tiles are 16 consecutive positions; NT = ceil(rows * S / 16) of them,
 *     dealt to the PG position groups of the waves in runs of ceil(NT / PG) (a wave's accumulators are sized for 20x20, tiles a shape does
 *     not have are skipped by wave-uniform branches).
 *   - The k-loop is tap-major with the activation fragments of all tiles of a wave read per (tap, 32-channel chunk): a tile is 16
 *     positions = a whole period of the XOR chunk swizzle, so every LDS address is one per-lane base per tap + an immediate.  Nothing in
 *     the loop divides: the only run-time divisions by S (cell of a position: the epilogue's mask, the input conv's plane index) are a
 *     multiply and a shift (Shape::magic), a few times per lane and board.
 *   - Residual values through a per-workgroup global scratch, written and read by the same lane (conv3x3_inplace of nn_forward.hip).
 *   - The value head's dense layers are not launched here: agx_res::launch() (nn_forward.hip) runs value_head_kernel behind the tower for all
 *     boards of the launch, K = 4 * rows * cols padded to 32 (agx_res::Net::kpad(), handed to launch() for the row stride of NetParams::vhead_x).
 *   - The types, the launch record and the helpers shared with nn_forward.hip are in nn_device.hpp.
 *
 * Slower per FLOP than the two specialised kernels (DESIGN.md 3.1 has the measured ratios): no row- or column-stationary reuse of
 * activation fragments, one fragment read per (tap, tile) for MT = 2 MFMAs.
 */
#include "nn_device.hpp"
#include "nn_any_board.hpp"

#include <cmath>

namespace
{
	struct Shape
	{
			int rows, cols;
			int S;        // row stride in positions: cols + 1
			int NT;       // 16-position tiles of the output: ceil(rows * S / 16)
			int ntw;      // tiles per position group: ceil(NT / PG)
			int HW;
			int kpad;     // value-head dense input length (the host's agx_res::Net::kpad()): 4 HW rounded up to 32
			int plane16;  // 16-byte units of the activation plane: (1 + S + NT * 16 + S + 2) positions
			int S5;       // row stride of the padded input plane: S + 4
			int npos5;    // its positions: (rows + 4) * S5 + 4
			int magic;    // position / S == (position * magic) >> 16 for every position of a plane (65536 / S + 1: exact below 65536 / S)
	};

	template<int F>
	struct Cfg
	{
			static_assert(F == 64 || F == 128, "filters");
			static constexpr int CH = F / 8;                        // 16-byte chunks per position
			static constexpr int PPR_SHIFT = (F == 128) ? 0 : 1;    // log2 of the positions per 256-byte bank row
			static constexpr int CG = (F >= 128) ? 4 : 2;           // channel groups x position groups of the 8 waves (Geometry of nn_forward.hip: 4 x 2, 2 x 4)
			static constexpr int CG_SHIFT = (F >= 128) ? 2 : 1;
			static constexpr int PG = 8 / CG;
			static constexpr int MT = F / (16 * CG);                // 16-channel output tiles per wave
			static constexpr int MTILES = F / 16;
			static constexpr int KC = F / 32;                       // k-steps per tap
			static constexpr int D = (2 * F < 256) ? 2 * F : 256;
			static constexpr int NT_MAX = (agx_any::MAX_SIDE * (agx_any::MAX_SIDE + 1) + 15) / 16;                 // 27
			static constexpr int NTW = (NT_MAX + PG - 1) / PG;      // accumulator tiles of a wave (the largest board's)
			static constexpr int NPOS_MAX = 1 + (agx_any::MAX_SIDE + 1) + NT_MAX * 16 + (agx_any::MAX_SIDE + 1) + 2; // 477
			static constexpr int POS_BYTES = F * 2;
			static constexpr int PLANE_MAX = NPOS_MAX * POS_BYTES;
			static constexpr int NPOS5_MAX = (agx_any::MAX_SIDE + 4) * (agx_any::MAX_SIDE + 5) + 4;
			static_assert(NPOS5_MAX * 64 <= PLANE_MAX, "the padded input plane of every shape lies inside the plane area");
			static constexpr int PS = NT_MAX * 16;                  // stride of the heads' partial-sum rows
			static constexpr int THREADS = 512;
			static constexpr int SKIP_PER_WG = 8 * MT * NTW * 64;   // half4 elements of residual scratch per workgroup
			// plane + value conv1x1 fragments [KC][64] half8 + reduction scratch + wp2 [F] + wq2 [F][4] + policy partial sums [CG][PS] + q sums [3][PS]
			static constexpr int LDS_BYTES = PLANE_MAX + KC * 64 * 16 + (8 + 8) * 4 + F * 4 + F * 16 + CG * PS * 4 + 3 * PS * 4;
			static_assert(LDS_BYTES <= 163840, "does not fit in LDS");
			__device__ static __forceinline__ int offset(int index, int chunk)
			{ // byte offset of a 16-byte chunk of stored position `index` (= position + 1): XOR-swizzled inside the position's bank row
				return index * POS_BYTES + ((chunk ^ ((index >> PPR_SHIFT) & (CH - 1))) * 16);
			}
	};

	/* what a wave owns: channels [mg * 16 * MT, (mg + 1) * 16 * MT) of tiles n0 .. n0 + count - 1 (wave-uniform, in scalar registers) */
	struct WaveTiles
	{
			int mg, n0, count;
	};
	template<int F>
	__device__ __forceinline__ WaveTiles wave_tiles(const Shape &sh, int wave)
	{
		typedef Cfg<F> C;
		WaveTiles w;
		w.mg = __builtin_amdgcn_readfirstlane(wave & (C::CG - 1));
		const int first = __builtin_amdgcn_readfirstlane((wave >> C::CG_SHIFT) * sh.ntw);
		const int left = sh.NT - first;
		w.count = (left < 0) ? 0 : ((left < sh.ntw) ? left : sh.ntw);
		w.n0 = (w.count > 0) ? first : 0; // (a wave without tiles computes nothing; its addresses stay inside the plane)
		return w;
	}
	__device__ __forceinline__ int div_stride(const Shape &sh, int position)
	{
		return (position * sh.magic) >> 16;
	}

	template<int F>
	struct SkipCarry
	{ // the residual input of a block's second layer, requested by its first layer behind its k-loop
			uint2 v[Cfg<F>::MT][Cfg<F>::NTW];
	};
	template<int F>
	__device__ __forceinline__ void request_bias(const float *__restrict__ bias, const WaveTiles &wt, int lane, BiasCarry<Cfg<F>::MT> &carry)
	{
#pragma unroll
		for (int i = 0; i < Cfg<F>::MT; i++)
			carry.b[i] = *reinterpret_cast<const floatx4*>(bias + (wt.mg * Cfg<F>::MT + i) * 16 + 4 * (lane >> 4));
	}

	/*
	 * acc += the 3x3 convolution of the plane, tap-major: 9 * KC k-steps (one = 32 input channels of one tap), the weight fragments
	 * of a k-step requested RING - 1 steps ahead, the activation fragments of a step in groups of at most 8 tiles.
	 */
	template<int F>
	__device__ __forceinline__ void conv3x3_mac(const char *src, const half8 *__restrict__ wpk, const Shape &sh, const WaveTiles &wt, int lane,
			floatx4 (&acc)[Cfg<F>::MT][Cfg<F>::NTW])
	{
		typedef Cfg<F> C;
		const int r = lane & 15;
		const int q4 = lane >> 4;
		constexpr int STEPS = 9 * C::KC;
		constexpr int RING = (C::KC == 4) ? 4 : 2;
		static_assert(C::KC % RING == 0, "static ring index inside the unrolled k loop");
		constexpr int TILE_BYTES = 16 * C::POS_BYTES; // a tile further on: whole bank rows, the same swizzle
		const half8 *wp = wpk + (wt.mg * C::MT) * 64 + lane;
		half8 a_ring[RING][C::MT];
#pragma unroll
		for (int u = 0; u < RING - 1; u++)
#pragma unroll
			for (int i = 0; i < C::MT; i++)
				a_ring[u][i] = wp[(u * C::MTILES + i) * 64];
		const int centre = 1 + sh.S + wt.n0 * 16 + r; // stored index of this lane's position in the wave's first tile
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
				for (int kc = 0; kc < C::KC; kc++)
				{
					// (past the layer's end the requests wrap to its own first fragments instead of branching around the fetch)
					const int step = (dyi * 3 + dxi) * C::KC + kc + RING - 1;
					const int ahead = (step < STEPS) ? step : (step - STEPS);
#pragma unroll
					for (int i = 0; i < C::MT; i++)
						a_ring[(kc + RING - 1) % RING][i] = wp[(ahead * C::MTILES + i) * 64];
					const char *chunk_ptr = src0 + (((kc * 4 + q4) ^ swz0) * 16);
					constexpr int BG = 8;
#pragma unroll
					for (int g0 = 0; g0 < C::NTW; g0 += BG)
					{
						if (g0 < wt.count)
						{
							half8 b[BG];
#pragma unroll
							for (int n = 0; n < BG; n++)
								if (g0 + n < C::NTW)
									b[n] = *reinterpret_cast<const half8*>(chunk_ptr + ((g0 + n < wt.count) ? (g0 + n) : 0) * TILE_BYTES);
							__builtin_amdgcn_iglp_opt(0);
#pragma unroll
							for (int n = 0; n < BG; n++)
								if (g0 + n < C::NTW && g0 + n < wt.count)
								{
#pragma unroll
									for (int i = 0; i < C::MT; i++)
										acc[i][g0 + n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_ring[kc % RING][i], b[n], acc[i][g0 + n], 0, 0, 0);
								}
						}
					}
				}
			}
		}
	}

	/*
	 * One 3x3 layer over its own input (conv3x3_inplace of nn_forward.hip).
	 * MODE 0: first conv of a block (ReLU)   MODE 1: second conv (+ skip, ReLU, new skip saved)
	 * MODE 2: policy conv + ReLU folded with the 1x1 policy conv: per-channel-group partial logits into `ppart` [CG][PS]
	 * MODE 3: action-values conv + tanh folded with its 1x1 conv to 3 outputs: `ppart` is [3][PS], the channel groups add their
	 *         partial sums one after the other (a fixed order: results do not depend on wave timing).
	 * valid_bits: bit n = this lane's cell of the wave's tile n is on the board.
	 * (The head epilogues of modes 2 and 3, the policy softmax and the value head's conv1x1 stand here a second time on purpose: written once
	 *  over a tile map, each of them moved the register allocation of the fixed-shape kernels — DESIGN.md 3.1.)
	 */
	template<int F, int MODE>
	__device__ __forceinline__ void conv3x3_layer(char *plane, const half8 *__restrict__ wpk, BiasCarry<Cfg<F>::MT> &bias_carry, const float *__restrict__ next_bias,
			half4 *skip, const float *__restrict__ wp2, float *ppart, const Shape &sh, const WaveTiles &wt, int wave, int lane, uint32_t valid_bits,
			SkipCarry<F> *skip_carry = nullptr)
	{
		typedef Cfg<F> C;
		const int r = lane & 15;
		const int q4 = lane >> 4;
		floatx4 acc[C::MT][C::NTW];
		typedef __attribute__((address_space(1))) half4 global_half4;
		int skip_lane = lane;
		asm volatile("" : "+v"(skip_lane)); // (the lane's part of the scratch addresses is this layer's own: scalar base + lane offset + immediates)
		global_half4 *my_skip = (global_half4*) (skip + __builtin_amdgcn_readfirstlane(wave * C::MT * C::NTW * 64)) + skip_lane;
#pragma unroll
		for (int i = 0; i < C::MT; i++)
		{ // modes 0 and 1: the accumulators start from bias (+ the residual input)
			const floatx4 bv = (MODE == 0 || MODE == 1) ? bias_carry.b[i] : floatx4 { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
			{
				floatx4 v = bv;
				if (MODE == 1)
				{
					const uint2 sk = skip_carry->v[i][n];
					v = bias_plus_residual(sk, bv);
				}
				acc[i][n] = v;
			}
		}
		conv3x3_mac<F>(plane, wpk, sh, wt, lane, acc);
		const BiasCarry<C::MT> bias_now = bias_carry; // (modes 2 and 3 add the bias behind the k-loop)
		if (next_bias != nullptr)
			request_bias<F>(next_bias, wt, lane, bias_carry);
		const int tile0 = wt.n0 * 16; // position (stride S, 0 = cell (0, 0)) of lane 0's cell in the wave's first tile

		if (MODE == 3)
		{
			float part[3][C::NTW];
#pragma unroll
			for (int o = 0; o < 3; o++)
#pragma unroll
				for (int n = 0; n < C::NTW; n++)
					part[o][n] = 0.0f;
#pragma unroll
			for (int i = 0; i < C::MT; i++)
			{
				const int ch = (wt.mg * C::MT + i) * 16 + 4 * q4;
				const floatx4 bv = bias_now.b[i];
#pragma unroll
				for (int n = 0; n < C::NTW; n++)
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
				for (int n = 0; n < C::NTW; n++)
				{
					part[o][n] += __shfl_xor(part[o][n], 16);
					part[o][n] += __shfl_xor(part[o][n], 32);
				}
			for (int group = 0; group < C::CG; group++)
			{
				if (wt.mg == group && q4 == 0)
				{
#pragma unroll
					for (int o = 0; o < 3; o++)
#pragma unroll
						for (int n = 0; n < C::NTW; n++)
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
		if (MODE == 2)
		{
			float part[C::NTW];
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
				part[n] = 0.0f;
#pragma unroll
			for (int i = 0; i < C::MT; i++)
			{
				const int ch = (wt.mg * C::MT + i) * 16 + 4 * q4;
				const floatx4 bv = bias_now.b[i];
				const floatx4 wv = *reinterpret_cast<const floatx4*>(wp2 + ch);
#pragma unroll
				for (int n = 0; n < C::NTW; n++)
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
			for (int n = 0; n < C::NTW; n++)
			{
				float s = part[n];
				s += __shfl_xor(s, 16);
				s += __shfl_xor(s, 32);
				if (q4 == 0 && n < wt.count)
					ppart[wt.mg * C::PS + tile0 + n * 16 + r] = s;
			}
			return;
		}

		// ReLU after the conversion on packed halves (rounding is monotonic); cells that are not on the board — the spare column, the last
		// tile's overhang — are masked to zero by an AND
		uint2 out[C::MT][C::NTW];
#pragma unroll
		for (int i = 0; i < C::MT; i++)
		{
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
			{
				const floatx4 v = acc[i][n];
				half2 lo { static_cast<half_t>(v[0]), static_cast<half_t>(v[1]) }, hi { static_cast<half_t>(v[2]), static_cast<half_t>(v[3]) };
				const half2 zero2 { static_cast<half_t>(0.0f), static_cast<half_t>(0.0f) };
				lo = __builtin_elementwise_max(lo, zero2);
				hi = __builtin_elementwise_max(hi, zero2);
				const uint32_t keep = ((valid_bits >> n) & 1u) ? 0xFFFFFFFFu : 0u;
				const uint2 packed { __builtin_bit_cast(uint32_t, lo) & keep, __builtin_bit_cast(uint32_t, hi) & keep };
				out[i][n] = packed;
				if (MODE == 1 && n < wt.count)
					my_skip[(i * C::NTW + n) * 64] = __builtin_bit_cast(half4, packed);
			}
		}
		if (MODE == 0)
		{ // (the accumulators are dead: room for the next layer's residual input, in flight through the barrier and the plane write)
#pragma unroll
			for (int i = 0; i < C::MT; i++)
#pragma unroll
				for (int n = 0; n < C::NTW; n++)
					skip_carry->v[i][n] = (n < wt.count) ? __builtin_bit_cast(uint2, my_skip[(i * C::NTW + n) * 64]) : uint2 { 0u, 0u };
		}
		lds_barrier(); // every wave has consumed the plane: it can be overwritten now
		int r_write = r;
		asm volatile("" : "+v"(r_write)); // (this layer's own address arithmetic, not kernel-wide constants kept in scratch)
		const int index0 = 1 + sh.S + tile0 + r_write;
#pragma unroll
		for (int i = 0; i < C::MT; i++)
		{
			const int ch = (wt.mg * C::MT + i) * 16 + 4 * q4;
			char *out0 = plane + C::offset(index0, ch / 8) + (ch % 8) * 2; // (a tile further on: 16 positions, the same swizzle)
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
				if (n < wt.count)
					*reinterpret_cast<uint2*>(out0 + n * 16 * C::POS_BYTES) = out[i][n];
		}
	}

	/*
	 * Input block: 5x5 convolution of the bit-unpacked padded input plane `in5` (stride S5; 32 channels: 64 bytes per position,
	 * chunk-swizzled by (index >> 2) & 3; RAW: 8 channels, 16 bytes per position, one k-step = four horizontal taps) + bias + ReLU.
	 * `in5` aliases the plane: the plane is cleared and written behind a barrier; the outputs are also the first block's residual input.
	 */
	template<int F, bool RAW>
	__device__ __forceinline__ void conv5x5_input(char *plane, const half8 *__restrict__ wpk, const float *__restrict__ bias, half4 *skip, const Shape &sh,
			const WaveTiles &wt, int wave, int lane, uint32_t valid_bits)
	{
		typedef Cfg<F> C;
		int r = lane & 15;
		asm volatile("" : "+v"(r));
		const int q4 = lane >> 4;
		const char *in5 = plane;
		floatx4 acc[C::MT][C::NTW];
#pragma unroll
		for (int i = 0; i < C::MT; i++)
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
				acc[i][n] = floatx4 { 0.0f, 0.0f, 0.0f, 0.0f };
		// padded-plane index of the (dy = 0, dx = 0) input cell of this lane's position in every tile: with position p = (y + 1) S + x,
		// (y + 2) S5 + (x + 2) = p + S + 4 y + 10
		int q0[C::NTW];
#pragma unroll
		for (int n = 0; n < C::NTW; n++)
		{
			const int pos = sh.S + (wt.n0 + n) * 16 + r;
			q0[n] = pos + sh.S + 4 * (div_stride(sh, pos) - 1) + 10 + (RAW ? q4 : 0);
		}
		constexpr int TAPS = RAW ? 10 : 25; // RAW: k-step t = 2 * dy + column group (dx 0-3, dx 4 + three zero-weight taps)
		const half8 *wp = wpk + (wt.mg * C::MT) * 64 + lane;
		half8 a_next[C::MT];
#pragma unroll
		for (int i = 0; i < C::MT; i++)
			a_next[i] = wp[i * 64];
		int dy = -2, step = 0; // t = dy-major; `step` = the tap's column (RAW: column group) inside the row
#pragma unroll 1
		for (int t = 0; t < TAPS; t++)
		{
			const int off = dy * sh.S5 + (RAW ? (4 * step - 2) : (step - 2));
			half8 a[C::MT];
#pragma unroll
			for (int i = 0; i < C::MT; i++)
				a[i] = a_next[i];
			const int tn = (t + 1 < TAPS) ? (t + 1) : 0;
#pragma unroll
			for (int i = 0; i < C::MT; i++)
				a_next[i] = wp[(tn * C::MTILES + i) * 64];
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
				if (n < wt.count)
				{
					int q = q0[n] + off;
					q = (q < 0) ? 0 : ((q >= sh.npos5) ? (sh.npos5 - 1) : q); // only dummy positions (and RAW's zero-weight taps) can fall outside
					const half8 b = RAW ? *reinterpret_cast<const half8*>(in5 + q * 16)
							: *reinterpret_cast<const half8*>(in5 + (q * 4 + (q4 ^ ((q >> 2) & 3))) * 16);
#pragma unroll
					for (int i = 0; i < C::MT; i++)
						acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b, acc[i][n], 0, 0, 0);
				}
			if (++step == (RAW ? 2 : 5))
			{
				step = 0;
				dy++;
			}
		}
		__syncthreads();
		const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
		for (int i = wave * 64 + lane; i < sh.plane16; i += C::THREADS)
			reinterpret_cast<uint4*>(plane)[i] = zero4;
		__syncthreads();
		typedef __attribute__((address_space(1))) half4 global_half4;
		int skip_lane = lane;
		asm volatile("" : "+v"(skip_lane));
		global_half4 *my_skip = (global_half4*) (skip + __builtin_amdgcn_readfirstlane(wave * C::MT * C::NTW * 64)) + skip_lane;
		const int index0 = 1 + sh.S + wt.n0 * 16 + r;
#pragma unroll
		for (int i = 0; i < C::MT; i++)
		{
			const int ch = (wt.mg * C::MT + i) * 16 + 4 * q4;
			const floatx4 bv = *reinterpret_cast<const floatx4*>(bias + ch);
			char *out0 = plane + C::offset(index0, ch / 8) + (ch % 8) * 2;
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
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
					my_skip[(i * C::NTW + n) * 64] = o;
				}
		}
	}

	template<int F, bool QHEAD, bool RAW>
	__global__ __launch_bounds__(512) void nn_any_board_kernel(NetParams p, Shape sh, const uint32_t *__restrict__ features, float *__restrict__ policy)
	{
		typedef Cfg<F> C;
		__shared__ __attribute__((aligned(16))) char lds[C::LDS_BYTES];
		char *plane = lds;
		half8 *s_wv1f = reinterpret_cast<half8*>(lds + C::PLANE_MAX);     // [KC][64]: A fragments of the value head's conv1x1 (4 real units of 16)
		float *red = reinterpret_cast<float*>(s_wv1f + C::KC * 64);       // [8] wave partials (+ 8 spare)
		float *s_wp2 = red + 16;                                          // [F] policy-head 1x1 weights
		float *s_wq2 = s_wp2 + F;                                         // [F][4] action-values head 1x1 weights
		float *ppart = s_wq2 + F * 4;                                     // [CG][PS] policy partial logits
		float *qpart = ppart + C::CG * C::PS;                             // [3][PS] action-value logits
		half4 *skip = p.skip + static_cast<size_t>(blockIdx.x) * C::SKIP_PER_WG;

		const int tid = threadIdx.x;
		const int wave = tid >> 6;
		const int lane = tid & 63;
		const int layer_halves8 = 9 * C::KC * C::MTILES * 64; // half8 elements per packed 3x3 layer
		const WaveTiles wt = wave_tiles<F>(sh, wave);

		stage_head_weights<F, C::THREADS, QHEAD>(p.wv1, p.wp2, p.wq2, tid, s_wv1f, s_wp2, s_wq2);

		// once per kernel: this thread's cell (one feature word / one policy output per thread) and this lane's on-board mask of the wave's tiles
		const int cell_y = (tid < sh.HW) ? tid / sh.cols : 0, cell_x = (tid < sh.HW) ? tid - cell_y * sh.cols : 0;
		const int cell_q5 = (cell_y + 2) * sh.S5 + (cell_x + 2);   // in the padded input plane
		const int cell_pos = cell_y * sh.S + cell_x;               // position (stride S)
		uint32_t valid_bits = 0;
		for (int n = 0; n < wt.count; n++)
		{
			const int pos = sh.S + (wt.n0 + n) * 16 + (lane & 15);
			const int y1 = div_stride(sh, pos); // y + 1
			if (pos - y1 * sh.S < sh.cols && y1 - 1 < sh.rows)
				valid_bits |= 1u << n;
		}

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
			conv5x5_input<F, RAW>(plane, p.w_in, p.bias, skip, sh, wt, wave, lane, valid_bits);
			BiasCarry<C::MT> bias_carry; // the first tower layer's bias values (with no block: the policy conv's), then each layer's successor's
			request_bias<F>(p.bias + F, wt, lane, bias_carry);
			__syncthreads();

			// ---- residual tower ----
			for (int blk = 0; blk < p.blocks; blk++)
			{
				SkipCarry<F> skip_carry;
				conv3x3_layer<F, 0>(plane, p.w_tower + (2 * blk) * layer_halves8, bias_carry, p.bias + (2 + 2 * blk) * F, skip, nullptr, nullptr, sh, wt, wave, lane,
						valid_bits, &skip_carry);
				lds_barrier();
				conv3x3_layer<F, 1>(plane, p.w_tower + (2 * blk + 1) * layer_halves8, bias_carry, p.bias + (3 + 2 * blk) * F, skip, nullptr, nullptr, sh, wt, wave, lane,
						valid_bits, &skip_carry);
				lds_barrier();
			}

			// ---- value head, stage 1: conv1x1 F -> 4 + ReLU as one 16 x 16 MFMA tile per 16 positions (4 of the 16 units are real), the tiles dealt
			//      round-robin to the waves; the dense layers run in value_head_kernel (nn_forward.hip) for all boards of the launch ----
			{
				const int r = lane & 15, q4 = lane >> 4;
				for (int n = wave; n < sh.NT; n += C::THREADS / 64)
				{
					floatx4 v { p.bv1[0], p.bv1[1], p.bv1[2], p.bv1[3] };
					const int index0 = 1 + sh.S + n * 16 + r;
#pragma unroll
					for (int kc = 0; kc < C::KC; kc++)
					{
						const half8 bfrag = *reinterpret_cast<const half8*>(plane + C::offset(index0, kc * 4 + q4));
						v = __builtin_amdgcn_mfma_f32_16x16x32_f16(s_wv1f[kc * 64 + lane], bfrag, v, 0, 0, 0);
					}
					// lanes with q4 == 0 hold outputs 0 .. 3 of position r of tile n
					const int pos = sh.S + n * 16 + r;
					const int y1 = div_stride(sh, pos);
					const int x = pos - y1 * sh.S, y = y1 - 1;
					if (q4 == 0 && x < sh.cols && y < sh.rows)
					{
						half4 o;
						o[0] = static_cast<half_t>(fmaxf(v[0], 0.0f));
						o[1] = static_cast<half_t>(fmaxf(v[1], 0.0f));
						o[2] = static_cast<half_t>(fmaxf(v[2], 0.0f));
						o[3] = static_cast<half_t>(fmaxf(v[3], 0.0f));
						*reinterpret_cast<half4*>(p.vhead_x + static_cast<size_t>(bi) * sh.kpad + (y * sh.cols + x) * 4) = o;
					}
				}
			}
			// ---- policy head: conv3x3 + ReLU folded with the conv1x1 F -> 1 ----
			conv3x3_layer<F, 2>(plane, p.w_tower + (2 * p.blocks) * layer_halves8, bias_carry, QHEAD ? p.bias + (2 + 2 * p.blocks) * F : nullptr, skip, s_wp2, ppart, sh, wt,
					wave, lane, valid_bits);
			__syncthreads();
			// the next board's input: requested here, consumed by the staging at the top
			if (bi + static_cast<int>(gridDim.x) < batch && tid < sh.HW)
			{
				const int nb = bi + static_cast<int>(gridDim.x);
				next_word = features[static_cast<size_t>((p.slot_list != nullptr) ? p.slot_list[nb] : nb) * sh.HW + tid];
			}
			{ // bias, softmax over the rows * cols real cells (one per thread)
				float logit = -3.0e38f;
				if (tid < sh.HW)
				{
					logit = p.bp2 + sum_partial_logits<C::CG, C::PS>(ppart, cell_pos);
				}
				const float m = block_reduce_max(logit, red, tid);
				const float e = (tid < sh.HW) ? __expf(logit - m) : 0.0f;
				const float sum = block_reduce_sum(e, red, tid);
				if (tid < sh.HW)
					policy[static_cast<size_t>(b) * sh.HW + tid] = e / sum;
			}
			// ---- action-values head: conv3x3 + tanh, conv1x1 F -> 3 + bias, softmax over the 3 per cell ----
			if (QHEAD)
			{
				__syncthreads(); // the policy head is done with the partial-sum buffers
				conv3x3_layer<F, 3>(plane, p.w_tower + (2 * p.blocks + 1) * layer_halves8, bias_carry, nullptr, skip, s_wq2, qpart, sh, wt, wave, lane, valid_bits);
				if (tid < sh.HW)
				{
					const float z0 = p.bq2[0] + qpart[cell_pos], z1 = p.bq2[1] + qpart[C::PS + cell_pos], z2 = p.bq2[2] + qpart[2 * C::PS + cell_pos];
					const float2 win_draw = softmax3_win_draw(z0, z1, z2);
					float *out = p.q + (static_cast<size_t>(b) * sh.HW + tid) * 2;
					out[0] = win_draw.x;
					out[1] = win_draw.y;
				}
			}
		}
	}

	Shape make_shape(int rows, int cols, int position_groups, int kpad)
	{
		Shape sh;
		sh.rows = rows;
		sh.cols = cols;
		sh.S = cols + 1;
		sh.NT = (rows * sh.S + 15) / 16;
		sh.ntw = (sh.NT + position_groups - 1) / position_groups;
		sh.HW = rows * cols;
		sh.kpad = kpad;
		sh.S5 = sh.S + 4;
		sh.npos5 = (rows + 4) * sh.S5 + 4;
		sh.magic = 65536 / sh.S + 1;
		return sh;
	}
}

namespace agx_any
{
	size_t skip_bytes_per_workgroup(int filters)
	{
		return sizeof(half4) * static_cast<size_t>((filters == 128) ? Cfg<128>::SKIP_PER_WG : Cfg<64>::SKIP_PER_WG);
	}

	int launch(const NetParams &p, int rows, int cols, int filters, bool raw, int grid, int kpad, const uint32_t *d_features, float *d_policy, hipStream_t stream)
	{
		AGX_REQUIRE(rows >= MIN_SIDE && rows <= MAX_SIDE && cols >= MIN_SIDE && cols <= MAX_SIDE && (filters == 64 || filters == 128), AGX_ERR_UNSUPPORTED,
				"agx_nn_forward: no kernel for a %dx%d board with %d filters", rows, cols, filters);
		AGX_REQUIRE(p.skip != nullptr && p.vhead_x != nullptr && grid > 0, AGX_ERR_STATE, "agx_nn_forward: launch scratch missing");
		const bool qhead = (p.q != nullptr);
		AGX_REQUIRE(!(qhead && raw), AGX_ERR_UNSUPPORTED, "agx_nn_forward: no action-values head on an 8-channel network");
		const dim3 g(grid), t(512);
#define AGX_ANY_TOWER(FF, QH, RW) do { Shape sh = make_shape(rows, cols, Cfg<FF>::PG, kpad); sh.plane16 = (1 + sh.S + sh.NT * 16 + sh.S + 2) * Cfg<FF>::POS_BYTES / 16; \
		hipLaunchKernelGGL((nn_any_board_kernel<FF, QH, RW>), g, t, 0, stream, p, sh, d_features, d_policy); } while (0)
#define AGX_ANY_VARIANTS(FF) do { if (qhead) AGX_ANY_TOWER(FF, true, false); else if (raw) AGX_ANY_TOWER(FF, false, true); else AGX_ANY_TOWER(FF, false, false); } while (0)
		if (filters == 128)
			AGX_ANY_VARIANTS(128);
		else
			AGX_ANY_VARIANTS(64);
#undef AGX_ANY_VARIANTS
#undef AGX_ANY_TOWER
		AGX_HIP_CHECK(hipGetLastError());
		return AGX_OK;
	}
}
