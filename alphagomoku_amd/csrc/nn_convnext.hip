/*
 * nn_convnext.hip — the ConvNeXt towers ConvNextPVQraw / ConvNextPVQMraw (networks.cpp:1078-1219 of the reference, batch norms folded) for any
 * board with 5 <= rows, cols <= 20, gfx950 (CDNA4).
 *
 *   conv_in   5x5, 8 -> F, + b, relu
 *   blocks x  y = depthwise 7x7 (x) + bd ; y = relu(W1 . y + b1) ; x = W2 . y + b2 + x ; x = x * sigmoid(Ws2 . relu(Ws1 . mean_hw(x) + bs1) + bs2)
 *   heads     policy / value / q (/ m): a 1x1 convolution each, folded with what follows it
 *
 * One run-time-shaped kernel, templated on the filter count only, in the shape of nn_any_board.hip: a persistent grid, one workgroup of 8
 * waves carries a board through the whole network in LDS, positions come from an optional device-side slot list.  No global scratch.
 *
 *   - ONE activation plane x [NT * 16 positions][F] fp16 (position = row * cols + col, no spare cells; 16-byte chunks XOR-swizzled inside a
 *     position's bank row like the other towers).  20x20x128 is 102 400 bytes: a second plane does not fit, so a block runs in place:
 *       1. depthwise 7x7 and the first 1x1 are fused over 32-channel k-chunks: all 512 threads compute the depthwise outputs of one chunk
 *          into the chunk buffer ybuf [positions][32] (25.6 KB), then every wave adds W1[:, chunk] . ybuf to its accumulators (MFMA
 *          16x16x32 f16, weights as the A operand).  y never exists as a whole plane.
 *       2. every lane takes the residual values of its accumulator layout out of the plane into registers and writes relu(y1) over them
 *          (the same 8 bytes: no other lane reads or writes them between the two).
 *       3. the second 1x1 starts from bias + residual, reads relu(y1) from the plane; its outputs stay in registers through the
 *          squeeze-and-excitation (per-channel sums of the fp32 accumulators -> mean -> two fp32 dense layers -> gate) and are written
 *          once, gated, as fp16.
 *   - The depthwise convolution is VALU work on LDS reads: a thread owns (position, 8 channels), walks the 49 taps in (dy, dx) order and skips
 *     the ones off the board ("same" zero padding for every shape, boards smaller than the window included).  fp16 x fp16 products are exact
 *     in fp32, accumulation is fp32.
 *   - Numerics: activations stored as fp16, 1x1 / depthwise / input weights fp16, every accumulation fp32; pooled means, the SE layers, the
 *     dense layers of the value and moves-left heads and all biases fp32 (fmaf); sigmoid = 1 / (1 + __expf(-z)).  A head's hidden 1x1
 *     activation is rounded to fp16 like a stored plane before what follows it.  Every reduction over lanes and waves runs in an order
 *     fixed by the board shape alone: results do not depend on the grid, the batch or the slot list.
 *
 * The host side (packing of the canonical blob with the packers of nn_pack.hpp, the launch) is at the end; nn_net.cpp dispatches here
 * (nn_convnext.hpp).
 */
#include "nn_device.hpp"
#include "nn_pack.hpp"
#include "nn_convnext.hpp"

#include <vector>

namespace
{
	constexpr int MIN_SIDE = 5, MAX_SIDE = 20;
	constexpr int VALUE_HIDDEN = 256, ML_FILTERS = 32, ML_HIDDEN = 128;

	struct Params
	{
			const half_t *h;           // fp16 weights (Layout::h_*)
			const float *f;            // fp32 weights and biases (Layout::f_*)
			const uint32_t *features;
			const int *slot_list;      // optional: batch element i is slot slot_list[i]
			const int *count_ptr;      // optional: batch size read on the device
			float *policy, *value, *q, *m; // q, m: null = head not evaluated
			int blocks, batch;
			int rows, cols, HW;
			int NT;                    // 16-position tiles: ceil(HW / 16)
			int ntw;                   // tiles per position group of the tower's wave layout: ceil(NT / PG)
			int ntw4;                  // tiles per position group of the moves-left head (4 groups): ceil(NT / 4)
			int S5, npos5;             // padded input plane: row stride cols + 4, (rows + 4) * S5 + 4 positions
			float inv_hw;
	};

	/* where the parts of a network lie in the two device buffers (element offsets), for the packer and the kernel alike */
	template<int F>
	struct Layout
	{
			static constexpr int KC = F / 32, MTILES = F / 16;
			static constexpr int H_IN = 10 * MTILES * 512;             // pack of the 5x5 input conv: [10][MTILES][lane][8]
			static constexpr int H_WD = 49 * F, H_W = F * F;           // depthwise [49][F]; a 1x1 as A fragments [KC][MTILES][lane][8]
			static constexpr int H_BLOCK = H_WD + 2 * H_W;             // wd, w1, w2
			__host__ __device__ static constexpr size_t h_block(int b) { return H_IN + static_cast<size_t>(b) * H_BLOCK; }
			// heads behind the blocks: wp1, wv1, wq1 (F x F), wm1 (F x 32: [KC][2][lane][8])
			static constexpr int F_BLOCK = 5 * F + 2 * F * F;          // bd, b1, b2, ws1 [F][F], bs1, ws2 [F][F], bs2
			__host__ __device__ static constexpr size_t f_block(int b) { return F + static_cast<size_t>(b) * F_BLOCK; } // (b_in [F] in front)
			// heads behind the blocks, in this order (scalars and 3-vectors padded to 4):
			static constexpr int FH_BP1 = 0, FH_WP2 = FH_BP1 + F, FH_BP2 = FH_WP2 + F, FH_BV1 = FH_BP2 + 4, FH_WV2 = FH_BV1 + F,
					FH_BV2 = FH_WV2 + F * VALUE_HIDDEN, FH_WV3 = FH_BV2 + VALUE_HIDDEN, FH_BV3 = FH_WV3 + VALUE_HIDDEN * 4, FH_BQ1 = FH_BV3 + 4,
					FH_WQ2 = FH_BQ1 + F, FH_BQ2 = FH_WQ2 + F * 4, FH_BM1 = FH_BQ2 + 4, FH_WM2 = FH_BM1 + ML_FILTERS,
					FH_BM2 = FH_WM2 + ML_FILTERS * ML_HIDDEN, FH_WM3 = FH_BM2 + ML_HIDDEN; // wm3 [128][HW], then bm3 [HW]
	};

	template<int F>
	struct Cfg
	{
			static_assert(F == 64 || F == 128, "filters");
			static constexpr int CH = F / 8;                        // 16-byte chunks per position
			static constexpr int PPR_SHIFT = (F == 128) ? 0 : 1;    // log2 of the positions per 256-byte bank row
			static constexpr int CG = (F >= 128) ? 4 : 2;           // channel groups x position groups of the 8 waves
			static constexpr int CG_SHIFT = (F >= 128) ? 2 : 1;
			static constexpr int PG = 8 / CG;
			static constexpr int MT = F / (16 * CG);                // 16-channel output tiles per wave
			static constexpr int MTILES = F / 16;
			static constexpr int KC = F / 32;
			static constexpr int NPOS_MAX = MAX_SIDE * MAX_SIDE;    // 400 = 25 whole tiles
			static constexpr int NT_MAX = (NPOS_MAX + 15) / 16;
			static constexpr int NTW = (NT_MAX + PG - 1) / PG;      // accumulator tiles of a wave (the largest board's)
			static constexpr int NTW4 = (NT_MAX + 3) / 4;           // the moves-left head's: 2 channel tiles x 4 position groups
			static constexpr int POS_BYTES = F * 2;
			static constexpr int PLANE_BYTES = NT_MAX * 16 * POS_BYTES;
			static constexpr int YBUF_BYTES = NT_MAX * 16 * 64;     // one 32-channel chunk of every position; the heads' partial sums; the padded input
			static constexpr int WD_BYTES = 49 * F * 2;             // a block's depthwise weights
			static constexpr int PS = NT_MAX * 16;                  // stride of the heads' partial-sum rows
			static constexpr int THREADS = 512;
			static constexpr int VEC = 256;                         // floats of a vector buffer (a pooled mean, a hidden layer)
			static constexpr int LDS_BYTES = PLANE_BYTES + YBUF_BYTES + WD_BYTES + NT_MAX * 16 * 2 + (3 * VEC + THREADS + 16) * 4;
			static_assert(LDS_BYTES <= 163840, "does not fit in LDS");
			static_assert((MAX_SIDE + 4) * (MAX_SIDE + 4) * 16 + 64 <= YBUF_BYTES, "the padded input plane lies inside the chunk buffer");
			static_assert((CG * 3 + 1) * PS * 4 <= YBUF_BYTES, "the heads' partial sums and the moves-left logits lie inside the chunk buffer");
			static_assert(PG * F <= VEC && 4 * ML_FILTERS <= VEC && VALUE_HIDDEN <= VEC && ML_HIDDEN <= VEC, "vector buffers");
			__device__ static __forceinline__ int offset(int position, int chunk)
			{ // byte offset of a 16-byte chunk of a position: XOR-swizzled inside the position's bank row
				return position * POS_BYTES + ((chunk ^ ((position >> PPR_SHIFT) & (CH - 1))) * 16);
			}
	};

	/* what a wave owns: channels [mg * 16 * MT, (mg + 1) * 16 * MT) of tiles n0 .. n0 + count - 1 (wave-uniform) */
	struct WaveTiles
	{
			int mg, pg, n0, count;
	};

	__device__ __forceinline__ half_t relu_half(float v)
	{ // a ReLU output as it would be stored
		return static_cast<half_t>(fmaxf(v, 0.0f));
	}

	/*
	 * out[j] = act(bias[j] + sum_i in[i] * W[i * ldw + j]) for j < n_out, fp32: the inputs are cut into `parts` runs (a power of two fixed
	 * by n_out alone), a thread adds one run for one output in index order, the runs are added in order.  act 0 none, 1 ReLU, 2 sigmoid.
	 * s_in and s_out are LDS vectors (distinct); barriers in front and behind.
	 */
	__device__ __forceinline__ void dense(const float *s_in, int n_in, const float *__restrict__ W, int ldw, const float *__restrict__ bias, int n_out, float *s_out,
			float *s_part, int act, int tid)
	{
		const int parts = (n_out <= 64) ? 8 : ((n_out <= 128) ? 4 : ((n_out <= 256) ? 2 : 1));
		__syncthreads();
		if (tid < parts * n_out)
		{
			const int part = tid / n_out, j = tid - part * n_out, len = n_in / parts, i0 = part * len;
			float s = 0.0f;
			for (int i = 0; i < len; i++)
				s = fmaf(s_in[i0 + i], W[static_cast<size_t>(i0 + i) * ldw + j], s);
			s_part[tid] = s;
		}
		__syncthreads();
		if (tid < n_out)
		{
			float s = bias[tid];
			for (int g = 0; g < parts; g++)
				s += s_part[g * n_out + tid];
			if (act == 1)
				s = fmaxf(s, 0.0f);
			else if (act == 2)
				s = 1.0f / (1.0f + __expf(-s));
			s_out[tid] = s;
		}
		__syncthreads();
	}

	/* acc += W . plane for a 1x1 convolution F -> F: A fragments `wfrag` [KC][MTILES][lane], B fragments from the plane */
	template<int F>
	__device__ __forceinline__ void mac1x1(const char *plane, const half8 *__restrict__ wfrag, const WaveTiles &wt, int lane, floatx4 (&acc)[Cfg<F>::MT][Cfg<F>::NTW])
	{
		typedef Cfg<F> C;
		lane = own(lane);
		const int r = lane & 15, q4 = lane >> 4;
		half8 a[C::KC][C::MT];
#pragma unroll
		for (int kc = 0; kc < C::KC; kc++)
#pragma unroll
			for (int i = 0; i < C::MT; i++)
				a[kc][i] = wfrag[(kc * C::MTILES + wt.mg * C::MT + i) * 64 + lane];
		const int p0 = wt.n0 * 16 + r;
#pragma unroll
		for (int kc = 0; kc < C::KC; kc++)
		{
			const char *src = plane + C::offset(p0, kc * 4 + q4); // (a tile further on: 16 positions, the same swizzle)
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
				if (n < wt.count)
				{
					const half8 b = *reinterpret_cast<const half8*>(src + n * 16 * C::POS_BYTES);
#pragma unroll
					for (int i = 0; i < C::MT; i++)
						acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[kc][i], b, acc[i][n], 0, 0, 0);
				}
		}
		mfma_settle(acc);
	}

	template<int F>
	__device__ __forceinline__ void init_bias(const float *__restrict__ bias, const WaveTiles &wt, int lane, floatx4 (&acc)[Cfg<F>::MT][Cfg<F>::NTW])
	{
		lane = own(lane);
#pragma unroll
		for (int i = 0; i < Cfg<F>::MT; i++)
		{
			const floatx4 bv = *reinterpret_cast<const floatx4*>(bias + (wt.mg * Cfg<F>::MT + i) * 16 + 4 * (lane >> 4));
#pragma unroll
			for (int n = 0; n < Cfg<F>::NTW; n++)
				acc[i][n] = bv;
		}
	}

	/* per-channel sums over the board of a wave's values (cells off the board excluded by valid_bits): tiles in order, then the 16 lanes of a
	 * position row by a butterfly, into s_sum [PG][F]; the position groups are added by the caller in order */
	template<int F>
	__device__ __forceinline__ void channel_sums(const floatx4 (&v)[Cfg<F>::MT][Cfg<F>::NTW], const WaveTiles &wt, int lane, uint32_t valid_bits, float *s_sum)
	{
		typedef Cfg<F> C;
		lane = own(lane);
#pragma unroll
		for (int i = 0; i < C::MT; i++)
		{
			floatx4 s { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
			for (int n = 0; n < C::NTW; n++)
				if (n < wt.count && ((valid_bits >> n) & 1u))
					s += v[i][n];
#pragma unroll
			for (int o = 1; o < 16; o <<= 1)
			{
				s[0] += __shfl_xor(s[0], o);
				s[1] += __shfl_xor(s[1], o);
				s[2] += __shfl_xor(s[2], o);
				s[3] += __shfl_xor(s[3], o);
			}
			if ((lane & 15) == 0)
				*reinterpret_cast<floatx4*>(s_sum + wt.pg * F + (wt.mg * C::MT + i) * 16 + 4 * (lane >> 4)) = s;
		}
	}

	/* the depthwise 7x7 outputs (+ bias) of channels kc * 32 .. + 31 of every position into ybuf [position][4 chunks] (chunk-swizzled by
	 * (position >> 2) & 3); positions of the last tile beyond the board get zero */
	template<int F>
	__device__ __forceinline__ void depthwise_chunk(const char *plane, const half8 *s_wd, const float *__restrict__ bd, char *ybuf, const unsigned short *s_yx,
			const Params &p, int kc, int tid)
	{
		typedef Cfg<F> C;
		tid = own(tid);
		const int qc = tid & 3, chunk = kc * 4 + qc;
		const floatx4 b_lo = *reinterpret_cast<const floatx4*>(bd + chunk * 8), b_hi = *reinterpret_cast<const floatx4*>(bd + chunk * 8 + 4);
		for (int pos = tid >> 2; pos < p.NT * 16; pos += C::THREADS / 4)
		{
			half8 out;
#pragma unroll
			for (int j = 0; j < 8; j++)
				out[j] = static_cast<half_t>(0.0f);
			if (pos < p.HW)
			{
				const int yx = s_yx[pos], y = yx >> 8, x = yx & 255;
				float a[8] = { b_lo[0], b_lo[1], b_lo[2], b_lo[3], b_hi[0], b_hi[1], b_hi[2], b_hi[3] };
#pragma unroll 1
				for (int dy = -3; dy <= 3; dy++)
				{
					if (static_cast<unsigned>(y + dy) >= static_cast<unsigned>(p.rows))
						continue;
					const int row_pos = pos + dy * p.cols;
					const half8 *w_row = s_wd + (dy + 3) * 7 * C::CH + chunk;
#pragma unroll
					for (int dx = -3; dx <= 3; dx++)
						if (static_cast<unsigned>(x + dx) < static_cast<unsigned>(p.cols))
						{
							const half8 h = *reinterpret_cast<const half8*>(plane + C::offset(row_pos + dx, chunk));
							const half8 w = w_row[(dx + 3) * C::CH];
#pragma unroll
							for (int j = 0; j < 8; j++)
								a[j] = fmaf(static_cast<float>(h[j]), static_cast<float>(w[j]), a[j]); // (the product of two halves is exact in fp32)
						}
				}
#pragma unroll
				for (int j = 0; j < 8; j++)
					out[j] = static_cast<half_t>(a[j]);
			}
			*reinterpret_cast<half8*>(ybuf + (pos * 4 + (qc ^ ((pos >> 2) & 3))) * 16) = out;
		}
	}

	template<int F>
	__global__ __launch_bounds__(512) void nn_convnext_kernel(Params p)
	{
		typedef Cfg<F> C;
		typedef Layout<F> L;
		__shared__ __attribute__((aligned(16))) char lds[C::LDS_BYTES];
		char *plane = lds;
		char *ybuf = plane + C::PLANE_BYTES;
		half8 *s_wd = reinterpret_cast<half8*>(ybuf + C::YBUF_BYTES);                               // [49][CH]
		unsigned short *s_yx = reinterpret_cast<unsigned short*>(ybuf + C::YBUF_BYTES + C::WD_BYTES); // [NT * 16]: row << 8 | col of a position
		float *s_sum = reinterpret_cast<float*>(s_yx + C::NT_MAX * 16);                             // [PG][F] channel sums of the position groups
		float *s_vec = s_sum + C::VEC;                                                               // a dense layer's input
		float *s_hid = s_vec + C::VEC;                                                               // a hidden layer
		float *s_part = s_hid + C::VEC;                                                              // [THREADS] dense(): partial sums
		float *red = s_part + C::THREADS;                                                            // [8] wave partials (+ 8 spare)
		float *hpart = reinterpret_cast<float*>(ybuf);                                               // [CG][3][PS] the heads' partial logits (chunk buffer idle)
		float *s_logit = hpart + C::CG * 3 * C::PS;                                                  // [PS] moves-left logits

		const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
		WaveTiles wt;
		wt.mg = __builtin_amdgcn_readfirstlane(wave & (C::CG - 1));
		wt.pg = __builtin_amdgcn_readfirstlane(wave >> C::CG_SHIFT);
		{
			const int first = wt.pg * p.ntw, left = p.NT - first;
			wt.count = (left < 0) ? 0 : ((left < p.ntw) ? left : p.ntw);
			wt.n0 = (wt.count > 0) ? first : 0; // (a wave without tiles computes nothing; its addresses stay inside the plane)
		}
		for (int i = tid; i < p.NT * 16; i += C::THREADS)
		{ // (positions of the last tile beyond the board repeat the last cell: addresses made from them stay inside every buffer)
			const int cell = (i < p.HW) ? i : (p.HW - 1), y = cell / p.cols;
			s_yx[i] = static_cast<unsigned short>((y << 8) | (cell - y * p.cols));
		}
		uint32_t valid_bits = 0; // bit n = this lane's position of the wave's tile n is on the board
		for (int n = 0; n < wt.count; n++)
			if ((wt.n0 + n) * 16 + (lane & 15) < p.HW)
				valid_bits |= 1u << n;
// this phase's own lane indices: r = position inside a tile, q4 = quarter of the wave, p0 = this lane's position in the wave's first tile
#define AGX_CNX_LANE() const int lane_own = own(lane), r = lane_own & 15, q4 = lane_own >> 4, p0 = wt.n0 * 16 + r; (void) r; (void) q4; (void) p0

		const int batch = (p.count_ptr != nullptr) ? min(*p.count_ptr, p.batch) : p.batch;
		const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

		for (int bi = blockIdx.x; bi < batch; bi += gridDim.x)
		{
			const int b = (p.slot_list != nullptr) ? p.slot_list[bi] : bi;
			// (the weight pointers are this board's own: seen as loop constants, every weight and bias the heads and the input conv load would be
			//  fetched once in front of the loop and kept in registers - some 400 of them, in scratch - for the whole kernel)
			const half_t *wh = p.h;
			const float *wf = p.f;
			asm volatile("" : "+s"(wh), "+s"(wf));
			const half8 *w_in = reinterpret_cast<const half8*>(wh);
			const half_t *h_heads = wh + L::h_block(p.blocks);
			const float *f_heads = wf + L::f_block(p.blocks);
			// ---- the 8 low bits of every feature word, unpacked into the padded input plane (in the chunk buffer) ----
			__syncthreads();
			for (int i = tid; i < p.npos5; i += C::THREADS)
				reinterpret_cast<uint4*>(ybuf)[i] = zero4;
			__syncthreads();
			if (tid < p.HW)
			{
				const int yx = s_yx[tid];
				const uint32_t word = p.features[static_cast<size_t>(b) * p.HW + tid];
				reinterpret_cast<uint4*>(ybuf)[((yx >> 8) + 2) * p.S5 + (yx & 255) + 2] = unpack_feature_byte(word & 255u);
			}
			__syncthreads();
			{ // ---- conv 5x5, 8 -> F, + bias, ReLU: k-step t = 2 * dy + g holds the taps dx = 4 g + (lane >> 4) (zero weights beyond dx = 4) ----
				AGX_CNX_LANE();
				floatx4 acc[C::MT][C::NTW];
				init_bias<F>(wf, wt, lane, acc);
				int q0[C::NTW];
#pragma unroll
				for (int n = 0; n < C::NTW; n++)
				{
					const int yx = s_yx[(n < wt.count) ? (p0 + n * 16) : p0];
					q0[n] = (yx >> 8) * p.S5 + (yx & 255) + q4;
				}
#pragma unroll 1
				for (int t = 0; t < 10; t++)
				{
					half8 a[C::MT];
#pragma unroll
					for (int i = 0; i < C::MT; i++)
						a[i] = w_in[(t * C::MTILES + wt.mg * C::MT + i) * 64 + lane];
					const int off = (t >> 1) * p.S5 + 4 * (t & 1);
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
						if (n < wt.count)
						{
							const half8 bf = *reinterpret_cast<const half8*>(ybuf + (q0[n] + off) * 16);
#pragma unroll
							for (int i = 0; i < C::MT; i++)
								acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bf, acc[i][n], 0, 0, 0);
						}
				}
				mfma_settle(acc);
				{
					AGX_CNX_LANE();
#pragma unroll
					for (int i = 0; i < C::MT; i++)
					{
						const int ch = (wt.mg * C::MT + i) * 16 + 4 * q4;
						char *out0 = plane + C::offset(p0, ch / 8) + (ch % 8) * 2;
#pragma unroll
						for (int n = 0; n < C::NTW; n++)
							if (n < wt.count)
							{
								const bool valid = (valid_bits >> n) & 1u;
								half4 o;
#pragma unroll
								for (int j = 0; j < 4; j++)
									o[j] = valid ? relu_half(acc[i][n][j]) : static_cast<half_t>(0.0f);
								*reinterpret_cast<half4*>(out0 + n * 16 * C::POS_BYTES) = o;
							}
					}
				}
			}

			// ---- blocks ----
			for (int blk = 0; blk < p.blocks; blk++)
			{
				const half_t *hb = wh + L::h_block(blk);
				const float *fb = wf + L::f_block(blk);
				const half8 *w1 = reinterpret_cast<const half8*>(hb + L::H_WD), *w2 = reinterpret_cast<const half8*>(hb + L::H_WD + L::H_W);
				const float *bd = fb, *b1 = fb + F, *b2 = fb + 2 * F, *ws1 = fb + 3 * F, *bs1 = ws1 + F * F, *ws2 = bs1 + F, *bs2 = ws2 + F * F;
				for (int i = tid; i < 49 * C::CH; i += C::THREADS)
					s_wd[i] = reinterpret_cast<const half8*>(hb)[i];
				floatx4 acc[C::MT][C::NTW];
				init_bias<F>(b1, wt, lane, acc);
				__syncthreads(); // the plane and the depthwise weights are written
				// depthwise 7x7 fused with the first 1x1, one 32-channel chunk at a time
#pragma unroll 1
				for (int kc = 0; kc < C::KC; kc++)
				{
					depthwise_chunk<F>(plane, s_wd, bd, ybuf, s_yx, p, kc, tid);
					half8 a[C::MT];
#pragma unroll
					for (int i = 0; i < C::MT; i++)
						a[i] = w1[(kc * C::MTILES + wt.mg * C::MT + i) * 64 + own(lane)];
					__syncthreads();
					AGX_CNX_LANE();
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
						if (n < wt.count)
						{
							const int pos = p0 + n * 16;
							const half8 bf = *reinterpret_cast<const half8*>(ybuf + (pos * 4 + (q4 ^ ((pos >> 2) & 3))) * 16);
#pragma unroll
							for (int i = 0; i < C::MT; i++)
								acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bf, acc[i][n], 0, 0, 0);
						}
					__syncthreads(); // the chunk buffer is consumed (and, behind the last chunk, the plane: no depthwise read is left)
				}
				mfma_settle(acc);
				// the residual values of this lane's accumulator layout out of the plane, relu(y1) over them
				uint2 res[C::MT][C::NTW];
				AGX_CNX_LANE();
#pragma unroll
				for (int i = 0; i < C::MT; i++)
				{
					const int ch = (wt.mg * C::MT + i) * 16 + 4 * q4;
					char *cell0 = plane + C::offset(p0, ch / 8) + (ch % 8) * 2;
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
					{
						res[i][n] = uint2 { 0u, 0u };
						if (n < wt.count)
						{
							res[i][n] = *reinterpret_cast<const uint2*>(cell0 + n * 16 * C::POS_BYTES);
							const bool valid = (valid_bits >> n) & 1u;
							half4 o;
#pragma unroll
							for (int j = 0; j < 4; j++)
								o[j] = valid ? relu_half(acc[i][n][j]) : static_cast<half_t>(0.0f);
							*reinterpret_cast<half4*>(cell0 + n * 16 * C::POS_BYTES) = o;
						}
					}
				}
				// second 1x1 from bias + residual
#pragma unroll
				for (int i = 0; i < C::MT; i++)
				{
					const floatx4 bv = *reinterpret_cast<const floatx4*>(b2 + (wt.mg * C::MT + i) * 16 + 4 * q4);
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
						acc[i][n] = bias_plus_residual(res[i][n], bv);
				}
				__syncthreads(); // relu(y1) is written
				mac1x1<F>(plane, w2, wt, lane, acc);
				// squeeze and excitation on the fp32 outputs
				channel_sums<F>(acc, wt, lane, valid_bits, s_sum);
				__syncthreads(); // (every wave is also done reading relu(y1))
				if (tid < F)
				{
					float s = 0.0f;
					for (int g = 0; g < C::PG; g++)
						s += s_sum[g * F + tid];
					s_vec[tid] = s * p.inv_hw;
				}
				dense(s_vec, F, ws1, F, bs1, F, s_hid, s_part, 1, tid);
				dense(s_hid, F, ws2, F, bs2, F, s_vec, s_part, 2, tid);
				{
					AGX_CNX_LANE();
#pragma unroll
					for (int i = 0; i < C::MT; i++)
					{
						const int ch = (wt.mg * C::MT + i) * 16 + 4 * q4;
						const floatx4 gate = *reinterpret_cast<const floatx4*>(s_vec + ch);
						char *cell0 = plane + C::offset(p0, ch / 8) + (ch % 8) * 2;
#pragma unroll
						for (int n = 0; n < C::NTW; n++)
							if (n < wt.count)
							{
								const bool valid = (valid_bits >> n) & 1u;
								half4 o;
#pragma unroll
								for (int j = 0; j < 4; j++)
									o[j] = valid ? static_cast<half_t>(acc[i][n][j] * gate[j]) : static_cast<half_t>(0.0f);
								*reinterpret_cast<half4*>(cell0 + n * 16 * C::POS_BYTES) = o;
							}
					}
				}
			}
			__syncthreads(); // the tower's output is in the plane; the chunk buffer is free for the heads' partial sums

			// ---- policy head: 1x1 F -> F + ReLU folded with the 1x1 F -> 1, softmax over the board ----
			{
				AGX_CNX_LANE();
				floatx4 acc[C::MT][C::NTW];
				init_bias<F>(f_heads + L::FH_BP1, wt, lane, acc);
				mac1x1<F>(plane, reinterpret_cast<const half8*>(h_heads), wt, lane, acc);
				float part[C::NTW];
#pragma unroll
				for (int n = 0; n < C::NTW; n++)
					part[n] = 0.0f;
#pragma unroll
				for (int i = 0; i < C::MT; i++)
				{
					const floatx4 wv = *reinterpret_cast<const floatx4*>(f_heads + L::FH_WP2 + (wt.mg * C::MT + i) * 16 + 4 * q4);
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
#pragma unroll
						for (int j = 0; j < 4; j++)
							part[n] = fmaf(static_cast<float>(relu_half(acc[i][n][j])), wv[j], part[n]);
				}
#pragma unroll
				for (int n = 0; n < C::NTW; n++)
				{
					float s = part[n];
					s += __shfl_xor(s, 16);
					s += __shfl_xor(s, 32);
					if (q4 == 0 && n < wt.count)
						hpart[wt.mg * C::PS + p0 + n * 16] = s;
				}
				__syncthreads();
				float logit = -3.0e38f;
				if (tid < p.HW)
					logit = f_heads[L::FH_BP2] + sum_partial_logits<C::CG, C::PS>(hpart, tid);
				const float mx = block_reduce_max(logit, red, tid);
				const float e = (tid < p.HW) ? __expf(logit - mx) : 0.0f;
				const float sum = block_reduce_sum(e, red, tid);
				if (tid < p.HW)
					p.policy[static_cast<size_t>(b) * p.HW + tid] = e / sum;
			}
			// ---- value head: 1x1 F -> F + ReLU, mean over the board, dense F -> 256 + ReLU, dense 256 -> 3, softmax ----
			{
				floatx4 acc[C::MT][C::NTW];
				init_bias<F>(f_heads + L::FH_BV1, wt, lane, acc);
				mac1x1<F>(plane, reinterpret_cast<const half8*>(h_heads + L::H_W), wt, lane, acc);
#pragma unroll
				for (int i = 0; i < C::MT; i++)
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
#pragma unroll
						for (int j = 0; j < 4; j++)
							acc[i][n][j] = static_cast<float>(relu_half(acc[i][n][j]));
				__syncthreads();
				channel_sums<F>(acc, wt, lane, valid_bits, s_sum);
				__syncthreads();
				if (tid < F)
				{
					float s = 0.0f;
					for (int g = 0; g < C::PG; g++)
						s += s_sum[g * F + tid];
					s_vec[tid] = s * p.inv_hw;
				}
				dense(s_vec, F, f_heads + L::FH_WV2, VALUE_HIDDEN, f_heads + L::FH_BV2, VALUE_HIDDEN, s_hid, s_part, 1, tid);
				dense(s_hid, VALUE_HIDDEN, f_heads + L::FH_WV3, 4, f_heads + L::FH_BV3, 3, s_vec, s_part, 0, tid);
				if (tid == 0)
				{
					const float z0 = s_vec[0], z1 = s_vec[1], z2 = s_vec[2];
					const float mx = fmaxf(z0, fmaxf(z1, z2));
					const float e0 = __expf(z0 - mx), e1 = __expf(z1 - mx), e2 = __expf(z2 - mx);
					const float inv = 1.0f / (e0 + e1 + e2);
					p.value[static_cast<size_t>(b) * 3 + 0] = e0 * inv;
					p.value[static_cast<size_t>(b) * 3 + 1] = e1 * inv;
					p.value[static_cast<size_t>(b) * 3 + 2] = e2 * inv;
				}
			}
			// ---- action-values head: 1x1 F -> F + ReLU folded with the 1x1 F -> 3, softmax over the 3 per cell ----
			if (p.q != nullptr)
			{
				AGX_CNX_LANE();
				floatx4 acc[C::MT][C::NTW];
				init_bias<F>(f_heads + L::FH_BQ1, wt, lane, acc);
				mac1x1<F>(plane, reinterpret_cast<const half8*>(h_heads + 2 * L::H_W), wt, lane, acc);
				float part[3][C::NTW];
#pragma unroll
				for (int o = 0; o < 3; o++)
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
						part[o][n] = 0.0f;
#pragma unroll
				for (int i = 0; i < C::MT; i++)
				{
					const float *wq = f_heads + L::FH_WQ2 + ((wt.mg * C::MT + i) * 16 + 4 * q4) * 4;
#pragma unroll
					for (int j = 0; j < 4; j++)
					{
						const floatx4 w = *reinterpret_cast<const floatx4*>(wq + j * 4);
#pragma unroll
						for (int n = 0; n < C::NTW; n++)
						{
							const float t = static_cast<float>(relu_half(acc[i][n][j]));
							part[0][n] = fmaf(t, w[0], part[0][n]);
							part[1][n] = fmaf(t, w[1], part[1][n]);
							part[2][n] = fmaf(t, w[2], part[2][n]);
						}
					}
				}
				__syncthreads(); // the policy head is done with the partial-sum rows
#pragma unroll
				for (int o = 0; o < 3; o++)
#pragma unroll
					for (int n = 0; n < C::NTW; n++)
					{
						float s = part[o][n];
						s += __shfl_xor(s, 16);
						s += __shfl_xor(s, 32);
						if (q4 == 0 && n < wt.count)
							hpart[(o * C::CG + wt.mg) * C::PS + p0 + n * 16] = s;
					}
				__syncthreads();
				if (tid < p.HW)
				{
					const float *bq2 = f_heads + L::FH_BQ2;
					const float z0 = bq2[0] + sum_partial_logits<C::CG, C::PS>(hpart, tid);
					const float z1 = bq2[1] + sum_partial_logits<C::CG, C::PS>(hpart + C::CG * C::PS, tid);
					const float z2 = bq2[2] + sum_partial_logits<C::CG, C::PS>(hpart + 2 * C::CG * C::PS, tid);
					const float2 win_draw = softmax3_win_draw(z0, z1, z2);
					float *out = p.q + (static_cast<size_t>(b) * p.HW + tid) * 2;
					out[0] = win_draw.x;
					out[1] = win_draw.y;
				}
			}
			// ---- moves-left head: 1x1 F -> 32 + ReLU (2 channel tiles x 4 position groups), mean, dense 32 -> 128 + ReLU, dense 128 -> HW, softmax ----
			if (p.m != nullptr)
			{
				const int lane_own = own(lane), r = lane_own & 15, q4 = lane_own >> 4;
				const int mt = __builtin_amdgcn_readfirstlane(wave & 1), pg4 = __builtin_amdgcn_readfirstlane(wave >> 1);
				const int first = pg4 * p.ntw4, left = p.NT - first;
				const int count4 = (left < 0) ? 0 : ((left < p.ntw4) ? left : p.ntw4);
				const int q0 = ((count4 > 0) ? first : 0) * 16 + r;
				const half8 *wm1 = reinterpret_cast<const half8*>(h_heads + 3 * L::H_W);
				const float *bm1 = f_heads + L::FH_BM1;
				floatx4 acc[C::NTW4];
				const floatx4 bv = *reinterpret_cast<const floatx4*>(bm1 + mt * 16 + 4 * q4);
#pragma unroll
				for (int n = 0; n < C::NTW4; n++)
					acc[n] = bv;
#pragma unroll
				for (int kc = 0; kc < C::KC; kc++)
				{
					const half8 a = wm1[(kc * 2 + mt) * 64 + lane_own];
					const char *src = plane + C::offset(q0, kc * 4 + q4);
#pragma unroll
					for (int n = 0; n < C::NTW4; n++)
						if (n < count4)
							acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, *reinterpret_cast<const half8*>(src + n * 16 * C::POS_BYTES), acc[n], 0, 0, 0);
				}
				mfma_settle(acc);
				floatx4 s { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
				for (int n = 0; n < C::NTW4; n++)
					if (n < count4 && q0 + n * 16 < p.HW)
#pragma unroll
						for (int j = 0; j < 4; j++)
							s[j] += static_cast<float>(relu_half(acc[n][j]));
#pragma unroll
				for (int o = 1; o < 16; o <<= 1)
				{
					s[0] += __shfl_xor(s[0], o);
					s[1] += __shfl_xor(s[1], o);
					s[2] += __shfl_xor(s[2], o);
					s[3] += __shfl_xor(s[3], o);
				}
				__syncthreads();
				if (r == 0)
					*reinterpret_cast<floatx4*>(s_sum + pg4 * ML_FILTERS + mt * 16 + 4 * q4) = s;
				__syncthreads();
				if (tid < ML_FILTERS)
					s_vec[tid] = (((s_sum[tid] + s_sum[ML_FILTERS + tid]) + s_sum[2 * ML_FILTERS + tid]) + s_sum[3 * ML_FILTERS + tid]) * p.inv_hw;
				const float *wm3 = f_heads + L::FH_WM3;
				dense(s_vec, ML_FILTERS, f_heads + L::FH_WM2, ML_HIDDEN, f_heads + L::FH_BM2, ML_HIDDEN, s_hid, s_part, 1, tid);
				dense(s_hid, ML_HIDDEN, wm3, p.HW, wm3 + static_cast<size_t>(ML_HIDDEN) * p.HW, p.HW, s_logit, s_part, 0, tid);
				const float logit = (tid < p.HW) ? s_logit[tid] : -3.0e38f;
				const float mx = block_reduce_max(logit, red, tid);
				const float e = (tid < p.HW) ? __expf(logit - mx) : 0.0f;
				const float sum = block_reduce_sum(e, red, tid);
				if (tid < p.HW)
					p.m[static_cast<size_t>(b) * p.HW + tid] = e / sum;
			}
		}
#undef AGX_CNX_LANE
	}

	template<int F>
	void pack_blob(const AgxNetDesc &d, int moves_left, const float *ptr, std::vector<half_t> &h, std::vector<float> &f)
	{
		typedef Layout<F> L;
		const int HW = d.rows * d.cols;
		auto floats = [&](int n, int padded = 0)
		{
			f.insert(f.end(), ptr, ptr + n);
			f.insert(f.end(), (padded > n) ? padded - n : 0, 0.0f);
			ptr += n;
		};
		auto halves = [&](int n)
		{
			for (int i = 0; i < n; i++)
				h.push_back(static_cast<half_t>(ptr[i]));
			ptr += n;
		};
		auto conv1x1 = [&](int cout)
		{ // [cin / 32][cout / 16][lane][8]
			pack_conv(ptr, 1, F, cout, h);
			ptr += F * cout;
		};
		auto rows_padded = [&](int rows, int n, int padded)
		{ // [rows][n] -> [rows][padded]
			for (int i = 0; i < rows; i++)
				floats(n, padded);
		};
		pack_conv5x5_raw(ptr, F, h);
		ptr += 25 * 8 * F;
		floats(F);
		for (int b = 0; b < d.blocks; b++)
		{
			halves(49 * F);  // wd
			floats(F);       // bd
			conv1x1(F);      // w1
			floats(F);       // b1
			conv1x1(F);      // w2
			floats(F);       // b2
			floats(F * F);   // ws1
			floats(F);       // bs1
			floats(F * F);   // ws2
			floats(F);       // bs2
		}
		// the heads' fp16 parts are wp1, wv1, wq1, wm1; the canonical order is policy, value, q, m with each head's parts together
		const float *policy = ptr, *value = policy + F * F + F + F + 1, *q = value + F * F + F + F * VALUE_HIDDEN + VALUE_HIDDEN + VALUE_HIDDEN * 3 + 3,
				*m = q + F * F + F + F * 3 + 3;
		ptr = policy;
		conv1x1(F);
		ptr = value;
		conv1x1(F);
		ptr = q;
		conv1x1(F);
		if (moves_left)
		{
			ptr = m;
			conv1x1(ML_FILTERS);
		}
		const size_t f_heads = f.size();
		ptr = policy + F * F;
		floats(F);                             // bp1
		floats(F);                             // wp2
		floats(1, 4);                          // bp2
		ptr = value + F * F;
		floats(F);                             // bv1
		floats(F * VALUE_HIDDEN);              // wv2
		floats(VALUE_HIDDEN);                  // bv2
		rows_padded(VALUE_HIDDEN, 3, 4);       // wv3
		floats(3, 4);                          // bv3
		ptr = q + F * F;
		floats(F);                             // bq1
		rows_padded(F, 3, 4);                  // wq2
		floats(3, 4);                          // bq2
		if (moves_left)
		{
			ptr = m + F * ML_FILTERS;
			floats(ML_FILTERS);                // bm1
			floats(ML_FILTERS * ML_HIDDEN);    // wm2
			floats(ML_HIDDEN);                 // bm2
			floats(ML_HIDDEN * HW);            // wm3
			floats(HW);                        // bm3
		}
		(void) f_heads;
		static_assert(L::FH_BM1 == 3 * F + 4 + F * VALUE_HIDDEN + VALUE_HIDDEN + VALUE_HIDDEN * 4 + 4 + F + F * 4 + 4, "the heads' fp32 parts as the kernel indexes them");
	}
}

namespace agx_cnx
{
	struct Net
	{
			AgxNetDesc desc;
			int moves_left = 0;
			void *d_h = nullptr, *d_f = nullptr;
	};

	bool supported(const AgxNetDesc &d, int moves_left)
	{
		return d.rows >= MIN_SIDE && d.rows <= MAX_SIDE && d.cols >= MIN_SIDE && d.cols <= MAX_SIDE && (d.filters == 64 || d.filters == 128) && d.blocks >= 0
				&& d.in_channels == 8 && d.action_values == 1 && d.value_hidden == VALUE_HIDDEN && (moves_left == 0 || moves_left == 1);
	}

	size_t blob_floats(const AgxNetDesc &d, int moves_left)
	{
		const size_t F = d.filters, HW = static_cast<size_t>(d.rows) * d.cols;
		size_t n = 25 * 8 * F + F;
		n += static_cast<size_t>(d.blocks) * (49 * F + F + 2 * (F * F + F) + 2 * (F * F + F));
		n += F * F + F + F + 1;
		n += F * F + F + F * VALUE_HIDDEN + VALUE_HIDDEN + VALUE_HIDDEN * 3 + 3;
		n += F * F + F + F * 3 + 3;
		if (moves_left)
			n += F * ML_FILTERS + ML_FILTERS + ML_FILTERS * ML_HIDDEN + ML_HIDDEN + ML_HIDDEN * HW + HW;
		return n;
	}

	void destroy(Net *net)
	{
		if (net == nullptr)
			return;
		if (net->d_h != nullptr)
			(void) hipFree(net->d_h);
		if (net->d_f != nullptr)
			(void) hipFree(net->d_f);
		delete net;
	}

	int load(const AgxNetDesc &desc, int moves_left, const float *h_blob, Net **out)
	{
		AGX_REQUIRE(supported(desc, moves_left) && h_blob != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_net_load_weights: invalid ConvNeXt network");
		std::vector<half_t> h;
		std::vector<float> f;
		if (desc.filters == 128)
			pack_blob<128>(desc, moves_left, h_blob, h, f);
		else
			pack_blob<64>(desc, moves_left, h_blob, h, f);
		Net *net = new Net();
		net->desc = desc;
		net->moves_left = moves_left;
		hipError_t e = hipMalloc(&net->d_h, h.size() * sizeof(half_t));
		if (e == hipSuccess)
			e = hipMalloc(&net->d_f, f.size() * sizeof(float));
		if (e == hipSuccess)
			e = hipMemcpy(net->d_h, h.data(), h.size() * sizeof(half_t), hipMemcpyHostToDevice);
		if (e == hipSuccess)
			e = hipMemcpy(net->d_f, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice);
		if (e != hipSuccess)
		{
			destroy(net);
			agx::set_error("agx_net_load_weights: %s", hipGetErrorString(e));
			return AGX_ERR_HIP;
		}
		*out = net;
		return AGX_OK;
	}

	int launch(const Net *net, int grid, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int batch, float *d_policy, float *d_value,
			float *d_action_values, float *d_moves_left, hipStream_t stream)
	{
		AGX_REQUIRE(net != nullptr && grid > 0, AGX_ERR_STATE, "agx_nn_forward: ConvNeXt weights not loaded");
		const AgxNetDesc &d = net->desc;
		Params p;
		p.h = static_cast<const half_t*>(net->d_h);
		p.f = static_cast<const float*>(net->d_f);
		p.features = d_features;
		p.slot_list = d_slot_list;
		p.count_ptr = d_count;
		p.policy = d_policy;
		p.value = d_value;
		p.q = d_action_values;
		p.m = d_moves_left;
		p.blocks = d.blocks;
		p.batch = batch;
		p.rows = d.rows;
		p.cols = d.cols;
		p.HW = d.rows * d.cols;
		p.NT = (p.HW + 15) / 16;
		const int pg = (d.filters == 128) ? Cfg<128>::PG : Cfg<64>::PG;
		p.ntw = (p.NT + pg - 1) / pg;
		p.ntw4 = (p.NT + 3) / 4;
		p.S5 = d.cols + 4;
		p.npos5 = (d.rows + 4) * p.S5 + 4;
		p.inv_hw = 1.0f / static_cast<float>(p.HW);
		const dim3 g(grid), t(512);
		if (d.filters == 128)
			hipLaunchKernelGGL((nn_convnext_kernel<128>), g, t, 0, stream, p);
		else
			hipLaunchKernelGGL((nn_convnext_kernel<64>), g, t, 0, stream, p);
		AGX_HIP_CHECK(hipGetLastError());
		return AGX_OK;
	}
}
