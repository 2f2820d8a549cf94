/*
 * nn_layered.hip — the layered residual towers: ResnetPV / ResnetPVraw / ResnetPVQ with 192 .. 512 filters (and 64 / 128 with AGX_NN_LAYERED=1).
 *
 * The other tower kernels carry a board through the whole network in one LDS-resident activation plane, which ends at 128 filters.  Here the
 * activations live in global memory and a layer boundary is a kernel boundary:
 *
 *   planes   two per stream, X and Y: fp16, [board][F / 32][NPOS][32] — NHWC cut into the 32-channel chunks of an MFMA k-step, so that the B
 *            fragment of 16 consecutive cells is 1 KB of consecutive bytes (cell-major NHWC it is 16 pieces of 64 B, a cache line each: measured
 *            at 10 x 256 that layout ran at 0.15 of the MFMA peak with the vector memory pipe as the limit).  A board is stored like the
 *            run-time-shaped kernel's plane: row stride S = cols + 1 (the spare column is the left / right halo), S + 1 cells in front of and
 *            behind the rows, so that the nine taps of a 3x3 convolution are the flat offsets (dy - 1) S + (dx - 1).  Halo cells are zeroed when
 *            the planes are allocated and never written.
 *   layer    conv3x3_layer_kernel: out = act(bias (+ residual) + W * in), an implicit GEMM.  A wave owns 64 positions x 64 output channels
 *            (4 x 4 MFMA 16x16x32 tiles) of one board and walks K = 9 taps x Cin / 32 in a fixed order, both operands straight from global
 *            memory (L2 / Infinity Cache at pool batch sizes), the next step's fragments requested in front of the current step's MFMAs.  No
 *            LDS, no barrier: waves are independent, the list of (board, position chunk, channel chunk) items is walked with a grid stride.
 *   input    conv5x5_input_kernel: the same wave tile, B fragments unpacked from the feature words on the fly.
 *   block    Y = relu(conv(X)); X = relu(X + conv(Y)) in place: an element of X is read (as residual) and written by the same lane only.
 *   heads    policy: conv X -> Y, then heads_kernel (1x1 F -> 1 + board softmax; also the value head's 1x1 F -> 4 from X);
 *            value: value_head_kernel (nn_device.hpp) once over the launch; action values: conv + tanh X -> Y, then q_kernel.
 *
 * Numerics (the contract of nn_any_board_kernel.hpp): fp16 for what feeds the matrix cores, fp32 accumulation starting from the bias
 * (+ residual), one rounding to fp16 per stored activation, the last 1x1 of policy / q and all biases in fp32, q's tanh rounded to fp16.
 * Every sum's order is fixed by the network and the board shape: a position's outputs do not depend on the batch, its place in it, the grid
 * or the launch width.
 */
#include "agx_internal.hpp"
#include "nn_device.hpp"
#include "nn_pack.hpp"
#include "nn_any_board.hpp"
#include "nn_resnet.hpp"
#include "nn_layered.hpp"

#include <vector>
#include <mutex>
#include <cmath>

namespace
{
	constexpr int NTW = 4, MTW = 4;       // a wave's tile: NTW 16-position tiles x MTW 16-channel tiles
	constexpr int WAVES = 4;              // waves of a layer workgroup (independent of each other)
	constexpr int WG_PER_CU = 2;          // layer workgroups per compute unit of the launch width (8 waves, 2 per SIMD)
	constexpr size_t PLANE_BUDGET = static_cast<size_t>(128) << 20; // bytes of both planes together (inside the 256 MB Infinity Cache) ...
	constexpr int MIN_PLANE_BOARDS = 256; // ... but never fewer boards than this per slice

	enum Epilogue
	{
		RELU,     // bias + ReLU
		RES_RELU, // bias + residual + ReLU
		TANH      // bias + tanh
	};

	/* a board in a plane (nn_layered.hpp) */
	struct Shape
	{
			int rows, cols;
			int s;    // row stride in cells
			int nt;   // 16-position tiles of the output
			int npos; // stored cells
			int pc;   // position chunks of NTW tiles
	};
	Shape shape_of(int rows, int cols)
	{
		Shape g;
		g.rows = rows;
		g.cols = cols;
		g.s = cols + 1;
		g.nt = (rows * g.s + 15) / 16;
		g.npos = g.nt * 16 + 2 * g.s + 2;
		g.pc = (g.nt + NTW - 1) / NTW;
		return g;
	}

	/* the boards of one slice of a launch: list entries first .. first + boards - 1 */
	struct Slice
	{
			const int *slot_list; // optional: list entry i is slot slot_list[i]
			const int *count_ptr; // optional: entries of the list, read on the device
			int batch;            // ... capped at this
			int first;
			int capacity;         // boards the planes hold
	};
	__device__ __forceinline__ int slice_boards(const Slice &sl)
	{
		const int n = (sl.count_ptr != nullptr) ? min(*sl.count_ptr, sl.batch) : sl.batch;
		return max(0, min(n - sl.first, sl.capacity));
	}

	/* a wave's work item -> (board of the slice, first tile, first channel tile); false behind the last one */
	struct Item
	{
			int board, tile0, mt0;
	};
	__device__ __forceinline__ Item item_of(int item, int pc, int cc)
	{
		Item it;
		it.mt0 = (item % cc) * MTW;
		it.tile0 = ((item / cc) % pc) * NTW;
		it.board = item / (cc * pc);
		return it;
	}

	/* halves from a board's first to channels c .. c + 7 (c a multiple of 8, or of 4 for four channels) of stored cell `cell` */
	__host__ __device__ __forceinline__ size_t plane_at(int npos, int cell, int c)
	{
		return (static_cast<size_t>(c >> 5) * npos + cell) * 32 + (c & 31);
	}

	/* Epilogue of a wave tile: lane holds out-channels ch .. ch + 3 (tile i) of position r of tile n.  acc already holds bias (+ residual). */
	template<int EPI>
	__device__ __forceinline__ void store_tile(const floatx4 &acc, half_t *out_cell)
	{
		half4 h;
#pragma unroll
		for (int e = 0; e < 4; e++)
			h[e] = static_cast<half_t>((EPI == TANH) ? tanhf(acc[e]) : fmaxf(acc[e], 0.0f));
		*reinterpret_cast<half4*>(out_cell) = h;
	}

	/*
	 * One 3x3 convolution layer Cin -> Cout over the boards of a slice.  w: pack_conv's [tap][Cin / 32][Cout / 16][lane] fragments, bias [Cout];
	 * in, out and res are planes of cin and cout channels (res may be out: the block's second convolution runs in place).
	 */
	template<int EPI>
	__global__ __launch_bounds__(64 * WAVES) void conv3x3_layer_kernel(const half_t *in, half_t *out, const half_t *res, const half8 *__restrict__ w,
			const float *__restrict__ bias, int cin, int cout, Shape g, Slice sl)
	{
		const int lane = threadIdx.x & 63, r = lane & 15, q4 = lane >> 4;
		const int kcs = cin / 32, mtiles = cout / 16, cc = mtiles / MTW;
		const int items = slice_boards(sl) * g.pc * cc;
		const int steps = 9 * kcs;
		for (int item = blockIdx.x * WAVES + (threadIdx.x >> 6); item < items; item += gridDim.x * WAVES)
		{
			const Item it = item_of(item, g.pc, cc);
			const half_t *in_b = in + static_cast<size_t>(it.board) * g.npos * cin;
			const size_t out_b = static_cast<size_t>(it.board) * g.npos * cout;
			int cell[NTW];   // stored cell of this lane's position of tile n (a tile behind the last one repeats the last: computed, never stored)
			bool valid[NTW];
			floatx4 acc[MTW][NTW];
#pragma unroll
			for (int n = 0; n < NTW; n++)
			{
				const int tile = min(it.tile0 + n, g.nt - 1);
				const int q = tile * 16 + r, row = q / g.s, col = q - row * g.s;
				cell[n] = q + g.s + 1;
				valid[n] = (it.tile0 + n < g.nt) && row < g.rows && col < g.cols;
			}
#pragma unroll
			for (int i = 0; i < MTW; i++)
			{
				const int ch = (it.mt0 + i) * 16 + 4 * q4;
				const floatx4 b = *reinterpret_cast<const floatx4*>(bias + ch);
#pragma unroll
				for (int n = 0; n < NTW; n++)
				{
					acc[i][n] = b;
					if (EPI == RES_RELU && valid[n])
					{
						const half4 x = *reinterpret_cast<const half4*>(res + out_b + plane_at(g.npos, cell[n], ch));
#pragma unroll
						for (int e = 0; e < 4; e++)
							acc[i][n][e] = static_cast<float>(x[e]) + b[e];
					}
				}
			}
			// k-loop: step = (tap, 32-channel chunk), taps outermost; the fragments of step + 1 are requested in front of the MFMAs of step
			const half8 *wp = w + it.mt0 * 64 + lane;
			const half_t *bp[NTW];
#pragma unroll
			for (int n = 0; n < NTW; n++)
				bp[n] = in_b + plane_at(g.npos, cell[n], 8 * q4);
			half8 a_cur[MTW], b_cur[NTW], a_nxt[MTW], b_nxt[NTW];
			int tap = 0, kc = 0;
			auto request = [&](half8 (&a)[MTW], half8 (&b)[NTW])
			{
				const int off = (kc * g.npos + (tap / 3 - 1) * g.s + (tap % 3 - 1)) * 32;
#pragma unroll
				for (int i = 0; i < MTW; i++)
					a[i] = wp[(static_cast<size_t>(tap * kcs + kc) * mtiles + i) * 64];
#pragma unroll
				for (int n = 0; n < NTW; n++)
					b[n] = *reinterpret_cast<const half8*>(bp[n] + off);
			};
			request(a_cur, b_cur);
			for (int step = 0; step < steps; step++)
			{
				if (step + 1 < steps)
				{
					if (++kc == kcs)
					{
						kc = 0;
						tap++;
					}
					request(a_nxt, b_nxt);
				}
#pragma unroll
				for (int i = 0; i < MTW; i++)
#pragma unroll
					for (int n = 0; n < NTW; n++)
						acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_cur[i], b_cur[n], acc[i][n], 0, 0, 0);
#pragma unroll
				for (int i = 0; i < MTW; i++)
					a_cur[i] = a_nxt[i];
#pragma unroll
				for (int n = 0; n < NTW; n++)
					b_cur[n] = b_nxt[n];
			}
			mfma_settle(acc);
#pragma unroll
			for (int i = 0; i < MTW; i++)
#pragma unroll
				for (int n = 0; n < NTW; n++)
					if (valid[n])
						store_tile<EPI>(acc[i][n], out + out_b + plane_at(g.npos, cell[n], (it.mt0 + i) * 16 + 4 * q4));
		}
	}

	/*
	 * The input block: feature words -> conv5x5 + bias + ReLU -> plane X, the wave tile of the layer kernel.  B fragments are unpacked from
	 * the words as they are needed: with 32 input channels a k-step is a tap and a lane's eight channels are byte (lane >> 4) of the cell's
	 * word (w: pack_conv's [25][1][F / 16][lane]); with 8 (RAW) a k-step is four horizontal taps of the low byte (w: pack_conv5x5_raw's
	 * [10][F / 16][lane], taps beyond the fifth zero).  Cells off the board are zero.
	 */
	template<bool RAW>
	__global__ __launch_bounds__(64 * WAVES) void conv5x5_input_kernel(const uint32_t *__restrict__ features, half_t *__restrict__ out, const half8 *__restrict__ w,
			const float *__restrict__ bias, int cout, Shape g, Slice sl)
	{
		const int lane = threadIdx.x & 63, r = lane & 15, q4 = lane >> 4;
		const int mtiles = cout / 16, cc = mtiles / MTW;
		const int items = slice_boards(sl) * g.pc * cc;
		const int hw = g.rows * g.cols;
		constexpr int STEPS = RAW ? 10 : 25;
		for (int item = blockIdx.x * WAVES + (threadIdx.x >> 6); item < items; item += gridDim.x * WAVES)
		{
			const Item it = item_of(item, g.pc, cc);
			const int entry = sl.first + it.board;
			const int slot = (sl.slot_list != nullptr) ? sl.slot_list[entry] : entry;
			const uint32_t *f = features + static_cast<size_t>(slot) * hw;
			const size_t out_b = static_cast<size_t>(it.board) * g.npos * cout;
			int row[NTW], col[NTW], cell[NTW];
			bool valid[NTW];
			floatx4 acc[MTW][NTW];
#pragma unroll
			for (int n = 0; n < NTW; n++)
			{
				const int tile = min(it.tile0 + n, g.nt - 1);
				const int q = tile * 16 + r;
				row[n] = q / g.s;
				col[n] = q - row[n] * g.s;
				cell[n] = q + g.s + 1;
				valid[n] = (it.tile0 + n < g.nt) && row[n] < g.rows && col[n] < g.cols;
			}
#pragma unroll
			for (int i = 0; i < MTW; i++)
			{
				const floatx4 b = *reinterpret_cast<const floatx4*>(bias + (it.mt0 + i) * 16 + 4 * q4);
#pragma unroll
				for (int n = 0; n < NTW; n++)
					acc[i][n] = b;
			}
			const half8 *wp = w + it.mt0 * 64 + lane;
			for (int step = 0; step < STEPS; step++)
			{
				const int dy = RAW ? step / 2 : step / 5;
				const int dx = RAW ? 4 * (step % 2) + q4 : step % 5;
				half8 a[MTW], b[NTW];
#pragma unroll
				for (int i = 0; i < MTW; i++)
					a[i] = wp[(static_cast<size_t>(step) * mtiles + i) * 64];
#pragma unroll
				for (int n = 0; n < NTW; n++)
				{
					const int rr = row[n] + dy - 2, c2 = col[n] + dx - 2;
					uint32_t bits = 0;
					if (dx < 5 && rr >= 0 && rr < g.rows && c2 >= 0 && c2 < g.cols)
						bits = RAW ? (f[rr * g.cols + c2] & 0xFFu) : ((f[rr * g.cols + c2] >> (8 * q4)) & 0xFFu);
					const uint4 u = unpack_feature_byte(bits);
					b[n] = __builtin_bit_cast(half8, u);
				}
#pragma unroll
				for (int i = 0; i < MTW; i++)
#pragma unroll
					for (int n = 0; n < NTW; n++)
						acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[n], acc[i][n], 0, 0, 0);
			}
			mfma_settle(acc);
#pragma unroll
			for (int i = 0; i < MTW; i++)
#pragma unroll
				for (int n = 0; n < NTW; n++)
					if (valid[n])
						store_tile<RELU>(acc[i][n], out + out_b + plane_at(g.npos, cell[n], (it.mt0 + i) * 16 + 4 * q4));
		}
	}

	constexpr int HEAD_THREADS = 512; // a board's cells, one per thread (HW <= 400); block_reduce_* are over 8 waves

	/*
	 * Behind the policy convolution, one workgroup per board: the policy head's 1x1 F -> 1 (fp32 weights, bias last) over plane P and the
	 * softmax over the board; the value head's 1x1 F -> 4 + ReLU over plane X (weights rounded to fp16 like the fragments of the other towers,
	 * fp32 sums starting from the bias) into the launch's value-head input rows [entry][kpad].  Channels are added in ascending order.
	 */
	__global__ __launch_bounds__(HEAD_THREADS) void heads_kernel(const half_t *__restrict__ x, const half_t *__restrict__ p, const float *__restrict__ wp2, float bp2,
			const float *__restrict__ wv1, float bv10, float bv11, float bv12, float bv13, int filters, Shape g, Slice sl, int kpad, half_t *__restrict__ vhead,
			float *__restrict__ policy)
	{
		__shared__ float s_wp2[agx_lay::MAX_FILTERS];
		__shared__ float s_wv1[agx_lay::MAX_FILTERS * 4];
		__shared__ float red[8];
		const int tid = threadIdx.x;
		const int boards = slice_boards(sl);
		if (static_cast<int>(blockIdx.x) >= boards)
			return;
		for (int i = tid; i < filters; i += HEAD_THREADS)
			s_wp2[i] = wp2[i];
		for (int i = tid; i < filters * 4; i += HEAD_THREADS)
			s_wv1[i] = static_cast<float>(static_cast<half_t>(wv1[i]));
		__syncthreads();
		const int hw = g.rows * g.cols;
		const int row = tid / g.cols, col = tid - row * g.cols;
		const int cell = row * g.s + col + g.s + 1;
		for (int board = blockIdx.x; board < boards; board += gridDim.x)
		{
			const int entry = sl.first + board;
			const int slot = (sl.slot_list != nullptr) ? sl.slot_list[entry] : entry;
			float logit = -INFINITY;
			if (tid < hw)
			{
				const size_t base = static_cast<size_t>(board) * g.npos * filters;
				float sum = 0.0f;
				floatx4 v = { bv10, bv11, bv12, bv13 };
				for (int c = 0; c < filters; c += 8)
				{
					const half8 hp = *reinterpret_cast<const half8*>(p + base + plane_at(g.npos, cell, c));
					const half8 hx = *reinterpret_cast<const half8*>(x + base + plane_at(g.npos, cell, c));
#pragma unroll
					for (int j = 0; j < 8; j++)
					{
						sum += static_cast<float>(hp[j]) * s_wp2[c + j];
						const float xv = static_cast<float>(hx[j]);
#pragma unroll
						for (int u = 0; u < 4; u++)
							v[u] += xv * s_wv1[(c + j) * 4 + u];
					}
				}
				logit = sum + bp2;
				half4 hv;
#pragma unroll
				for (int u = 0; u < 4; u++)
					hv[u] = static_cast<half_t>(fmaxf(v[u], 0.0f));
				*reinterpret_cast<half4*>(vhead + static_cast<size_t>(entry) * kpad + tid * 4) = hv;
			}
			const float m = block_reduce_max(logit, red, tid);
			const float e = (tid < hw) ? __expf(logit - m) : 0.0f;
			const float total = block_reduce_sum(e, red, tid);
			if (tid < hw)
				policy[static_cast<size_t>(slot) * hw + tid] = e * (1.0f / total);
		}
	}

	/* Behind the action-values convolution (+ tanh) into plane T: its 1x1 F -> 3 (fp32 weights wq2 [F][4], 3 used; bias last) and the softmax
	 * over the three per cell; stores (win, draw). */
	__global__ __launch_bounds__(HEAD_THREADS) void q_kernel(const half_t *__restrict__ t, const float *__restrict__ wq2, float bq0, float bq1, float bq2, int filters,
			Shape g, Slice sl, float *__restrict__ q)
	{
		__shared__ float s_wq2[agx_lay::MAX_FILTERS * 4];
		const int tid = threadIdx.x;
		const int boards = slice_boards(sl);
		if (static_cast<int>(blockIdx.x) >= boards)
			return;
		for (int i = tid; i < filters * 4; i += HEAD_THREADS)
			s_wq2[i] = wq2[i];
		__syncthreads();
		const int hw = g.rows * g.cols;
		if (tid >= hw)
			return;
		const int row = tid / g.cols, col = tid - row * g.cols;
		const int cell = row * g.s + col + g.s + 1;
		for (int board = blockIdx.x; board < boards; board += gridDim.x)
		{
			const int entry = sl.first + board;
			const int slot = (sl.slot_list != nullptr) ? sl.slot_list[entry] : entry;
			const size_t base = static_cast<size_t>(board) * g.npos * filters;
			float z[3] = { 0.0f, 0.0f, 0.0f };
			for (int c = 0; c < filters; c += 8)
			{
				const half8 ht = *reinterpret_cast<const half8*>(t + base + plane_at(g.npos, cell, c));
#pragma unroll
				for (int j = 0; j < 8; j++)
				{
					const float tv = static_cast<float>(ht[j]);
#pragma unroll
					for (int o = 0; o < 3; o++)
						z[o] += tv * s_wq2[(c + j) * 4 + o];
				}
			}
			const float2 wd = softmax3_win_draw(z[0] + bq0, z[1] + bq1, z[2] + bq2);
			*reinterpret_cast<float2*>(q + (static_cast<size_t>(slot) * hw + tid) * 2) = wd;
		}
	}

	template<typename T>
	int upload(void **dst, const std::vector<T> &src)
	{
		AGX_HIP_CHECK(hipMalloc(dst, src.size() * sizeof(T)));
		AGX_HIP_CHECK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
		return AGX_OK;
	}
}

namespace agx_lay
{
	struct Net
	{
			AgxNetDesc desc;
			void *d_w_in = nullptr;    // input conv fragments (pack_conv / pack_conv5x5_raw)
			void *d_w_tower = nullptr; // 3x3 fragments (pack_conv): 2 * blocks layers, the policy conv, the action-values conv
			void *d_bias = nullptr;    // [1 + 2 * blocks + 1 (+ 1)][F]
			void *d_wp2 = nullptr;     // [F]
			void *d_wv1 = nullptr;     // [F][4]
			void *d_wv2 = nullptr;     // pack_value_dense
			void *d_bv2 = nullptr;     // [D]
			void *d_wv3 = nullptr;     // [D][3]
			void *d_wq2 = nullptr;     // [F][4] (3 used), only with desc.action_values
			float bp2 = 0.0f;
			float bv1[4] = { 0, 0, 0, 0 };
			float bv3[3] = { 0, 0, 0 };
			float bq2[3] = { 0, 0, 0 };
			// launches on different streams may overlap (pool slices driven from several streams share one network): a scratch per stream
			std::mutex scratch_mutex;
			struct StreamScratch
			{
					hipStream_t stream;
					void *planes;     // X and Y: 2 x [plane_boards][F / 32][npos][32] halves, halo cells zero
					int plane_boards;
					void *vhead;      // value-head inputs of one launch: [boards][kpad] halves, the padding zero
					int vhead_boards;
			};
			std::vector<StreamScratch> scratch_by_stream;
	};

	bool supported(const AgxNetDesc &d, int moves_left)
	{
		return moves_left == 0 && d.rows >= agx_any::MIN_SIDE && d.rows <= agx_any::MAX_SIDE && d.cols >= agx_any::MIN_SIDE && d.cols <= agx_any::MAX_SIDE
				&& d.filters >= MIN_FILTERS && d.filters <= MAX_FILTERS && d.filters % 64 == 0 && d.blocks >= 0
				&& (d.in_channels == 32 || (d.in_channels == 8 && d.action_values == 0))
				&& d.value_hidden == ((2 * d.filters < 256) ? 2 * d.filters : 256) && (d.action_values == 0 || d.action_values == 1);
	}

	size_t blob_floats(const AgxNetDesc &d)
	{
		return agx_res::blob_floats(d);
	}

	int plane_boards(const AgxNetDesc &d)
	{
		const size_t per_board = static_cast<size_t>(2) * shape_of(d.rows, d.cols).npos * d.filters * sizeof(half_t);
		const size_t n = PLANE_BUDGET / per_board;
		return (n < static_cast<size_t>(MIN_PLANE_BOARDS)) ? MIN_PLANE_BOARDS : static_cast<int>(n);
	}

	void destroy(Net *net)
	{
		if (net == nullptr)
			return;
		for (void *p : { net->d_w_in, net->d_w_tower, net->d_bias, net->d_wp2, net->d_wv1, net->d_wv2, net->d_bv2, net->d_wv3, net->d_wq2 })
			if (p != nullptr)
				(void) hipFree(p);
		for (auto &slice : net->scratch_by_stream)
		{
			if (slice.planes != nullptr)
				(void) hipFree(slice.planes);
			if (slice.vhead != nullptr)
				(void) hipFree(slice.vhead);
		}
		delete net;
	}

	int load(const AgxNetDesc &desc, const float *h_blob, Net **out)
	{
		AGX_REQUIRE(supported(desc, 0) && h_blob != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_net_load_weights: invalid layered residual network");
		Net *net = new Net();
		net->desc = desc;
		const int F = desc.filters, C = desc.in_channels, HW = desc.rows * desc.cols, D = desc.value_hidden;
		const float *ptr = h_blob;
		std::vector<half_t> w_in, w_tower, wv2;
		std::vector<float> bias, wq2;

		if (C == 8)
			pack_conv5x5_raw(ptr, F, w_in);
		else
			pack_conv(ptr, 25, C, F, w_in);
		ptr += 25 * C * F;
		bias.insert(bias.end(), ptr, ptr + F);
		ptr += F;
		auto conv3x3 = [&]()
		{
			pack_conv(ptr, 9, F, F, w_tower);
			ptr += 9 * F * F;
			bias.insert(bias.end(), ptr, ptr + F);
			ptr += F;
		};
		for (int l = 0; l < 2 * desc.blocks + 1; l++)
			conv3x3();
		const std::vector<float> wp2(ptr, ptr + F);
		ptr += F;
		net->bp2 = *ptr++;
		const std::vector<float> wv1(ptr, ptr + F * 4);
		ptr += F * 4;
		for (int i = 0; i < 4; i++)
			net->bv1[i] = *ptr++;
		pack_value_dense(ptr, HW, D, wv2);
		ptr += static_cast<size_t>(HW) * 4 * D;
		const std::vector<float> bv2(ptr, ptr + D);
		ptr += D;
		const std::vector<float> wv3(ptr, ptr + D * 3);
		ptr += D * 3;
		for (int i = 0; i < 3; i++)
			net->bv3[i] = *ptr++;
		if (desc.action_values)
		{
			conv3x3();
			wq2.assign(static_cast<size_t>(F) * 4, 0.0f);
			for (int c = 0; c < F; c++)
				for (int o = 0; o < 3; o++)
					wq2[c * 4 + o] = ptr[c * 3 + o];
			ptr += F * 3;
			for (int i = 0; i < 3; i++)
				net->bq2[i] = *ptr++;
		}
		int status = AGX_OK;
		if ((status = upload(&net->d_w_in, w_in)) != AGX_OK || (status = upload(&net->d_w_tower, w_tower)) != AGX_OK
				|| (status = upload(&net->d_bias, bias)) != AGX_OK || (status = upload(&net->d_wp2, wp2)) != AGX_OK
				|| (status = upload(&net->d_wv1, wv1)) != AGX_OK || (status = upload(&net->d_wv2, wv2)) != AGX_OK
				|| (status = upload(&net->d_bv2, bv2)) != AGX_OK || (status = upload(&net->d_wv3, wv3)) != AGX_OK
				|| (!wq2.empty() && (status = upload(&net->d_wq2, wq2)) != AGX_OK))
		{
			(void) hipGetLastError(); // (the failed call's error is in the status; the next launch must not find it)
			destroy(net);
			return status;
		}
		*out = net;
		return AGX_OK;
	}

	/* a fresh zeroed allocation of `bytes` in *slot (the old one, if any, freed behind the stream's work); *slot is null on failure */
	static int regrow(void **slot, size_t bytes, hipStream_t s)
	{
		if (*slot != nullptr)
		{
			AGX_HIP_CHECK(hipStreamSynchronize(s));
			AGX_HIP_CHECK(hipFree(*slot));
			*slot = nullptr;
		}
		void *fresh = nullptr;
		const hipError_t e = hipMalloc(&fresh, bytes);
		if (e != hipSuccess)
		{
			(void) hipGetLastError();
			AGX_REQUIRE(false, AGX_ERR_HIP, "agx_nn_forward: no device memory for %zu bytes of layered-tower scratch (%s)", bytes, hipGetErrorString(e));
		}
		const hipError_t z = hipMemsetAsync(fresh, 0, bytes, s);
		if (z != hipSuccess)
		{
			(void) hipFree(fresh);
			AGX_HIP_CHECK(z);
		}
		*slot = fresh;
		return AGX_OK;
	}

	int launch(Net *net, int width, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int batch, float *d_policy, float *d_value,
			float *d_action_values, hipStream_t s)
	{
		AGX_REQUIRE(net != nullptr && width > 0 && batch > 0, AGX_ERR_STATE, "agx_nn_forward: weights not loaded");
		const AgxNetDesc &d = net->desc;
		const int F = d.filters, blocks = d.blocks;
		const Shape g = shape_of(d.rows, d.cols);
		const int kpad = value_kpad(d.rows, d.cols);
		const int capacity = (batch < plane_boards(d)) ? batch : plane_boards(d);
		const size_t plane_halves = static_cast<size_t>(g.npos) * F; // per board
		half_t *x = nullptr, *y = nullptr, *vhead = nullptr;
		{
			std::lock_guard<std::mutex> lock(net->scratch_mutex);
			Net::StreamScratch *mine = nullptr;
			for (auto &slice : net->scratch_by_stream)
				if (slice.stream == s)
					mine = &slice;
			if (mine == nullptr)
			{
				net->scratch_by_stream.push_back(Net::StreamScratch { s, nullptr, 0, nullptr, 0 });
				mine = &net->scratch_by_stream.back();
			}
			if (mine->plane_boards < capacity)
			{ // grows to the largest launch seen on this stream; the halo cells are zeroed here and never written
				mine->plane_boards = 0;
				const int status = regrow(&mine->planes, 2 * plane_halves * capacity * sizeof(half_t), s);
				if (status != AGX_OK)
					return status;
				mine->plane_boards = capacity;
			}
			if (mine->vhead_boards < batch)
			{ // the k-padding stays zero: heads_kernel writes the first 4 HW halves of a row only
				mine->vhead_boards = 0;
				const int status = regrow(&mine->vhead, static_cast<size_t>(batch) * kpad * sizeof(half_t), s);
				if (status != AGX_OK)
					return status;
				mine->vhead_boards = batch;
			}
			x = static_cast<half_t*>(mine->planes);
			y = x + plane_halves * mine->plane_boards;
			vhead = static_cast<half_t*>(mine->vhead);
		}
		const half8 *w_tower = static_cast<const half8*>(net->d_w_tower);
		const float *bias = static_cast<const float*>(net->d_bias);
		const size_t layer_frags = static_cast<size_t>(9) * (F / 32) * (F / 16) * 64; // half8 fragments of one 3x3 layer
		const dim3 t(64 * WAVES), ht(HEAD_THREADS);
		for (int first = 0; first < batch; first += capacity)
		{
			const int boards = (batch - first < capacity) ? batch - first : capacity;
			const Slice sl { d_slot_list, d_count, batch, first, capacity };
			const int wave_items = boards * g.pc * (F / (16 * MTW));
			const int wanted = (wave_items + WAVES - 1) / WAVES;
			const dim3 lg((wanted < width * WG_PER_CU) ? wanted : width * WG_PER_CU), hg((boards < width) ? boards : width);
			if (d.in_channels == 8)
				hipLaunchKernelGGL(conv5x5_input_kernel<true>, lg, t, 0, s, d_features, x, static_cast<const half8*>(net->d_w_in), bias, F, g, sl);
			else
				hipLaunchKernelGGL(conv5x5_input_kernel<false>, lg, t, 0, s, d_features, x, static_cast<const half8*>(net->d_w_in), bias, F, g, sl);
			int layer = 0; // 3x3 layers behind the input conv
			for (int blk = 0; blk < blocks; blk++, layer += 2)
			{
				hipLaunchKernelGGL(conv3x3_layer_kernel<RELU>, lg, t, 0, s, x, y, nullptr, w_tower + layer * layer_frags, bias + (1 + layer) * F, F, F, g, sl);
				hipLaunchKernelGGL(conv3x3_layer_kernel<RES_RELU>, lg, t, 0, s, y, x, x, w_tower + (layer + 1) * layer_frags, bias + (2 + layer) * F, F, F, g, sl);
			}
			hipLaunchKernelGGL(conv3x3_layer_kernel<RELU>, lg, t, 0, s, x, y, nullptr, w_tower + layer * layer_frags, bias + (1 + layer) * F, F, F, g, sl);
			hipLaunchKernelGGL(heads_kernel, hg, ht, 0, s, x, y, static_cast<const float*>(net->d_wp2), net->bp2, static_cast<const float*>(net->d_wv1), net->bv1[0],
					net->bv1[1], net->bv1[2], net->bv1[3], F, g, sl, kpad, vhead, d_policy);
			if (d_action_values != nullptr)
			{
				layer++;
				hipLaunchKernelGGL(conv3x3_layer_kernel<TANH>, lg, t, 0, s, x, y, nullptr, w_tower + layer * layer_frags, bias + (1 + layer) * F, F, F, g, sl);
				hipLaunchKernelGGL(q_kernel, hg, ht, 0, s, y, static_cast<const float*>(net->d_wq2), net->bq2[0], net->bq2[1], net->bq2[2], F, g, sl, d_action_values);
			}
		}
		{ // the value head's dense layers for all boards of the launch
			const dim3 vg((batch + 15) / 16), vt(256);
#define AGX_LAUNCH_VALUE(DD) hipLaunchKernelGGL((value_head_kernel<DD>), vg, vt, 0, s, vhead, static_cast<const half8*>(net->d_wv2), static_cast<const float*>(net->d_bv2), \
		static_cast<const float*>(net->d_wv3), net->bv3[0], net->bv3[1], net->bv3[2], d_slot_list, d_count, batch, kpad, d_value)
			if (d.value_hidden == 256)
				AGX_LAUNCH_VALUE(256);
			else
				AGX_LAUNCH_VALUE(128);
#undef AGX_LAUNCH_VALUE
		}
		AGX_HIP_CHECK(hipGetLastError());
		return AGX_OK;
	}
}
