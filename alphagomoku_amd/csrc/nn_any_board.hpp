/*
 * nn_any_board.hpp — the run-time-shaped tower kernel (nn_any_board.hip: residual and bottleneck blocks in one frame) as the residual towers'
 * host code (agx_res in nn_forward.hip) sees it.
 */
#ifndef AGX_NN_ANY_BOARD_HPP_
#define AGX_NN_ANY_BOARD_HPP_

#include "agx_internal.hpp"

namespace agx_nn
{
	struct NetParams; // nn_device.hpp
}

namespace agx_any
{
	constexpr int MIN_SIDE = 5, MAX_SIDE = 20;

	/* the block kind of a tower, between the same input block and heads */
	enum Block
	{
		RESIDUAL,   // two 3x3 convolutions F -> F: ResnetPV / PVraw / PVQ
		BOTTLENECK  // 1x1 F -> F/2, 3x3 F/2 -> F/2, 3x3 F/2 -> F: BottleneckPV / BottleneckPVraw / BottleneckPVQ
	};

	/* bytes of residual scratch one workgroup of the persistent grid needs (the same for every board shape and block kind) */
	size_t skip_bytes_per_workgroup(int filters);
	/* The tower kernel (`grid` workgroups) for a launch record filled by agx_res::launch() on `stream`; an AGX_* status.  p.skip is
	 * grid x skip_bytes_per_workgroup(filters), p.vhead_x [batch][kpad] halves with the padding zero; weight fragments are in the tap-major order
	 * of pack_conv() (nn_pack.hpp): [tap][k-step][16-channel tile][lane][8], the raw input conv in pack_conv5x5_raw()'s.  p.w_tower holds per
	 * block W1, W2 (9 taps, F -> F) or W1 (1 tap, F -> F/2), W2 (9 taps, F/2 -> F/2), W3 (9 taps, F/2 -> F), then the policy conv and the
	 * action-values conv (9 taps, F -> F); p.bias is [F] of the input conv, per block [F][F] or [F/2][F/2][F], then [F] per head conv. */
	int launch(const agx_nn::NetParams &p, Block block, int rows, int cols, int filters, bool raw, int grid, int kpad, const uint32_t *d_features, float *d_policy,
			hipStream_t stream);
}

#endif /* AGX_NN_ANY_BOARD_HPP_ */
