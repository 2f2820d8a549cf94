/*
 * nn_bottleneck.hpp — the bottleneck tower kernel (nn_bottleneck.hip: BottleneckPV / BottleneckPVraw / BottleneckPVQ) as the residual towers'
 * host code (agx_res in nn_forward.hip) sees it: a block kind of agx_res::Net, launched in the place of the run-time-shaped residual kernel.
 */
#ifndef AGX_NN_BOTTLENECK_HPP_
#define AGX_NN_BOTTLENECK_HPP_

#include "agx_internal.hpp"

namespace agx_nn
{
	struct NetParams; // nn_device.hpp
}

namespace agx_btl
{
	/* bytes of residual scratch one workgroup of the persistent grid needs (the same for every board shape) */
	size_t skip_bytes_per_workgroup(int filters);
	/* The tower kernel (`grid` workgroups) for a launch record filled by agx_res::launch() on `stream`; an AGX_* status.  p.skip is
	 * grid x skip_bytes_per_workgroup(filters), p.vhead_x [batch][kpad] halves with the padding zero.  p.w_tower holds, in the tap-major order
	 * of pack_conv() (nn_pack.hpp), per block W1 (1 tap, F -> F/2), W2 (9 taps, F/2 -> F/2), W3 (9 taps, F/2 -> F), then the policy conv and the
	 * action-values conv (9 taps, F -> F); p.bias is [F] of the input conv, per block [F/2][F/2][F], then [F] per head conv. */
	int launch(const agx_nn::NetParams &p, int rows, int cols, int filters, bool raw, int grid, int kpad, const uint32_t *d_features, float *d_policy, hipStream_t stream);
}

#endif /* AGX_NN_BOTTLENECK_HPP_ */
