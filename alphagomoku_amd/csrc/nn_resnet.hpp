/*
 * nn_resnet.hpp — the residual towers (nn_forward.hip: the 15x15 and 20x20 kernels, the run-time-shaped one of nn_any_board.hip behind them, the
 * value head's dense layers) as nn_net.cpp sees them: the entry points of the C ABI dispatch here for an AgxNet whose architecture is
 * AGX_ARCH_RESNET — and, as a block kind of the same Net, the bottleneck towers (AGX_ARCH_BOTTLENECK: the bottleneck block of nn_any_board.hip's kernel between the
 * residual networks' input block and heads; `bottleneck` below).
 */
#ifndef AGX_NN_RESNET_HPP_
#define AGX_NN_RESNET_HPP_

#include "agx_internal.hpp"

namespace agx_res
{
	struct Net; // the packed weights of one residual network on the device and its per-stream scratch (opaque to nn_net.cpp)

	/* ResnetPV / ResnetPVQ / ResnetPVraw and BottleneckPV / BottleneckPVQ / BottleneckPVraw: boards 5..20 x 5..20, F in {64, 128}, 32 input channels, or 8 without the action-values head; no
	 * moves-left head */
	bool supported(const AgxNetDesc &desc, int moves_left);
	/* fp32 values of the canonical blob (layout: include/agx.h) */
	size_t blob_floats(const AgxNetDesc &desc, bool bottleneck = false);
	/* packs and uploads a canonical blob of blob_floats() values into a fresh Net, its residual scratch sized for a grid of num_cus workgroups;
	 * reads AGX_NN_ANY_BOARD and AGX_NN_SINGLE_PLANE.  *out replaces nothing (the caller destroys the old one) and is left alone on failure; an
	 * AGX_* status */
	int load(const AgxNetDesc &desc, int num_cus, const float *h_blob, Net **out, bool bottleneck = false);
	void destroy(Net *net);
	/* One launch of `grid` workgroups (at most load()'s num_cus) on `stream`, the value head's dense layers behind the tower: positions
	 * 0 .. batch - 1 (or the device-side list d_slot_list / *d_count, capped at batch).  d_action_values may be null (head skipped) and is for a network with that head only, which
	 * launch_forward() (nn_net.cpp) checks with the other arguments.  Finds or grows the stream's scratch in `net`. */
	int launch(Net *net, int grid, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int batch, float *d_policy, float *d_value,
			float *d_action_values, hipStream_t stream);
}

#endif /* AGX_NN_RESNET_HPP_ */
