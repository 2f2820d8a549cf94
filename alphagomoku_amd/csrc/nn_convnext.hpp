/*
 * nn_convnext.hpp — the ConvNeXt tower (nn_convnext.hip) as nn_net.cpp sees it: the entry points of the C ABI dispatch here for an AgxNet
 * whose architecture is AGX_ARCH_CONVNEXT (the residual towers' counterpart is nn_resnet.hpp).
 */
#ifndef AGX_NN_CONVNEXT_HPP_
#define AGX_NN_CONVNEXT_HPP_

#include "agx_internal.hpp"

namespace agx_cnx
{
	struct Net; // the device-side weights of one ConvNeXt network (opaque to nn_net.cpp)

	/* ConvNextPVQraw / ConvNextPVQMraw: boards 5..20 x 5..20, 8 input channels, the action-values head, 256 hidden value units, F in {64, 128} */
	bool supported(const AgxNetDesc &desc, int moves_left);
	/* fp32 values of the canonical blob (layout: include/agx.h) */
	size_t blob_floats(const AgxNetDesc &desc, int moves_left);
	/* packs and uploads a canonical blob of blob_floats() values; *out replaces nothing (the caller destroys the old one); an AGX_* status */
	int load(const AgxNetDesc &desc, int moves_left, const float *h_blob, Net **out);
	void destroy(Net *net);
	/* One launch of `grid` workgroups on `stream`: positions 0 .. batch - 1 (or the device-side list d_slot_list / *d_count, capped at batch).
	 * d_action_values and d_moves_left may be null (head skipped); d_moves_left is for a network loaded with moves_left only, which
	 * launch_forward() (nn_net.cpp) checks with the other arguments. */
	int launch(const Net *net, int grid, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int batch, float *d_policy, float *d_value,
			float *d_action_values, float *d_moves_left, hipStream_t stream);
}

#endif /* AGX_NN_CONVNEXT_HPP_ */
