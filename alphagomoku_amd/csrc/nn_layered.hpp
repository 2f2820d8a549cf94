/*
 * nn_layered.hpp — the layered residual towers (nn_layered.hip) as nn_net.cpp sees them: ResnetPV / ResnetPVraw / ResnetPVQ wider than one
 * LDS-resident activation plane allows.  Activations live in a per-stream global scratch as fp16 and every convolution layer is a launch of
 * its own (an implicit GEMM on the matrix cores); the canonical blob is the residual networks' (include/agx.h), unchanged.
 *
 * Scratch: a position (one board of a launch) costs 2 planes x NPOS x F x 2 bytes + 8 x ceil(HW / 8) bytes of value-head input, with
 * S = cols + 1, NPOS = 16 x ceil(rows x S / 16) + 2 S + 2 stored cells per plane: 280 576 + 1 824 bytes for F = 256 on 15x15, 974 848 + 3 200
 * for F = 512 on 20x20.  The planes hold at most plane_boards() positions (a launch with more runs the tower slice by slice), so they stay
 * within 128 MiB, or 256 positions where that is more.
 */
#ifndef AGX_NN_LAYERED_HPP_
#define AGX_NN_LAYERED_HPP_

#include "agx_internal.hpp"

namespace agx_lay
{
	struct Net; // the packed weights of one network on the device and its per-stream scratch (opaque to nn_net.cpp)

	constexpr int MIN_FILTERS = 64, MAX_FILTERS = 512; // multiples of 64; nn_net.cpp sends 64 and 128 here only with AGX_NN_LAYERED=1

	/* ResnetPV / ResnetPVQ / ResnetPVraw: boards 5..20 x 5..20, F a multiple of 64 up to 512, blocks >= 0, hidden min(256, 2F), 32 input
	 * channels, or 8 without the action-values head; no moves-left head */
	bool supported(const AgxNetDesc &desc, int moves_left);
	/* fp32 values of the canonical blob (layout: include/agx.h; the residual networks' formula) */
	size_t blob_floats(const AgxNetDesc &desc);
	/* positions the activation planes of a stream hold at most */
	int plane_boards(const AgxNetDesc &desc);
	/* packs and uploads a canonical blob of blob_floats() values into a fresh Net.  *out replaces nothing (the caller destroys the old one) and
	 * is left alone on failure; an AGX_* status */
	int load(const AgxNetDesc &desc, const float *h_blob, Net **out);
	void destroy(Net *net);
	/* One forward pass on `stream`, a launch per convolution layer, each at most `width` compute units wide: positions 0 .. batch - 1 (or the
	 * device-side list d_slot_list / *d_count, capped at batch; the host never reads the count).  d_action_values may be null (head skipped).
	 * Finds or grows the stream's scratch in `net`; an allocation that fails is an AGX_* status and leaves the scratch as it was. */
	int launch(Net *net, int width, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int batch, float *d_policy, float *d_value,
			float *d_action_values, hipStream_t stream);
}

#endif /* AGX_NN_LAYERED_HPP_ */
