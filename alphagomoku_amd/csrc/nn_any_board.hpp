/*
 * nn_any_board.hpp — the run-time-shaped tower kernel (nn_any_board.hip) as nn_forward.hip's host code sees it.
 */
#ifndef AGX_NN_ANY_BOARD_HPP_
#define AGX_NN_ANY_BOARD_HPP_

#include "agx_internal.hpp"

namespace agx_any
{
	constexpr int MIN_SIDE = 5, MAX_SIDE = 20;

	/* One launch: the fields of nn_forward.hip's NetParams (device pointers untyped) + the board shape.  Weight fragments are in the
	 * tap-major order of pack_conv(): [tap][k-step][16-channel tile][lane][8]; the raw input conv in pack_conv5x5_raw()'s. */
	struct Params
	{
			const void *w_in;
			const void *w_tower;
			const float *bias;
			const float *wp2;
			const float *wv1;
			const void *wv2;
			void *vhead_x;        // [batch][kpad] halves, the padding zero
			const float *bv2;
			const float *wv3;
			float bp2;
			float bv1[4];
			float bv3[3];
			int blocks;
			int batch;
			const int *slot_list;
			const int *count_ptr;
			const float *wq2;     // null: the action-values head is not evaluated
			float bq2[3];
			float *q;
			void *skip;           // grid x skip_bytes_per_workgroup(filters)
			int rows, cols;
	};

	/* bytes of residual scratch one workgroup of the persistent grid needs (the same for every board shape) */
	size_t skip_bytes_per_workgroup(int filters);
	/* the tower kernel (`grid` workgroups) and the value head's dense layers behind it, on `stream`; an AGX_* status */
	int launch(const Params &p, int filters, bool raw, int grid, const uint32_t *d_features, float *d_policy, float *d_value, hipStream_t stream);
}

#endif /* AGX_NN_ANY_BOARD_HPP_ */
