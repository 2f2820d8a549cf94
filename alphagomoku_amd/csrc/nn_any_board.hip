/*
 * nn_any_board.hip — the run-time-shaped towers' entry (agx_any, nn_any_board.hpp) and the residual instantiations of the one kernel template
 * of nn_any_board_kernel.hpp; the bottleneck instantiations are a module of their own (nn_any_board_bottleneck.hip: that header says why).
 */
#include "nn_any_board_kernel.hpp"

namespace agx_any
{
	size_t skip_bytes_per_workgroup(int filters)
	{
		return sizeof(half4) * static_cast<size_t>((filters == 128) ? SKIP_PER_WG<128> : SKIP_PER_WG<64>);
	}

	int launch(const NetParams &p, Block block, int rows, int cols, int filters, bool raw, int grid, int kpad, const uint32_t *d_features, float *d_policy,
			hipStream_t stream)
	{
		AGX_REQUIRE(rows >= MIN_SIDE && rows <= MAX_SIDE && cols >= MIN_SIDE && cols <= MAX_SIDE && (filters == 64 || filters == 128), AGX_ERR_UNSUPPORTED,
				"agx_nn_forward: no %skernel for a %dx%d board with %d filters", (block == BOTTLENECK) ? "bottleneck " : "", rows, cols, filters);
		AGX_REQUIRE(p.skip != nullptr && p.vhead_x != nullptr && grid > 0, AGX_ERR_STATE, "agx_nn_forward: launch scratch missing");
		AGX_REQUIRE(!(p.q != nullptr && raw), AGX_ERR_UNSUPPORTED, "agx_nn_forward: no action-values head on an 8-channel network");
		return (block == BOTTLENECK) ? launch_bottleneck(p, rows, cols, filters, raw, grid, kpad, d_features, d_policy, stream)
				: launch_block<RESIDUAL>(p, rows, cols, filters, raw, grid, kpad, d_features, d_policy, stream);
	}
}
