/*
 * nn_any_board_bottleneck.hip — the bottleneck instantiations of the one kernel template of nn_any_board_kernel.hpp, a module of their own
 * (that header says why); agx_any::launch() (nn_any_board.hip) is the way in.
 */
#include "nn_any_board_kernel.hpp"

namespace agx_any
{
	int launch_bottleneck(const NetParams &p, int rows, int cols, int filters, bool raw, int grid, int kpad, const uint32_t *d_features, float *d_policy,
			hipStream_t stream)
	{
		return launch_block<BOTTLENECK>(p, rows, cols, filters, raw, grid, kpad, d_features, d_policy, stream);
	}
}
