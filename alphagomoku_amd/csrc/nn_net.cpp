/*
 * nn_net.cpp — AgxNet and every network entry point of the C ABI (include/agx.h): the small thing above the towers.  An architecture is a
 * namespace with supported / blob_floats / load / destroy / launch over an opaque Net: agx_res (nn_resnet.hpp; the kernels and their host
 * side are in nn_forward.hip; the bottleneck towers are a block kind of the same Net and of the run-time-shaped kernel, nn_any_board.hip), agx_lay
 * (nn_layered.hpp, nn_layered.hip: the residual networks wider than 128 filters, a launch per layer) and agx_cnx (nn_convnext.hpp, nn_convnext.hip).
 * Each function below checks its arguments once and forks on the architecture in one place.
 */
#include "agx_internal.hpp"
#include "nn_resnet.hpp"
#include "nn_layered.hpp"
#include "nn_convnext.hpp"

#include <cstdlib>

struct AgxNet
{
		AgxNetDesc desc;
		int architecture = AGX_ARCH_RESNET;
		int moves_left = 0;
		int num_cus = 256;
		int launch_width = 0; // 0 = every CU
		// the loaded weights: the pointer of `architecture` is non-null once agx_net_load_weights succeeded, the others stay null
		// (`resnet` carries the residual and the bottleneck towers, `layered` the residual networks the kernels behind `resnet` do not take)
		agx_res::Net *resnet = nullptr;
		agx_lay::Net *layered = nullptr;
		agx_cnx::Net *convnext = nullptr;
};

/* A residual network goes to the layered tower when its width is beyond the single-plane kernels (agx_res::supported refuses it) — or, for
 * tests and A/B runs, whenever AGX_NN_LAYERED=1 is set while its weights are loaded. */
static bool runs_layered(const AgxNetDesc &desc, int architecture)
{
	if (architecture != AGX_ARCH_RESNET || !agx_lay::supported(desc, 0))
		return false;
	const char *force = getenv("AGX_NN_LAYERED");
	return !agx_res::supported(desc, 0) || (force != nullptr && force[0] == '1');
}

extern "C" {

size_t agx_net_blob_floats_ex(const AgxNetDesc *d, int architecture, int moves_left)
{
	if (d == nullptr)
		return 0;
	switch (architecture)
	{
		case AGX_ARCH_RESNET:
			return (moves_left == 0) ? agx_res::blob_floats(*d) : 0; // (agx_lay::blob_floats is the same formula: one blob layout for every width)
		case AGX_ARCH_CONVNEXT:
			return agx_cnx::blob_floats(*d, moves_left);
		case AGX_ARCH_BOTTLENECK:
			return (moves_left == 0 && agx_res::supported(*d, 0)) ? agx_res::blob_floats(*d, true) : 0;
		default:
			return 0;
	}
}

size_t agx_net_blob_floats(const AgxNetDesc *d)
{
	return agx_net_blob_floats_ex(d, AGX_ARCH_RESNET, 0);
}

int agx_net_create_ex(const AgxNetDesc *desc, int architecture, int moves_left, AgxNet **out)
{
	AGX_REQUIRE(desc != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_net_create: null argument");
	switch (architecture)
	{
		case AGX_ARCH_RESNET:
			AGX_REQUIRE(moves_left == 0, AGX_ERR_UNSUPPORTED, "agx_net_create_ex: unsupported architecture %d with moves_left=%d (the residual networks have no moves-left head)",
					architecture, moves_left);
			AGX_REQUIRE(agx_res::supported(*desc, moves_left) || agx_lay::supported(*desc, moves_left), AGX_ERR_UNSUPPORTED,
					"agx_net_create: unsupported network %dx%d blocks=%d filters=%d cin=%d hidden=%d (supported: 5..20 rows and cols, F a multiple of 64 from 64 to 512, hidden min(256, 2F), cin 32, or cin 8 without the action-values head)",
					desc->rows, desc->cols, desc->blocks, desc->filters, desc->in_channels, desc->value_hidden);
			break;
		case AGX_ARCH_BOTTLENECK:
			AGX_REQUIRE(agx_res::supported(*desc, moves_left), AGX_ERR_UNSUPPORTED,
					"agx_net_create_ex: unsupported bottleneck network %dx%d blocks=%d filters=%d cin=%d hidden=%d action_values=%d moves_left=%d (supported: 5..20 rows and cols, F in {64,128}, blocks >= 0, hidden min(256, 2F), cin 32, or cin 8 without the action-values head, no moves-left head)",
					desc->rows, desc->cols, desc->blocks, desc->filters, desc->in_channels, desc->value_hidden, desc->action_values, moves_left);
			break;
		case AGX_ARCH_CONVNEXT:
			AGX_REQUIRE(agx_cnx::supported(*desc, moves_left), AGX_ERR_UNSUPPORTED,
					"agx_net_create_ex: unsupported ConvNeXt network %dx%d blocks=%d filters=%d cin=%d hidden=%d action_values=%d moves_left=%d (supported: 5..20 rows and cols, F in {64,128}, cin 8, hidden 256, with the action-values head)",
					desc->rows, desc->cols, desc->blocks, desc->filters, desc->in_channels, desc->value_hidden, desc->action_values, moves_left);
			break;
		default:
			AGX_REQUIRE(false, AGX_ERR_UNSUPPORTED, "agx_net_create_ex: unsupported architecture %d with moves_left=%d", architecture, moves_left);
	}
	AgxNet *net = new AgxNet();
	net->desc = *desc;
	net->architecture = architecture;
	net->moves_left = moves_left;
	int dev = 0;
	hipDeviceProp_t prop;
	if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
		net->num_cus = prop.multiProcessorCount;
	*out = net;
	return AGX_OK;
}

int agx_net_create(const AgxNetDesc *desc, AgxNet **out)
{
	return agx_net_create_ex(desc, AGX_ARCH_RESNET, 0, out);
}

int agx_net_architecture(const AgxNet *net, int *architecture, int *moves_left)
{
	AGX_REQUIRE(net != nullptr && architecture != nullptr && moves_left != nullptr, AGX_ERR_INVALID, "agx_net_architecture: null argument");
	*architecture = net->architecture;
	*moves_left = net->moves_left;
	return AGX_OK;
}

/* One reload discipline for every architecture: a fresh tower is packed and uploaded first, and only when that succeeded the old one is
 * waited for, destroyed and replaced — a failed reload leaves the old weights loaded. */
int agx_net_load_weights(AgxNet *net, const float *h_blob, size_t n_floats)
{
	AGX_REQUIRE(net != nullptr && h_blob != nullptr, AGX_ERR_INVALID, "agx_net_load_weights: null argument");
	const size_t expected = agx_net_blob_floats_ex(&net->desc, net->architecture, net->moves_left);
	AGX_REQUIRE(n_floats == expected, AGX_ERR_INVALID, "agx_net_load_weights: blob has %zu floats, expected %zu", n_floats, expected);
	agx_res::Net *resnet = nullptr;
	agx_lay::Net *layered = nullptr;
	agx_cnx::Net *convnext = nullptr;
	int status = AGX_ERR_STATE;
	switch (net->architecture)
	{
		case AGX_ARCH_RESNET:
		case AGX_ARCH_BOTTLENECK:
			if (runs_layered(net->desc, net->architecture))
				status = agx_lay::load(net->desc, h_blob, &layered);
			else
				status = agx_res::load(net->desc, net->num_cus, h_blob, &resnet, net->architecture == AGX_ARCH_BOTTLENECK);
			break;
		case AGX_ARCH_CONVNEXT:
			status = agx_cnx::load(net->desc, net->moves_left, h_blob, &convnext);
			break;
	}
	if (status != AGX_OK)
		return status;
	if (net->resnet != nullptr || net->layered != nullptr || net->convnext != nullptr)
	{ // (launches of the old weights may be in flight)
		AGX_HIP_CHECK(hipDeviceSynchronize());
		agx_res::destroy(net->resnet);
		agx_lay::destroy(net->layered);
		agx_cnx::destroy(net->convnext);
	}
	net->resnet = resnet;
	net->layered = layered;
	net->convnext = convnext;
	return AGX_OK;
}

static int launch_forward(AgxNet *net, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int batch, float *d_policy, float *d_value,
		float *d_action_values, void *stream, float *d_moves_left = nullptr)
{
	AGX_REQUIRE(net != nullptr, AGX_ERR_INVALID, "agx_nn_forward: null network");
	AGX_REQUIRE(net->resnet != nullptr || net->layered != nullptr || net->convnext != nullptr, AGX_ERR_STATE, "agx_nn_forward: weights not loaded");
	AGX_REQUIRE(batch >= 0, AGX_ERR_INVALID, "agx_nn_forward: negative batch");
	if (batch == 0)
		return AGX_OK;
	AGX_REQUIRE(d_features != nullptr && d_policy != nullptr && d_value != nullptr, AGX_ERR_INVALID, "agx_nn_forward: null buffer");
	AGX_REQUIRE(d_moves_left == nullptr || net->moves_left, AGX_ERR_INVALID, "agx_nn_forward: the network has no moves-left head");
	AGX_REQUIRE(d_action_values == nullptr || net->desc.action_values, AGX_ERR_INVALID, "agx_nn_forward: the network has no action-values head");
	// persistent grid: one workgroup per CU it may use.  A pool stepped as pipelined slices narrows the launch (agx_net_set_launch_width) so that
	// the CUs it leaves free run the OTHER slice's search kernels at the same time: a tower workgroup fills its CU's LDS and registers, so
	// the two kinds of work never share a CU, they share the chip
	const int width = (net->launch_width > 0 && net->launch_width < net->num_cus) ? net->launch_width : net->num_cus;
	const int grid = (batch < width) ? batch : width;
	hipStream_t s = static_cast<hipStream_t>(stream);
	switch (net->architecture)
	{
		case AGX_ARCH_RESNET:
		case AGX_ARCH_BOTTLENECK:
			if (net->layered != nullptr) // (a launch per layer: the width caps every one of them)
				return agx_lay::launch(net->layered, width, d_features, d_slot_list, d_count, batch, d_policy, d_value, d_action_values, s);
			return agx_res::launch(net->resnet, grid, d_features, d_slot_list, d_count, batch, d_policy, d_value, d_action_values, s);
		case AGX_ARCH_CONVNEXT:
			return agx_cnx::launch(net->convnext, grid, d_features, d_slot_list, d_count, batch, d_policy, d_value, d_action_values, d_moves_left, s);
	}
	return AGX_ERR_STATE; // (agx_net_create_ex admits no other architecture)
}

int agx_nn_forward(AgxNet *net, const uint32_t *d_features, int batch, float *d_policy, float *d_value, void *stream)
{
	return launch_forward(net, d_features, nullptr, nullptr, batch, d_policy, d_value, nullptr, stream);
}
int agx_nn_forward_pvq(AgxNet *net, const uint32_t *d_features, int batch, float *d_policy, float *d_value, float *d_action_values, void *stream)
{
	return launch_forward(net, d_features, nullptr, nullptr, batch, d_policy, d_value, d_action_values, stream);
}
int agx_nn_forward_indirect(AgxNet *net, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int max_batch, float *d_policy,
		float *d_value, void *stream)
{
	AGX_REQUIRE(d_slot_list != nullptr && d_count != nullptr, AGX_ERR_INVALID, "agx_nn_forward_indirect: null list");
	return launch_forward(net, d_features, d_slot_list, d_count, max_batch, d_policy, d_value, nullptr, stream);
}
int agx_nn_forward_indirect_pvq(AgxNet *net, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int max_batch, float *d_policy,
		float *d_value, float *d_action_values, void *stream)
{
	AGX_REQUIRE(d_slot_list != nullptr && d_count != nullptr, AGX_ERR_INVALID, "agx_nn_forward_indirect_pvq: null list");
	return launch_forward(net, d_features, d_slot_list, d_count, max_batch, d_policy, d_value, d_action_values, stream);
}

int agx_nn_forward_pvqm(AgxNet *net, const uint32_t *d_features, int batch, float *d_policy, float *d_value, float *d_action_values, float *d_moves_left,
		void *stream)
{
	return launch_forward(net, d_features, nullptr, nullptr, batch, d_policy, d_value, d_action_values, stream, d_moves_left);
}
int agx_nn_forward_indirect_pvqm(AgxNet *net, const uint32_t *d_features, const int *d_slot_list, const int *d_count, int max_batch, float *d_policy,
		float *d_value, float *d_action_values, float *d_moves_left, void *stream)
{
	AGX_REQUIRE(d_slot_list != nullptr && d_count != nullptr, AGX_ERR_INVALID, "agx_nn_forward_indirect_pvqm: null list");
	return launch_forward(net, d_features, d_slot_list, d_count, max_batch, d_policy, d_value, d_action_values, stream, d_moves_left);
}

int agx_net_set_launch_width(AgxNet *net, int workgroups)
{
	AGX_REQUIRE(net != nullptr && workgroups >= 0, AGX_ERR_INVALID, "agx_net_set_launch_width: invalid argument");
	net->launch_width = workgroups;
	return AGX_OK;
}

int agx_net_description(const AgxNet *net, AgxNetDesc *out)
{
	AGX_REQUIRE(net != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_net_description: null argument");
	*out = net->desc;
	return AGX_OK;
}

int agx_net_destroy(AgxNet *net)
{
	if (net == nullptr)
		return AGX_OK;
	agx_res::destroy(net->resnet);
	agx_lay::destroy(net->layered);
	agx_cnx::destroy(net->convnext);
	delete net;
	return AGX_OK;
}

} /* extern "C" */
