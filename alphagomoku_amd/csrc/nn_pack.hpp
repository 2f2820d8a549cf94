/*
 * nn_pack.hpp — the host-side weight packers that more than one network file uses (nn_forward.hip, nn_convnext.hip,
 * nn_layered.hip): canonical fp32 weights to fp16 MFMA A fragments.  A packer that feeds one kernel only stays with that kernel (pack_conv_rows).
 */
#ifndef AGX_NN_PACK_HPP_
#define AGX_NN_PACK_HPP_

#include "nn_device.hpp"

#include <vector>

namespace
{
	/*
	 * Canonical [kh][kw][cin][cout] fp32 weights, appended to dst in MFMA A-fragment order
	 * [tap][kc][mtile][lane][8]: lane l holds out-channel mtile*16 + (l & 15), in-channels kc*32 + 8*(l >> 4) + j.  A 1x1 convolution is one tap.
	 */
	inline void pack_conv(const float *w, int taps, int cin, int cout, std::vector<half_t> &dst)
	{
		const int kcs = cin / 32;
		const int mtiles = cout / 16;
		const size_t base = dst.size();
		dst.resize(base + static_cast<size_t>(taps) * kcs * mtiles * 512);
		half_t *out = dst.data() + base;
		for (int t = 0; t < taps; t++)
			for (int kc = 0; kc < kcs; kc++)
				for (int mt = 0; mt < mtiles; mt++)
					for (int lane = 0; lane < 64; lane++)
						for (int j = 0; j < 8; j++)
						{
							const int oc = mt * 16 + (lane & 15);
							const int ic = kc * 32 + 8 * (lane >> 4) + j;
							const float v = w[(static_cast<size_t>(t) * cin + ic) * cout + oc];
							out[(((static_cast<size_t>(t) * kcs + kc) * mtiles + mt) * 64 + lane) * 8 + j] = static_cast<half_t>(v);
						}
	}

	/* conv5x5 of an 8-channel input (ResnetPVraw, the ConvNeXt towers) for conv5x5_input<.., RAW> and its like: k-step t = 2 * dy + g holds the
	 * four horizontal taps dx = 4 g + (lane >> 4) x 8 channels (taps beyond dx = 4 are zero): [10][cout / 16][lane][8].  Replaces dst. */
	inline void pack_conv5x5_raw(const float *w, int cout, std::vector<half_t> &dst)
	{
		const int mtiles = cout / 16;
		dst.assign(static_cast<size_t>(10) * mtiles * 512, static_cast<half_t>(0.0f));
		for (int t = 0; t < 10; t++)
			for (int mt = 0; mt < mtiles; mt++)
				for (int lane = 0; lane < 64; lane++)
				{
					const int dy = t / 2, dx = 4 * (t % 2) + (lane >> 4);
					if (dx >= 5)
						continue;
					for (int j = 0; j < 8; j++)
						dst[((static_cast<size_t>(t) * mtiles + mt) * 64 + lane) * 8 + j] = static_cast<half_t>(w[(static_cast<size_t>(dy * 5 + dx) * 8 + j) * cout + mt * 16 + (lane & 15)]);
				}
	}

	/* value-head dense input length: 4 HW padded to whole MFMA k-steps */
	inline int value_kpad(int rows, int cols)
	{
		return (rows * cols * 4 + 31) / 32 * 32;
	}

	/* the value head's dense layer 4 HW -> D ([4 HW][D] fp32) in MFMA A-fragment order [k-step][16-unit tile][lane][8] for value_head_kernel
	 * (nn_device.hpp), zero beyond the last input.  Replaces dst. */
	inline void pack_value_dense(const float *w, int hw, int d, std::vector<half_t> &dst)
	{
		const int kpad = (hw * 4 + 31) / 32 * 32, mtiles = d / 16;
		dst.assign(static_cast<size_t>(kpad) * d, static_cast<half_t>(0.0f));
		for (int kc = 0; kc < kpad / 32; kc++)
			for (int mt = 0; mt < mtiles; mt++)
				for (int lane = 0; lane < 64; lane++)
					for (int j = 0; j < 8; j++)
					{
						const int unit = mt * 16 + (lane & 15), k = kc * 32 + 8 * (lane >> 4) + j;
						if (k < hw * 4)
							dst[((static_cast<size_t>(kc) * mtiles + mt) * 64 + lane) * 8 + j] = static_cast<half_t>(w[static_cast<size_t>(k) * d + unit]);
					}
	}
}

#endif /* AGX_NN_PACK_HPP_ */
