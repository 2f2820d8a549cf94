/*
 * layered_main.cpp — a residual network wider than 128 filters through the reference-named classes (include/alphagomoku_agx/networks.hpp)
 * from a compiled program.
 *
 *   agx_layered_test <weight container> <features file> <positions>
 *
 * The container is what synthetic.save_weights writes for a ResnetPVQ network with 1 block of 256 filters; the features file holds
 * <positions> x rows x cols uint32 feature words.  The program
 *   1. builds ag::AGNetwork(config, "ResnetPVQ", 1, 256) and compares name(), getOutputConfig() and numberOfWeights() with the network read from
 *      the container (ag::loadAGNetwork); builds ResnetPV and ResnetPVraw with 256 filters and checks their weight counts; checks that 96 and
 *      576 filters are still refused;
 *   2. packs the feature words, runs forward and unpacks the outputs;
 *   3. saves the network, reads the copy back and requires the same outputs bit for bit.
 * It prints "name <name>", "outputs <config>", "values <largest policy> <win> <win of cell 7>" of the last position (%.9g) and "ok";
 * tests/test_nn_layered_gpu.py compares them with the Python wrapper's.
 */
#include "../../include/agx.hpp"
#include "../../include/alphagomoku_agx/networks.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace
{
	struct Outputs
	{
			std::vector<float> policy, value, action_values;
	};
	Outputs run(ag::AGNetwork &network, const std::vector<uint32_t> &features, int n, int hw)
	{
		Outputs result;
		network.setBatchSize(n);
		for (int i = 0; i < n; i++)
			network.packInputData(i, features.data() + static_cast<size_t>(i) * hw);
		network.forward(n);
		for (int i = 0; i < n; i++)
		{
			std::vector<float> policy;
			std::vector<ag::Value> q;
			ag::Value value;
			float moves_left = -1.0f;
			network.unpackOutput(i, policy, q, value, moves_left);
			result.policy.insert(result.policy.end(), policy.begin(), policy.end());
			result.value.push_back(value.win_rate);
			result.value.push_back(value.draw_rate);
			for (const ag::Value &v : q)
			{
				result.action_values.push_back(v.win_rate);
				result.action_values.push_back(v.draw_rate);
			}
		}
		return result;
	}
	bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
	{
		return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0);
	}
	void expect(bool condition, const std::string &what)
	{
		if (!condition)
			throw std::runtime_error(what);
	}
	bool refused(const ag::GameConfig &config, int filters)
	{
		try
		{
			ag::AGNetwork network(config, "ResnetPV", 1, filters);
		} catch (const std::exception &e)
		{
			return true;
		}
		return false;
	}
}

int main(int argc, char **argv)
{
	if (argc != 4)
	{
		std::fprintf(stderr, "usage: %s <weight container> <features file> <positions>\n", argv[0]);
		return 2;
	}
	try
	{
		const int n = std::atoi(argv[3]);
		std::unique_ptr<ag::AGNetwork> network = ag::loadAGNetwork(argv[1]);
		const ag::GameConfig config = network->getGameConfig();
		const int hw = config.rows * config.cols;

		std::vector<uint32_t> features(static_cast<size_t>(n) * hw);
		std::ifstream features_file(argv[2], std::ifstream::binary);
		features_file.read(reinterpret_cast<char*>(features.data()), static_cast<std::streamsize>(features.size() * sizeof(uint32_t)));
		if (!features_file)
			throw std::runtime_error("the features file is too short");

		ag::AGNetwork built(config, "ResnetPVQ", 1, 256);
		expect(built.name() == network->name() && built.getOutputConfig() == network->getOutputConfig() && built.numberOfWeights() == network->numberOfWeights(),
				"the network built by name is not the container's: " + built.name() + " / " + network->name());
		{
			ag::AGNetwork pv(config, "ResnetPV", 1, 256), raw(config, "ResnetPVraw", 1, 256);
			expect(pv.name() == "ResnetPV" && pv.getOutputConfig() == "pv", "ResnetPV is a 'pv' network of that name");
			expect(raw.name() == "ResnetPVraw" && raw.getOutputConfig() == "pv", "ResnetPVraw is a 'pv' network of that name");
			expect(raw.numberOfWeights() + 25 * 24 * 256 == pv.numberOfWeights(), "the raw network reads 8 of the 32 input channels");
			expect(pv.numberOfWeights() + 9 * 256 * 256 + 256 + 256 * 3 + 3 == built.numberOfWeights(), "the action-values head is a 3x3 and a 1x1 convolution");
			expect(refused(config, 96) && refused(config, 576), "96 and 576 filters are still refused");
		}

		const Outputs first = run(*network, features, n, hw);
		const std::string copy_path = std::string(argv[1]) + ".copy";
		network->saveToFile(copy_path);
		std::unique_ptr<ag::AGNetwork> copy = ag::loadAGNetwork(copy_path);
		const Outputs second = run(*copy, features, n, hw);
		expect(copy->name() == network->name() && same_bits(first.policy, second.policy) && same_bits(first.value, second.value)
				&& same_bits(first.action_values, second.action_values), "a saved and reloaded network gives other outputs");

		const int last = n - 1;
		const float top = *std::max_element(first.policy.begin() + static_cast<size_t>(last) * hw, first.policy.begin() + static_cast<size_t>(last + 1) * hw);
		std::printf("name %s\n", network->name().c_str());
		std::printf("outputs %s\n", network->getOutputConfig().c_str());
		std::printf("values %.9g %.9g %.9g\n", top, first.value[2 * last], first.action_values[(static_cast<size_t>(last) * hw + 7) * 2]);
		std::printf("ok\n");
		return 0;
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
}
