/*
 * position_eval_main.cpp — ag::AGNetwork::packInputData(index, board, signToMove) (include/alphagomoku_agx/networks.hpp) from a compiled
 * program, the way the reference's callers outside the search use the network (AGNetwork.hpp:60).
 *
 *   agx_position_eval_test <positions file> <weights file> <rules> <board size> <architecture> <blocks> <filters> <output file>
 *
 * The positions file holds, per position, board_size^2 bytes (0 empty, 1 cross, 2 circle) and one byte for the sign to move; the weights
 * file the canonical float32 blob.  The program
 *   1. packs every position as a board, runs forward and unpacks the outputs;
 *   2. gets the feature words of the same positions from agx::PositionEvaluator::encode (include/agx.hpp), packs THOSE with
 *      packInputData(index, features), runs forward again and requires the same bits;
 *   3. packs the odd indices as boards and the even ones as features (forward then encodes runs of indices) and requires the same bits;
 *   4. packs a board with an ILLEGAL cell and expects std::logic_error from forward.
 * It writes the feature words, then the policies (float32) to the output file and prints "same <positions>", "refused: <message>", "ok".
 * tests/test_position_eval_gpu.py compares the words with the oracle's and the policies with AGNetwork.evaluate_positions.
 */
#include "../../include/agx.hpp"
#include "../../include/alphagomoku_agx/networks.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

namespace
{
	struct Outputs
	{
			std::vector<float> policy, value, action_values;
	};
	Outputs run(ag::AGNetwork &network, int n)
	{
		Outputs result;
		network.forward(n);
		for (int i = 0; i < n; i++)
		{
			std::vector<float> policy;
			std::vector<ag::Value> q;
			ag::Value value;
			float moves_left = 0.0f;
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
	bool same(const Outputs &a, const Outputs &b)
	{
		return same_bits(a.policy, b.policy) && same_bits(a.value, b.value) && same_bits(a.action_values, b.action_values);
	}
}

int main(int argc, char **argv)
{
	if (argc != 9)
	{
		std::fprintf(stderr, "usage: %s <positions file> <weights file> <rules> <board size> <architecture> <blocks> <filters> <output file>\n", argv[0]);
		return 2;
	}
	try
	{
		const int rules = std::atoi(argv[3]), size = std::atoi(argv[4]), hw = size * size;
		std::ifstream positions_file(argv[1], std::ifstream::binary);
		const std::vector<char> bytes((std::istreambuf_iterator<char>(positions_file)), std::istreambuf_iterator<char>());
		const int n = static_cast<int>(bytes.size() / (hw + 1));
		if (n == 0 || bytes.size() != static_cast<size_t>(n) * (hw + 1))
			throw std::runtime_error("the positions file does not hold whole positions");

		ag::AGNetwork network(ag::GameConfig(static_cast<ag::GameRules>(rules), size), argv[5], std::atoi(argv[6]), std::atoi(argv[7]));
		std::vector<float> blob(network.numberOfWeights());
		std::ifstream weights(argv[2], std::ifstream::binary);
		weights.read(reinterpret_cast<char*>(blob.data()), static_cast<std::streamsize>(blob.size() * sizeof(float)));
		if (!weights)
			throw std::runtime_error("the weights file is too short");
		network.loadWeights(blob);
		network.setBatchSize(n);

		std::vector<ag::matrix<ag::Sign>> boards(n, ag::matrix<ag::Sign>(size, size));
		std::vector<ag::Sign> signs(n);
		std::vector<uint8_t> flat_boards(static_cast<size_t>(n) * hw), flat_signs(n);
		for (int i = 0; i < n; i++)
		{
			const char *p = bytes.data() + static_cast<size_t>(i) * (hw + 1);
			for (int c = 0; c < hw; c++)
			{
				boards[i][c] = static_cast<ag::Sign>(p[c]);
				flat_boards[static_cast<size_t>(i) * hw + c] = static_cast<uint8_t>(p[c]);
			}
			signs[i] = static_cast<ag::Sign>(p[hw]);
			flat_signs[i] = static_cast<uint8_t>(p[hw]);
		}

		for (int i = 0; i < n; i++)
			network.packInputData(i, boards[i], signs[i]);
		const Outputs from_boards = run(network, n);

		agx::PositionEvaluator evaluator(rules, size, n);
		void *d_boards = nullptr, *d_signs = nullptr, *d_features = nullptr;
		agx::check(agx_malloc(&d_boards, flat_boards.size()));
		agx::check(agx_malloc(&d_signs, flat_signs.size()));
		agx::check(agx_malloc(&d_features, sizeof(uint32_t) * n * hw));
		agx::check(agx_memcpy_h2d(d_boards, flat_boards.data(), flat_boards.size()));
		agx::check(agx_memcpy_h2d(d_signs, flat_signs.data(), flat_signs.size()));
		evaluator.encode(n, static_cast<const uint8_t*>(d_boards), static_cast<const uint8_t*>(d_signs), 0x01, static_cast<uint32_t*>(d_features));
		agx::check(agx_device_synchronize());
		std::vector<uint32_t> features(static_cast<size_t>(n) * hw);
		agx::check(agx_memcpy_d2h(features.data(), d_features, sizeof(uint32_t) * features.size()));
		agx::check(agx_free(d_boards));
		agx::check(agx_free(d_signs));
		agx::check(agx_free(d_features));

		for (int i = 0; i < n; i++)
			network.packInputData(i, features.data() + static_cast<size_t>(i) * hw);
		const Outputs from_features = run(network, n);
		if (!same(from_boards, from_features))
		{
			std::printf("packed boards and packed feature words give different outputs\n");
			return 1;
		}
		for (int i = 0; i < n; i++)
			if (i % 2)
				network.packInputData(i, boards[i], signs[i]);
			else
				network.packInputData(i, features.data() + static_cast<size_t>(i) * hw);
		if (!same(from_boards, run(network, n)))
		{
			std::printf("a batch packed half as boards, half as feature words gives different outputs\n");
			return 1;
		}
		std::printf("same %d\n", n);

		ag::matrix<ag::Sign> broken = boards[0];
		broken[hw / 2] = ag::Sign::ILLEGAL;
		network.packInputData(0, broken, ag::Sign::CROSS);
		try
		{
			network.forward(n);
			std::printf("a board with an ILLEGAL cell was accepted\n");
			return 1;
		}
		catch (const std::logic_error &e)
		{
			std::printf("refused: %s\n", e.what());
		}

		std::ofstream out(argv[8], std::ofstream::binary);
		out.write(reinterpret_cast<const char*>(features.data()), static_cast<std::streamsize>(sizeof(uint32_t) * features.size()));
		out.write(reinterpret_cast<const char*>(from_boards.policy.data()), static_cast<std::streamsize>(sizeof(float) * from_boards.policy.size()));
		if (!out)
			throw std::runtime_error("cannot write the output file");
		std::printf("ok\n");
		return 0;
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
}
