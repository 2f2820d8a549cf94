/*
 * net_score_main.cpp — ag::getAccuracy (include/alphagomoku_agx/dataset.hpp) from a compiled program, the way the reference's
 * SupervisedLearning calls it behind a validation batch.
 *
 *   agx_net_score_test <fragment file> <samples file> <weights file> <board size> <blocks> <filters>
 *
 * The samples file holds "game sample augmentation" triples (fragment 7 is used for all of them), the weights file the canonical float32
 * blob of a ResnetPV network.  Prints "accuracy <count> <top-1> .. <top-4>", "top2 ..." for top_k = 2, then asks for top_k = 5 and
 * prints "refused: <message>" when that throws std::invalid_argument.  Then the same samples through the facade over the C ABI
 * (include/agx.hpp: agx::TrainingDataset::score -> agx::NetScore): "facade <samples> <policy_ce> <value_ce> <q_ce> <q_cells> <hits 1..4>",
 * "means <policy_loss> <value_loss> <q_loss> <accuracy 1..4>" (17 significant digits: the doubles round-trip), and "refused: ..." again
 * for accuracy(5).  tests/test_net_score_gpu.py compares all numbers with TrainingDataset.score.
 */
#include "../../include/agx.hpp"
#include "../../include/alphagomoku_agx/dataset.hpp"
#include "../../include/alphagomoku_agx/networks.hpp"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <stdexcept>
#include <vector>

int main(int argc, char **argv)
{
	if (argc != 7)
	{
		std::fprintf(stderr, "usage: %s <fragment file> <samples file> <weights file> <board size> <blocks> <filters>\n", argv[0]);
		return 2;
	}
	try
	{
		const int fragment = 7;
		ag::load_dataset_fragment(fragment, argv[1]);
		std::vector<ag::Sample_t> samples;
		std::ifstream list(argv[2]);
		int game, sample, augmentation;
		while (list >> game >> sample >> augmentation)
			samples.push_back(ag::Sample_t { fragment, game, sample, augmentation });

		ag::AGNetwork network(ag::GameConfig(ag::GameRules::FREESTYLE, std::atoi(argv[4])), "ResnetPV", std::atoi(argv[5]), std::atoi(argv[6]));
		std::vector<float> blob(network.numberOfWeights());
		std::ifstream weights(argv[3], std::ifstream::binary);
		weights.read(reinterpret_cast<char*>(blob.data()), static_cast<std::streamsize>(blob.size() * sizeof(float)));
		if (!weights)
			throw std::runtime_error("the weights file is too short");
		network.loadWeights(blob);

		const std::vector<float> four = ag::getAccuracy(network, samples);
		std::printf("accuracy");
		for (float x : four)
			std::printf(" %.0f", x);
		const std::vector<float> two = ag::getAccuracy(network, samples, 2);
		std::printf("\ntop2");
		for (float x : two)
			std::printf(" %.0f", x);
		std::printf("\n");
		try
		{
			ag::getAccuracy(network, samples, 5);
			std::printf("top_k = 5 was accepted\n");
			return 1;
		}
		catch (const std::invalid_argument &e)
		{
			std::printf("refused: %s\n", e.what());
		}
		ag::unload_dataset_fragment(fragment);

		agx::GameConfig cfg;
		cfg.rows = cfg.cols = std::atoi(argv[4]);
		agx::AGNetwork facade_network(cfg, std::atoi(argv[5]), std::atoi(argv[6]));
		facade_network.loadWeights(blob);
		agx::TrainingDataset dataset(AGX_FREESTYLE, cfg.rows, cfg.cols);
		dataset.load(fragment, argv[1]);
		std::vector<AgxDatasetSample> facade_samples;
		for (const ag::Sample_t &s : samples)
			facade_samples.push_back(AgxDatasetSample { fragment, s.game_index, s.sample_index, s.augmentation });
		const agx::NetScore score = dataset.score(facade_network, facade_samples);
		std::printf("facade %lld %.17g %.17g %.17g %lld", static_cast<long long>(score.samples), score.policy_ce, score.value_ce, score.q_ce,
				static_cast<long long>(score.q_cells));
		for (int k = 0; k < 4; k++)
			std::printf(" %lld", static_cast<long long>(score.topk_hit[k]));
		std::printf("\nmeans %.17g %.17g %.17g", score.policy_loss(), score.value_loss(), score.q_loss());
		for (int k = 1; k <= 4; k++)
			std::printf(" %.17g", score.accuracy(k));
		std::printf("\n");
		try
		{
			score.accuracy(5);
			std::printf("accuracy(5) was accepted\n");
			return 1;
		}
		catch (const std::invalid_argument &e)
		{
			std::printf("refused: %s\n", e.what());
		}
		std::printf("ok\n");
		return 0;
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
}
