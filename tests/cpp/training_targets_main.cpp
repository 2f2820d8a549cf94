/*
 * training_targets_main.cpp — the reference's default training targets through the facade over the C ABI (include/agx.hpp), from a
 * compiled program: agx::TrainingDataset::loadBatch with an AgxBatchTensors (policy of SamplerValues, action_values_weight), the weighted
 * agx::head_loss_grad overload and agx::TrainingDataset::score with a policy flag and the weighted action-value term.
 *
 *   agx_training_targets_test <fragment file> <samples file> <weights file> <rules> <board size> <blocks> <filters> <output file>
 *
 * The samples file holds "game sample augmentation" triples (fragment 0 is used for all of them), the weights file the canonical float32
 * blob of a ResnetPVQ network.  The program writes policy [n][hw], action values [n][hw][3] and action_values_weight [n][hw] of the batch
 * to the output file as raw float32 and prints
 *   "batch <n> <hw>"
 *   "loss <samples> <policy_ce> <value_ce> <q_ce> <q_cells>"    head_loss_grad on all-zero logits with the batch's weights (losses only)
 *   "score <samples> <policy_ce> <value_ce> <q_ce> <q_cells> <hits 1..4>"   score(net, samples, 7, AGX_BATCH_POLICY_VALUES, true)
 *   "ok"
 * with 17 significant digits: the doubles round-trip.  tests/test_training_targets_gpu.py compares all of it with the Python calls.
 */
#include "../../include/agx.hpp"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <stdexcept>
#include <vector>

namespace
{
	struct DeviceFloats
	{ // device memory of the library's own runtime
			float *p = nullptr;
			size_t count;
			explicit DeviceFloats(size_t n) :
					count(n)
			{
				agx::check(agx_malloc(reinterpret_cast<void**>(&p), n * sizeof(float)));
			}
			DeviceFloats(const DeviceFloats&) = delete;
			DeviceFloats& operator=(const DeviceFloats&) = delete;
			~DeviceFloats()
			{
				agx_free(p);
			}
			std::vector<float> download() const
			{
				std::vector<float> out(count);
				agx::check(agx_memcpy_d2h(out.data(), p, count * sizeof(float)));
				return out;
			}
			void zero()
			{
				const std::vector<float> zeros(count, 0.0f);
				agx::check(agx_memcpy_h2d(p, zeros.data(), count * sizeof(float)));
			}
	};
}

int main(int argc, char **argv)
{
	if (argc != 9)
	{
		std::fprintf(stderr, "usage: %s <fragment file> <samples file> <weights file> <rules> <board size> <blocks> <filters> <output file>\n", argv[0]);
		return 2;
	}
	try
	{
		const int fragment = 0, rules = std::atoi(argv[4]), size = std::atoi(argv[5]);
		std::vector<AgxDatasetSample> samples;
		std::ifstream list(argv[2]);
		int game, sample, augmentation;
		while (list >> game >> sample >> augmentation)
			samples.push_back(AgxDatasetSample { fragment, game, sample, augmentation });
		if (samples.empty())
			throw std::runtime_error("the samples file names no samples");
		const size_t n = samples.size(), hw = static_cast<size_t>(size) * size;

		agx::TrainingDataset dataset(rules, size, size);
		dataset.load(fragment, argv[1]);
		DeviceFloats policy(n * hw), value(n * 3), moves_left(n), action_values(n * hw * 3), weight(n * hw);
		AgxBatchTensors tensors { };
		tensors.policy = policy.p;
		tensors.value = value.p;
		tensors.moves_left = moves_left.p;
		tensors.action_values = action_values.p;
		tensors.action_values_weight = weight.p;
		dataset.loadBatch(samples, tensors, AGX_BATCH_POLICY_VALUES);
		agx::check(agx_device_synchronize());
		std::ofstream out(argv[8], std::ofstream::binary);
		for (const DeviceFloats *t : { &policy, &action_values, &weight })
		{
			const std::vector<float> host = t->download();
			out.write(reinterpret_cast<const char*>(host.data()), static_cast<std::streamsize>(host.size() * sizeof(float)));
		}
		out.close();
		std::printf("batch %zu %zu\n", n, hw);

		DeviceFloats policy_logits(n * hw), value_logits(n * 3), q_logits(n * hw * 3);
		policy_logits.zero();
		value_logits.zero();
		q_logits.zero();
		AgxSampleScore *d_records = nullptr;
		AgxNetScore *d_total = nullptr;
		agx::check(agx_malloc(reinterpret_cast<void**>(&d_records), n * sizeof(AgxSampleScore)));
		agx::check(agx_malloc(reinterpret_cast<void**>(&d_total), sizeof(AgxNetScore)));
		agx::check(agx_net_score_clear(d_total, nullptr));
		agx::head_loss_grad(size, size, static_cast<int>(n), policy_logits.p, value_logits.p, q_logits.p, policy.p, value.p, action_values.p, weight.p, 1.0f, 1.0f, 0.05f,
				nullptr, nullptr, nullptr, d_records, d_total);
		agx::check(agx_device_synchronize());
		agx::NetScore loss;
		agx::check(agx_memcpy_d2h(static_cast<AgxNetScore*>(&loss), d_total, sizeof(AgxNetScore)));
		agx_free(d_records);
		agx_free(d_total);
		std::printf("loss %lld %.17g %.17g %.17g %lld\n", static_cast<long long>(loss.samples), loss.policy_ce, loss.value_ce, loss.q_ce, static_cast<long long>(loss.q_cells));

		agx::GameConfig cfg;
		cfg.rules = rules;
		cfg.rows = cfg.cols = size;
		agx::AGNetwork network(cfg, std::atoi(argv[6]), std::atoi(argv[7]), "ResnetPVQ");
		std::vector<float> blob(network.numberOfWeights());
		std::ifstream weights(argv[3], std::ifstream::binary);
		weights.read(reinterpret_cast<char*>(blob.data()), static_cast<std::streamsize>(blob.size() * sizeof(float)));
		if (!weights)
			throw std::runtime_error("the weights file is too short");
		network.loadWeights(blob);
		const agx::NetScore score = dataset.score(network, samples, 7, AGX_BATCH_POLICY_VALUES, true);
		std::printf("score %lld %.17g %.17g %.17g %lld", static_cast<long long>(score.samples), score.policy_ce, score.value_ce, score.q_ce,
				static_cast<long long>(score.q_cells));
		for (int k = 0; k < 4; k++)
			std::printf(" %lld", static_cast<long long>(score.topk_hit[k]));
		std::printf("\nok\n");
		return 0;
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
}
