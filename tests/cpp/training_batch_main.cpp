/*
 * training_batch_main.cpp — the reference's dataset entry points (include/alphagomoku_agx/dataset.hpp = dataset/torch_api.h) called the
 * way its Python binding calls them: load a fragment, ask for the sizes and shapes, load one batch into host memory.
 *
 *   agx_training_batch_test <fragment file> <samples file> <output file>
 *
 * The samples file holds "game sample augmentation" triples (fragment 7 is used for all of them); the output file receives the five
 * tensors as raw float32, in the order input, policy, value, moves left, action values.  tests/test_training_batch_gpu.py compares
 * them bit by bit with the restatement in tests/training_batch_ref.py.
 */
#include "../../include/alphagomoku_agx/dataset.hpp"

#include <cstdio>
#include <exception>
#include <fstream>
#include <vector>

static size_t elements(const ag::TensorSize_t &t)
{
	size_t n = 1;
	for (int i = 0; i < t.rank; i++)
		n *= static_cast<size_t>(t.dim[i]);
	return n;
}

int main(int argc, char **argv)
{
	if (argc != 4)
	{
		std::fprintf(stderr, "usage: %s <fragment file> <samples file> <output file>\n", argv[0]);
		return 2;
	}
	try
	{
		const int fragment = 7;
		ag::load_dataset_fragment(fragment, argv[1]);
		ag::TensorSize_t shape;
		ag::get_dataset_size(&shape, nullptr);
		std::vector<int> sizes(static_cast<size_t>(shape.dim[0]) * 4);
		ag::get_dataset_size(nullptr, sizes.data());
		std::printf("games %d\n", shape.dim[0]);
		for (int g = 0; g < shape.dim[0]; g++)
			std::printf("game %d %d %d %d\n", sizes[4 * g], sizes[4 * g + 1], sizes[4 * g + 2], sizes[4 * g + 3]);

		std::vector<ag::Sample_t> samples;
		std::ifstream list(argv[2]);
		int game, sample, augmentation;
		while (list >> game >> sample >> augmentation)
			samples.push_back(ag::Sample_t { fragment, game, sample, augmentation });
		const int n = static_cast<int>(samples.size());
		ag::TensorSize_t in, pol, val, ml, av;
		ag::get_tensor_shapes(n, samples.data(), &in, &pol, &val, &ml, &av);
		std::printf("shapes %d %d %d %d %d | %d %d %d %d\n", in.rank, in.dim[0], in.dim[1], in.dim[2], in.dim[3], pol.rank, pol.dim[3], val.dim[1], av.dim[3]);
		std::vector<float> input(elements(in), -7.0f), policy(elements(pol), -7.0f), value(elements(val), -7.0f), moves_left(elements(ml), -7.0f),
				action_values(elements(av), -7.0f);
		ag::load_batch(n, samples.data(), input.data(), policy.data(), value.data(), moves_left.data(), action_values.data());
		std::ofstream out(argv[3], std::ofstream::binary);
		for (const std::vector<float> *t : { &input, &policy, &value, &moves_left, &action_values })
			out.write(reinterpret_cast<const char*>(t->data()), static_cast<std::streamsize>(t->size() * sizeof(float)));
		ag::print_dataset_info();
		ag::unload_dataset_fragment(fragment);
		std::printf("ok\n");
		return out.good() ? 0 : 1;
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
}
