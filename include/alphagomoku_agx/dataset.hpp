/*
 * alphagomoku_agx/dataset.hpp — the reference's dataset reader for PyTorch (include/alphagomoku/dataset/torch_api.h), same names and
 * signatures, on a process-wide dataset as in src/dataset/torch_api.cpp:26-30:
 *
 *     load_dataset_fragment(i, path);                    a file written by GameDataBuffer::save
 *     get_dataset_size(&shape, nullptr);  get_dataset_size(nullptr, sizes);     (fragment, game, samples, symmetries) per game
 *     get_tensor_shapes(n, samples, ...);  load_batch(n, samples, input, policy, value, moves_left, action_values);
 *
 * load_batch takes HOST float pointers like the reference's: one launch on the device (one wavefront per sample,
 * csrc/training_batch.hip), one copy back per tensor.  Callers that keep their tensors on the device use agx_dataset_load_batch
 * (agx.h) or alphagomoku_amd.dataset.TrainingDataset instead.
 * Differences: the game configuration of the dataset is the first loaded fragment's — a fragment with another one is refused when
 * it is LOADED (the reference refuses the batch that mixes them); sample b's action values are written at index b (the reference
 * never advances that pointer, torch_api.cpp:274-277); errors are std::logic_error / std::runtime_error with agx_last_error()'s text.
 */
#ifndef ALPHAGOMOKU_AGX_DATASET_HPP_
#define ALPHAGOMOKU_AGX_DATASET_HPP_

#include <vector>

namespace ag
{
	extern "C"
	{
		typedef struct
		{
				int buffer_index;
				int game_index;
				int sample_index;
				int augmentation;
		} Sample_t;

		typedef struct
		{
				int rank;
				int dim[4];
		} TensorSize_t;

		void load_dataset_fragment(int i, const char *path);
		void unload_dataset_fragment(int i);
		void print_dataset_info();
		void get_dataset_size(TensorSize_t *shape, int *size);

		void get_tensor_shapes(int batch_size, const Sample_t *samples, TensorSize_t *input, TensorSize_t *policy_target, TensorSize_t *value_target,
				TensorSize_t *moves_left_target, TensorSize_t *action_values_target);
		void load_batch(int batch_size, const Sample_t *samples, float *input, float *policy_target, float *value_target, float *moves_left_target,
				float *action_values_target);
	}

	/* getAccuracy (include/alphagomoku/networks/NetworkDataPack.hpp, src/networks/NetworkDataPack.cpp:321-345) for samples of the loaded
	 * dataset: the reference's vector of 1 + top_k floats — the number of samples, then for k = 1 .. top_k the samples whose best target
	 * move (pickMove of the policy target) is among the network's k best — ready for averageStats.  The reference reads the outputs and
	 * targets of a NetworkDataPack on the host; here batch, network and counting run on the device (agx.h: agx_net_score_dataset).
	 * top_k is 1 .. 4 (std::invalid_argument otherwise: the device counts four ranks). */
	class AGNetwork;
	std::vector<float> getAccuracy(const AGNetwork &network, const std::vector<Sample_t> &samples, int top_k = 4);
} /* namespace ag */

#endif /* ALPHAGOMOKU_AGX_DATASET_HPP_ */
