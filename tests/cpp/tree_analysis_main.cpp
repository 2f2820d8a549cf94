/*
 * tree_analysis_main.cpp — the analysis calls of the reference-named Tree on a one-game Tree / Search pair: a search, then the principal
 * variation walked on the host with Tree::getInfo(path) and the "best" final selector ply by ply, compared with the device's one-launch
 * variation (Tree::getPrincipalVariation -> agx_engine_principal_variation); then a set-board with forceRemoveRootNode = true.
 * Usage: tree_analysis_test <network file> <simulations>.  Prints one JSON line; tests/test_tree_analysis_gpu.py compiles and runs it.
 */
#include "../../include/alphagomoku_agx/selfplay.hpp"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>
#include <vector>

using namespace ag;

namespace
{
	void search_position(Tree &tree, Search &search, NNEvaluator &evaluator, const matrix<Sign> &board, Sign sign, int sims, bool force_remove_root)
	{
		search.cleanup(tree);
		tree.setBoard(board, sign, force_remove_root);
		search.setBoard(board, sign);
		const MCTSConfig &mcts = search.getConfig().mcts_config;
		std::unique_ptr<EdgeSelector> puct = EdgeSelector::create(mcts.edge_selector_config);
		tree.setEdgeSelector(*puct);
		tree.setEdgeGenerator(UnifiedGenerator(mcts.max_children, mcts.policy_expansion_threshold, mcts.policy_temperature));
		while (!tree.isRootProven() && tree.getSimulationCount() < sims)
		{
			search.select(tree, sims);
			search.solve();
			search.scheduleToNN(evaluator);
			evaluator.evaluateGraph();
			search.generateEdges(tree);
			search.expand(tree);
			search.backup(tree);
		}
		search.cleanup(tree);
	}
	bool same_moves(const std::vector<Move> &a, const std::vector<Move> &b)
	{
		if (a.size() != b.size())
			return false;
		for (size_t i = 0; i < a.size(); i++)
			if (a[i].row != b[i].row || a[i].col != b[i].col)
				return false;
		return true;
	}
}

int main(int argc, char **argv)
{
	if (argc < 3)
	{
		std::fprintf(stderr, "usage: %s <network file> <simulations>\n", argv[0]);
		return 2;
	}
	try
	{
		const int n = 15, sims = std::atoi(argv[2]);
		GameConfig game_config(GameRules::FREESTYLE, n);
		SearchConfig search_config;
		search_config.max_batch_size = 8;
		search_config.tss_config.hash_table_size = 1 << 14;
		search_config.tree_config.node_bucket_size = 4096;
		search_config.tree_config.edge_bucket_size = 65536;
		DeviceConfig device;
		device.batch_size = 64;
		NNEvaluator evaluator(device);
		evaluator.loadGraph(NetworkLoader(argv[1]));
		evaluator.useSymmetries(false);
		Tree tree(search_config.tree_config);
		Search search(game_config, search_config);
		search.setBatchSize(search_config.max_batch_size);

		matrix<Sign> board(n, n);
		board.fill(Sign::NONE);
		board.at(7, 7) = Sign::CROSS;
		board.at(7, 8) = Sign::CIRCLE;
		board.at(8, 8) = Sign::CROSS;
		search_position(tree, search, evaluator, board, Sign::CIRCLE, sims, false);

		// the host walk: getInfo(pv) and the final selector until the node has no edges (or is not cached)
		EdgeSelectorConfig best;
		best.policy = "best";
		std::unique_ptr<EdgeSelector> selector = EdgeSelector::create(best);
		std::vector<Move> host_pv;
		while (true)
		{
			const Node node = tree.getInfo(host_pv);
			if (node.numberOfEdges() == 0)
				break;
			host_pv.push_back(selector->select(&node)->getMove());
		}
		const std::vector<Move> device_pv = tree.getPrincipalVariation();
		// the same from one ply in: the variation of the first move's child
		std::vector<Move> host_tail(host_pv.begin() + (host_pv.empty() ? 0 : 1), host_pv.end());
		const std::vector<Move> first(host_pv.begin(), host_pv.begin() + (host_pv.empty() ? 0 : 1));
		const std::vector<Move> device_tail = tree.getPrincipalVariation(first);
		const int root_visits = tree.getSimulationCount();
		const int nodes_before = tree.getNodeCount();

		// an occupied cell on the path: the reference's empty Node()
		const Node occupied = tree.getInfo(std::vector<Move> { Move(7, 7) });

		// forceRemoveRootNode on the position just searched: the root is gone, its children are not
		search.cleanup(tree);
		tree.setBoard(board, Sign::CIRCLE, true);
		const int nodes_after_force = tree.getNodeCount();
		const int root_visits_after_force = tree.getSimulationCount();
		const Node child_after_force = host_pv.empty() ? Node() : tree.getInfo(first);

		std::printf("{\"mode\": \"tree_analysis\", \"root_visits\": %d, \"pv_length\": %d, \"pv_equal\": %d, \"tail_equal\": %d, \"occupied_edges\": %d, "
				"\"occupied_visits\": %d, \"nodes_before\": %d, \"nodes_after_force\": %d, \"root_visits_after_force\": %d, \"child_visits_after_force\": %d}\n",
				root_visits, static_cast<int>(host_pv.size()), same_moves(host_pv, device_pv) ? 1 : 0, same_moves(host_tail, device_tail) ? 1 : 0,
				occupied.numberOfEdges(), occupied.getVisits(), nodes_before, nodes_after_force, root_visits_after_force, child_after_force.getVisits());
		return 0;
	} catch (std::exception &e)
	{
		std::fprintf(stderr, "exception: %s\n", e.what());
		return 1;
	}
}
