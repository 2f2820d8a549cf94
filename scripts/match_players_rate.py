"""Throughput record of evaluation matches between two players with search settings of their own, on ONE network (the base-against-tested
run of a tuning loop): `pairs` pairs, player 0 and player 1 set with GeneratorPool.set_player_search, merged match steps.  Prints one JSON
line: simulations/s, each player's simulations per move (mean root visits of its recorded moves), the match score and its elo.
usage: python scripts/match_players_rate.py [--pairs 1024] [--steps 1500] [--warmup 30]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# player A: 60 playouts, batch 4, otherwise the defaults; player B: the other end of every field (tests/match_players_ref.py plays the same two)
PLAYER_A = dict(max_simulations=60, max_batch_size=4)
PLAYER_B = dict(max_simulations=100, max_batch_size=8, exploration_constant=0.8, exploration_scaling=0.25, init_to=3, information_leak_threshold=1.0,
                max_children=20, policy_temperature=0.5, tss_max_positions=30, final_selector=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--filters", type=int, default=128)
    args = ap.parse_args()
    from alphagomoku_amd import build
    build.build(verbose=False)
    from alphagomoku_amd import lib, check, synthetic, selfplay, evaluation
    from alphagomoku_amd.networks import AGNetwork
    check(lib.agx_set_device(0))
    desc = synthetic.net_desc(blocks=args.blocks, filters=args.filters)
    net = AGNetwork(desc)
    net.loadWeights(synthetic.make_weights(desc, seed=1234)[0])
    cfg = selfplay.default_config(rules=0, board_size=15, n_games=2 * args.pairs, max_batch_size=8, max_simulations=100, tss_table_entries=1 << 20,
                                  solver_yield_fraction=0.6, match_mode=1, speculative_solver=1,
                                  record_capacity=2 * args.pairs * 150, record_edge_capacity=2 * args.pairs * 150 * 128)   # (A's roots keep ~120 edges)
    pool = selfplay.GeneratorPool(cfg)
    pool.set_player_search(0, **PLAYER_A)
    pool.set_player_search(1, **PLAYER_B)
    pool.begin(selfplay.pack_openings(synthetic.make_openings(15, args.pairs * 3, seed0=7000, rules=0)))
    for _ in range(args.warmup):
        pool.step_match(net, net)
    pool.records(drain=True)
    s0 = pool.stats()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pool.step_match(net, net)
    check(lib.agx_device_synchronize())
    dt = time.perf_counter() - t0
    s1 = pool.stats()
    if s1["first_error"] != 0:
        raise RuntimeError("device engine stopped with error code %d" % s1["first_error"])
    recs, _ = pool.records()
    visits = [[r.root_visits for r in recs if (r.game_slot >= args.pairs) == bool(p)] for p in (0, 1)]
    summary = pool.match_summary()
    line = dict(workload="evaluation matches A against B on one %dx%d network, freestyle 15x15, %d pairs" % (args.blocks, args.filters, args.pairs),
                players=[pool.player_search(0), pool.player_search(1)],
                simulations_per_sec=(s1["evaluated_nodes"] - s0["evaluated_nodes"]) / dt, ms_per_step=1e3 * dt / args.steps,
                moves_per_sec=(s1["moves_played"] - s0["moves_played"]) / dt,
                simulations_per_move=[sum(v) / max(len(v), 1) for v in visits], moves_recorded=[len(v) for v in visits],
                simulations_per_move_pool=(s1["evaluated_nodes"] - s0["evaluated_nodes"]) / max(1, s1["moves_played"] - s0["moves_played"]), summary=summary)
    if summary["wins"] + summary["draws"] + summary["losses"] > 0:
        line["elo"] = evaluation.elo(summary["wins"], summary["draws"], summary["losses"])
    print(json.dumps(line))
    pool.close()
    net.close()


if __name__ == "__main__":
    main()
