"""What the sample sink costs the position searcher, and the rate of a reanalysis pass.

    python scripts/reanalyse_rate.py [--positions 1024] [--slots 256] [--sims 400] [--batch 8] [--games 48] [--out profiles/reanalyse_rate.json]

A. agx_position_searcher_search with and without a sink on the 1024 clustered 15x15 positions of scripts/position_search_rate.py (6x128
   synthetic network, 400 simulations, batch 8).  The parent commit's time for the same call is the "position_searcher" line of the same
   slot count in profiles/position_search_rate.json, quoted beside them.
B. TrainingDataset.reanalyse of a self-play buffer (a pool of `--games` games played to the end with the same network), samples per second.
C. the host route the parent commit offers for the same buffer: search -> the dense numpy rows -> one pack per position on one thread
   (tests/reanalyse_ref.sample_bytes: the restatement the tests hold against the oracle) -> agx_game_buffer_add_reanalysed.
One run each after a warm-up, HIP events around the calls of A, wall clock around B and C (they end on the host).  Reported, not asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import position_search_rate as psr  # noqa: E402
import reanalyse_ref as rref  # noqa: E402
import training_batch_ref as ref  # noqa: E402
from alphagomoku_amd import selfplay, synthetic  # noqa: E402
from alphagomoku_amd._lib import lib  # noqa: E402
from alphagomoku_amd.dataset import TrainingDataset  # noqa: E402
from alphagomoku_amd.networks import AGNetwork  # noqa: E402
from alphagomoku_amd.search import PositionSearcher  # noqa: E402

N = psr.N


def sink_lines(boards, signs, net, slots, sims, batch):
    ps = PositionSearcher(**psr.config(slots, sims, batch))
    timer = psr.Timer()
    ps.search(boards, signs, net, samples=True)        # warm-up
    lines = []
    for samples in (False, True, False, True):
        timer.start()
        out = ps.search(boards, signs, net, samples=samples)
        ms = timer.stop_ms()     # (the numpy form: the upload of the boards and the download of the outputs are inside, as in position_search_rate.py)
        lines.append(dict(path="search", sink=samples, slots=slots, positions=len(boards), ms=ms, positions_per_s=len(boards) / ms * 1e3,
                          sample_bytes=int(out["sample_bytes"].sum()) if samples else 0))
    ps.close()
    return lines


def selfplay_buffer(net, games, sims, batch, max_steps=40000):
    cfg = selfplay.default_config(rules=0, board_size=N, n_games=games, max_batch_size=batch, max_simulations=sims, record_format=2, tss_table_entries=1 << 16,
                                  node_capacity=max(4096, 8 * sims), edge_capacity=max(65536, 192 * sims), arena_reserve=3.0, record_sample_capacity=1 << 24,
                                  record_capacity=1 << 16, game_end_capacity=4 * games)
    pool = selfplay.GeneratorPool(cfg)
    pool.begin(selfplay.pack_openings(synthetic.make_openings(N, games, seed0=21)))
    buffer = selfplay.GameBuffer(0, N, N)
    for step in range(max_steps):
        pool.step(net)
        if step % 64 == 63:
            buffer.collect(pool)
            if buffer.stats()["games"] >= games or pool.stats()["active_games"] == 0:
                break
    buffer.collect(pool)
    pool.close()
    return buffer


def host_route(ds, buffer, ps, net):
    """what a user of the parent commit would write: positions replayed on the host, search, rows packed one by one"""
    out = selfplay.GameBuffer(0, N, N)
    games = [ref.parse_game(buffer.game(i)) for i in range(buffer.stats()["games"])]
    boards, signs, stones = [], [], []
    for game in games:
        for s in game["samples"]:
            k = int(np.asarray(s[8:10]).view(np.uint16)[0])
            board = np.zeros(N * N, np.uint8)
            for m in game["moves"][:k]:
                board[((int(m) >> 2) & 127) * N + ((int(m) >> 9) & 127)] = int(m) & 3
            boards.append(board)
            signs.append(int(game["moves"][k]) & 3)
            stones.append(k)
    got = ps.search(np.stack(boards), np.array(signs, np.uint8), net, serials=np.arange(len(boards), dtype=np.int32), max_pv=1)
    j = 0
    for i, game in enumerate(games):
        fresh = []
        for _ in game["samples"]:
            fresh.append(rref.sample_of_position(N, got, j, stones[j]) if got["status"][j] == 0 else None)
            j += 1
        out.add_reanalysed(buffer.game(i), fresh)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--games", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reanalyse_rate.json"))
    args = ap.parse_args()
    desc = synthetic.net_desc(blocks=6, filters=128)
    blob, _ = synthetic.make_weights(desc)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    boards, signs = psr.clustered_positions(args.positions)
    for line in sink_lines(boards, signs, net, args.slots, args.sims, args.batch):
        report(line)
    parent = None
    recorded = os.path.join(ROOT, "profiles", "position_search_rate.json")
    if os.path.exists(recorded):
        for line in json.load(open(recorded))["lines"]:
            if line["path"] == "position_searcher" and line["slots"] == args.slots and line["positions"] == args.positions:
                parent = line["ms"]

    buffer = selfplay_buffer(net, args.games, args.sims, args.batch)
    stats = buffer.stats()
    ds = TrainingDataset(0, N, N)
    ds.add_fragment(buffer, index=0)
    ps = PositionSearcher(**psr.config(args.slots, args.sims, args.batch))
    ds.reanalyse(ps, net)[0].close()                    # warm-up (the fragment goes to the device, the kernels are loaded)
    t0 = time.perf_counter()
    out, rs = ds.reanalyse(ps, net)
    seconds = time.perf_counter() - t0
    report(dict(path="reanalyse", slots=args.slots, games=stats["games"], samples=stats["samples"], seconds=seconds, samples_per_s=stats["samples"] / seconds,
                replaced=rs["replaced"], kept=rs["kept"], status=rs["status"], slot_steps=rs["steps"]))
    t0 = time.perf_counter()
    host = host_route(ds, buffer, ps, net)
    seconds = time.perf_counter() - t0
    same = [host.game(i).tobytes() for i in range(stats["games"])] == [out.game(i).tobytes() for i in range(stats["games"])]
    report(dict(path="host_route", slots=args.slots, games=stats["games"], samples=stats["samples"], seconds=seconds, samples_per_s=stats["samples"] / seconds,
                same_bytes_as_reanalyse=same))
    for b in (out, host, buffer):
        b.close()
    ps.close()
    ds.close()
    net.close()
    with open(args.out, "w") as f:
        json.dump(dict(build=lib.agx_build_hash().decode(), parent_search_ms=parent,
                       workload=dict(board=N, rules="freestyle", positions=args.positions, simulations=args.sims, batch=args.batch, network="6x128 synthetic",
                                     selfplay_games=args.games), lines=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
