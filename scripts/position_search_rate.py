"""Rate of the position searcher (agx_position_searcher_search) against the only path the engine offered before it: the same
positions through agx_engine_set_board into a pool of the same size, in rounds of n_games, each round stepped with select_solve / evaluate /
expand_group until agx_engine_root_summary says every game's move rule has fired.

    python scripts/position_search_rate.py [--positions 1024] [--slots 256 1024] [--sims 400] [--batch 8] [--out profiles/position_search_rate.json]

1024 clustered 15x15 freestyle positions (random walks of 0-59 stones, the generator of DESIGN 3.11's table), a 6x128 synthetic network,
HIP events around the call after one warm-up call.  Reported, not asserted."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphagomoku_amd import selfplay, synthetic  # noqa: E402
from alphagomoku_amd._lib import lib, check  # noqa: E402
from alphagomoku_amd.networks import AGNetwork  # noqa: E402
from alphagomoku_amd.search import PositionSearcher  # noqa: E402

N = 15


def clustered_positions(count, seed=9):
    rng = np.random.default_rng(seed)
    boards = np.zeros((count, N, N), np.uint8)
    for b in boards:
        r = c = N // 2
        for k in range(int(rng.integers(0, 60))):
            r, c = int(np.clip(r + rng.integers(-2, 3), 0, N - 1)), int(np.clip(c + rng.integers(-2, 3), 0, N - 1))
            if b[r, c] == 0:
                b[r, c] = 1 + (k & 1)
    signs = np.array([1 if int((b == 1).sum()) == int((b == 2).sum()) else 2 for b in boards], np.uint8)
    return boards.reshape(count, -1), signs


class Timer:
    def __init__(self):
        self.h = ctypes.c_void_p()
        check(lib.agx_timer_create(ctypes.byref(self.h)))

    def start(self):
        check(lib.agx_timer_start(self.h, None))

    def stop_ms(self):
        check(lib.agx_timer_stop(self.h, None))
        ms = ctypes.c_float()
        check(lib.agx_timer_elapsed_ms(self.h, ctypes.byref(ms)))
        return float(ms.value)


def config(slots, sims, batch):
    # the arenas as bench.py sizes them; a solver table of 65 536 entries per slot (1 MB: it is cleared for every position)
    return dict(rules=0, board_size=N, n_games=slots, max_batch_size=batch, max_simulations=sims, speculative_solver=1, solver_yield_fraction=0.5,
                tss_table_entries=1 << 16, node_capacity=max(4096, 8 * sims), edge_capacity=max(65536, 192 * sims), arena_reserve=3.0)


def searcher_line(boards, signs, net, slots, sims, batch, runs):
    ps = PositionSearcher(**config(slots, sims, batch))
    timer = Timer()
    ps.search(boards, signs, net)                      # warm-up
    times, out = [], None
    for _ in range(runs):
        timer.start()
        out = ps.search(boards, signs, net)
        times.append(timer.stop_ms())
    ms = float(np.median(times))
    busy = int(out["info"][:, 2].astype(np.int64).sum())    # steps the slots spent on positions
    visits = int(out["root"][:, 0].astype(np.int64).sum())
    # the steps of a call, counted in a staged pass of the same job (untimed; the finished counter is read every 4 steps, as search does)
    ps.begin(boards, signs)
    total_steps = 0
    while ps.finished() < len(boards):
        for _ in range(4):
            ps.select_solve()
            ps.evaluate(net)
            ps.expand()
            ps.harvest()
        total_steps += 4
    line = dict(path="position_searcher", slots=slots, positions=len(boards), ms=ms, runs=runs, positions_per_s=len(boards) / ms * 1e3,
                simulations_per_s=visits / ms * 1e3, steps=total_steps, slot_steps=total_steps * slots, slot_steps_busy=busy,
                idle_share=1.0 - busy / float(total_steps * slots), status_counts=np.bincount(out["status"], minlength=4).tolist(),
                device_bytes=ps.device_bytes)
    ps.close()
    return line


def set_board_line(boards, signs, net, slots, sims, batch, runs, poll_every=4):
    cfg = selfplay.default_config(**dict(config(slots, sims, batch), max_simulations=1 << 24))   # (the budget is set below: Player's way)
    pool = selfplay.GeneratorPool(cfg)
    pool.begin(selfplay.pack_openings([[] for _ in range(slots)]))
    pool.set_max_simulations(sims)
    summary = (ctypes.c_int * 4)()
    timer = Timer()

    def one_pass():
        steps = slot_steps = visits = 0
        for first in range(0, len(boards), slots):
            count = min(slots, len(boards) - first)
            for g in range(count):
                pool.set_board(g, boards[first + g], int(signs[first + g]), force_remove_root=True)
            pending = list(range(count))
            while pending:
                for _ in range(poll_every):
                    pool.select_solve()
                    pool.evaluate(net)
                    pool.expand_only()
                steps += poll_every
                slot_steps += poll_every * slots
                still = []
                for g in pending:   # the host asks game by game
                    check(lib.agx_engine_root_summary(pool._h, g, None, summary))
                    if summary[1] or summary[0] > sims:
                        visits += summary[0]
                    else:
                        still.append(g)
                pending = still
        check(lib.agx_device_synchronize())
        return steps, slot_steps, visits
    one_pass()                                          # warm-up
    times, last = [], None
    for _ in range(runs):
        timer.start()
        last = one_pass()
        times.append(timer.stop_ms())
    pool.close()
    ms = float(np.median(times))
    steps, slot_steps, visits = last
    return dict(path="set_board_rounds", slots=slots, positions=len(boards), ms=ms, runs=runs, positions_per_s=len(boards) / ms * 1e3,
                simulations_per_s=visits / ms * 1e3, steps=steps, slot_steps=slot_steps, poll_every=poll_every)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1024)
    ap.add_argument("--slots", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_search_rate.json"))
    args = ap.parse_args()
    boards, signs = clustered_positions(args.positions)
    desc = synthetic.net_desc(blocks=6, filters=128)
    blob, _ = synthetic.make_weights(desc)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    lines = []
    for slots in args.slots:
        for fn in (searcher_line, set_board_line):
            line = fn(boards, signs, net, slots, args.sims, args.batch, args.runs)
            print(json.dumps(line), flush=True)
            lines.append(line)
    net.close()
    with open(args.out, "w") as f:
        json.dump(dict(workload=dict(board=N, rules="freestyle", positions=args.positions, simulations=args.sims, batch=args.batch, network="6x128 synthetic"),
                       lines=lines), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
