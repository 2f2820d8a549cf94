"""Samples per second of agx_dataset_load_batch (batch 1024, HIP events over 50 launches after 10 warm-up launches) against the host path that
existed before it: one agx_sample_v201_unpack per sample on one thread (which only dequantises: no board, no symmetry, no features).

    python scripts/training_batch_rate.py [output.json] [--policy torch_api,visits,values] [--q-weights] [--repeats 3]
        [--launches 50] [--warmup 10]

--policy measures every named policy target on the same samples (default: torch_api alone), --q-weights adds the action_values_weight
output, --repeats runs the timed loop that many times per policy (the spread between them is the run-to-run spread), --launches and
--warmup size the timed window and the launches before it (a window of 50 launches lasts 2 ms: after seconds of host work the device's
clocks have not come up yet, and the first window measured shows it).
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as ol  # noqa: E402
import training_batch_ref as ref  # noqa: E402
from alphagomoku_amd import lib, check  # noqa: E402
from alphagomoku_amd.dataset import TrainingDataset  # noqa: E402
from alphagomoku_amd.networks import DeviceBuffer  # noqa: E402

BATCH, LAUNCHES, WARMUP = 1024, 50, 10


def measure(olib, rules, n, only_cross=False, policies=("torch_api",), q_weights=False, repeats=1, launches=LAUNCHES, warmup=WARMUP):
    games = [ref.oracle_game(olib, ol.RULES[rules], n, 100 + k, sims=32) for k in range(6)]
    parsed = [ref.parse_game(g) for g in games]
    path = os.path.join(tempfile.mkdtemp(), "fragment.bin")
    ref.write_fragment(path, rules, n, games)
    ds = TrainingDataset(ol.RULES[rules], n, n)
    ds.add_fragment(path, index=0)
    rows = np.array([(0, g, k, a) for g, game in enumerate(parsed) for k in range(len(game["samples"])) for a in range(8)
                     if not only_cross or (int(game["moves"][int(game["samples"][k][8:10].view(np.uint16)[0])]) & 3) == 1], np.int32)
    rng = np.random.default_rng(1)
    samples = rows[rng.integers(0, len(rows), BATCH)]
    options = dict(q_weights=True) if q_weights else {}     # (only named when asked for)
    shapes = ds.tensor_shapes(BATCH, **options)
    bufs = {k: DeviceBuffer(int(np.prod(s)) * 4) for k, s in shapes.items()}
    pointers = {k: b.ptr.value for k, b in bufs.items()}
    timer = ctypes.c_void_p()
    check(lib.agx_timer_create(ctypes.byref(timer)))
    ms = ctypes.c_float()
    timed = {}
    for policy in policies:
        for _ in range(warmup):
            ds.load_batch_pointers(samples, pointers, policy=policy, **options)
        timed[policy] = []
        for _ in range(repeats):
            check(lib.agx_device_synchronize())
            check(lib.agx_timer_start(timer, None))
            for _ in range(launches):
                ds.load_batch_pointers(samples, pointers, policy=policy, **options)
            check(lib.agx_timer_stop(timer, None))
            check(lib.agx_timer_elapsed_ms(timer, ctypes.byref(ms)))
            timed[policy].append(ms.value)
    check(lib.agx_timer_destroy(timer))
    # the host path: dequantise the same samples, one after the other
    hw = n * n
    visits, prior, value, score = np.zeros(hw, np.int32), np.zeros(hw, np.float32), np.zeros((hw, 2), np.float32), np.zeros(hw, np.uint16)
    header, mm = np.zeros(3, np.int32), np.zeros(2, np.float32)
    blobs = [np.ascontiguousarray(parsed[g]["samples"][k]) for _, g, k, _ in samples]
    t0 = time.perf_counter()
    for blob in blobs:
        lib.agx_sample_v201_unpack(ol.ptr(blob), blob.size, n, n, ol.ptr(visits), ol.ptr(prior), ol.ptr(value), ol.ptr(score), ol.ptr(header), ol.ptr(mm), None)
    host = time.perf_counter() - t0
    for b in bufs.values():
        b.free()
    ds.close()
    first = timed[policies[0]][0]
    out = dict(rules=rules, board=n, cross_to_move_only=only_cross, batch=BATCH, launches=launches, ms_per_batch=first / launches,
               device_samples_per_s=BATCH * launches / (first * 1e-3), host_unpack_only_samples_per_s=BATCH / host)
    if len(policies) > 1 or repeats > 1 or q_weights:
        out["q_weights"] = q_weights
        out["samples_per_s"] = {policy: [BATCH * launches / (x * 1e-3) for x in runs] for policy, runs in timed.items()}
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("output", nargs="?")
    parser.add_argument("--policy", default="torch_api")
    parser.add_argument("--q-weights", action="store_true")
    parser.add_argument("--repeats", type=int, default=1)
    parser.add_argument("--launches", type=int, default=LAUNCHES)
    parser.add_argument("--warmup", type=int, default=WARMUP)
    args = parser.parse_args()
    more = dict(policies=tuple(args.policy.split(",")), q_weights=args.q_weights, repeats=args.repeats, launches=args.launches, warmup=args.warmup)
    olib = ol.load()
    out = [measure(olib, "FREESTYLE", 15, **more), measure(olib, "RENJU", 15, only_cross=True, **more), measure(olib, "CARO5", 20, **more)]
    text = json.dumps(dict(build=lib.agx_build_hash().decode(), results=out), indent=1)
    print(text)
    if args.output:
        with open(args.output, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
