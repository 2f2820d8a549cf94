"""Samples per second of agx_dataset_load_batch (batch 1024, HIP events over 50 launches after 10 warm-up launches) against the host path that
existed before it: one agx_sample_v201_unpack per sample on one thread (which only dequantises: no board, no symmetry, no features).

    python scripts/training_batch_rate.py [output.json]
"""
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


def measure(olib, rules, n, only_cross=False):
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
    shapes = ds.tensor_shapes(BATCH)
    bufs = {k: DeviceBuffer(int(np.prod(s)) * 4) for k, s in shapes.items()}
    pointers = {k: b.ptr.value for k, b in bufs.items()}
    timer = ctypes.c_void_p()
    check(lib.agx_timer_create(ctypes.byref(timer)))
    for _ in range(WARMUP):
        ds.load_batch_pointers(samples, pointers)
    check(lib.agx_device_synchronize())
    check(lib.agx_timer_start(timer, None))
    for _ in range(LAUNCHES):
        ds.load_batch_pointers(samples, pointers)
    check(lib.agx_timer_stop(timer, None))
    ms = ctypes.c_float()
    check(lib.agx_timer_elapsed_ms(timer, ctypes.byref(ms)))
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
    return dict(rules=rules, board=n, cross_to_move_only=only_cross, batch=BATCH, launches=LAUNCHES, ms_per_batch=ms.value / LAUNCHES,
                device_samples_per_s=BATCH * LAUNCHES / (ms.value * 1e-3), host_unpack_only_samples_per_s=BATCH / host)


def main():
    olib = ol.load()
    out = [measure(olib, "FREESTYLE", 15), measure(olib, "RENJU", 15, only_cross=True), measure(olib, "CARO5", 20)]
    text = json.dumps(dict(build=lib.agx_build_hash().decode(), results=out), indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
