"""Two rates of the training step, timed with HIP events on torch's stream:
  1. the loss of the heads with its logit gradients at batch 1024 on 15x15 with action values: agx_head_loss_grad (csrc/head_loss.hip, one
     call = its two launches) against head_loss_reference forward + backward (the torch composite), 50 runs after 10 warm-up runs each;
  2. a whole Trainer.step (load_batch -> TowerModule -> head_loss -> backward -> RAdam) of a 6x128 PV network on 15x15 freestyle games, batch 256,
     20 steps after 10, in samples per second.

    python scripts/head_loss_rate.py [output.json]
"""
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from alphagomoku_amd import _lib  # noqa: E402

_lib.share_torch_hip_runtime()

import torch  # noqa: E402

import oracle_lib as ol  # noqa: E402
import training_batch_ref as ref  # noqa: E402
from alphagomoku_amd import lib, check, synthetic, training  # noqa: E402
from alphagomoku_amd.dataset import TrainingDataset  # noqa: E402

N, BATCH, RUNS, WARMUP = 15, 1024, 50, 10
STEP_BATCH, STEPS, STEP_WARMUP = 256, 20, 10


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(runs):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / runs


def loss_rates():
    g = torch.Generator(device="cuda").manual_seed(1)
    hw = N * N
    logits = [3.0 * torch.randn(s, generator=g, device="cuda") for s in ((BATCH, hw), (BATCH, 3), (BATCH, N, N, 3))]
    policy = torch.rand((BATCH, hw), generator=g, device="cuda") * (torch.rand((BATCH, hw), generator=g, device="cuda") < 0.15)   # ~34 edges per sample
    policy[:, 0] += 0.1
    targets = dict(policy_target=(policy / policy.sum(1, keepdim=True)).reshape(BATCH, N, N), value_target=torch.softmax(torch.randn((BATCH, 3), generator=g, device="cuda"), 1),
                   action_values_target=torch.softmax(torch.randn((BATCH, N, N, 3), generator=g, device="cuda"), 3))
    grads = [torch.empty_like(t) for t in logits]
    records = torch.empty((BATCH, 6), dtype=torch.float64, device="cuda")
    total = torch.zeros(9, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    weights = training.LOSS_WEIGHTS

    def kernel():
        check(lib.agx_head_loss_grad(N, N, BATCH, p(logits[0]), p(logits[1]), p(logits[2]), p(targets["policy_target"]), p(targets["value_target"]),
                                     p(targets["action_values_target"]), weights[0] / BATCH, weights[1] / BATCH, weights[2] / BATCH, p(grads[0]), p(grads[1]),
                                     p(grads[2]), p(records), p(total), stream))

    leaves = [t.clone().requires_grad_(True) for t in logits]

    def composite():
        for t in leaves:
            t.grad = None
        loss, _ = training.head_loss_reference(leaves[0], leaves[1], leaves[2], targets, weights)
        loss.backward()

    kernel_ms, composite_ms = timed(kernel, RUNS, WARMUP), timed(composite, RUNS, WARMUP)
    return dict(board=N, batch=BATCH, runs=RUNS, head_loss_kernel_ms=kernel_ms, head_loss_reference_forward_backward_ms=composite_ms,
                kernel_samples_per_s=BATCH / (kernel_ms * 1e-3), speedup=composite_ms / kernel_ms)


def step_rate():
    olib = ol.load()
    games = [ref.oracle_game(olib, 0, N, 100 + k, sims=32) for k in range(2)]
    parsed = [ref.parse_game(g) for g in games]
    path = os.path.join(tempfile.mkdtemp(), "fragment.bin")
    ref.write_fragment(path, "FREESTYLE", N, games)
    ds = TrainingDataset(0, N, N)
    ds.add_fragment(path, index=0)
    rows = np.array([(0, g, k, a) for g, game in enumerate(parsed) for k in range(len(game["samples"])) for a in range(8)], np.int32)
    samples = rows[np.random.default_rng(1).integers(0, len(rows), STEP_BATCH)]
    desc = synthetic.net_desc(rows=N, cols=N, blocks=6, filters=128)
    torch.manual_seed(1)
    trainer = training.Trainer(training.TowerModule(desc).cuda(), ds)
    ms = timed(lambda: trainer.step(samples), STEPS, STEP_WARMUP)
    ds.close()
    return dict(network="6x128 PV", board=N, batch=STEP_BATCH, steps=STEPS, ms_per_step=ms, samples_per_s=STEP_BATCH / (ms * 1e-3))


def main():
    out = dict(build=lib.agx_build_hash().decode(), loss=loss_rates(), trainer_step=step_rate(), selfplay_pool_samples_per_s_per_gpu=5000)
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
