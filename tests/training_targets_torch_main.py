"""Run by tests/test_training_targets_gpu.py in a process of its own (argv: a format-201 fragment of 15x15 freestyle games, an .npy file of
samples): training on what the reference's default configuration trains on.  1. load_batch(policy="values", q_weights=True) into torch tensors,
and again into them through out=; 2. head_loss with the weights (csrc/head_loss.hip: agx_head_loss_grad_weighted through torch.autograd)
against head_loss_reference in float64 on the same device tensors, within the tolerances tests/training_torch_main.py uses for the unweighted
pair; 3. one Trainer step on a 1-block, 64-filter ResnetPVQ module, batch 32, returns finite components, and Trainer.evaluate reports q_loss
as q_ce / samples; 4. TrainingDataset.score(policy="values", q_weights=True) does not depend on chunk."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from alphagomoku_amd import _lib  # noqa: E402

_lib.share_torch_hip_runtime()   # before the library or torch touches the GPU

import torch  # noqa: E402

from alphagomoku_amd import synthetic, training  # noqa: E402
from alphagomoku_amd.dataset import TrainingDataset  # noqa: E402
from alphagomoku_amd.networks import AGNetwork  # noqa: E402

N = 15
GRAD_TOL = 2e-6                   # x scale (test_head_loss_gpu.py); the weights are <= 1
WEIGHTS = (1.0, 1.0, 0.05)


def loss_bar(want, spread):
    return 1e-5 * abs(want) + 2.0 ** -20 * max(16.0, spread)


def check_loss_and_gradients(batch):
    n = batch["policy_target"].shape[0]
    g = torch.Generator(device="cuda").manual_seed(2)
    shapes = dict(policy=(n, N * N), value=(n, 3), q=(n, N, N, 3))
    logits = {k: (3.0 * torch.randn(s, generator=g, device="cuda")).requires_grad_(True) for k, s in shapes.items()}
    exact = {k: v.detach().double().requires_grad_(True) for k, v in logits.items()}
    want_loss, want_components = training.head_loss_reference(exact["policy"], exact["value"], exact["q"], batch, WEIGHTS)
    want_loss.backward()
    loss, components = training.head_loss(logits["policy"], logits["value"], logits["q"], batch, WEIGHTS)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda and not components.requires_grad
    loss.backward()
    counts = (batch["action_values_weight"] > 0).reshape(-1)
    rows = dict(policy=exact["policy"].detach(), value=exact["value"].detach(), q=exact["q"].detach().reshape(-1, 3)[counts])   # one softmax per row
    spreads = [float((rows[k].max(1).values - rows[k].min(1).values).max()) + 6.0 for k in ("policy", "value", "q")]
    bars = [loss_bar(float(want_components[i]) * n, spreads[i]) for i in range(3)]
    for i, k in enumerate(("policy_ce", "value_ce", "q_ce")):
        got, want = float(components[i]) * n, float(want_components[i]) * n
        print("head_loss %s: device %.17g reference %.17g deviation %.3g (bar %.3g)" % (k, got, want, abs(got - want), bars[i]))
        assert abs(got - want) <= bars[i], k
    bar = sum(w * b for w, b in zip(WEIGHTS, bars)) / n + 2.0 ** -23 * abs(float(want_loss))    # + the float32 of the scalar
    print("head_loss loss: device %.9g reference %.17g deviation %.3g (bar %.3g)" % (float(loss), float(want_loss), abs(float(loss) - float(want_loss)), bar))
    assert abs(float(loss) - float(want_loss)) <= bar
    for i, k in enumerate(("policy", "value", "q")):
        deviation = float((logits[k].grad.double() - exact[k].grad).abs().max())
        print("head_loss gradient of the %s logits: largest deviation %.3g (bar %.3g)" % (k, deviation, GRAD_TOL * WEIGHTS[i] / n))
        assert deviation <= GRAD_TOL * WEIGHTS[i] / n and float(logits[k].grad.abs().max()) > 0, k
    dead = ~counts
    assert bool((logits["q"].grad.reshape(-1, 3)[dead] == 0).all()) and int(dead.sum()) > 0
    # the weighted mean per sample is not the unweighted sum over the edges
    plain = {k: v for k, v in batch.items() if k != "action_values_weight"}
    with torch.no_grad():
        _, unweighted = training.head_loss(logits["policy"], logits["value"], logits["q"], plain, WEIGHTS)
    assert torch.equal(unweighted[:2], components[:2]) and float(unweighted[2]) != float(components[2])


def main():
    assert torch.cuda.is_available()
    path, samples = sys.argv[1], np.load(sys.argv[2])
    ds = TrainingDataset(0, N, N)
    ds.add_fragment(path, index=0)
    batch = ds.load_batch(samples, **training.Trainer.reference_targets())
    assert batch["action_values_weight"].shape == (len(samples), N, N) and batch["action_values_weight"].is_cuda
    sums = batch["action_values_weight"].double().reshape(len(samples), -1).sum(1)
    bar = (N * N + 1) * 2.0 ** -24     # sequential float32 sums of up to N * N positive terms, one more rounding per cell
    assert bool(((sums - 1).abs() <= bar).logical_or(sums == 0).all())
    assert bool(((batch["policy_target"].double().reshape(len(samples), -1).sum(1) - 1).abs() <= bar).all())
    again = {k: torch.full_like(v, -7) for k, v in batch.items()}
    assert ds.load_batch(samples, out=again, policy="values", q_weights=True) is again
    assert all(torch.equal(again[k], batch[k]) for k in batch)
    default = ds.load_batch(samples)
    assert "action_values_weight" not in default and not torch.equal(default["policy_target"], batch["policy_target"])
    check_loss_and_gradients(batch)

    desc = synthetic.net_desc(rows=N, cols=N, blocks=1, filters=64, action_values=1)
    torch.manual_seed(7)
    module = training.TowerModule(desc).cuda()
    trainer = training.Trainer(module, ds, lr=1e-3, weights=WEIGHTS, policy="values", q_weights=True)
    components = trainer.step(samples[:32])
    assert components.is_cuda and components.shape == (3,) and bool(torch.isfinite(components).all()) and bool((components > 0).all())
    print("one step: components %s" % components.cpu().numpy())
    mine = trainer.evaluate(samples)
    assert mine["q_cells"] == int((batch["action_values_weight"] > 0).sum()) and abs(mine["q_loss"] - mine["q_ce"] / mine["samples"]) < 1e-15

    net = AGNetwork(desc)
    trainer.export_to(net)
    score = ds.score(net, samples, policy="values", q_weights=True)
    for chunk in (1, 32, 95):
        assert ds.score(net, samples, chunk=chunk, policy="values", q_weights=True) == score
    assert score["q_cells"] == mine["q_cells"] and score["samples"] == len(samples)
    print("score: policy_loss %.6f value_loss %.6f weighted q per sample %.6f (Trainer.evaluate %.6f %.6f %.6f)" % (
        score["policy_loss"], score["value_loss"], score["q_ce"] / score["samples"], mine["policy_loss"], mine["value_loss"], mine["q_loss"]))
    net.close()
    ds.close()
    print("ok")


if __name__ == "__main__":
    main()
