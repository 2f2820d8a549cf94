"""Run by tests/test_training_gpu.py in a process of its own (argv: a format-201 fragment of 9x9 freestyle games, an .npy file of samples):
alphagomoku_amd/training.py on the device.  1. head_loss (csrc/head_loss.hip through torch.autograd) against head_loss_reference in float64 on
the same device tensors; 2. an untrained TowerModule exported into an AGNetwork against the module itself; 3. 60 Trainer steps lower the
losses TrainingDataset.score reports for the exported network, and Trainer.evaluate agrees with score; 4. the export of the trained module."""
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

N = 9
POLICY_TOL = VALUE_TOL = 4e-3     # fp16 storage against fp32, shallow networks (test_nn_gpu.py:13-14); the (win, draw) action values likewise
GRAD_TOL = 2e-6                   # x scale (test_head_loss_gpu.py)
WEIGHTS = (1.0, 1.0, 0.05)


def loss_bar(want, spread):
    return 1e-5 * abs(want) + 2.0 ** -20 * max(16.0, spread)


def check_loss_and_gradients(batch):
    n = batch["policy_target"].shape[0]
    g = torch.Generator(device="cuda").manual_seed(1)
    shapes = dict(policy=(n, N * N), value=(n, 3), q=(n, N, N, 3))
    logits = {k: (3.0 * torch.randn(s, generator=g, device="cuda")).requires_grad_(True) for k, s in shapes.items()}
    exact = {k: v.detach().double().requires_grad_(True) for k, v in logits.items()}
    want_loss, want_components = training.head_loss_reference(exact["policy"], exact["value"], exact["q"], batch, WEIGHTS)
    want_loss.backward()
    loss, components = training.head_loss(logits["policy"], logits["value"], logits["q"], batch, WEIGHTS)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda and not components.requires_grad
    loss.backward()
    first = {k: v.grad.clone() for k, v in logits.items()}
    edge = (batch["policy_target"] > 0).reshape(-1)
    rows = dict(policy=exact["policy"].detach(), value=exact["value"].detach(), q=exact["q"].detach().reshape(-1, 3)[edge])   # one softmax per row
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
        deviation = float((first[k].double() - exact[k].grad).abs().max())
        print("head_loss gradient of the %s logits: largest deviation %.3g (bar %.3g)" % (k, deviation, GRAD_TOL * WEIGHTS[i] / n))
        assert deviation <= GRAD_TOL * WEIGHTS[i] / n, k
    for v in logits.values():
        v.grad = None
    loss, _ = training.head_loss(logits["policy"], logits["value"], logits["q"], batch, WEIGHTS)
    loss.backward(torch.tensor(3.0, device="cuda"))
    for k, v in logits.items():    # one float32 multiplication by 3
        assert torch.equal(v.grad, first[k] * 3.0) and float(first[k].abs().max()) > 0, k
    # without the action-values head, and losses only
    with torch.no_grad():
        loss_pv, components_pv = training.head_loss(logits["policy"], logits["value"], None, batch, WEIGHTS)
    assert float(components_pv[2]) == 0.0 and torch.equal(components_pv[:2], components[:2])


def compare_export(module, features, what):
    desc = module.desc
    net = AGNetwork(desc)
    net.load_module(module)
    got = net.forward(features)
    planes = torch.from_numpy(((features[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.float32).reshape(len(features), N, N, 32)).cuda()
    was_training = module.training
    module.eval()
    with torch.no_grad():
        policy, value, q = module(planes)
    module.train(was_training)
    want = [torch.softmax(policy, 1).cpu().numpy(), torch.softmax(value, 1).cpu().numpy(), torch.softmax(q, 3).reshape(len(features), -1, 3)[:, :, :2].cpu().numpy()]
    for name, g, w, tol in zip(("policy", "value", "action values"), got, want, (POLICY_TOL, VALUE_TOL, VALUE_TOL)):
        deviation = float(np.abs(g - w).max())
        print("%s, %s: tower against module, largest deviation %.3g (bar %.3g)" % (what, name, deviation, tol))
        assert g.shape == w.shape and deviation <= tol, (what, name, deviation)
    return net


def main():
    assert torch.cuda.is_available()
    path, samples = sys.argv[1], np.load(sys.argv[2])
    ds = TrainingDataset(0, N, N)
    ds.add_fragment(path, index=0)
    batch = ds.load_batch(samples)
    check_loss_and_gradients(batch)
    features = batch["features"].cpu().numpy().view(np.uint32)

    desc = synthetic.net_desc(rows=N, cols=N, blocks=1, filters=64, action_values=1)
    torch.manual_seed(7)
    module = training.TowerModule(desc).cuda()
    net_before = compare_export(module, features, "untrained")
    before = ds.score(net_before, samples)

    trainer = training.Trainer(module, ds, lr=1e-3, weights=WEIGHTS)
    rng = np.random.default_rng(11)
    for _ in range(60):
        components = trainer.step(samples[rng.integers(0, len(samples), 32)])
    assert components.is_cuda and bool(torch.isfinite(components).all())
    net_after = compare_export(module, features, "trained")
    after = ds.score(net_after, samples)
    print("score: policy_loss %.6f -> %.6f, value_loss %.6f -> %.6f, q_loss %.6f -> %.6f" % (before["policy_loss"], after["policy_loss"], before["value_loss"],
                                                                                              after["value_loss"], before["q_loss"], after["q_loss"]))
    assert after["policy_loss"] < before["policy_loss"] and after["value_loss"] < before["value_loss"]
    mine = trainer.evaluate(samples)
    assert mine["samples"] == after["samples"] and mine["q_cells"] == after["q_cells"]
    for k in ("policy_loss", "value_loss", "q_loss"):
        print("%s: Trainer.evaluate %.9g TrainingDataset.score %.9g relative %.3g" % (k, mine[k], after[k], abs(mine[k] - after[k]) / after[k]))
    for k in ("policy_loss", "value_loss", "q_loss"):   # the gap measured on MI355X is in DESIGN 3.10
        assert abs(mine[k] - after[k]) <= 5e-2 * after[k], k
    fresh = AGNetwork(desc)
    trainer.export_to(fresh)
    assert ds.score(fresh, samples) == after
    for net in (net_before, net_after, fresh):
        net.close()
    ds.close()
    print("ok")


if __name__ == "__main__":
    main()
