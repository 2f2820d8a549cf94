"""alphagomoku_amd/training.py on the CPU: the bridge between a TowerModule and the tower's weight blob against the numpy oracle
(oracle/nn_ref.py), head_loss_reference against tests/head_loss_ref.py, and a short training run.  No GPU: the HIP loss kernel has its own
tests (test_head_loss_gpu.py, test_training_gpu.py)."""
import numpy as np
import pytest
import torch

import head_loss_ref as ref
from oracle import nn_ref


@pytest.fixture(scope="module")
def training(agx_lib):   # (agx_net_blob_floats is host code of the library)
    from alphagomoku_amd import training
    return training


def random_statistics(module, seed):
    """running statistics and shifts as a trained module has them"""
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=g, dtype=torch.float64))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g, dtype=torch.float64))
    for name, p in module.named_parameters():
        if name.endswith("shift") or name.endswith("bias"):
            with torch.no_grad():
                p.copy_(0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64))


def softmaxed(module, desc, features):
    """the module's eval-mode outputs in the form AGNetwork.forward returns: policy [n, hw], value [n, 3], q [n, hw, 2] = (win, draw)"""
    planes = torch.from_numpy(nn_ref.unpack_input(features, desc["rows"], desc["cols"], 32)).to(next(module.parameters()))
    with torch.no_grad():
        policy, value, q = module(planes)
    out = [torch.softmax(policy, 1).cpu().numpy(), torch.softmax(value, 1).cpu().numpy()]
    if q is not None:
        out.append(torch.softmax(q, 3).reshape(q.shape[0], -1, 3)[:, :, :2].cpu().numpy())
    return out


FOLD_TOL = 2e-6   # the oracle accumulates in float32; a prototype of this comparison (9x7, 2x64, PVQ) measured at most 5.2e-8


@pytest.mark.parametrize("rows,cols,blocks,in_channels,action_values", [(9, 7, 2, 32, 1), (5, 5, 1, 32, 0), (6, 6, 1, 8, 0)],
                         ids=["9x7_2x64_pvq", "5x5_1x64_pv", "6x6_1x64_raw"])
def test_fold_against_the_oracle(training, rows, cols, blocks, in_channels, action_values):
    from alphagomoku_amd import synthetic
    desc = synthetic.net_desc(rows=rows, cols=cols, blocks=blocks, filters=64, in_channels=in_channels, action_values=action_values)
    torch.manual_seed(rows * 100 + cols)
    module = training.TowerModule(desc).double().eval()
    random_statistics(module, seed=rows)
    blob = training.export_blob(module)
    assert blob.dtype == np.float32 and blob.size == training.blob_floats(desc)
    features = synthetic.random_features(4, rows, cols, seed=3)
    want = nn_ref.forward(desc, blob, features)         # (split_blob's own assertion pins the length)
    got = softmaxed(module, desc, features)
    assert len(got) == len(want) == 2 + action_values
    for name, g, w in zip(("policy", "value", "action values"), got, want):
        deviation = float(np.abs(g - w).max())
        print("%dx%d %s: largest deviation %.3g" % (rows, cols, name, deviation))
        assert g.shape == w.shape and deviation <= FOLD_TOL, (name, deviation)


@pytest.mark.parametrize("action_values,in_channels", [(1, 32), (0, 8)], ids=["pvq", "raw"])
def test_round_trip(training, action_values, in_channels):
    """export_blob(import_blob(m, blob)) == blob within 2 float32 ulp relative (one rounding when the value becomes a parameter, one at the
    export); the biases exactly"""
    from alphagomoku_amd import synthetic
    desc = synthetic.net_desc(rows=7, cols=6, blocks=2, filters=64, in_channels=in_channels, action_values=action_values)
    blob, parts = synthetic.make_weights(desc, seed=9)
    module = training.import_blob(training.TowerModule(desc), blob)
    for m in module.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            assert float(m.running_mean.abs().max()) == 0.0 and float((m.running_var - 1).abs().max()) == 0.0
    back = training.export_blob(module)
    assert back.shape == blob.shape
    relative = np.abs(back.astype(np.float64) - blob) / np.maximum(np.abs(blob.astype(np.float64)), np.finfo(np.float32).tiny)
    print("round trip: largest relative deviation %.3g" % relative.max())
    assert relative.max() <= 2.4e-7
    pos = 0
    for name, array in parts:
        if name.endswith((".b", ".b1", ".b2", ".b3")):
            assert np.array_equal(back[pos:pos + array.size].view(np.uint32), array.reshape(-1).view(np.uint32)), name
        pos += array.size
    # and the imported module computes what the blob's network computes
    features = synthetic.random_features(3, 7, 6, seed=1)
    for g, w in zip(softmaxed(module.double().eval(), desc, features), nn_ref.forward(desc, blob, features)):
        assert float(np.abs(g - w).max()) <= 1e-5
    with pytest.raises(Exception):
        training.import_blob(module, blob[:-1])


def crafted_batch(rows, cols, n, seed):
    rng = np.random.default_rng(seed)
    hw = rows * cols
    target = rng.dirichlet(np.full(hw, 0.3), n) * (rng.random((n, hw)) < 0.3)
    target[np.arange(n), rng.integers(0, hw, n)] += 0.1
    target = (target / target.sum(axis=1, keepdims=True)).astype(np.float32)
    target[1] *= np.float32(0.5)
    target[2] *= np.float32(2.0)
    value_target = rng.dirichlet(np.ones(3), n).astype(np.float32)
    value_target[0] = (0.0, 1.0, 0.0)
    q_target = rng.dirichlet(np.ones(3), (n, hw)).astype(np.float32)
    q_target[~(target > 0)] = np.nan                       # filler on the cells without an edge
    logits = dict(policy=(3 * rng.standard_normal((n, hw))).astype(np.float32), value=(2 * rng.standard_normal((n, 3))).astype(np.float32),
                  q=(2 * rng.standard_normal((n, rows, cols, 3))).astype(np.float32))
    logits["policy"][3] = -40.0
    logits["policy"][3, 5] = 40.0                          # the other cells' probabilities underflow next to it
    targets = dict(policy_target=target.reshape(n, rows, cols), value_target=value_target, action_values_target=q_target.reshape(n, rows, cols, 3))
    return logits, targets


@pytest.mark.parametrize("with_q", [True, False], ids=["q", "no_q"])
def test_head_loss_reference(training, with_q):
    """the torch composite against the float64 numpy restatement, and its autograd gradient against the closed form p * T - t, mask included"""
    rows, cols, n = 7, 6, 9
    weights = (1.0, 0.5, 0.05)
    logits, targets = crafted_batch(rows, cols, n, seed=12)
    _, want, want_grads, _ = ref.batch_loss(logits["policy"], logits["value"], targets["policy_target"].reshape(n, -1), targets["value_target"],
                                            logits["q"].reshape(n, -1, 3) if with_q else None, targets["action_values_target"].reshape(n, -1, 3) if with_q else None)
    z = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in logits.items()}
    t = {k: torch.from_numpy(v) for k, v in targets.items()}
    loss, components = training.head_loss_reference(z["policy"], z["value"], z["q"] if with_q else None, t, weights)
    want_components = np.array([want["policy_ce"], want["value_ce"], want["q_ce"]]) / n
    assert np.abs(components.detach().numpy() - want_components).max() <= 1e-12 * max(1.0, np.abs(want_components).max())
    assert abs(float(loss.detach()) - float((np.array(weights) * want_components).sum())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert with_q == (want["q_ce"] > 0)
    (3.0 * loss).backward()
    for i, k in enumerate(("policy", "value", "q")):
        if k == "q" and not with_q:
            assert z["q"].grad is None
            continue
        got = z[k].grad.numpy().reshape(want_grads[k].shape)
        assert np.isfinite(got).all()
        assert np.abs(got - 3.0 * weights[i] / n * want_grads[k]).max() <= 1e-12
    if with_q:
        no_edge = ~(targets["policy_target"] > 0)
        assert (z["q"].grad.numpy()[no_edge] == 0.0).all()
    # float32, the dtype the trainer runs it in
    loss32, _ = training.head_loss_reference(*[torch.from_numpy(logits[k]) if (with_q or k != "q") else None for k in ("policy", "value", "q")], t, weights)
    assert loss32.dtype == torch.float32 and abs(float(loss32) - float(loss.detach())) <= 1e-5 * abs(float(loss.detach()))


class RandomDataset:
    """what a Trainer needs of a TrainingDataset, on the CPU: fixed random samples; samples[:, 2] is the index"""

    def __init__(self, rows, cols, count, seed):
        g = torch.Generator().manual_seed(seed)
        hw = rows * cols
        self.count = count
        self.input = (torch.rand((count, rows, cols, 32), generator=g) < 0.3).float()
        policy = torch.rand((count, hw), generator=g) * (torch.rand((count, hw), generator=g) < 0.1)
        policy[torch.arange(count), torch.randint(0, hw, (count,), generator=g)] += 1.0
        self.policy = (policy / policy.sum(1, keepdim=True)).reshape(count, rows, cols)
        self.value = torch.eye(3)[torch.randint(0, 3, (count,), generator=g)]
        q = torch.rand((count, rows, cols, 3), generator=g)
        self.q = q / q.sum(3, keepdim=True)

    def load_batch(self, samples, *, out=None, features=True):
        index = torch.from_numpy(np.asarray(samples, np.int64).reshape(-1, 4)[:, 2])
        fresh = dict(input=self.input[index], policy_target=self.policy[index], value_target=self.value[index], action_values_target=self.q[index],
                     moves_left_target=torch.zeros((len(index), 1)))
        if out is None:
            return fresh
        for k, v in fresh.items():
            out[k].copy_(v)
        return out

    def sample(self, batch_size, generator):
        out = np.zeros((batch_size, 4), np.int32)
        out[:, 2] = generator.integers(0, self.count, batch_size)
        return out


def test_cpu_training_run(training):
    """60 RAdam steps of batch 32 on 100 fixed samples lower the eval-mode policy and value losses (RAdam warms up: 20 steps are not enough)"""
    from alphagomoku_amd import synthetic
    rows = cols = 8
    desc = synthetic.net_desc(rows=rows, cols=cols, blocks=1, filters=64, action_values=1)
    torch.manual_seed(4)
    module = training.TowerModule(desc)
    data = RandomDataset(rows, cols, 100, seed=8)
    trainer = training.Trainer(module, data, lr=1e-3)
    assert isinstance(trainer.optimizer, torch.optim.RAdam)
    assert not any(isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)) and m.affine for m in module.modules())   # no learnable scale
    everything = np.zeros((100, 4), np.int32)
    everything[:, 2] = np.arange(100)
    before = trainer.evaluate(everything)
    curve = trainer.train(60, 32, np.random.default_rng(5))
    after = trainer.evaluate(everything)
    print("policy %.4f -> %.4f, value %.4f -> %.4f, q %.4f -> %.4f" % (before["policy_loss"], after["policy_loss"], before["value_loss"], after["value_loss"],
                                                                      before["q_loss"], after["q_loss"]))
    assert curve.shape == (60, 3) and bool(torch.isfinite(curve).all())
    assert after["policy_loss"] < before["policy_loss"] and after["value_loss"] < before["value_loss"]
    assert before["samples"] == 100 and before["q_cells"] == int((data.policy > 0).sum())
    assert module.training   # evaluate leaves the mode as it found it
    # what comes out can be handed to the tower: the blob has the length of the description and the oracle computes the module's outputs from it
    blob = training.export_blob(module)
    features = synthetic.random_features(2, rows, cols, seed=2)
    for g, w in zip(softmaxed(module.eval(), desc, features), nn_ref.forward(desc, blob, features)):
        assert float(np.abs(g - w).max()) <= 1e-4
