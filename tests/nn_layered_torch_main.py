"""Run by tests/test_nn_layered_gpu.py in a process of its own (argv: a format-201 fragment of 9x9 freestyle games, an .npy file of samples):
training.TowerModule with 192 filters on the device.  1. an untrained 1 x 192 ResnetPVQ module exported into a wide AGNetwork (load_module)
against module.eval(), within the bound of the tolerance test (nn_layered_cases.tolerance: 1e-3, or 4 x the restatement's own forwards /
backwards gap where that is larger); 2. TrainingDataset.score runs on that network; 3. three Trainer.steps on one batch: finite, decreasing
total loss, the block's weights changed; 4. Trainer.export_to of the trained module, compared like 1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from alphagomoku_amd import _lib  # noqa: E402

_lib.share_torch_hip_runtime()   # before the library or torch touches the GPU

import torch  # noqa: E402

import nn_layered_cases as lc  # noqa: E402
from alphagomoku_amd import synthetic, training  # noqa: E402
from alphagomoku_amd.dataset import TrainingDataset  # noqa: E402
from alphagomoku_amd.networks import AGNetwork  # noqa: E402

N = 9


def compare_export(module, features, ds, samples, trainer=None):
    desc = module.desc
    net = AGNetwork(desc)
    if trainer is None:
        net.load_module(module)
    else:
        assert trainer.export_to(net) is net
    got = net.forward(features)
    planes = torch.from_numpy(((features[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.float32).reshape(len(features), N, N, 32)).cuda()
    module.eval()
    with torch.no_grad():
        policy, value, q = module(planes)
    module.train()
    want = [torch.softmax(policy, 1), torch.softmax(value, 1), torch.softmax(q, 3).reshape(len(features), -1, 3)[:, :, :2]]
    bounds, gaps = lc.tolerance(desc, training.export_blob(module), features)
    for name, g, w, bound, gap in zip(("policy", "value", "action values"), got, want, bounds, gaps):
        deviation = float(np.abs(g - w.cpu().numpy()).max())
        print("tower against module, %s: largest deviation %.3g (bound %.3g, the restatement's own gap %.3g)" % (name, deviation, bound, gap))
        assert g.shape == tuple(w.shape) and deviation <= bound, (name, deviation)
    score = ds.score(net, samples[:48], chunk=16)
    print("score of 48 samples: policy loss %.6f, value loss %.6f" % (score["policy_loss"], score["value_ce"] / 48))
    assert score["samples"] == 48 and np.isfinite(score["policy_ce"]) and np.isfinite(score["value_ce"]) and score["q_cells"] > 0
    assert score == ds.score(net, samples[:48])                 # another chunking, the same bits
    net.close()


def main():
    assert torch.cuda.is_available()
    path, samples = sys.argv[1], np.load(sys.argv[2])
    ds = TrainingDataset(0, N, N)
    ds.add_fragment(path, index=0)
    features = ds.load_batch(samples[:16])["features"].cpu().numpy().view(np.uint32)

    desc = synthetic.net_desc(N, N, blocks=1, filters=192, action_values=1)
    torch.manual_seed(7)
    module = training.TowerModule(desc).cuda()
    compare_export(module, features, ds, samples)

    trainer = training.Trainer(module, ds, lr=1e-3)
    before = [p.detach().clone() for p in module.blocks.parameters()]
    totals = []
    for _ in range(3):
        c = trainer.step(samples[:32])
        assert c.shape == (3,) and c.is_cuda and bool(torch.isfinite(c).all())
        totals.append(sum(w * float(x) for w, x in zip(training.LOSS_WEIGHTS, c)))
    print("total loss of three steps on one batch: %.6f %.6f %.6f" % tuple(totals))
    assert totals[0] > totals[1] > totals[2]
    assert any(not torch.equal(a, b) for a, b in zip(before, module.blocks.parameters()))
    compare_export(module, features, ds, samples, trainer)      # Trainer.export_to: the trained module, batch norms folded
    ds.close()
    print("ok")


if __name__ == "__main__":
    main()
