"""Training on the device through torch (alphagomoku_amd/training.py): the HIP loss kernel under torch.autograd, the export of a TowerModule into
the tower, a short training run scored by TrainingDataset.score.  In a process of its own (tests/training_torch_main.py): torch's HIP runtime has
to be shared with the library before either touches the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import training_batch_ref as tb

pytestmark = pytest.mark.gpu


def test_training_through_torch(agx_lib, tmp_path):
    olib = ol.load()
    n = 9
    games = [tb.oracle_game(olib, 0, n, 40, sims=32), tb.crafted_game(olib, n)]
    path = tmp_path / "freestyle_9.bin"
    tb.write_fragment(path, "FREESTYLE", n, games)
    parsed = [tb.parse_game(g) for g in games]
    samples = np.array([(0, g, k, a) for g, game in enumerate(parsed) for k in range(len(game["samples"])) for a in range(8)], np.int32)
    samples = samples[::(len(samples) // 100) | 1]     # odd step: keeps all 8 symmetries in the selection
    assert 60 <= len(samples) <= 200 and len(set(int(a) for a in samples[:, 3])) == 8
    listing = tmp_path / "samples.npy"
    np.save(listing, samples)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "training_torch_main.py")
    run = subprocess.run([sys.executable, script, str(path), str(listing)], capture_output=True, text=True, timeout=600)
    print(run.stdout[-6000:])
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout[-3000:] + run.stderr[-3000:]
