"""Run by tests/test_training_batch_gpu.py in a process of its own: TrainingDataset.load_batch into torch tensors on a torch stream, two
batches back to back, compared bit by bit with tests/training_batch_ref.py.  Guard zones around every tensor must survive."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from alphagomoku_amd import _lib  # noqa: E402

_lib.share_torch_hip_runtime()   # before the library or torch touches the GPU

import torch  # noqa: E402

import oracle_lib as ol  # noqa: E402
import training_batch_ref as ref  # noqa: E402
from alphagomoku_amd.dataset import TrainingDataset  # noqa: E402

GUARD, SENTINEL = 333, 0x5A


def guarded(shapes, dtype):
    whole, out = {}, {}
    for k, shape in shapes.items():
        t = dtype if k == "input" else (torch.int32 if k == "features" else torch.float32)
        count = int(np.prod(shape))
        flat = torch.empty(count + 2 * GUARD, dtype=t, device="cuda")
        flat.view(torch.uint8).fill_(SENTINEL)
        whole[k], out[k] = flat, flat[GUARD:GUARD + count].view(shape)
    return whole, out


def main():
    assert torch.cuda.is_available()
    olib = ol.load()
    n, rules = 15, "RENJU"
    games = [ref.oracle_game(olib, ol.RULES[rules], n, 21, sims=32), ref.crafted_game(olib, n)]
    parsed = [ref.parse_game(g) for g in games]
    path = os.path.join(tempfile.mkdtemp(), "fragment.bin")
    ref.write_fragment(path, rules, n, games)
    ds = TrainingDataset(ol.RULES[rules], n, n)
    ds.add_fragment(path, index=0)
    samples = np.array([(0, g, k, a) for g, game in enumerate(parsed) for k in range(len(game["samples"])) for a in range(8)], np.int32)
    parts = [(samples[:200], torch.float32, "torch_api"), (samples[200:], torch.float16, "visits")]
    stream = torch.cuda.Stream()
    staged = []
    with torch.cuda.stream(stream):
        for part, dtype, policy in parts:
            staged.append(guarded(ds.tensor_shapes(len(part)), dtype))
        stream.synchronize()
        for (part, dtype, policy), (whole, out) in zip(parts, staged):
            ds.load_batch(part, dtype=dtype, out=out, policy=policy)      # no host wait between the two
        stream.synchronize()
    for (part, dtype, policy), (whole, out) in zip(parts, staged):
        want = ref.reference_batch(olib, ol.RULES[rules], n, {0: parsed}, part, policy=policy, dtype=np.float16 if dtype == torch.float16 else np.float32)
        want["features"] = want["features"].view(np.int32)
        for k in out:
            raw = whole[k].view(torch.uint8).cpu().numpy()
            item = whole[k].element_size()
            assert (raw[:GUARD * item] == SENTINEL).all() and (raw[-GUARD * item:] == SENTINEL).all(), "guard zone of %s overwritten" % k
            got = np.ascontiguousarray(out[k].cpu().numpy())
            assert got.shape == want[k].shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k
    fresh = ds.load_batch(samples[:8])   # torch allocates
    assert fresh["input"].shape == (8, n, n, 32) and fresh["input"].is_cuda and fresh["policy_target"].dtype == torch.float32
    torch.cuda.synchronize()
    assert np.array_equal(fresh["action_values_target"].cpu().numpy().view(np.uint32),
                          ref.reference_batch(olib, ol.RULES[rules], n, {0: parsed}, samples[:8])["action_values_target"].view(np.uint32))
    only_words = {k: t for k, t in fresh.items() if k != "input"}      # a caller who wants the feature words alone
    only_words["features"].zero_()
    ds.load_batch(samples[8:16], out=only_words)
    torch.cuda.synchronize()
    assert np.array_equal(only_words["features"].cpu().numpy().view(np.uint32), ref.reference_batch(olib, ol.RULES[rules], n, {0: parsed}, samples[8:16])["features"])
    ds.close()
    print("ok: %d samples into torch tensors on a torch stream" % len(samples))


if __name__ == "__main__":
    main()
