"""Run by tests/test_position_solve_gpu.py in a process of its own: solver.PositionSolver.solve and AGNetwork.evaluate_positions(solver=...)
with device torch tensors on a non-default torch stream, the outputs written into tensors the caller gives, compared bit by bit with the
numpy form of the same calls (which tests/test_position_solve_gpu.py pins against the oracle and the restatement).  Guard zones around every
tensor must survive."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from alphagomoku_amd import _lib  # noqa: E402

_lib.share_torch_hip_runtime()   # before the library or torch touches the GPU

import torch  # noqa: E402

from alphagomoku_amd import synthetic  # noqa: E402
from alphagomoku_amd.networks import AGNetwork  # noqa: E402
from alphagomoku_amd.solver import PositionSolver  # noqa: E402

GUARD, SENTINEL = 333, 0x5A
KINDS = {np.dtype(np.uint16): torch.int16, np.dtype(np.uint32): torch.int32, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


def guarded(shape, dtype):
    count = int(np.prod(shape))
    flat = torch.empty(count + 2 * GUARD, dtype=dtype, device="cuda")
    flat.view(torch.uint8).fill_(SENTINEL)
    return flat, flat[GUARD:GUARD + count].view(shape)


def same_bits(whole, tensor, want, what):
    raw, item = whole.view(torch.uint8).cpu().numpy(), whole.element_size()
    assert (raw[:GUARD * item] == SENTINEL).all() and (raw[-GUARD * item:] == SENTINEL).all(), "guard zone of %s overwritten" % what
    got = np.ascontiguousarray(tensor.cpu().numpy())
    assert got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


def main():
    assert torch.cuda.is_available()
    n, count, top_k, rules = 15, 70, 3, 2
    rng = np.random.default_rng(9)
    boards = np.zeros((count, n, n), np.uint8)
    for b in boards:   # clustered stones: threats for the solver to find
        r = c = n // 2
        for k in range(int(rng.integers(0, 40))):
            r, c = int(np.clip(r + rng.integers(-2, 3), 0, n - 1)), int(np.clip(c + rng.integers(-2, 3), 0, n - 1))
            if b[r, c] == 0:
                b[r, c] = 1 + (k & 1)
    signs = (1 + np.arange(count) % 2).astype(np.uint8)
    desc = synthetic.net_desc(blocks=1, filters=64, action_values=1)
    blob, _ = synthetic.make_weights(desc, seed=4)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    solver = PositionSolver(rules, n, count, max_positions=100, table_entries=1 << 12)
    want_solved = solver.solve(boards, signs)
    want = net.evaluate_positions(boards, signs, rules, symmetries=0xFF, flags=3, top_k=top_k, solver=solver)
    assert any(((int(s) >> 13) & 3) != 2 for s in want_solved["score"]) and any(((int(s) >> 13) & 3) == 2 for s in want_solved["score"])

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_boards, t_signs = torch.from_numpy(boards).cuda(), torch.from_numpy(signs).cuda()
        whole, out = {}, {}
        for k, w in want_solved.items():
            whole[k], out[k] = guarded(w.shape, KINDS[w.dtype])
        stream.synchronize()
        given = solver.solve(t_boards, t_signs, out=out)   # on torch's current stream
        assert given is out
        stream.synchronize()
        for k, w in want_solved.items():
            same_bits(whole[k], out[k], w, k)
        whole, out = {}, {"solved": {}}
        for k, w in want.items():
            if k != "solved":
                whole[k], out[k] = guarded(w.shape, KINDS[w.dtype])
        for k in ("score", "n_actions"):   # the others stay in the solver's workspace
            whole["solved." + k], out["solved"][k] = guarded(want_solved[k].shape, KINDS[want_solved[k].dtype])
        stream.synchronize()
        given = net.evaluate_positions(t_boards, t_signs, rules, symmetries=0xFF, flags=3, top_k=top_k, out=out, solver=solver)
        assert given is out
        stream.synchronize()
        for k, w in want.items():
            if k != "solved":
                same_bits(whole[k], out[k], w, k)
        for k in ("score", "n_actions"):
            same_bits(whole["solved." + k], out["solved"][k], want["solved"][k], "solved." + k)
        fresh = solver.solve(t_boards[:5], t_signs[:5])   # torch allocates
        stream.synchronize()
    assert fresh["moves"].is_cuda and fresh["moves"].shape == (5, n * n) and fresh["moves"].dtype == torch.int16
    assert np.array_equal(fresh["nodes"].cpu().numpy().view(np.uint32), want_solved["nodes"][:5])
    try:
        solver.solve(t_boards, t_signs, out=dict(score=torch.empty(count, dtype=torch.int32, device="cuda")))
    except ValueError:
        pass
    else:
        raise AssertionError("an output of another dtype must be refused")
    solver.close()
    net.close()
    print("ok: %d positions from torch tensors on a torch stream" % count)


if __name__ == "__main__":
    main()
