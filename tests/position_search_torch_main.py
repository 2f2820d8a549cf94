"""Run by tests/test_position_search_gpu.py in a process of its own: search.PositionSearcher.search with device torch tensors on a non-default
torch stream, the outputs written into tensors the caller gives, compared bit by bit with the numpy form of the same call (which
tests/test_position_search_gpu.py pins against the staged run and the oracle).  Guard zones around every tensor must survive."""
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
from alphagomoku_amd.search import PositionSearcher  # noqa: E402

GUARD, SENTINEL = 333, 0x5A
KINDS = {np.dtype(np.uint16): torch.int16, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


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
    n, count, rules = 15, 14, 2
    rng = np.random.default_rng(11)
    boards = np.zeros((count, n, n), np.uint8)
    for b in boards:   # clustered stones: threats for the solver to find
        r = c = n // 2
        for k in range(int(rng.integers(0, 40))):
            r, c = int(np.clip(r + rng.integers(-2, 3), 0, n - 1)), int(np.clip(c + rng.integers(-2, 3), 0, n - 1))
            if b[r, c] == 0:
                b[r, c] = 1 + (k & 1)
    signs = (1 + np.arange(count) % 2).astype(np.uint8)
    serials = (3 * np.arange(count)).astype(np.int32)
    desc = synthetic.net_desc(blocks=2, filters=64)
    blob, _ = synthetic.make_weights(desc, seed=4)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    searcher = PositionSearcher(rules=rules, board_size=n, n_games=4, max_batch_size=4, max_simulations=60, tss_table_entries=1 << 14, tss_max_positions=100,
                                node_capacity=4096, edge_capacity=65536, use_symmetries=1)
    want = searcher.search(boards, signs, net, serials=serials, max_pv=6)
    assert (want["status"] == 0).all() and (want["root"][:, 0] > 0).all()

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_boards, t_signs, t_serials = torch.from_numpy(boards).cuda(), torch.from_numpy(signs).cuda(), torch.from_numpy(serials).cuda()
        whole, out = {}, {}
        for k, w in want.items():
            whole[k], out[k] = guarded(w.shape, KINDS[w.dtype])
        stream.synchronize()
        given = searcher.search(t_boards, t_signs, net, serials=t_serials, max_pv=6, out=out)   # on torch's current stream
        assert given is out
        for k, w in want.items():   # (the call returns with the stream drained)
            same_bits(whole[k], out[k], w, k)
        fresh = searcher.search(t_boards[:5], t_signs[:5], net, serials=t_serials[:5], max_pv=6)   # torch allocates
        some = searcher.search(t_boards[:5], t_signs[:5], net, serials=t_serials[:5], max_pv=6, out=dict(best_move=torch.empty(5, dtype=torch.int16, device="cuda")))
    assert fresh["visits"].is_cuda and fresh["visits"].shape == (5, n * n) and fresh["edge_index"].dtype == torch.int16
    assert np.array_equal(fresh["best_move"].cpu().numpy().view(np.uint16), want["best_move"][:5])
    assert list(some) == ["best_move"] and np.array_equal(some["best_move"].cpu().numpy().view(np.uint16), want["best_move"][:5])
    try:
        searcher.search(t_boards, t_signs, net, out=dict(status=torch.empty(count, dtype=torch.int16, device="cuda")))
    except ValueError:
        pass
    else:
        raise AssertionError("an output of another dtype must be refused")
    searcher.close()
    net.close()
    print("ok: %d positions from torch tensors on a torch stream" % count)


if __name__ == "__main__":
    main()
