"""Run by tests/test_reanalyse_gpu.py in a process of its own (the library has to share torch's HIP runtime from the start); argv: (rules,
board size, fragment file) triples.  1. TrainingDataset.positions as device torch tensors on a non-default torch stream against the games'
moves replayed in numpy, and against the numpy form of the same call.  2. the 9x9 fragment reanalysed with a synthetic tower: a dataset of
the output buffer yields a load_batch that Trainer.step accepts."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from alphagomoku_amd import _lib  # noqa: E402

_lib.share_torch_hip_runtime()   # before the library or torch touches the GPU

import torch  # noqa: E402

import training_batch_ref as ref  # noqa: E402
from alphagomoku_amd import synthetic, training  # noqa: E402
from alphagomoku_amd.dataset import TrainingDataset  # noqa: E402


def games_of(path):
    """the parsed games of an uncompressed or compressed fragment file, through the library's own loader"""
    from alphagomoku_amd import selfplay
    import ctypes
    rules, rows, cols = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.agx_game_buffer_file_config(str(path).encode(), ctypes.byref(rules), ctypes.byref(rows), ctypes.byref(cols)))
    buffer = selfplay.GameBuffer(rules.value, rows.value, cols.value)
    buffer.load(path)
    games = [ref.parse_game(buffer.game(i)) for i in range(buffer.stats()["games"])]
    buffer.close()
    return games


def replayed(game, n):
    boards, signs = [], []
    for s in game["samples"]:
        k = int(np.asarray(s[8:10]).view(np.uint16)[0])
        board = np.zeros(n * n, np.uint8)
        for m in game["moves"][:k]:
            board[((int(m) >> 2) & 127) * n + ((int(m) >> 9) & 127)] = int(m) & 3
        boards.append(board)
        signs.append(int(game["moves"][k]) & 3)
    return np.stack(boards), np.array(signs, np.uint8)


def positions(args):
    checked = 0
    for rules, n, path in zip(args[0::3], args[1::3], args[2::3]):
        rules, n = int(rules), int(n)
        game = games_of(path)[0]
        want_boards, want_signs = replayed(game, n)
        count = len(game["samples"])
        samples = np.array([[0, 0, k, 0] for k in range(count)], np.int32)
        ds = TrainingDataset(rules, n, n)
        ds.add_fragment(path, index=0)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            boards, signs = ds.positions(samples)       # on torch's current stream, nothing synchronised
            total = boards.sum(dtype=torch.int64)       # torch work behind it on the same stream
        stream.synchronize()
        assert boards.is_cuda and boards.dtype == torch.uint8 and tuple(boards.shape) == (count, n * n) and tuple(signs.shape) == (count,)
        assert np.array_equal(boards.cpu().numpy(), want_boards) and np.array_equal(signs.cpu().numpy(), want_signs)
        assert int(total) == int(want_boards.sum(dtype=np.int64))
        b, s = ds.positions(samples, torch_tensors=False)
        assert np.array_equal(b, want_boards) and np.array_equal(s, want_signs)
        ds.close()
        checked += count
    return checked


def train(rules, n, path):
    from alphagomoku_amd.networks import AGNetwork
    from alphagomoku_amd.search import PositionSearcher
    games = games_of(path)
    total = sum(len(g["samples"]) for g in games)
    source = TrainingDataset(rules, n, n)
    source.add_fragment(path, index=0)
    desc = synthetic.net_desc(blocks=2, filters=64, rows=n, cols=n)
    blob, _ = synthetic.make_weights(desc, seed=3)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    searcher = PositionSearcher(rules=rules, board_size=n, draw_after=n * n, n_games=16, max_batch_size=4, max_simulations=70, tss_table_entries=1 << 14,
                                tss_max_positions=100, node_capacity=4096, edge_capacity=65536)
    stream = torch.cuda.Stream()
    out, stats = source.reanalyse(searcher, net, stream=stream.cuda_stream)
    assert stats["games"] == len(games) and stats["samples"] == total and stats["replaced"] + stats["kept"] == total and stats["replaced"] > 0, stats
    searcher.close()
    net.close()
    source.close()
    ds = TrainingDataset(rules, n, n)
    ds.add_fragment(out, index=0)
    out.close()
    samples = np.array([[0, g, k, (g + k) % 8] for g, game in enumerate(games) for k in range(len(game["samples"]))], np.int32)
    batch = ds.load_batch(samples)
    torch.cuda.synchronize()
    policy = batch["policy_target"].reshape(total, -1)
    assert bool(torch.isfinite(policy).all()) and bool(((policy.sum(1) - 1).abs() < 1e-4).all())
    assert bool(torch.isfinite(batch["action_values_target"]).all()) and bool((batch["value_target"].sum(1) == 1).all())
    desc = synthetic.net_desc(rows=n, cols=n, blocks=1, filters=64, action_values=1)
    torch.manual_seed(7)
    module = training.TowerModule(desc).cuda()
    trainer = training.Trainer(module, ds, lr=1e-3, weights=(1.0, 1.0, 0.05))
    components = trainer.step(samples[:32])
    assert components.is_cuda and bool(torch.isfinite(components).all()) and float(components[0]) > 0
    ds.close()
    return total


if __name__ == "__main__":
    assert torch.cuda.is_available()
    triples = [(int(r), int(n), p) for r, n, p in zip(sys.argv[1::3], sys.argv[2::3], sys.argv[3::3])]
    checked = positions([x for t in triples for x in t])
    trained = [train(*t) for t in triples if t[1] == 9]
    assert len(trained) == 1
    print("ok: %d positions as torch tensors on a torch stream, a training step on %d reanalysed samples" % (checked, trained[0]))
