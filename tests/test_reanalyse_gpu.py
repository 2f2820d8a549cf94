"""Saved games reanalysed on the device.  1. the searcher's sample sink (csrc/engine.hip: position_write_sample) against the oracle: the
bytes of every position are record 0 (ago_game_record_v201) of a fresh oracle game begun on the position's move list; 2. what the sink
does per status; 3. agx_dataset_positions against the games' moves replayed in numpy; 4. TrainingDataset.reanalyse end to end against the
per-position oracle records framed by agx_game_buffer_add_reanalysed.  Every comparison is on the bytes.  Settings and helpers are those
of tests/test_position_search_gpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import position_search_ref as pref
import reanalyse_ref as rref
import test_position_search_gpu as tps
import training_batch_ref as ref
from test_engine_gpu import _stand_in_evaluator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMS, BATCH, TABLE = tps.SIMS, tps.BATCH, tps.TABLE
DEFAULT_STEPS = (SIMS + 2) * (2 * BATCH + 1) + 6     # agx.h: agx_position_searcher_begin


@pytest.fixture(scope="module")
def olib():
    return ol.load()


# ---- the oracle's record for a position ----------------------------------------------------------------------------------------------
def oracle_sample(olib, rules, n, moves, serial, evaluator, opts):
    """(steps, bytes): record 0 of a fresh game begun on `moves`, as SearchDataStorage_v201 bytes; the game is stepped until it moves"""
    ocfg = ol.default_search_config(max_batch_size=BATCH, max_simulations=SIMS, table_entries=TABLE, use_symmetries=opts.get("use_symmetries", 0))
    h = olib.ago_game_create_ex(rules, n, n, 0, ctypes.byref(ocfg))
    olib.ago_game_set_serial(h, serial)
    olib.ago_game_begin(h, ol.ptr(np.array(list(moves) + [0], np.uint16)), len(moves))
    steps, moved = 0, 0
    while not moved:
        f = np.zeros((BATCH, n * n), np.uint32)
        c = olib.ago_game_step_select(h, ol.ptr(f), BATCH)
        out = evaluator(f[:c])
        if opts.get("action_values"):
            moved = olib.ago_game_step_expand_q(h, ol.ptr(np.ascontiguousarray(out[0])), ol.ptr(np.ascontiguousarray(out[1])), ol.ptr(np.ascontiguousarray(out[2])))
        else:
            moved = olib.ago_game_step_expand(h, ol.ptr(np.ascontiguousarray(out[0])), ol.ptr(np.ascontiguousarray(out[1])))
        steps += 1
        assert steps <= DEFAULT_STEPS, "the oracle's search did not end within the searcher's default step bound"
    buf = np.zeros(16 + 6 * n * n, np.uint8)
    size = olib.ago_game_record_v201(h, 0, ol.ptr(buf), buf.size)
    olib.ago_game_destroy(h)
    assert size >= 16
    return steps, buf[:size].copy()


def run_staged(ps, boards, signs, evaluator, action_values=False, max_steps=None, samples=True, serials=None):
    """tps.run_staged with the sample sink"""
    n, hw = len(boards), ps.board_size ** 2
    ps.begin(boards, signs, serials=serials, max_steps=max_steps, samples=samples)
    steps = 0
    while ps.finished() < n:
        ps.select_solve()
        slots, feats = ps.scheduled()
        out = evaluator(feats) if len(slots) else (np.zeros((0, hw), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, hw, 2), np.float32))
        v3 = np.concatenate([out[1], 1 - out[1].sum(1, keepdims=True)], 1).astype(np.float32)
        ps.provide(slots, out[0], v3, np.ascontiguousarray(out[2], dtype=np.float32) if action_values else None)
        ps.expand()
        ps.harvest()
        steps += 1
        assert steps < 20000
    return ps.results()


def sample_of(got, i):
    return got["sample"][i][:got["sample_bytes"][i]]


def banded(base, n, rows):
    """a stand-in policy with its mass on the given rows only (renormalised in float32): the visited cells lie there"""
    mask = np.zeros((n, 1), np.float32)
    mask[list(rows)] = 1.0

    def evaluator(feats):
        out = base(feats)
        pol = (out[0].reshape(-1, n, n) * mask[None]).astype(np.float32)
        pol = (pol / pol.sum(axis=(1, 2), keepdims=True, dtype=np.float32)).astype(np.float32)
        return (np.ascontiguousarray(pol.reshape(-1, n * n)),) + tuple(out[1:])
    return evaluator


def position_lists(olib, rules, n):
    lists = tps.positions_for(olib, rules, n)
    if n == 15:
        _, game = tps.oracle_game_moves(olib, rules, n, 1)
        lists = [lists[i] for i in (0, 2, 5, 9, 13, 14, 15, 18, 19, 20, 21, 22, 23)] + [game[:30], game[:71], game[:45], game[:58], game[:86], game[:101], game[:64]]
        assert [] in lists and tps.open_four() in lists and tps.forced_defence() in lists and len(lists) == 20
    return lists


# ---- 1. the sample equals the oracle's record ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speculative", [0, 1], ids=["serial", "speculative"])
@pytest.mark.parametrize("rules,n,action_values", [(0, 15, 0), (2, 15, 0), (0, 15, 1), (0, 9, 0), (3, 20, 0), (3, 20, 1)],
                         ids=["freestyle15", "renju15", "freestyle15q", "freestyle9", "caro20", "caro20q"])
def test_sample_is_the_oracles_first_record(agx_lib, olib, rules, n, action_values, speculative):
    opts = dict(speculative_solver=1, solver_yield_fraction=0.5) if speculative else dict(speculative_solver=0)
    if action_values:
        opts["action_values"] = 1
    base = _stand_in_evaluator(olib, n * n)
    plain = tps.q_evaluator(base, n * n) if action_values else base
    jobs = [(position_lists(olib, rules, n), plain, False)]
    if n == 20:
        # the moves of a search lie around the stones: stones on rows 0-1 and 18-19, and on rows 18-19 only, under a policy with its mass on
        # those rows — the kept cells then lie at the ends of the board, 255 cells or more apart or past cell 0
        both_ends = [tps.mv(1, 0, 4), tps.mv(2, 1, 12), tps.mv(1, 19, 6), tps.mv(2, 18, 14)]
        far_end = [tps.mv(1, 19, 6), tps.mv(2, 18, 14), tps.mv(1, 18, 3), tps.mv(2, 19, 11)]
        for rows in ((0, 1, 18, 19), (18, 19)):
            ev = banded(base, n, rows)
            jobs.append(([both_ends, far_end], tps.q_evaluator(ev, n * n) if action_values else ev, True))
    ps = tps.make_searcher(rules, n, 5, **opts)
    proven = unvisited_proven = one_edge = 0
    for lists, evaluator, wants_filler in jobs:
        boards, signs = tps.boards_and_signs(lists, n)
        want = [oracle_sample(olib, rules, n, moves, 0, evaluator, opts) for moves in lists]
        if wants_filler:     # the precondition of the >= 255 path, on the oracle's own bytes
            assert all(rref.has_filler(w[1]) for w in want), [rref.has_filler(w[1]) for w in want]
        got = run_staged(ps, boards, signs, evaluator, action_values=bool(action_values))
        assert (got["status"] == 0).all()
        for i, (steps, sample) in enumerate(want):
            mine = sample_of(got, i)
            assert mine.tobytes() == sample.tobytes(), (i, len(lists[i]), mine.tobytes().hex(), sample.tobytes().hex())
            assert int(mine[8:10].view(np.uint16)[0]) == len(lists[i])
            # the restatement on the dense rows of the same call agrees too
            assert rref.sample_of_position(n, got, i, len(lists[i])).tobytes() == sample.tobytes(), i
            entries = mine[16:].reshape(-1, 6)
            is_proven = ((int(got["root"][i][1]) >> 13) & 3) != 2
            proven += is_proven
            unvisited_proven += bool(((entries[:, 1] == 0) & ((entries[:, 3] >> 6) != 2)).any())
            one_edge += int(got["root"][i][3]) == 1
    ps.close()
    assert proven >= 1
    if n == 15:
        assert unvisited_proven >= 1 and one_edge >= 1     # the open four: edges with a proven score and no visit; the forced defence: one edge


# ---- 2. statuses --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def some_positions(olib):
    lists = tps.positions_for(olib, 1, 15)
    return [lists[i] for i in (0, 4, 9, 13, 15, 18, 19, 20, 21, 22)]


def _raw_job(agx_lib, ps, boards, signs, evaluator, stride, with_bytes=True, guard=256, sentinel=0xA5):
    """a job through agx_position_searcher_begin_ex on buffers of the test's own: every dense output, and a sink of the given stride in a
    sentinel-filled buffer with a guard zone behind the last stride"""
    from alphagomoku_amd import _lib
    from alphagomoku_amd._lib import check
    from alphagomoku_amd.networks import DeviceBuffer
    n, hw = len(boards), ps.board_size ** 2
    shapes = ps._shapes(8)
    c_out, bufs = _lib.AgxPositionSearchOutputs(), {}
    for k, (shape, dtype) in shapes.items():
        bufs[k] = DeviceBuffer(n * int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize)
        setattr(c_out, k, bufs[k].ptr)
    d_boards, d_signs, d_bytes, d_sizes = DeviceBuffer(boards.nbytes), DeviceBuffer(signs.nbytes), DeviceBuffer(n * stride + guard), DeviceBuffer(4 * n)
    d_boards.upload(boards)
    d_signs.upload(signs)
    d_bytes.upload(np.full(n * stride + guard, sentinel, np.uint8))
    d_sizes.upload(np.full(n, -7, np.int32))
    sink = _lib.AgxPositionSampleSink(d_bytes.ptr if with_bytes else None, stride, d_sizes.ptr)
    check(agx_lib.agx_position_searcher_begin_ex(ps.handle, n, d_boards.ptr, d_signs.ptr, None, ctypes.byref(c_out), ctypes.byref(sink), 8, 0, None))
    for _ in range(20000):
        if ps.finished() == n:
            break
        ps.select_solve()
        slots, feats = ps.scheduled()
        pol, val = evaluator(feats) if len(slots) else (np.zeros((0, hw), np.float32), np.zeros((0, 2), np.float32))
        ps.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
        ps.expand()
        ps.harvest()
    assert ps.finished() == n
    out = {k: buf.download((n,) + shapes[k][0], shapes[k][1]) for k, buf in bufs.items()}
    out["raw"], out["sizes"] = d_bytes.download((n * stride + guard,), np.uint8), d_sizes.download((n,), np.int32)
    for buf in list(bufs.values()) + [d_boards, d_signs, d_bytes, d_sizes]:
        buf.free()
    return out


def test_a_bad_board_leaves_its_bytes_alone_and_guards_survive(agx_lib, olib, some_positions):
    from alphagomoku_amd import _lib
    ev = _stand_in_evaluator(olib)
    boards, signs = tps.boards_and_signs(some_positions[:5], 15)
    stride = _lib.sample_stride(225) + 64                      # room between the strides: it must stay as it was
    ps = tps.make_searcher(1, 15, 2)
    want = _raw_job(agx_lib, ps, boards, signs, ev, stride)
    bad_boards, bad_signs = np.insert(boards, 2, 0, axis=0), np.insert(signs, 2, 1)
    bad_boards[2][17] = 3                                      # a cell of 3 in the middle of the batch
    got = _raw_job(agx_lib, ps, bad_boards, bad_signs, ev, stride)
    nothing = _raw_job(agx_lib, ps, bad_boards, bad_signs, ev, stride, with_bytes=False)      # d_bytes NULL: no samples at all
    plain = tps.run_staged(ps, bad_boards, bad_signs, ev)
    ps.close()
    assert got["status"].tolist() == [0, 0, 1, 0, 0, 0] and got["sizes"][2] == 0 and (want["sizes"] >= 16 + 6).all()
    for place, i in enumerate([0, 1, 3, 4, 5]):
        assert got["sizes"][i] == want["sizes"][place]
        assert got["raw"][i * stride:(i + 1) * stride].tobytes() == want["raw"][place * stride:(place + 1) * stride].tobytes(), i
    for out, n in ((want, 5), (got, 6)):
        for i in range(n):
            assert (out["raw"][i * stride + out["sizes"][i]:(i + 1) * stride] == 0xA5).all(), i      # behind the sample, the whole stride of the bad board
        assert (out["raw"][n * stride:] == 0xA5).all()
    assert (nothing["raw"] == 0xA5).all() and (nothing["sizes"] == -7).all()
    for k in tps.OUTPUT_NAMES:     # and the other outputs are those of a call without a sink
        assert nothing[k].tobytes() == plain[k].tobytes() and got[k].tobytes() == plain[k].tobytes(), k


def test_step_limit_samples_the_root_as_it_stands(agx_lib, olib, some_positions):
    ev = _stand_in_evaluator(olib)
    boards, signs = tps.boards_and_signs(some_positions, 15)
    ps = tps.make_searcher(1, 15, 3)
    got = run_staged(ps, boards, signs, ev, max_steps=2)
    one = run_staged(ps, boards, signs, ev, max_steps=1)
    ps.close()
    assert 3 in got["status"] and 0 in got["status"]
    for out in (got, one):
        for i, moves in enumerate(some_positions):
            if out["root"][i][3] == 0 and out["status"][i] == 3:     # no root yet: nothing to sample
                assert out["sample_bytes"][i] == 0, i
            else:
                assert sample_of(out, i).tobytes() == rref.sample_of_position(15, out, i, len(moves)).tobytes(), i
    assert (got["sample_bytes"][got["status"] == 3] > 16).any()


def test_sink_refusals(agx_lib, olib):
    from alphagomoku_amd import _lib
    from alphagomoku_amd.networks import DeviceBuffer
    INVALID = 1
    ps = tps.make_searcher(0, 15, 2)
    boards, signs = tps.boards_and_signs([[], tps.open_four()], 15)
    d_boards, d_signs, d_bytes, d_sizes = DeviceBuffer(boards.nbytes), DeviceBuffer(signs.nbytes), DeviceBuffer(2 * 2048), DeviceBuffer(8)
    d_boards.upload(boards)
    d_signs.upload(signs)
    out = _lib.AgxPositionSearchOutputs()
    needed = 16 + 6 * 225
    for stride in (0, needed - 2, needed - 6, needed + 1, -1368):          # too small, and no multiple of 4
        sink = _lib.AgxPositionSampleSink(d_bytes.ptr, stride, d_sizes.ptr)
        assert agx_lib.agx_position_searcher_begin_ex(ps.handle, 2, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), ctypes.byref(sink), 8, 0, None) == INVALID, stride
        assert b"stride" in agx_lib.agx_last_error()
        assert agx_lib.agx_position_searcher_search_ex(ps.handle, ctypes.c_void_p(1), 2, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), ctypes.byref(sink), 8, 0,
                                                       None) == INVALID, stride
    assert ps.finished() == 0 and (ps.slot_positions() == -1).all()          # nothing of the above reached the device
    sink = _lib.AgxPositionSampleSink(d_bytes.ptr, needed + 2, d_sizes.ptr)  # 1368: the smallest stride there is
    assert agx_lib.agx_position_searcher_begin_ex(ps.handle, 2, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), ctypes.byref(sink), 8, 0, None) == 0
    ev = _stand_in_evaluator(olib)
    for _ in range(20000):
        if ps.finished() == 2:
            break
        ps.select_solve()
        slots, feats = ps.scheduled()
        pol, val = ev(feats) if len(slots) else (np.zeros((0, 225), np.float32), np.zeros((0, 2), np.float32))
        ps.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
        ps.expand()
        ps.harvest()
    sizes = d_sizes.download((2,), np.int32)
    assert (sizes >= 22).all() and (sizes <= needed).all()
    ps.close()
    for buf in (d_boards, d_signs, d_bytes, d_sizes):
        buf.free()


# ---- 3. positions out of saved games --------------------------------------------------------------------------------------------------------
def replayed(game, n):
    """boards and signs of every sample: the first move_number moves, the colour of move move_number"""
    boards, signs = [], []
    for s in game["samples"]:
        k = int(np.asarray(s[8:10]).view(np.uint16)[0])
        boards.append(pref.board_of([int(m) for m in game["moves"][:k]], n))
        signs.append(int(game["moves"][k]) & 3)
    return np.stack(boards), np.array(signs, np.uint8)


@pytest.fixture(scope="module")
def saved_games(olib, tmp_path_factory):
    """(rules, n, path of a fragment, parsed games): oracle self-play games on 15x15, 20x20 and 9x9 and a crafted renju game"""
    where = tmp_path_factory.mktemp("reanalyse")
    out = []
    for name, rules, n, raw in (("FREESTYLE", 0, 15, ref.oracle_game(olib, 0, 15, 5, sims=32)), ("CARO5", 3, 20, ref.oracle_game(olib, 3, 20, 7, sims=24)),
                                ("RENJU", 2, 15, ref.crafted_game(olib, 15)), ("FREESTYLE", 0, 9, ref.oracle_game(olib, 0, 9, 5, sims=24))):
        path = where / ("%s_%d.bin" % (name.lower(), n))
        ref.write_fragment(path, name, n, [raw])
        out.append((rules, n, path, [ref.parse_game(raw)]))
    return out


def test_positions_are_the_moves_replayed(agx_lib, olib, saved_games):
    from alphagomoku_amd.dataset import TrainingDataset
    for rules, n, path, games in saved_games:
        ds = TrainingDataset(rules, n, n)
        ds.add_fragment(path, index=3)
        want_boards, want_signs = replayed(games[0], n)
        count = len(games[0]["samples"])
        samples = np.array([[3, 0, k, (5 * k) % 8] for k in range(count)], np.int32)      # (the augmentation is ignored)
        boards, signs = ds.positions(samples, torch_tensors=False)
        assert boards.shape == (count, n * n) and boards.dtype == np.uint8 and signs.shape == (count,)
        assert np.array_equal(boards, want_boards) and np.array_equal(signs, want_signs) and set(signs.tolist()) <= {1, 2}
        # three columns, another order, one sample, none; and more samples than a launch has waves (2048): the waves stride
        order = np.random.default_rng(3).permutation(count)
        b, s = ds.positions(samples[order][:, :3], torch_tensors=False)
        assert np.array_equal(b, want_boards[order]) and np.array_equal(s, want_signs[order])
        b, s = ds.positions(samples[-1:], torch_tensors=False)
        assert np.array_equal(b, want_boards[-1:]) and np.array_equal(s, want_signs[-1:])
        assert ds.positions(np.zeros((0, 4), np.int32), torch_tensors=False)[0].shape == (0, n * n)
        if n == 15 and rules == 0:
            many = np.resize(np.arange(count), 2048 + 37)
            b, s = ds.positions(samples[many], torch_tensors=False)
            assert np.array_equal(b, want_boards[many]) and np.array_equal(s, want_signs[many])
        with pytest.raises(Exception):
            ds.positions([[3, 0, count, 0]], torch_tensors=False)
        ds.close()


# ---- 4. the whole pass ----------------------------------------------------------------------------------------------------------------------
def short_game(olib, rules, n, seed, limit=40):
    """an oracle self-play game, of its samples at most `limit` (evenly spread: openings, middle games and the last moves)"""
    game = ref.parse_game(ref.oracle_game(olib, rules, n, seed, sims=24))
    keep = sorted(set(np.linspace(0, len(game["samples"]) - 1, min(limit, len(game["samples"]))).astype(int).tolist()))
    return ref.build_game([game["samples"][k] for k in keep], game["moves"], game["outcome"], n)


def buffer_games(buffer):
    return [buffer.game(i).tobytes() for i in range(buffer.stats()["games"])]


@pytest.mark.parametrize("n,use_symmetries", [(9, 0), (15, 1)], ids=["9x9", "15x15_symmetries"])
def test_reanalyse_end_to_end(agx_lib, olib, tmp_path, n, use_symmetries):
    from alphagomoku_amd import selfplay, synthetic
    from alphagomoku_amd.dataset import TrainingDataset
    from alphagomoku_amd.networks import AGNetwork
    rules, base_serial = 0, 1000
    raws = [short_game(olib, rules, n, 5), short_game(olib, rules, n, 6, limit=9)]
    games = [ref.parse_game(r) for r in raws]
    assert all(1 <= len(g["samples"]) <= 40 for g in games)
    source = selfplay.GameBuffer(rules, n, n)
    for raw, game in zip(raws, games):
        source.add_reanalysed(raw, [None] * len(game["samples"]))     # (the game as it is)
    assert buffer_games(source) == [r.tobytes() for r in raws]
    ds = TrainingDataset(rules, n, n)
    ds.add_fragment(source, index=0)
    desc = synthetic.net_desc(blocks=2, filters=64, rows=n, cols=n)
    blob, _ = synthetic.make_weights(desc, seed=3)
    net = AGNetwork(desc)
    net.loadWeights(blob)

    def evaluator(feats):
        p, v = net.forward(np.ascontiguousarray(feats, dtype=np.uint32))
        return p, np.ascontiguousarray(v[:, :2])

    # the oracle, position by position, fed the same tower's outputs; every search ends by the move rule within the default step bound
    # (asserted inside oracle_sample), so no sample may be kept
    opts = dict(use_symmetries=use_symmetries)
    expected = selfplay.GameBuffer(rules, n, n)
    j = 0
    for raw, game in zip(raws, games):
        boards, signs = replayed(game, n)
        fresh = []
        for k in range(len(game["samples"])):
            stones = int(np.asarray(game["samples"][k][8:10]).view(np.uint16)[0])
            moves = [int(m) for m in game["moves"][:stones]]
            assert signs[k] == (1 if not moves else 3 - (moves[-1] & 3))       # the searcher's side to move is the game's
            fresh.append(oracle_sample(olib, rules, n, moves, base_serial + j, evaluator, opts)[1])
            j += 1
        expected.add_reanalysed(raw, fresh)
    want = buffer_games(expected)
    assert want != [r.tobytes() for r in raws]
    total = sum(len(g["samples"]) for g in games)

    results = {}
    for slots, chunk in ((5, 0), (5, 7), (3, 0), (8, 0)):
        ps = tps.make_searcher(rules, n, slots, use_symmetries=use_symmetries)
        out, stats = ds.reanalyse(ps, net, fragment=0, chunk=chunk, serial_base=base_serial)
        ps.close()
        results[(slots, chunk)] = buffer_games(out)
        assert stats["games"] == 2 and stats["samples"] == total and stats["replaced"] == total and stats["kept"] == 0, stats
        assert stats["status"] == [total, 0, 0, 0] and stats["steps"] >= total
        if (slots, chunk) == (5, 0):
            for got, game in zip((ref.parse_game(out.game(i)) for i in range(2)), games):     # moves and outcome are the game's
                assert got["moves"].tolist() == game["moves"].tolist() and (got["outcome"], got["rows"], got["cols"]) == (game["outcome"], n, n)
            path = tmp_path / "reanalysed.bin"      # and the consumers take the result: save -> a dataset fragment -> a batch
            out.save(path)
            again = TrainingDataset(rules, n, n)
            again.add_fragment(path, index=1)
            assert again.games()[:, 2].tolist() == [len(g["samples"]) for g in games]
            batch = again.load_batch_host([[1, g, k, (g + k) % 8] for g, game in enumerate(games) for k in range(len(game["samples"]))])
            assert np.isfinite(batch["policy_target"]).all() and np.allclose(batch["policy_target"].reshape(total, -1).sum(1), 1.0, atol=1e-4)
            again.close()
        out.close()
    for key, got in results.items():
        assert got == want, key          # the oracle's records, game for game and byte for byte — whatever the chunk and the slot count

    # refusals before anything is launched: another board, other rules
    other = tps.make_searcher(1, n, 2)
    with pytest.raises(Exception) as e:
        ds.reanalyse(other, net)
    assert "agx error 1" in str(e.value)
    other.close()
    ps = tps.make_searcher(rules, n, 2)
    wrong = selfplay.GameBuffer(rules, n + 1, n + 1)
    with pytest.raises(Exception) as e:
        ds.reanalyse(ps, net, out=wrong)
    assert "agx error 1" in str(e.value) and wrong.stats()["games"] == 0
    with pytest.raises(Exception):
        ds.reanalyse(ps, net, fragment=4)
    ps.close()
    wrong.close()
    net.close()
    ds.close()
    for b in (source, expected):
        b.close()


def test_torch_tensors_on_a_torch_stream_and_a_training_step(agx_lib, saved_games):
    """in a process of its own (the library has to share torch's HIP runtime from the start): TrainingDataset.positions with device torch
    tensors on a non-default torch stream; and the 9x9 game reanalysed there, a dataset of the result, a batch, one Trainer.step"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    args = [x for rules, n, path, _ in saved_games for x in (str(rules), str(n), str(path))]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reanalyse_torch_main.py")] + args, capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0 and "ok:" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
