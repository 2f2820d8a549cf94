"""Training batches without a GPU: the CPU restatement of the reference's load_batch (tests/training_batch_ref.py) against hand-computed
values, the host half of the C ABI's dataset (csrc/training_batch.hip: fragments, index, sizes, shapes, refusals) and the Python sampler."""
import ctypes
import zlib

import numpy as np
import pytest

import oracle_lib as ol
import training_batch_ref as ref

F32 = np.float32


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@pytest.fixture(scope="module")
def fragment(olib, tmp_path_factory):
    games = [ref.oracle_game(olib, 0, 15, 5, sims=32), ref.oracle_game(olib, 0, 15, 6, sims=32), ref.crafted_game(olib, 15)]
    path = tmp_path_factory.mktemp("fragment") / "freestyle_15.bin"
    ref.write_fragment(path, "FREESTYLE", 15, games)
    return dict(path=path, raw=games, games=[ref.parse_game(g) for g in games])


def test_helper_on_a_crafted_sample(olib):
    """sample 0 of the crafted game: a proven win (cell 20), a proven loss (40, 5 visits), a proven draw without visits (41) and an ordinary
    edge (100, 37 visits -> 37 after the 5-bit visit code: 37 / 37 * max), cross to move, cross won the game"""
    n = 15
    game = ref.parse_game(ref.crafted_game(olib, n))
    st = ref.sample_stats(olib, game, 0, n)
    assert (st["wins"], st["losses"], st["draws"], st["draws_without_visits"]) == (1, 1, 1, 1)
    r = ref.reference_sample(olib, 0, n, game, 0, 0)
    total = F32(F32(F32(F32(0.0) + F32(1.0e6)) + F32(1.0e-6)) + F32(1.0)) + F32(37.0)     # cell order: 20, 40, 41, 100
    scale = F32(1.0) / total
    expect = {20: F32(1.0e6) * scale, 40: F32(1.0e-6) * scale, 41: F32(1.0) * scale, 100: F32(37.0) * scale}
    for cell in range(n * n):
        assert r["policy"][cell] == expect.get(cell, F32(0.0)), cell
    assert abs(float(r["policy"].sum(dtype=np.float64)) - 1.0) < 1e-6
    assert list(r["action_values"][20]) == [1.0, 0.0, 0.0] and list(r["action_values"][40]) == [0.0, 0.0, 1.0] and list(r["action_values"][41]) == [0.0, 1.0, 0.0]
    w, d = r["action_values"][100][:2]                      # the stored (0.45, 0.25) within the 4-bit value code
    assert abs(w - 0.45) < 0.03 and abs(d - 0.25) < 0.03 and r["action_values"][100][2] == F32(1.0) - (w + d)
    assert list(r["action_values"][0]) == [0.0, 0.0, 1.0]   # a cell without an entry: Value() = (0, 0)
    assert r["sign"] == 1 and list(r["value"]) == [1.0, 0.0, 0.0] and r["moves_left"][0] == 1.0
    # SamplerVisits: the proven draw keeps its 0 visits
    v = ref.reference_sample(olib, 0, n, game, 0, 0, policy="visits")
    assert v["policy"][41] == 0.0 and v["policy"][100] == F32(37.0) * (F32(1.0) / (F32(F32(F32(1.0e6)) + F32(1.0e-6)) + F32(37.0)))
    # circle to move in a game cross won: a loss; a drawn game: a draw; circle won: a win
    c = ref.reference_sample(olib, 0, n, game, 2, 0)
    assert c["sign"] == 2 and list(c["value"]) == [0.0, 0.0, 1.0] and c["moves_left"][0] == 2.0
    for outcome, sign_sample, want in ((1, 0, [0.0, 1.0, 0.0]), (1, 2, [0.0, 1.0, 0.0]), (3, 2, [1.0, 0.0, 0.0]), (3, 0, [0.0, 0.0, 1.0])):
        assert list(ref.reference_sample(olib, 0, n, dict(game, outcome=outcome), sign_sample, 0)["value"]) == want
    # renju: (7, 7) joins two open threes of cross -> the foul bit, only with cross to move
    assert ((ref.reference_sample(olib, 2, n, game, 0, 0)["features"] >> 6) & 1).sum() == 1
    assert ((ref.reference_sample(olib, 2, n, game, 2, 0)["features"] >> 6) & 1).sum() == 0
    assert ((r["features"] >> 6) & 1).sum() == 0


def test_symmetry_then_its_inverse_is_the_identity(olib, fragment):
    n = 15
    game = fragment["games"][0]
    for k in (0, len(game["samples"]) // 2):
        plain = ref.reference_sample(olib, 0, n, game, k, 0)
        for s in range(8):
            r = ref.reference_sample(olib, 0, n, game, k, s)
            inv = olib.ago_inverse_symmetry(s)
            assert abs(float(r["policy"].sum(dtype=np.float64)) - 1.0) < 1e-5
            assert np.array_equal(ref.symmetric(olib, n, inv, r["board"]), plain["board"])
            for c in range(3):
                assert np.array_equal(ref.symmetric(olib, n, inv, np.ascontiguousarray(r["action_values"][:, c])), plain["action_values"][:, c])
            back = ref.symmetric(olib, n, inv, r["policy"])
            assert np.allclose(back, plain["policy"], rtol=1e-6, atol=0) and np.array_equal(back != 0, plain["policy"] != 0)   # (the sum's order differs)
            assert np.array_equal(r["value"], plain["value"]) and np.array_equal(r["moves_left"], plain["moves_left"])


def _dataset(lib, rules=0, n=15):
    from alphagomoku_amd import check
    h = ctypes.c_void_p()
    check(lib.agx_dataset_create(rules, n, n, ctypes.byref(h)))
    return h


def test_dataset_host_half(agx_lib, olib, fragment, tmp_path):
    from alphagomoku_amd import check, selfplay
    from alphagomoku_amd._lib import AgxGameBufferStats, AgxTensorShape, AgxDatasetSample
    lib = agx_lib
    packed = tmp_path / "packed.bin"
    packed.write_bytes(zlib.compress(fragment["path"].read_bytes()))
    buffer = selfplay.GameBuffer(0, 15, 15)
    check(lib.agx_game_buffer_load(buffer._h, str(fragment["path"]).encode()))
    h = _dataset(lib)
    check(lib.agx_dataset_add_fragment_file(h, 4, str(fragment["path"]).encode()))
    check(lib.agx_dataset_add_fragment_file(h, 2, str(packed).encode()))
    check(lib.agx_dataset_add_fragment_buffer(h, 7, buffer._h))
    games = ctypes.c_int()
    check(lib.agx_dataset_games(h, ctypes.byref(games)))
    assert games.value == 9
    sizes = np.zeros((9, 4), np.int32)
    check(lib.agx_dataset_sizes(h, ol.ptr(sizes), 9))
    counts = [len(g["samples"]) for g in fragment["games"]]
    assert sizes.tolist() == [[f, g, counts[g], 8] for f in (2, 4, 7) for g in range(3)]     # fragments in ascending order
    assert lib.agx_dataset_sizes(h, ol.ptr(sizes), 8) != 0
    st = AgxGameBufferStats()
    check(lib.agx_dataset_stats(h, ctypes.byref(st)))
    assert st.games == 9 and st.samples == 3 * sum(counts) and st.game_length == 3 * sum(len(g["moves"]) for g in fragment["games"])
    assert st.cross_win + st.draws + st.circle_win == 9
    shapes = [AgxTensorShape() for _ in range(6)]
    check(lib.agx_dataset_tensor_shapes(h, 5, *[ctypes.byref(s) for s in shapes]))
    assert [list(s.dim[:s.rank]) for s in shapes] == [[5, 15, 15, 32], [5, 225], [5, 15, 15], [5, 3], [5, 1], [5, 15, 15, 3]]
    # unload, reload under the same number, refuse a number in use and an unknown one
    check(lib.agx_dataset_unload_fragment(h, 4))
    check(lib.agx_dataset_games(h, ctypes.byref(games)))
    assert games.value == 6 and lib.agx_dataset_unload_fragment(h, 4) != 0
    assert lib.agx_dataset_add_fragment_file(h, 2, str(packed).encode()) != 0 and b"already loaded" in lib.agx_last_error()
    check(lib.agx_dataset_add_fragment_file(h, 4, str(packed).encode()))
    # an index out of range is refused before anything touches a device (there is none here)
    out = np.zeros(1 << 16, np.float32)
    for bad in ([3, 0, 0, 0], [2, 3, 0, 0], [2, 0, counts[0], 0], [2, 0, 0, 8], [2, 0, -1, 0], [2, -1, 0, 0]):
        rec = np.array([[2, 0, 0, 0], bad], np.int32)
        assert ctypes.sizeof(AgxDatasetSample) == 16
        assert lib.agx_dataset_load_batch_host(h, 2, ol.ptr(rec), None, None, ol.ptr(out), ol.ptr(out), ol.ptr(out), ol.ptr(out), 0) == 1, bad
        assert b"sample 1 names" in lib.agx_last_error()
        assert lib.agx_dataset_load_batch(h, 2, ol.ptr(rec), None, None, ol.ptr(out), ol.ptr(out), ol.ptr(out), ol.ptr(out), 0, None) == 1, bad
    check(lib.agx_dataset_destroy(h))
    buffer.close()


def test_dataset_refusals(agx_lib, olib, fragment, tmp_path):
    from alphagomoku_amd import check, selfplay
    lib = agx_lib
    path = str(fragment["path"]).encode()
    for rules, n, needle in ((1, 15, b"other rules"), (0, 20, b"15x15")):
        h = _dataset(lib, rules, n)
        assert lib.agx_dataset_add_fragment_file(h, 0, path) == 1 and needle in lib.agx_last_error(), lib.agx_last_error()
        buffer = selfplay.GameBuffer(0, 15, 15)
        assert lib.agx_dataset_add_fragment_buffer(h, 0, buffer._h) == 1
        buffer.close()
        check(lib.agx_dataset_destroy(h))
    h = _dataset(lib)
    raw = fragment["path"].read_bytes()
    cut = tmp_path / "cut.bin"
    cut.write_bytes(raw[:-40])                                   # the last game loses its tail
    assert lib.agx_dataset_add_fragment_file(h, 0, str(cut).encode()) == 1
    # layouts agx_game_buffer_load accepts but a reader must not follow: a sample beyond the game's moves, an entry beyond the board
    game = fragment["games"][2]
    late = [s.copy() for s in game["samples"]]
    late[1][8:10] = np.array([len(game["moves"])], np.uint16).view(np.uint8)
    far = [s.copy() for s in game["samples"]]
    far[0][16] = 250
    for samples, needle in ((late, b"at move"), (far, b"outside the board"), ([], b"no samples")):
        bad = tmp_path / "bad.bin"
        ref.write_fragment(bad, "FREESTYLE", 15, [ref.build_game(samples, game["moves"], 2, 15)])
        assert lib.agx_dataset_add_fragment_file(h, 0, str(bad).encode()) == 1 and needle in lib.agx_last_error(), lib.agx_last_error()
    games = ctypes.c_int(-1)
    check(lib.agx_dataset_games(h, ctypes.byref(games)))
    assert games.value == 0
    check(lib.agx_dataset_destroy(h))
    h = ctypes.c_void_p()
    assert lib.agx_dataset_create(0, 15, 20, ctypes.byref(h)) != 0 and lib.agx_dataset_create(7, 15, 15, ctypes.byref(h)) != 0
    rules, rows, cols = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib.agx_game_buffer_file_config(path, ctypes.byref(rules), ctypes.byref(rows), ctypes.byref(cols)))
    assert (rules.value, rows.value, cols.value) == (0, 15, 15)


def test_sampler(agx_lib, fragment):
    from alphagomoku_amd.dataset import TrainingDataset
    ds = TrainingDataset(0, 15, 15)
    assert ds.add_fragment(fragment["path"]) == 0 and ds.add_fragment(fragment["path"]) == 1
    games = ds.games()
    assert games.shape == (6, 4) and ds.number_of_games() == 6
    a = ds.sample(40, np.random.default_rng(123))
    ds2 = TrainingDataset(0, 15, 15)
    ds2.add_fragment(fragment["path"])
    ds2.add_fragment(fragment["path"])
    b = ds2.sample(40, np.random.default_rng(123))
    assert np.array_equal(a, b) and not np.array_equal(a, ds2.sample(40, np.random.default_rng(124)))
    counts = {(int(f), int(g)): int(k) for f, g, k, _ in games}
    for epoch in range(6):    # every game once per epoch
        rows = a[6 * epoch:6 * epoch + 6]
        assert sorted((int(f), int(g)) for f, g, _, _ in rows) == sorted(counts)
    assert all(0 <= k < counts[(int(f), int(g))] and 0 <= s < 8 for f, g, k, s in a)
    assert len({int(s) for s in a[:, 3]}) > 3 and ds.tensor_shapes(2)["input"] == (2, 15, 15, 32)
    with pytest.raises(Exception):
        ds.load_batch_host([[0, 0, 10 ** 6, 0]])
    ds.close()
    ds2.close()
