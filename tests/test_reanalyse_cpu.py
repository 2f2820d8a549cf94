"""Reanalysis without a GPU: the host framing of reanalysed games (csrc/game_buffer.cpp: agx_game_buffer_add_reanalysed) on oracle games,
and the numpy restatement of the searcher's sample sink (tests/reanalyse_ref.py) against hand-written bytes and against the oracle's
SearchDataStorage_v201::loadFrom + serialize (ago_sample_v201_pack).  Every comparison is on the bytes."""
import numpy as np
import pytest

import oracle_lib as ol
import reanalyse_ref as rref
import training_batch_ref as ref

F32 = np.float32
INVALID = 1
UNKNOWN = rref.UNKNOWN_SCORE


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@pytest.fixture(scope="module")
def games(olib):
    return [ref.oracle_game(olib, 0, 15, 5, sims=32), ref.oracle_game(olib, 0, 15, 6, sims=32), ref.crafted_game(olib, 15)]


def win_in(k):
    return (3 << 13) | (4000 - k)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def rows_of(n, edges):
    """dense rows from (cell, visits, prior, win, draw, score) tuples, in root order"""
    cells = n * n
    rows = dict(visits=np.zeros(cells, np.int32), prior=np.zeros(cells, F32), q=np.zeros((cells, 2), F32), score=np.zeros(cells, np.uint16),
                edge_index=np.full(cells, -1, np.int16))
    for i, (c, v, p, w, d, s) in enumerate(edges):
        rows["visits"][c], rows["prior"][c], rows["score"][c], rows["edge_index"][c] = v, p, s, i
        rows["q"][c] = (w, d)
    return rows


def oracle_pack(olib, n, stones, edges, root_score, flags):
    return ref.pack_sample(olib, n, stones, [e[0] for e in edges], [e[1] for e in edges], [[e[3], e[4]] for e in edges], [e[5] for e in edges],
                           prior=[e[2] for e in edges], root_score=root_score, flags=flags)


def H(text):
    return np.frombuffer(bytes.fromhex(text.replace(" ", "")), np.uint8)


# The codes below, by hand.  PriorFormat (4 exponent bits from -16, 4 mantissa bits) has the largest value 1.9375 / 2 = 0.96875, VisitFormat
# (3 from -8, 5) 1.96875 / 2 = 0.984375; a maximum m gets the scale m / largest, so the maximum itself encodes as 0xFF and half of it as 0xEF.
# ScaleFormat (5 exponent bits from -16, 11 mantissa bits): 1.0 -> 16 << 11 = 0x8000; 1 / 0.96875 = 1.032258 -> 0x8000 + int(0.032258 * 2048
# + 0.5) = 0x8042; 0.5 / 0.96875 = 1.032258 / 2 -> 0x7842; 1 / 0.984375 = 1.015873 -> 0x8000 + 33 = 0x8021; 3 / 0.984375 = 1.5238095 * 2 ->
# (17 << 11) + int(0.5238095 * 2048 + 0.5) = 0x8C31; 7 / 0.984375 = 1.7777778 * 4 -> (18 << 11) + 1593 = 0x9639.  1 visit of at most 3:
# 0.328125 = 1.3125 / 4 -> (6 << 5) | int(0.3125 * 32 + 0.5) = 0xCA.  Score() = unknown 0 -> 0x80; a win in 3 -> (3 << 6) | 3 = 0xC3.
# Header: value, prior and visit scale, root score (unknown 0 = 0x4FA0; a win in 4 = 0x6F9C), move number, flags, u32 entries.
HAND = [
    ("one edge", 15, 5, [(17, 1, 1.0, 0.5, 0.25, UNKNOWN)], UNKNOWN, 0,
     "4278 4280 2180 A04F 0500 0000 01000000" "11 FF FF 80 FF EF"),
    ("all priors 0", 15, 2, [(0, 3, 0.0, 0.0, 0.0, UNKNOWN), (224, 1, 0.0, 0.0, 0.0, UNKNOWN)], UNKNOWN, 0,
     "0080 0080 318C A04F 0200 0000 02000000" "00 FF 00 80 00 00" "E0 CA 00 80 00 00"),
    ("proven edge with 0 visits", 15, 4, [(10, 0, 0.5, 1.0, 0.0, win_in(3)), (11, 0, 0.5, 0.0, 0.0, UNKNOWN)], win_in(4), 2,
     "4280 4278 2180 9C6F 0400 0200 01000000" "0A 00 FF C3 FF 00"),
    ("20x20, first kept cell 300: a filler at 255", 20, 2, [(300, 7, 1.0, 0.5, 0.25, UNKNOWN)], UNKNOWN, 0,
     "4278 4280 3996 A04F 0200 0000 02000000" "FF 00 00 80 00 00" "2D FF FF 80 FF EF"),
    ("20x20, kept cells 3 and 399: a filler at 258", 20, 2, [(3, 1, 0.5, 0.5, 0.25, UNKNOWN), (399, 1, 0.5, 0.5, 0.25, UNKNOWN)], UNKNOWN, 0,
     "4278 4278 2180 A04F 0200 0000 03000000" "03 FF FF 80 FF EF" "FF 00 00 80 00 00" "8D FF FF 80 FF EF"),
]


@pytest.mark.parametrize("name,n,stones,edges,root_score,flags,text", HAND, ids=[h[0] for h in HAND])
def test_restatement_on_hand_written_bytes(olib, name, n, stones, edges, root_score, flags, text):
    want = H(text)
    got = rref.sample_bytes(n, rows_of(n, edges), root_score, stones, flags)
    assert got.tobytes() == want.tobytes(), (name, got.tobytes().hex(), want.tobytes().hex())
    assert oracle_pack(olib, n, stones, edges, root_score, flags).tobytes() == want.tobytes(), name     # and the oracle writes the same
    assert rref.has_filler(got) == ("filler" in name)


def test_restatement_equals_the_oracles_pack(olib):
    """random roots on 15x15 and 20x20: unvisited edges (not kept, or kept as a filler WITH its edge's values), proven scores of every kind,
    zero and tiny values, up to 400 edges"""
    rng = np.random.default_rng(11)
    fillers = with_edge = 0
    for trial in range(60):
        n = 15 if trial % 3 == 0 else 20
        cells = n * n
        count = int(rng.integers(1, cells + 1)) if trial % 4 == 0 else int(rng.integers(1, 12))
        where = rng.permutation(cells)[:count]
        if trial % 5 == 1:
            where = np.unique(np.concatenate([rng.integers(0, 40, 3), rng.integers(cells - 40, cells, 3)]))     # both ends only: fillers
        edges = []
        for c in where:
            kind = int(rng.integers(0, 6))
            visits = 0 if kind in (0, 1) else int(rng.integers(1, 200))
            score = [UNKNOWN, win_in(int(rng.integers(0, 80))), (0 << 13) | (4000 + int(rng.integers(0, 80))), (1 << 13) | (4000 + int(rng.integers(0, 80))),
                     (2 << 13) | (4000 + int(rng.integers(-900, 900))), UNKNOWN][kind]
            win = F32(rng.random()) * F32(0.9) if kind != 0 else F32(0.0)
            edges.append((int(c), visits, F32(rng.random()) if trial % 7 else F32(0.0), win, F32(F32(1.0) - win) * F32(rng.random()), score))
        if trial % 10 == 2:     # an edge on every cell, visits at both ends only: the filler in between carries its edge's prior and value
            edges = [(c, 0 if 5 < c < cells - 5 else 3, F32(rng.random()), F32(0.3), F32(0.2), UNKNOWN) for c in range(cells)]
        root_score = [UNKNOWN, win_in(5), (2 << 13) | 4123][trial % 3]
        stones, flags = int(rng.integers(0, cells - 1)), int(rng.integers(0, 8))
        got = rref.sample_bytes(n, rows_of(n, edges), root_score, stones, flags)
        want = oracle_pack(olib, n, stones, edges, root_score, flags)
        assert got.tobytes() == want.tobytes(), trial
        fillers += rref.has_filler(got)
        at = np.cumsum(got[16:].reshape(-1, 6)[:, 0].astype(np.int64))
        kept = {e[0] for e in edges if e[1] > 0 or rref.proven(e[5])}
        with_edge += any(int(c) not in kept and int(c) in {e[0] for e in edges} for c in at)
    assert fillers >= 5 and with_edge >= 1


# ---- framing ------------------------------------------------------------------------------------------------------------------------------
def buffer_games(buffer):
    return [buffer.game(i).tobytes() for i in range(buffer.stats()["games"])]


def repacked(olib, n, sample):
    """a sample's own content through the oracle's loadFrom + serialize again: ago_sample_v201_unpack, then ago_sample_v201_pack of the cells
    that carry an entry"""
    visits, prior, value, score, header = ref.unpack(olib, sample, n)
    entries = np.asarray(sample[16:], np.uint8).reshape(-1, 6)
    cells = np.cumsum(entries[:, 0].astype(np.int64))
    return ref.pack_sample(olib, n, int(header[1]), [int(c) for c in cells], visits[cells], value[cells], score[cells], prior=prior[cells],
                           root_score=int(header[0]) & 0xFFFF, flags=int(header[2]))


def test_framing_round_trip(agx_lib, olib, games):
    from alphagomoku_amd import selfplay
    n = 15
    out = selfplay.GameBuffer(0, n, n)
    changed = 0
    for raw in games:
        game = ref.parse_game(raw)
        # the game's own samples as replacements: the identical game
        out.add_reanalysed(raw, game["samples"])
        assert out.game(out.stats()["games"] - 1).tobytes() == raw.tobytes()
        # ... re-packed by the oracle (a second quantisation of already quantised values): framed as build_game frames them
        again = [repacked(olib, n, s) for s in game["samples"]]
        changed += sum(a.tobytes() != s.tobytes() for a, s in zip(again, game["samples"]))
        out.add_reanalysed(raw, again)
        assert out.game(out.stats()["games"] - 1).tobytes() == ref.build_game(again, game["moves"], game["outcome"], n).tobytes()
        # with some sizes 0 the old samples survive; moves, outcome, rows and cols stay
        mixed = [a if k % 3 == 1 else None for k, a in enumerate(again)]
        out.add_reanalysed(raw, mixed)
        want = [a if k % 3 == 1 else s for k, (a, s) in enumerate(zip(again, game["samples"]))]
        got = ref.parse_game(out.game(out.stats()["games"] - 1))
        assert [s.tobytes() for s in got["samples"]] == [s.tobytes() for s in want]
        assert got["moves"].tolist() == game["moves"].tolist() and (got["outcome"], got["rows"], got["cols"]) == (game["outcome"], n, n)
    stats = out.stats()
    assert stats["games"] == 9 and stats["samples"] == 3 * sum(len(ref.parse_game(g)["samples"]) for g in games)
    assert stats["game_length"] == 3 * sum(len(ref.parse_game(g)["moves"]) for g in games) and stats["cross_win"] + stats["draws"] + stats["circle_win"] == 9
    out.close()


def test_framing_refusals(agx_lib, olib, games):
    from alphagomoku_amd import selfplay
    lib = agx_lib
    raw = games[0]
    game = ref.parse_game(raw)
    out = selfplay.GameBuffer(0, 15, 15)

    def refused(game_bytes, samples, word):
        with pytest.raises(Exception) as e:
            out.add_reanalysed(game_bytes, samples)
        assert "agx error %d" % INVALID in str(e.value) and word in str(e.value), str(e.value)
        assert out.stats()["games"] == 0

    assert len(game["samples"]) >= 3
    wrong_move = list(game["samples"])
    wrong_move[1] = game["samples"][2]                                   # a whole sample, of another move
    refused(raw, wrong_move, "move")
    refused(raw, game["samples"][:-1], "samples given")                 # a count that differs from the game's
    refused(raw, list(game["samples"]) + [game["samples"][0]], "samples given")
    refused(raw[:-5], game["samples"], "bytes where its layout")        # truncated behind the moves
    refused(raw[:len(raw) // 2], game["samples"], "truncated")          # ... and inside a sample
    refused(raw[:10], game["samples"], "truncated")
    short = list(game["samples"])
    short[0] = game["samples"][0][:-6]                                   # a replacement that is no whole sample
    refused(raw, short, "entries need")
    other = selfplay.GameBuffer(0, 20, 20)
    with pytest.raises(Exception) as e:
        other.add_reanalysed(raw, game["samples"])
    assert "15x15" in str(e.value)
    assert lib.agx_game_buffer_add_reanalysed(None, None, 0, 0, None, None) == INVALID
    other.close()
    out.close()


def test_framing_feeds_the_consumers(agx_lib, olib, games, tmp_path):
    """the reanalysed buffer through save -> load and through a dataset fragment: the sample counts are the games'.  (What a batch of it holds
    is checked on the device, tests/test_reanalyse_gpu.py; without one, the loader's index check stands for it: sample `count` is refused
    before anything touches a device, sample count - 1 is not refused by that check.)"""
    from alphagomoku_amd import selfplay, dataset
    n = 15
    out = selfplay.GameBuffer(0, n, n)
    counts = []
    for raw in games:
        game = ref.parse_game(raw)
        out.add_reanalysed(raw, [repacked(olib, n, s) if k % 2 else None for k, s in enumerate(game["samples"])])
        counts.append(len(game["samples"]))
    path = tmp_path / "reanalysed.bin"
    out.save(path)
    loaded = selfplay.GameBuffer(0, n, n)
    loaded.load(path)
    assert buffer_games(loaded) == buffer_games(out) and loaded.stats() == out.stats()
    ds = dataset.TrainingDataset(0, n, n)
    assert ds.add_fragment(out) == 0 and ds.add_fragment(path) == 1
    assert ds.games().tolist() == [[f, g, counts[g], 8] for f in (0, 1) for g in range(3)]
    assert ds.stats()["samples"] == 2 * sum(counts)
    for g, count in enumerate(counts):
        with pytest.raises(Exception) as e:
            ds.load_batch_host([[0, g, count, 0]])
        assert "agx error %d" % INVALID in str(e.value) and "names sample %d of a game with %d" % (count, count) in str(e.value)
    # the same index checks stand in front of the positions kernel
    rec, dummy = np.array([[0, 0, 0, 0], [0, 0, counts[0], 0]], np.int32), np.zeros(2 * n * n, np.uint8)
    assert agx_lib.agx_dataset_positions(ds._h, 2, ol.ptr(rec), ol.ptr(dummy), ol.ptr(dummy), None) == INVALID and b"sample 1 names" in agx_lib.agx_last_error()
    for b in (out, loaded):
        b.close()
    ds.close()
