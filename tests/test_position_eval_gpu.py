"""Positions evaluated on the device (csrc/position_eval.hip, agx.h: agx_position_evaluator_*): the encode launch against the oracle's
NNInputFeatures::encode, the combine launch against its numpy float32 restatement (tests/position_eval_ref.py) on the tower's own rows.
Every comparison is on the raw bits; every output lies between two guard zones filled with a sentinel that must survive the launch."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import position_eval_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD, SENTINEL = 333, 0x5A
CONFIGS = [("FREESTYLE", 15), ("STANDARD", 15), ("RENJU", 15), ("CARO5", 15), ("CARO6", 15), ("FREESTYLE", 20), ("CARO5", 20), ("RENJU", 20)]
OUT_KINDS = dict(policy=np.float32, value=np.float32, action_values=np.float32, top_cells=np.int32, top_probs=np.float32, status=np.int32)


@pytest.fixture(scope="module")
def olib():
    return ol.load()


image_map = functools.lru_cache(maxsize=None)(ref.image_map)


class Guarded:
    """`count` elements of device memory between two guard zones"""

    def __init__(self, count, dtype):
        from alphagomoku_amd.networks import DeviceBuffer
        self.count, self.dtype = count, np.dtype(dtype)
        self.buf = DeviceBuffer((count + 2 * GUARD) * self.dtype.itemsize)
        self.buf.upload(np.full((count + 2 * GUARD) * self.dtype.itemsize, SENTINEL, np.uint8))
        self.ptr = self.buf.ptr.value + GUARD * self.dtype.itemsize

    def take(self, shape, what=""):
        flat = self.buf.download((self.count + 2 * GUARD,), self.dtype)
        self.buf.free()
        raw, item = flat.view(np.uint8), self.dtype.itemsize
        assert (raw[:GUARD * item] == SENTINEL).all() and (raw[-GUARD * item:] == SENTINEL).all(), "guard zone of %s overwritten" % what
        return flat[GUARD:GUARD + self.count].reshape(shape)

    def untouched(self):
        flat = self.buf.download((self.count + 2 * GUARD,), self.dtype)
        self.buf.free()
        return bool((flat.view(np.uint8) == SENTINEL).all())


class Evaluator:
    """the C ABI, driven through ctypes with guarded buffers"""

    def __init__(self, lib, rules, n, capacity):
        self.lib, self.n, self.hw = lib, n, n * n
        self.handle = ctypes.c_void_p()
        from alphagomoku_amd import check
        check(lib.agx_position_evaluator_create(rules, n, capacity, ctypes.byref(self.handle)))

    def upload(self, boards, signs):
        from alphagomoku_amd.networks import DeviceBuffer
        b = np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(len(signs), self.hw))
        s = np.ascontiguousarray(np.asarray(signs, np.uint8))
        d_b, d_s = DeviceBuffer(b.nbytes), DeviceBuffer(s.nbytes)
        d_b.upload(b)
        d_s.upload(s)
        return d_b, d_s

    def encode(self, boards, signs, mask, expect=0):
        """-> features [n * S, hw] uint32, status [n]; with `expect` != 0 the status code of a refused call"""
        from alphagomoku_amd import check
        n, S = len(signs), len(ref.symmetries_of(mask & 0xFF)) or 1
        d_b, d_s = self.upload(boards, signs)
        f, st = Guarded(n * S * self.hw, np.uint32), Guarded(n, np.int32)
        code = self.lib.agx_position_evaluator_encode(self.handle, n, d_b.ptr, d_s.ptr, mask, f.ptr, st.ptr, None)
        check(self.lib.agx_device_synchronize())
        d_b.free()
        d_s.free()
        if expect:
            assert code == expect and f.untouched() and st.untouched(), (code, self.lib.agx_last_error())
            return None
        check(code)
        return f.take((n * S, self.hw), "features"), st.take((n,), "status")

    def evaluate(self, net, boards, signs, mask, flags, top_k, with_q, expect=0, force_q=False):
        from alphagomoku_amd import check, _lib
        n = len(signs)
        d_b, d_s = self.upload(boards, signs)
        shapes = dict(policy=(n, self.hw), value=(n, 3), action_values=(n, self.hw, 2), top_cells=(n, max(top_k, 0)), top_probs=(n, max(top_k, 0)), status=(n,))
        names = [k for k in shapes if (with_q or force_q or k != "action_values")]
        bufs = {k: Guarded(int(np.prod(shapes[k])), OUT_KINDS[k]) for k in names}
        c_out = _lib.AgxPositionOutputs()
        for k, g in bufs.items():
            setattr(c_out, k, g.ptr)
        code = self.lib.agx_position_evaluator_evaluate(self.handle, net._net, n, d_b.ptr, d_s.ptr, mask, flags, top_k, ctypes.byref(c_out), None)
        check(self.lib.agx_device_synchronize())
        d_b.free()
        d_s.free()
        if expect:
            message = self.lib.agx_last_error().decode()
            assert code == expect and all(g.untouched() for g in bufs.values()) and message, (code, message)
            return message
        check(code)
        return {k: g.take(shapes[k], k) for k, g in bufs.items()}

    def combine(self, boards, mask, flags, top_k, features, rows, status_in, want_q, expect=0):
        """agx_position_evaluator_combine on rows the caller got from the tower; features / status_in / rows[2] may be None (NULL)"""
        from alphagomoku_amd import check, _lib
        from alphagomoku_amd.networks import DeviceBuffer
        n = len(boards)
        d_b, d_s = self.upload(boards, [1] * n)
        staged = []

        def device(a):
            if a is None:
                return None
            buf = DeviceBuffer(a.nbytes)
            buf.upload(a)
            staged.append(buf)
            return buf.ptr
        shapes = dict(policy=(n, self.hw), value=(n, 3), action_values=(n, self.hw, 2), top_cells=(n, top_k), top_probs=(n, top_k), status=(n,))
        bufs = {k: Guarded(int(np.prod(shapes[k])), OUT_KINDS[k]) for k in shapes if want_q or k != "action_values"}
        c_out = _lib.AgxPositionOutputs()
        for k, g in bufs.items():
            setattr(c_out, k, g.ptr)
        code = self.lib.agx_position_evaluator_combine(self.handle, n, d_b.ptr, mask, flags, top_k, device(features), device(rows[0]), device(rows[1]), device(rows[2]),
                                                       device(status_in), ctypes.byref(c_out), None)
        check(self.lib.agx_device_synchronize())
        for buf in staged + [d_b, d_s]:
            buf.free()
        if expect:
            assert code == expect and all(g.untouched() for g in bufs.values()), (code, self.lib.agx_last_error())
            return None
        check(code)
        return {k: g.take(shapes[k], k) for k, g in bufs.items()}

    def close(self):
        self.lib.agx_position_evaluator_destroy(self.handle)


@pytest.fixture(scope="module")
def nets(agx_lib):
    """1-block, 64-filter synthetic networks: (board size, 'pv' / 'pvq') -> AGNetwork"""
    from alphagomoku_amd import synthetic
    from alphagomoku_amd.networks import AGNetwork
    made = {}

    def get(n, kind):
        if (n, kind) not in made:
            desc = synthetic.net_desc(blocks=1, filters=64)
            desc.update(rows=n, cols=n, action_values=1 if kind == "pvq" else 0)
            blob, _ = synthetic.make_weights(desc, seed=3 + n)
            net = AGNetwork(desc)
            net.loadWeights(blob)
            made[(n, kind)] = (net, desc, blob)
        return made[(n, kind)][0]
    get.made = made
    yield get
    for net, _, _ in made.values():
        net.close()


def tower_rows(net, features):
    """the tower's own rows for the feature rows: policy [R, hw], value [R, 3], q [R, hw, 2] or None"""
    out = net.forward(features)
    return out[0], out[1], (out[2] if len(out) > 2 else None)


def embed(board, n):
    out = np.zeros((n, n), np.uint8)
    a = np.asarray(board, np.uint8)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def lds_overflow_boards(n):
    """the boards of test_pattern_state_with_lists_beyond_their_lds_capacity (tests/test_engine_gpu.py): two threes, then three twos, in
    every other row — threat lists of 30-56 cells, beyond the 24 (OPEN_3: 64 / 96) entries kept in LDS"""
    out = []
    for side in (1, 2):
        for starts, length in (((2, 9), 3), ((1, 6, 11), 2)):
            b = np.zeros((n, n), np.uint8)
            for r in range(0, n, 2):
                for c0 in starts:
                    b[r, c0:c0 + length] = side
            out.append(b)
    return out


def crafted_positions(n):
    empty = np.zeros((n, n), np.uint8)
    corners = empty.copy()
    corners[0, 0] = corners[n - 1, n - 1] = 1
    corners[0, n - 1] = corners[n - 1, 0] = 2
    edges = corners.copy()
    edges[0, 3:7], edges[n - 1, 5:8], edges[4:7, 0], edges[6:10, n - 1] = 1, 2, 2, 1
    full = np.fromfunction(lambda r, c: 1 + ((r // 2 + c) % 2), (n, n)).astype(np.uint8)
    full[n // 2, n // 3] = 0
    return [empty, corners, edges, full]


def golden_positions(n):
    """the boards of the reference's own feature and rule cases (tests/golden), in the top-left corner of an n x n board"""
    feature_cases = json.load(open(os.path.join(GOLDEN, "ref_features_cases.json")))
    rule_cases = json.load(open(os.path.join(GOLDEN, "ref_rules_cases.json")))
    return [embed(c["board"], n) for c in feature_cases + rule_cases]


def oracle_rows(olib, rules, n, board, sign, mask):
    rows = []
    for s in ref.symmetries_of(mask):
        shown = np.zeros(n * n, np.uint32)
        olib.ago_apply_symmetry(n, s, 0, ol.ptr(np.ascontiguousarray(board.reshape(-1).astype(np.uint32))), ol.ptr(shown))
        rows.append(ol.encode_features(olib, rules, shown.astype(np.uint8).reshape(n, n), sign).reshape(-1))
    return rows


@pytest.mark.parametrize("rules,n", CONFIGS)
def test_feature_words_against_the_oracle(agx_lib, olib, rules, n):
    """row p * S + j == NNInputFeatures::encode of the board under the j-th symmetry of the mask, all 8 of them, both signs to move"""
    boards = crafted_positions(n) + lds_overflow_boards(n) + golden_positions(n)
    positions = [(b, sign) for b in boards for sign in (1, 2)]
    pe = Evaluator(agx_lib, ol.RULES[rules], n, len(positions))
    features, status = pe.encode([b for b, _ in positions], [s for _, s in positions], 0xFF)
    assert not status.any()
    fouls = 0
    for p, (board, sign) in enumerate(positions):
        want = oracle_rows(olib, ol.RULES[rules], n, board, sign, 0xFF)
        for j in range(8):
            assert np.array_equal(features[p * 8 + j], want[j]), (rules, n, p, j, int((features[p * 8 + j] != want[j]).sum()))
        fouls += int(((want[0] >> 6) & 1).sum())
    assert (fouls > 0) == (rules == "RENJU")   # the renju cases with cross to move do carry fouls
    pe.close()


def test_batch_geometry(agx_lib, olib, nets):
    """n = 1, 63, 64, 65 and 300 positions x 8 symmetries = 2400 rows, more than the ENCODE launch has waves (2048; the combine launch has
    one wave per position: test_more_positions_than_waves); the same position at different batch indices gives identical rows and
    outputs; the guard zones survive (Guarded.take)"""
    n, rules = 15, ol.RULES["RENJU"]
    kinds = (crafted_positions(n) + lds_overflow_boards(n) + golden_positions(n)[-3:])[:7]
    want = [oracle_rows(olib, rules, n, b, 1 + k % 2, 0xFF) for k, b in enumerate(kinds)]
    pe = Evaluator(agx_lib, rules, n, 300)
    net = nets(n, "pv")
    for size in (1, 63, 64, 65, 300):
        which = [(5 * p + p // 7) % 7 for p in range(size)]
        boards, signs = [kinds[k] for k in which], [1 + k % 2 for k in which]
        features, status = pe.encode(boards, signs, 0xFF)
        assert not status.any()
        for p, k in enumerate(which):
            assert np.array_equal(features[p * 8:p * 8 + 8], np.stack(want[k])), (size, p)
        out = pe.evaluate(net, boards, signs, 0xFF, ref.RENORMALISE, 3, False)
        first = {}
        for p, k in enumerate(which):
            q = first.setdefault(k, p)
            for name in ("policy", "value", "top_cells", "top_probs"):
                assert np.array_equal(out[name][p].view(np.uint32), out[name][q].view(np.uint32)), (size, name, p, q)
    pe.close()


def test_more_positions_than_waves(agx_lib, olib, nets, monkeypatch):
    """2348 positions with one symmetry: both launches have 2048 waves, so 300 waves of each take a second turn of their grid-stride
    loop.  Rows against the oracle; evaluate against the same position at a low batch index and, for positions of the second turn,
    against the restatement on the tower's own rows; guard zones"""
    monkeypatch.setattr(ref, "image_map", image_map)
    n, rules, size = 15, ol.RULES["RENJU"], 2348
    kinds = [(b, s) for b, s in combine_positions(n)]
    want = [oracle_rows(olib, rules, n, b, s, 0x01)[0] for b, s in kinds]
    which = [(3 * p + p // len(kinds)) % len(kinds) for p in range(size)]
    boards, signs = [kinds[k][0] for k in which], [kinds[k][1] for k in which]
    pe = Evaluator(agx_lib, rules, n, size)
    net = nets(n, "pvq")
    features, status = pe.encode(boards, signs, 0x01)
    assert not status.any() and np.array_equal(features, np.stack([want[k] for k in which]))
    flags = ref.MASK_FORBIDDEN | ref.RENORMALISE
    out = pe.evaluate(net, boards, signs, 0x01, flags, 3, True)
    first = {}
    for p, k in enumerate(which):
        q = first.setdefault(k, p)
        for name in ("policy", "value", "action_values", "top_cells", "top_probs"):
            assert np.array_equal(out[name][p].view(np.uint32), out[name][q].view(np.uint32)), (name, p, q)
    assert max(first.values()) < 2048 and len({which[p] for p in range(2048, size)}) == len(kinds)
    policy_rows, value_rows, q_rows = tower_rows(net, features)
    for p in range(2048, 2048 + 2 * len(kinds)):
        ours = ref.combine(n, boards[p], 0x01, flags, 3, policy_rows[p:p + 1], value_rows[p:p + 1], q_rows[p:p + 1], features[p])
        for name in ("policy", "value", "action_values", "top_cells", "top_probs"):
            assert np.array_equal(np.ascontiguousarray(out[name][p]).reshape(-1).view(np.uint32), np.ascontiguousarray(ours[name]).reshape(-1).view(np.uint32)), (name, p)
    pe.close()


def test_combine_launch_alone(agx_lib, nets):
    """agx_position_evaluator_combine on rows the caller got from the tower == evaluate, bit for bit; its optional arguments as NULL"""
    n = 15
    positions = combine_positions(n)
    boards, signs = [b for b, _ in positions], [s for _, s in positions]
    pe = Evaluator(agx_lib, ol.RULES["RENJU"], n, len(positions))
    net = nets(n, "pvq")
    names = ("policy", "value", "top_cells", "top_probs", "status")
    for mask, flags, top_k in ((0xFF, 3, 8), (0x24, 2, 1), (0x01, 1, 4)):
        features, status = pe.encode(boards, signs, mask)
        rows = tower_rows(net, features)
        whole = pe.evaluate(net, boards, signs, mask, flags, top_k, True)
        alone = pe.combine(boards, mask, flags, top_k, features, rows, status, True)
        for name in names + ("action_values",):
            assert np.array_equal(alone[name].view(np.uint32), whole[name].view(np.uint32)), (name, hex(mask))
        # without status words every position counts as valid; without action-value rows none are asked for; the feature rows are
        # read for MASK_FORBIDDEN only
        bare = pe.combine(boards, mask, flags, top_k, features if flags & 1 else None, (rows[0], rows[1], None), None, False)
        for name in names:
            assert np.array_equal(bare[name].view(np.uint32), whole[name].view(np.uint32)), (name, hex(mask))
    features, status = pe.encode(boards, signs, 0x01)
    rows = tower_rows(net, features)
    status[1] = 1   # a status word handed in marks the position as no position
    marked = pe.combine(boards, 0x01, 0, 2, None, rows, status, True)
    assert marked["status"].tolist() == status.tolist() and not marked["policy"][1].any() and (marked["top_cells"][1] == -1).all() and marked["policy"][0].any()
    INVALID, UNSUPPORTED = 1, 3
    pe.combine(boards, 0x01, ref.MASK_FORBIDDEN, 0, None, rows, None, True, expect=INVALID)          # the flag needs the feature rows
    pe.combine(boards, 0x01, 0, 0, None, (rows[0], rows[1], None), None, True, expect=INVALID)      # action values without their rows
    pe.combine(boards, 0x24, ref.MASK_FORBIDDEN, 0, features, rows, None, True, expect=UNSUPPORTED)
    pe.combine(boards, 0x01, 0, 9, None, rows, None, True, expect=INVALID)
    pe.close()


def combine_positions(n):
    rule_cases = json.load(open(os.path.join(GOLDEN, "ref_rules_cases.json")))
    fouls = [embed(c["board"], n) for c in rule_cases if any(ch["kind"] == "forbidden" and ch["expected"] for ch in c["checks"])][:3]
    crafted = crafted_positions(n)
    return [(crafted[0], 1), (crafted[2], 2), (crafted[3], 1)] + [(b, 1) for b in fouls] + [(lds_overflow_boards(n)[1], 1)]


def check_against_restatement(out, n, positions, mask, flags, top_k, rows, features, status=None):
    S = len(ref.symmetries_of(mask))
    policy_rows, value_rows, q_rows = rows
    for p, (board, _) in enumerate(positions):
        want = ref.combine(n, board, mask, flags, top_k, policy_rows[p * S:(p + 1) * S], value_rows[p * S:(p + 1) * S],
                           None if q_rows is None else q_rows[p * S:(p + 1) * S], features[p * S], 0 if status is None else int(status[p]))
        for name in ("policy", "value", "action_values", "top_cells", "top_probs"):
            if want[name] is not None:
                got = np.ascontiguousarray(out[name][p]).reshape(-1).view(np.uint32)
                assert np.array_equal(got, np.ascontiguousarray(want[name]).reshape(-1).view(np.uint32)), (name, p, hex(mask), flags, top_k)


@pytest.mark.parametrize("n,kind", [(15, "pv"), (15, "pvq"), (20, "pv"), (20, "pvq")])
def test_combine_against_the_restatement(agx_lib, nets, monkeypatch, n, kind):
    """encode, then the tower on the returned rows, then the restatement on the tower's rows == evaluate, bit for bit: masks 0x01, 0xFF,
    0x24, every combination of the flags (MASK_FORBIDDEN needs symmetry 0 and is refused without it), top_k 0, 1, 8"""
    monkeypatch.setattr(ref, "image_map", image_map)
    positions = combine_positions(n)
    boards, signs = [b for b, _ in positions], [s for _, s in positions]
    pe = Evaluator(agx_lib, ol.RULES["RENJU"], n, len(positions))
    net = nets(n, kind)
    forbidden_seen = 0
    for mask in (0x01, 0xFF, 0x24):
        features, status = pe.encode(boards, signs, mask)
        rows = tower_rows(net, features)
        assert not status.any() and (rows[2] is not None) == (kind == "pvq")
        for flags in range(4):
            for top_k in (0, 1, 8):
                if (flags & ref.MASK_FORBIDDEN) and not (mask & 1):
                    assert "identity" in pe.evaluate(net, boards, signs, mask, flags, top_k, kind == "pvq", expect=3)
                    continue
                out = pe.evaluate(net, boards, signs, mask, flags, top_k, kind == "pvq")
                assert not out["status"].any()
                check_against_restatement(out, n, positions, mask, flags, top_k, rows, features)
                if flags & ref.RENORMALISE:
                    assert np.abs(out["policy"].sum(axis=1, dtype=np.float64) - 1.0).max() < 1e-5
        if mask & 1:
            forbidden_seen += int(((features[::len(ref.symmetries_of(mask))] >> 6) & 1).sum())
    assert forbidden_seen > 0   # MASK_FORBIDDEN had fouls to mask
    pe.close()


def test_one_symmetry_is_a_relabelling(agx_lib, nets):
    """evaluate(board, 1 << s) == evaluate(board under s, 0x01) mapped back cell by cell: the direction of the inverse map"""
    n = 15
    positions = combine_positions(n)[1:5]
    boards, signs = [b for b, _ in positions], [s for _, s in positions]
    pe = Evaluator(agx_lib, ol.RULES["RENJU"], n, len(positions))
    net = nets(n, "pvq")
    for s in range(8):
        a = pe.evaluate(net, boards, signs, 1 << s, 0, 0, True)
        b = pe.evaluate(net, [ref.transform_board(x, s) for x in boards], signs, 0x01, 0, 0, True)
        image = image_map(s, n)
        assert np.array_equal(a["policy"].view(np.uint32), b["policy"][:, image].view(np.uint32)), s
        assert np.array_equal(a["action_values"].view(np.uint32), b["action_values"][:, image].view(np.uint32)), s
        assert np.array_equal(a["value"].view(np.uint32), b["value"].view(np.uint32)), s
        assert s == 0 or not np.array_equal(a["policy"], b["policy"])
    pe.close()


def test_bad_input_is_reported_and_stays_alone(agx_lib, nets):
    """a cell value of 3 and a sign of 0 in the middle of a batch: non-zero status and zero outputs for those positions, the others as in
    a batch without them"""
    n = 15
    positions = combine_positions(n)[:5]
    boards, signs = [b.copy() for b, _ in positions], [s for _, s in positions]
    pe = Evaluator(agx_lib, ol.RULES["RENJU"], n, 8)
    net = nets(n, "pvq")
    clean = pe.evaluate(net, boards, signs, 0x03, ref.RENORMALISE, 4, True)
    boards[2][7, 7] = 3
    signs[3] = 0
    features, status = pe.encode(boards, signs, 0x03)
    assert status.tolist() == [0, 0, 1, 1, 0] and not features[4:8].any() and features[:4].all() and features[8:].all()
    out = pe.evaluate(net, boards, signs, 0x03, ref.RENORMALISE, 4, True)
    assert out["status"].tolist() == [0, 0, 1, 1, 0]
    for p in range(5):
        for name in ("policy", "value", "action_values", "top_cells", "top_probs"):
            if p in (2, 3):
                assert (out[name][p] == (-1 if name == "top_cells" else 0)).all(), (name, p)
            else:
                assert np.array_equal(out[name][p].view(np.uint32), clean[name][p].view(np.uint32)), (name, p)
    pe.close()


def test_refusals_launch_nothing(agx_lib, nets):
    """every refusal returns its code with a message and leaves the sentinel in every output buffer"""
    INVALID, UNSUPPORTED = 1, 3
    n = 15
    board, pe = np.zeros((n, n), np.uint8), Evaluator(agx_lib, 0, n, 4)
    pv, pvq, other = nets(n, "pv"), nets(n, "pvq"), nets(20, "pv")
    five, one = ([board] * 5, [1] * 5), ([board], [1])
    assert "created for 4" in pe.evaluate(pv, *five, 0x01, 0, 0, False, expect=INVALID)
    assert "mask" in pe.evaluate(pv, *one, 0, 0, 0, False, expect=INVALID)
    assert "mask" in pe.evaluate(pv, *one, 0x100, 0, 0, False, expect=INVALID)
    assert "top_k" in pe.evaluate(pv, *one, 0x01, 0, -1, False, expect=INVALID)
    assert "top_k" in pe.evaluate(pv, *one, 0x01, 0, 9, False, expect=INVALID)
    assert "flags" in pe.evaluate(pv, *one, 0x01, 4, 0, False, expect=INVALID)
    assert "20x20" in pe.evaluate(other, *one, 0x01, 0, 0, False, expect=INVALID)
    assert "head" in pe.evaluate(pv, *one, 0x01, 0, 0, False, expect=INVALID, force_q=True)
    assert "identity" in pe.evaluate(pvq, *one, 0x24, ref.MASK_FORBIDDEN, 0, True, expect=UNSUPPORTED)
    pe.encode(*five, 0x01, expect=INVALID)
    pe.encode(*one, 0, expect=INVALID)
    pe.encode(*one, 0x1FF, expect=INVALID)
    pe.close()
    handle = ctypes.c_void_p()
    assert agx_lib.agx_position_evaluator_create(0, 12, 4, ctypes.byref(handle)) == UNSUPPORTED and not handle.value
    assert agx_lib.agx_position_evaluator_create(7, 15, 4, ctypes.byref(handle)) == INVALID and not handle.value


def test_python_wrapper_with_numpy_arrays(agx_lib, nets):
    """AGNetwork.evaluate_positions: a host round trip, the same bits as the C ABI driven by hand"""
    n = 20
    positions = combine_positions(n)
    boards, signs = np.stack([b for b, _ in positions]), np.array([s for _, s in positions], np.uint8)
    net = nets(n, "pvq")
    got = net.evaluate_positions(boards, signs, ol.RULES["RENJU"], symmetries=0xFF, flags=3, top_k=5)
    pe = Evaluator(agx_lib, ol.RULES["RENJU"], n, len(positions))
    want = pe.evaluate(net, boards, signs, 0xFF, 3, 5, True)
    pe.close()
    assert got["policy"].shape == (len(positions), n, n) and got["action_values"].shape == (len(positions), n, n, 2) and got["top_cells"].dtype == np.int32
    for name, w in want.items():
        assert np.array_equal(got[name].reshape(w.shape).view(np.uint32), w.view(np.uint32)), name
    plain = nets(n, "pv").evaluate_positions(boards.reshape(len(positions), -1), signs, ol.RULES["RENJU"])
    assert sorted(plain) == ["policy", "status", "value"] and not plain["status"].any()


def test_reference_named_entry_point_from_a_compiled_program(agx_lib, olib, nets, tmp_path):
    """ag::AGNetwork::packInputData(index, board, signToMove) + forward + unpackOutput from tests/cpp/position_eval_main.cpp"""
    from alphagomoku_amd import build
    n, rules = 15, ol.RULES["RENJU"]
    positions = combine_positions(n)
    net = nets(n, "pvq")
    _, desc, blob = nets.made[(n, "pvq")]
    (tmp_path / "positions.bin").write_bytes(b"".join(b.tobytes() + bytes([s]) for b, s in positions))
    np.ascontiguousarray(blob, np.float32).tofile(tmp_path / "weights.bin")
    run = subprocess.run([build.POSITION_TEST, str(tmp_path / "positions.bin"), str(tmp_path / "weights.bin"), str(rules), str(n), "ResnetPVQ", str(desc["blocks"]),
                          str(desc["filters"]), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == "same %d" % len(positions) and lines[1].startswith("refused: ") and "no position" in lines[1] and lines[-1] == "ok"
    raw = np.fromfile(tmp_path / "out.bin", dtype=np.uint32)
    words, policy = raw[:len(positions) * n * n].reshape(len(positions), -1), raw[len(positions) * n * n:].reshape(len(positions), -1)
    for p, (board, sign) in enumerate(positions):
        assert np.array_equal(words[p], oracle_rows(olib, rules, n, board, sign, 0x01)[0]), p
    assert np.array_equal(policy, tower_rows(net, words)[0].view(np.uint32))   # unpackOutput hands out the tower's policy as it is


def test_torch_tensors_on_a_torch_stream(agx_lib):
    """AGNetwork.evaluate_positions with device torch tensors on a non-default torch stream.  In a process of its own: torch's HIP runtime
    has to be shared with the library before either touches the GPU."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "position_eval_torch_main.py")
    run = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1].startswith("ok"), run.stdout[-3000:] + run.stderr[-3000:]
