"""Positions solved on the device (csrc/engine.hip: k_solve_positions, agx.h: agx_position_solver_*) against the oracle's threat solver —
ago_solver_solve on a fresh solver per position — on the bits: action count, moves in order, move scores, result score, flags, node
count.  The solver in front of the position evaluator (agx_position_evaluator_evaluate_solved) against its numpy restatement
(tests/position_solve_ref.py) fed the tower's own rows and the solver's own outputs.  Every output lies between two guard zones."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import position_eval_ref as ref
import position_solve_ref as sref
import test_position_eval_gpu as pet

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
TABLE = 1 << 12   # entries per wave: 64 KB to clear per position, and small enough for a 1000-node solve to meet replaced entries
INVALID, UNSUPPORTED = 1, 3
OUT_KINDS = dict(score=np.uint16, flags=np.uint32, n_actions=np.int32, moves=np.uint16, move_scores=np.uint16, nodes=np.uint32, value=np.float32, status=np.int32)
Guarded = pet.Guarded
nets = pet.nets


@pytest.fixture(scope="module")
def olib():
    return ol.load()


# ---------------------------------------------------------------------------------------------------------------- positions
@functools.lru_cache(maxsize=None)
def game_positions(rules, n, skip=16, limit=30):
    """(board, sign to move) before plies skip .. skip + limit of one oracle self-play game from the empty board (20 playouts, batch 4, the
    oracle's stand-in evaluator); on boards too small for that many plies, the first `limit` of the game"""
    if skip + limit > n * n:
        skip = 0
    olib = ol.load()
    hw = n * n
    cfg = ol.default_search_config(max_batch_size=4, max_simulations=20, table_entries=1 << 14)
    h = olib.ago_game_create_ex(rules, n, n, hw, ctypes.byref(cfg))
    olib.ago_game_begin(h, ol.ptr(np.zeros(4, np.uint16)), 0)
    for _ in range(100000):
        if olib.ago_game_outcome(h) != 0 or olib.ago_game_num_records(h) >= skip + limit:
            break
        f = np.zeros((4, hw), np.uint32)
        c = olib.ago_game_step_select(h, ol.ptr(f), 4)
        p, v = np.zeros((4, hw), np.float32), np.zeros((4, 2), np.float32)
        olib.ago_fake_eval(c, hw, ol.ptr(f), ol.ptr(p), ol.ptr(v))
        olib.ago_game_step_expand(h, ol.ptr(p), ol.ptr(v))
    board, out = np.zeros((n, n), np.uint8), []
    for i in range(min(olib.ago_game_num_records(h), skip + limit)):
        mv, rv, rs = ctypes.c_uint16(), ctypes.c_int(), ctypes.c_uint16()
        rval = (ctypes.c_float * 2)()
        em, ev, ep, evl, es = np.zeros(512, np.uint16), np.zeros(512, np.int32), np.zeros(512, np.float32), np.zeros(1024, np.float32), np.zeros(512, np.uint16)
        olib.ago_game_record(h, i, ctypes.byref(mv), ctypes.byref(rv), rval, ctypes.byref(rs), ol.ptr(em), ol.ptr(ev), ol.ptr(ep), ol.ptr(evl), ol.ptr(es), 512)
        m = ol.short_to_move(mv.value)
        out.append((board.copy(), m["sign"]))
        board[m["row"], m["col"]] = m["sign"]
    olib.ago_game_destroy(h)
    return out[skip:]


def clustered(n, count=12):
    """boards of 6 .. 40 stones placed in a random walk of short steps (as tests/test_engine_gpu.py makes them): threats of both sides close
    together, a few of them won or lost within the node budget"""
    rng, out = np.random.default_rng(100 + n), []
    for _ in range(count):
        b = np.zeros((n, n), np.uint8)
        r = c = n // 2
        for k in range(int(rng.integers(6, 41))):
            for _ in range(100):
                rr, cc = r + int(rng.integers(-2, 3)), c + int(rng.integers(-2, 3))
                if 0 <= rr < n and 0 <= cc < n and b[rr, cc] == 0:
                    b[rr, cc] = 1 + (k & 1)
                    r, c = rr, cc
                    break
        out.append((b, 1 if int((b != 0).sum()) % 2 == 0 else 2))
    return out


def crafted(n):
    """name -> (board, sign to move).  The small boards (below 9x9) get the ones that fit."""
    out = {}
    empty = np.zeros((n, n), np.uint8)
    out["empty"] = (empty, 1)
    corner = empty.copy()
    corner[0, 0] = 1
    out["corner"] = (corner, 2)
    four = empty.copy()
    c0 = 1 if n >= 6 else 0
    four[n // 2, c0:c0 + 4] = 1          # an open four (on 5x5: a four with one end at the edge): cross wins in one
    four[0, 0:3] = 2
    four[n - 1, n - 1] = 2
    out["open_four"] = (four, 1)
    out["open_four_other"] = (four, 2)    # ... and circle, to move, has lost
    full = pet.crafted_positions(n)[3]    # full but for one cell
    out["full_but_one"] = (full, 1)
    if n >= 9:
        fork = empty.copy()
        fork[4, 1:4] = 1                  # (4, 4) makes a four in row 4 and a three in column 4
        fork[2:4, 4] = 1
        for r, c in ((n - 1, n - 1), (n - 1, n - 3), (n - 3, n - 1), (n - 3, n - 4), (n - 2, 0)):
            fork[r, c] = 2
        out["four_three"] = (fork, 1)
        out["four_three_other"] = (fork, 2)   # the same for the opponent: circle must defend
        double = empty.copy()
        double[4, 2:4] = 1                # (4, 4) makes two open threes: forbidden for cross under renju
        double[2:4, 4] = 1
        for r, c in ((n - 1, n - 1), (n - 1, n - 3), (n - 3, n - 1), (n - 3, n - 4)):
            double[r, c] = 2
        out["double_three"] = (double, 1)
    return out


def case_positions(rules, n):
    return list(game_positions(rules, n)) + (clustered(n) if n >= 9 else []) + list(crafted(n).values())


@functools.lru_cache(maxsize=None)
def oracle_results(rules, n, budget, table=TABLE):
    olib = ol.load()
    return [sref.oracle_solve(olib, rules, n, b, s, budget, table, SEED) for b, s in case_positions(rules, n)]


# ---------------------------------------------------------------------------------------------------------------- the C ABI by hand
class Solver:
    """agx_position_solver_* driven through ctypes with guarded buffers"""

    def __init__(self, lib, rules, n, capacity, budget, table=TABLE):
        from alphagomoku_amd import check
        self.lib, self.n, self.hw, self.capacity = lib, n, n * n, capacity
        self.handle = ctypes.c_void_p()
        check(lib.agx_position_solver_create(rules, n, capacity, budget, table, SEED, ctypes.byref(self.handle)))
        waves, per_wave, total = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.agx_position_solver_info(self.handle, ctypes.byref(waves), ctypes.byref(per_wave), ctypes.byref(total)))
        self.waves, self.bytes_per_wave, self.device_bytes = waves.value, per_wave.value, total.value

    def shapes(self, count):
        return dict(score=(count,), flags=(count,), n_actions=(count,), moves=(count, self.hw), move_scores=(count, self.hw), nodes=(count,), value=(count, 3),
                    status=(count,))

    def upload(self, boards, signs):
        from alphagomoku_amd.networks import DeviceBuffer
        b = np.ascontiguousarray(np.asarray(boards, np.uint8).reshape(len(signs), self.hw))
        s = np.ascontiguousarray(np.asarray(signs, np.uint8))
        d_b, d_s = DeviceBuffer(max(b.nbytes, 16)), DeviceBuffer(max(s.nbytes, 16))
        d_b.upload(b)
        d_s.upload(s)
        return d_b, d_s

    def solve(self, positions, names=None, expect=0, count=None):
        """-> dict of arrays; `names`: the outputs asked for (the others are passed as NULL); with `expect` != 0 the code of a refused call"""
        from alphagomoku_amd import check, _lib
        boards, signs = [b for b, _ in positions], [s for _, s in positions]
        size = len(signs)
        shapes = self.shapes(size)
        d_b, d_s = self.upload(boards, signs)
        bufs = {k: Guarded(int(np.prod(shapes[k])), OUT_KINDS[k]) for k in (names if names is not None else shapes)}
        c_out = _lib.AgxSolvedPositions()
        for k, g in bufs.items():
            setattr(c_out, k, g.ptr)
        code = self.lib.agx_position_solver_solve(self.handle, size if count is None else count, d_b.ptr, d_s.ptr, ctypes.byref(c_out), None)
        check(self.lib.agx_device_synchronize())
        d_b.free()
        d_s.free()
        if expect:
            message = self.lib.agx_last_error().decode()
            assert code == expect and all(g.untouched() for g in bufs.values()) and message, (code, message)
            return message
        check(code)
        return {k: g.take(shapes[k], k) for k, g in bufs.items()}

    def close(self):
        self.lib.agx_position_solver_destroy(self.handle)


def assert_equals_oracle(out, p, want, what):
    k = want["n_actions"]
    assert out["status"][p] == 0, what
    assert out["n_actions"][p] == k, (what, int(out["n_actions"][p]), k)
    assert np.array_equal(out["moves"][p, :k], want["moves"]), what                  # the same actions in the same ORDER
    assert np.array_equal(out["move_scores"][p, :k], want["move_scores"]), what
    assert not out["moves"][p, k:].any() and not out["move_scores"][p, k:].any(), what
    assert out["score"][p] == want["score"], (what, int(out["score"][p]), want["score"])
    assert out["nodes"][p] == want["nodes"], (what, int(out["nodes"][p]), want["nodes"])  # AlphaBetaSearch::solve's return value
    assert out["flags"][p] == sref.expected_flags(want), (what, int(out["flags"][p]), sref.expected_flags(want))
    assert np.array_equal(out["value"][p], sref.score_value(want["score"])), what


def same_position_result(a, p, b, q, what):
    for name in OUT_KINDS:
        assert np.array_equal(np.ascontiguousarray(a[name][p]).reshape(-1).view(np.uint8), np.ascontiguousarray(b[name][q]).reshape(-1).view(np.uint8)), (what, name, p, q)


CASES = [(0, 15), (1, 15), (2, 15), (3, 15), (4, 15), (0, 20), (3, 20), (0, 9), (0, 5)]


@pytest.mark.parametrize("rules,n,budget", [(r, n, b) for r, n in CASES for b in (1, 100)] + [(0, 15, 1000), (2, 15, 1000)])
def test_solver_matches_the_oracle_per_position(agx_lib, rules, n, budget):
    """all five rule sets on 15x15, freestyle and caro5 on 20x20, freestyle on 9x9 and 5x5 (the run-time-sized kernel); positions of an
    oracle self-play game and the crafted boards; node budgets 1, 100 and (15x15 freestyle and renju) 1000"""
    positions = case_positions(rules, n)
    want = oracle_results(rules, n, budget)
    solver = Solver(agx_lib, rules, n, len(positions), budget)
    out = solver.solve(positions)
    solver.close()
    for p in range(len(positions)):
        assert_equals_oracle(out, p, want[p], (rules, n, budget, p))
    names = list(crafted(n))
    by_name = {k: want[len(positions) - len(names) + i] for i, k in enumerate(names)}
    assert (by_name["open_four"]["score"] >> 13) & 3 == 3   # a proven win
    if n >= 9:
        assert (by_name["open_four_other"]["score"] >> 13) & 3 == 0 and by_name["four_three_other"]["must_defend"]   # a proven loss; a forced defence
    if budget >= 100 and n >= 9:
        assert sum(sref.is_proven(w["score"]) for w in want) > 3 and sum(w["nodes"] > 1 for w in want) > 3
        assert any(not sref.is_proven(w["score"]) for w in want)


@functools.lru_cache(maxsize=None)
def geometry_kinds():
    positions = case_positions(0, 15)
    want = oracle_results(0, 15, 100)
    pick = [0, 7, 19, 29, 33, 38] + list(range(len(positions) - 8, len(positions)))
    return [positions[i] for i in pick], [want[i] for i in pick]


@pytest.mark.parametrize("size", [1, 63, 64, 65])
def test_batch_geometry(agx_lib, size):
    """n = 1, 63, 64, 65: every position equals the oracle's result wherever it stands in the batch; the guard zones survive (Guarded.take)"""
    kinds, want = geometry_kinds()
    which = [(5 * p + p // len(kinds)) % len(kinds) for p in range(size)]
    solver = Solver(agx_lib, 0, 15, 65, 100)
    out = solver.solve([kinds[k] for k in which])
    assert solver.device_bytes >= solver.waves * solver.bytes_per_wave > 0
    solver.close()
    for p, k in enumerate(which):
        assert_equals_oracle(out, p, want[k], (size, p, k))


def test_more_positions_than_waves(agx_lib, monkeypatch):
    """AGX_POSSOLVE_MAX_WAVES=3 and 10 positions: every wave takes three or four turns of the grid-stride loop"""
    monkeypatch.setenv("AGX_POSSOLVE_MAX_WAVES", "3")
    kinds, want = geometry_kinds()
    solver = Solver(agx_lib, 0, 15, 10, 100)
    assert solver.waves == 3
    out = solver.solve(kinds[:10])
    solver.close()
    for p in range(10):
        assert_equals_oracle(out, p, want[p], p)


def table_sensitive_pair(rules, n, budget):
    """(A, B) among the case's positions such that the oracle, solving A on the table B's solve left behind, reports another node count for
    A than on an empty table — found on the CPU.  15x15 freestyle, budget 100, table of 4096 entries: A = position 3 and B = position 2
    of the case (plies 19 and 18 of the self-play game; B is A's predecessor: its solve leaves entries for positions A's solve meets again)."""
    olib = ol.load()
    positions, fresh = case_positions(rules, n), oracle_results(rules, n, budget)
    for a in range(1, len(positions)):
        b = a - 1
        if fresh[a]["nodes"] < 5:
            continue
        handle = olib.ago_solver_create(rules, n, n, TABLE, SEED, budget)
        sref.oracle_solve(olib, rules, n, *positions[b], budget, TABLE, SEED, keep=handle)
        again = sref.oracle_solve(olib, rules, n, *positions[a], budget, TABLE, SEED, keep=handle)
        olib.ago_solver_destroy(handle)
        if again["nodes"] != fresh[a]["nodes"]:
            return a, b
    raise AssertionError("no pair of positions whose solves interact through the table")


def test_results_do_not_depend_on_the_batch(agx_lib, monkeypatch):
    """a batch, its reverse and a shuffle give identical per-position results; with ONE wave the batch [A, B, A] reports A twice alike —
    which fails unless the table is cleared between positions, A and B being chosen so that B's leftover table changes A's solve"""
    positions, want = case_positions(0, 15), oracle_results(0, 15, 100)
    size = len(positions)
    solver = Solver(agx_lib, 0, 15, size, 100)
    forward = solver.solve(positions)
    backward = solver.solve(positions[::-1])
    order = np.random.default_rng(5).permutation(size)
    shuffled = solver.solve([positions[i] for i in order])
    solver.close()
    for p in range(size):
        same_position_result(forward, p, backward, size - 1 - p, "reverse")
        same_position_result(forward, int(order[p]), shuffled, p, "shuffle")
    a, b = table_sensitive_pair(0, 15, 100)
    assert (a, b) == (A_POSITION, B_POSITION)
    monkeypatch.setenv("AGX_POSSOLVE_MAX_WAVES", "1")
    solver = Solver(agx_lib, 0, 15, 3, 100)
    assert solver.waves == 1
    out = solver.solve([positions[a], positions[b], positions[a]])
    solver.close()
    same_position_result(out, 0, out, 2, "A, B, A")
    assert_equals_oracle(out, 0, want[a], "A")
    assert_equals_oracle(out, 1, want[b], "B")
    assert_equals_oracle(out, 2, want[a], "A again")


A_POSITION, B_POSITION = 3, 2   # table_sensitive_pair(0, 15, 100)


def test_bad_input_is_reported_and_stays_alone(agx_lib):
    """a cell value of 3 and a sign of 0 in the middle of a batch: status 1 and zeroed outputs for those, the others bit-equal to a run
    without the bad rows"""
    positions = [(b.copy(), s) for b, s in geometry_kinds()[0][:6]]
    solver = Solver(agx_lib, 0, 15, 8, 100)
    clean = solver.solve(positions)
    dirty = list(positions)
    dirty[2][0][7, 7] = 3
    dirty[3] = (dirty[3][0], 0)
    out = solver.solve(dirty)
    without = solver.solve([dirty[i] for i in (0, 1, 4, 5)])
    solver.close()
    assert out["status"].tolist() == [0, 0, 1, 1, 0, 0]
    for p in (2, 3):
        for name in OUT_KINDS:
            assert name == "status" or not np.asarray(out[name][p]).any(), (name, p)
    for q, p in enumerate((0, 1, 4, 5)):
        same_position_result(out, p, clean, p, "neighbour")
        same_position_result(out, p, without, q, "without the bad rows")


def test_null_outputs_and_refusals(agx_lib):
    """any output pointer may be NULL; every refusal returns its code with a message and leaves the sentinel in every output buffer"""
    positions = geometry_kinds()[0][:5]
    solver = Solver(agx_lib, 0, 15, 5, 100)
    whole = solver.solve(positions)
    for names in (["score"], ["moves", "nodes"], ["value", "status", "n_actions"], []):
        part = solver.solve(positions, names=names)
        for name in names:
            assert np.array_equal(part[name], whole[name]), name
    assert solver.solve(positions[:0])["score"].shape == (0,)
    assert "created for 5" in solver.solve(positions + positions[:1], expect=INVALID)
    assert "positions" in solver.solve(positions, expect=INVALID, count=-1)
    from alphagomoku_amd import _lib
    c_out = _lib.AgxSolvedPositions()
    d_b, d_s = solver.upload([b for b, _ in positions], [s for _, s in positions])
    assert agx_lib.agx_position_solver_solve(solver.handle, 5, None, d_s.ptr, ctypes.byref(c_out), None) == INVALID
    assert agx_lib.agx_position_solver_solve(solver.handle, 5, d_b.ptr, None, ctypes.byref(c_out), None) == INVALID
    assert agx_lib.agx_position_solver_solve(solver.handle, 5, d_b.ptr, d_s.ptr, None, None) == INVALID
    assert agx_lib.agx_position_solver_solve(None, 5, d_b.ptr, d_s.ptr, ctypes.byref(c_out), None) == INVALID
    d_b.free()
    d_s.free()
    solver.close()
    handle = ctypes.c_void_p()
    for args, code in (((0, 4, 4, 100, TABLE), UNSUPPORTED), ((0, 21, 4, 100, TABLE), UNSUPPORTED), ((0, 15, 4, 0, TABLE), UNSUPPORTED),
                       ((0, 15, 4, 1001, TABLE), UNSUPPORTED), ((5, 15, 4, 100, TABLE), INVALID), ((0, 15, 0, 100, TABLE), INVALID),
                       ((0, 15, 4, 100, (1 << 32) + 1), INVALID)):
        assert agx_lib.agx_position_solver_create(*args, SEED, ctypes.byref(handle)) == code and not handle.value, args


def test_calls_on_two_streams_are_ordered_on_the_device(agx_lib, monkeypatch):
    """calls on one solver share its per-wave areas: with ONE wave, a solve enqueued on a second stream right behind a solve on a first
    one runs on the same table, stack and task — both must still equal the oracle (agx_position_solver_solve orders the second behind
    the first with an event, nothing waits on the host in between)"""
    from alphagomoku_amd import check, _lib
    monkeypatch.setenv("AGX_POSSOLVE_MAX_WAVES", "1")
    positions, want = case_positions(0, 15), oracle_results(0, 15, 1000)
    first, second = list(range(0, 12)), list(range(12, 24))
    solver = Solver(agx_lib, 0, 15, 12, 1000)
    assert solver.waves == 1
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for st in streams:
        check(agx_lib.agx_stream_create(ctypes.byref(st)))

    def enqueue(which, stream):
        d_b, d_s = solver.upload([positions[i][0] for i in which], [positions[i][1] for i in which])
        shapes = solver.shapes(len(which))
        bufs = {k: Guarded(int(np.prod(shapes[k])), OUT_KINDS[k]) for k in shapes}
        c_out = _lib.AgxSolvedPositions()
        for k, g in bufs.items():
            setattr(c_out, k, g.ptr)
        check(agx_lib.agx_position_solver_solve(solver.handle, len(which), d_b.ptr, d_s.ptr, ctypes.byref(c_out), stream))
        return bufs, shapes, (d_b, d_s)

    a = enqueue(first, streams[0])
    b = enqueue(second, streams[1])
    c = enqueue(first, streams[0])
    check(agx_lib.agx_device_synchronize())
    for (bufs, shapes, staged), which in ((a, first), (b, second), (c, first)):
        out = {k: g.take(shapes[k], k) for k, g in bufs.items()}
        for p, i in enumerate(which):
            assert_equals_oracle(out, p, want[i], (which[0], p))
        for buf in staged:
            buf.free()
    assert sum(want[i]["nodes"] for i in first + second) > 5000   # solves long enough to overlap if nothing ordered them
    solver.close()
    for st in streams:
        check(agx_lib.agx_stream_destroy(st))


# ---------------------------------------------------------------------------------------------------------------- evaluate_solved
def evaluate_solved(lib, pe, solver, net, positions, mask, flags, top_k, with_q, want_solved=True, expect=0):
    from alphagomoku_amd import check, _lib
    boards, signs = [b for b, _ in positions], [s for _, s in positions]
    size, hw = len(signs), pe.hw
    d_b, d_s = pe.upload(boards, signs)
    shapes = dict(policy=(size, hw), value=(size, 3), action_values=(size, hw, 2), top_cells=(size, top_k), top_probs=(size, top_k), status=(size,))
    bufs = {k: Guarded(int(np.prod(shapes[k])), pet.OUT_KINDS[k]) for k in shapes if with_q or k != "action_values"}
    c_out, c_solved = _lib.AgxPositionOutputs(), _lib.AgxSolvedPositions()
    for k, g in bufs.items():
        setattr(c_out, k, g.ptr)
    solved_shapes = solver.shapes(size)
    solved_bufs = {k: Guarded(int(np.prod(solved_shapes[k])), OUT_KINDS[k]) for k in solved_shapes} if want_solved else {}
    for k, g in solved_bufs.items():
        setattr(c_solved, k, g.ptr)
    code = lib.agx_position_evaluator_evaluate_solved(pe.handle, solver.handle, net._net, size, d_b.ptr, d_s.ptr, mask, flags, top_k, ctypes.byref(c_out),
                                                      ctypes.byref(c_solved) if want_solved else None, None)
    check(lib.agx_device_synchronize())
    d_b.free()
    d_s.free()
    if expect:
        message = lib.agx_last_error().decode()
        assert code == expect and all(g.untouched() for g in list(bufs.values()) + list(solved_bufs.values())) and message, (code, message)
        return message
    check(code)
    return {k: g.take(shapes[k], k) for k, g in bufs.items()}, {k: g.take(solved_shapes[k], k) for k, g in solved_bufs.items()}


def solved_positions(n):
    """a proven position, a must-defend position, quiet ones, a renju double three, a lost one — and one that is no position"""
    c = crafted(n)
    bad = c["corner"][0].copy()
    bad[3, 3] = 3
    return [c[k] for k in ("open_four", "four_three_other", "corner", "empty", "double_three", "open_four_other", "four_three", "full_but_one")] + [(bad, 1)] \
        + list(game_positions(2, n)[10:14])


@pytest.mark.parametrize("n,kind", [(15, "pv"), (15, "pvq"), (20, "pv"), (20, "pvq")])
def test_evaluate_solved_against_the_restatement(agx_lib, nets, monkeypatch, n, kind):
    """solve, encode, tower, combine in one call == the restatement on the tower's own rows and the solver's own outputs, bit for bit:
    masks 0x01 and 0xFF, with and without RENORMALISE (and MASK_FORBIDDEN: renju), top_k 0, 1, 8, a 'pv' and a 'pvq' network of 1x64"""
    monkeypatch.setattr(ref, "image_map", pet.image_map)
    rules, with_q = ol.RULES["RENJU"], kind == "pvq"
    positions = solved_positions(n)
    size = len(positions)
    pe = pet.Evaluator(agx_lib, rules, n, size)
    solver = Solver(agx_lib, rules, n, size, 100)
    net = nets(n, kind)
    alone = solver.solve(positions)
    assert alone["status"].tolist() == [0] * 8 + [1] + [0] * 4
    proven = [sref.is_proven(s) for s in alone["score"]]
    assert proven[0] and proven[5] and (alone["flags"][1] & 1) and not proven[2] and not proven[3]   # proven, must defend, quiet
    for mask in (0x01, 0xFF):
        S = len(ref.symmetries_of(mask))
        features, status = pe.encode([b for b, _ in positions], [s for _, s in positions], mask)
        rows = pet.tower_rows(net, features)
        for flags in (0, ref.RENORMALISE, ref.RENORMALISE | ref.MASK_FORBIDDEN):
            for top_k in (0, 1, 8):
                out, solved = evaluate_solved(agx_lib, pe, solver, net, positions, mask, flags, top_k, with_q)
                for name in OUT_KINDS:
                    assert np.array_equal(solved[name], alone[name]), name      # the solver's own outputs, as from agx_position_solver_solve
                for p, (board, _) in enumerate(positions):
                    k = int(solved["n_actions"][p])
                    want = sref.combine_solved(n, board, mask, flags, top_k, rows[0][p * S:(p + 1) * S], rows[1][p * S:(p + 1) * S],
                                               None if rows[2] is None else rows[2][p * S:(p + 1) * S], features[p * S], int(solved["score"][p]),
                                               solved["moves"][p, :k], solved["move_scores"][p, :k], int(status[p]), int(solved["status"][p]))
                    assert out["status"][p] == want["status"], p
                    for name in ("policy", "value", "action_values", "top_cells", "top_probs"):
                        if want[name] is not None:
                            got = np.ascontiguousarray(out[name][p]).reshape(-1).view(np.uint32)
                            assert np.array_equal(got, np.ascontiguousarray(want[name]).reshape(-1).view(np.uint32)), (name, p, hex(mask), flags, top_k)
                    if not proven[p] and status[p] == 0:
                        cells = [sref.move_cell(m, n) for m in solved["moves"][p, :k]]
                        assert not np.delete(out["policy"][p], cells).any()         # nothing outside the action list
                    if proven[p]:
                        assert out["value"][p].tolist() == sref.score_value(solved["score"][p]).tolist() and (k == 0 or abs(float(out["policy"][p].sum()) - 1) < 1e-6)
    # without room for the solver's outputs the combine launch reads them from the solver's workspace
    out, solved = evaluate_solved(agx_lib, pe, solver, net, positions, 0xFF, ref.RENORMALISE, 8, with_q)
    bare, _ = evaluate_solved(agx_lib, pe, solver, net, positions, 0xFF, ref.RENORMALISE, 8, with_q, want_solved=False)
    for name in out:
        assert np.array_equal(out[name].view(np.uint32), bare[name].view(np.uint32)), name
    pe.close()
    solver.close()


def test_evaluate_solved_refusals(agx_lib, nets):
    n = 15
    positions = [crafted(n)["corner"]] * 3
    pe = pet.Evaluator(agx_lib, 0, n, 4)
    net = nets(n, "pv")
    small, other_rules, other_board = Solver(agx_lib, 0, n, 2, 100), Solver(agx_lib, 2, n, 4, 100), Solver(agx_lib, 0, 20, 4, 100)
    assert "created for 2" in evaluate_solved(agx_lib, pe, small, net, positions, 0x01, 0, 0, False, expect=INVALID)
    assert "rules" in evaluate_solved(agx_lib, pe, other_rules, net, positions, 0x01, 0, 0, False, expect=INVALID)
    assert "20x20" in evaluate_solved(agx_lib, pe, other_board, net, positions, 0x01, 0, 0, False, expect=INVALID)
    good = Solver(agx_lib, 0, n, 4, 100)
    assert "top_k" in evaluate_solved(agx_lib, pe, good, net, positions, 0x01, 0, 9, False, expect=INVALID)
    assert "mask" in evaluate_solved(agx_lib, pe, good, net, positions, 0, 0, 0, False, expect=INVALID)
    assert "created for 4" in evaluate_solved(agx_lib, pe, good, net, positions * 2, 0x01, 0, 0, False, expect=INVALID)
    for s in (small, other_rules, other_board, good):
        s.close()
    pe.close()


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_python_wrapper_with_numpy_arrays(agx_lib, nets):
    """solver.PositionSolver.solve and AGNetwork.evaluate_positions(solver=...): a host round trip, the same bits as the C ABI driven by hand"""
    from alphagomoku_amd.solver import PositionSolver
    n, rules = 15, ol.RULES["RENJU"]
    positions = solved_positions(n)
    boards, signs = np.stack([b for b, _ in positions]), np.array([s for _, s in positions], np.uint8)
    wrapper = PositionSolver(rules, n, len(positions), max_positions=100, table_entries=TABLE, zobrist_seed=SEED)
    assert wrapper.waves == len(positions) and wrapper.device_bytes >= wrapper.waves * wrapper.bytes_per_wave
    got = wrapper.solve(boards, signs)
    by_hand = Solver(agx_lib, rules, n, len(positions), 100)
    want = by_hand.solve(positions)
    for name in OUT_KINDS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    net = nets(n, "pvq")
    full = net.evaluate_positions(boards, signs, rules, symmetries=0xFF, flags=3, top_k=5, solver=wrapper)
    pe = pet.Evaluator(agx_lib, rules, n, len(positions))
    out, solved = evaluate_solved(agx_lib, pe, by_hand, net, positions, 0xFF, 3, 5, True)
    for name, w in out.items():
        assert np.array_equal(full[name].reshape(w.shape).view(np.uint32), w.view(np.uint32)), name
    for name, w in solved.items():
        assert np.array_equal(full["solved"][name], w), name
    plain = net.evaluate_positions(boards, signs, rules, symmetries=0xFF, flags=3, top_k=5)
    assert "solved" not in plain and not np.array_equal(plain["policy"], full["policy"])
    pe.close()
    by_hand.close()
    wrapper.close()


def test_torch_tensors_on_a_torch_stream(agx_lib):
    """PositionSolver.solve and evaluate_positions(solver=...) with device torch tensors on a non-default torch stream.  In a process of its
    own: torch's HIP runtime has to be shared with the library before either touches the GPU."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "position_solve_torch_main.py")
    run = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1].startswith("ok"), run.stdout[-3000:] + run.stderr[-3000:]
