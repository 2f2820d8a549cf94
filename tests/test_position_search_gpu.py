"""Positions searched on the device (csrc/engine.hip: k_load_positions / k_harvest_positions; agx.h: agx_position_searcher_*) against the
oracle: every position is what a fresh oracle game finds for its first move after an "opening" that is the position's move list
(ago_game_begin -> select / evaluate / expand until the move rule fires -> record 0), bit for bit.  Both sides are fed by the stand-in
evaluator independently, the device through the staged calls and provide().  The dense per-cell rows are held against
tests/position_search_ref.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import position_search_ref as pref
from test_engine_gpu import _oracle_root, _stand_in_evaluator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMS, BATCH, TABLE = 70, 4, 1 << 14
OUTPUT_NAMES = ["status", "root", "root_value", "best_move", "visits", "prior", "q", "score", "edge_index", "pv", "pv_length", "info"]


@pytest.fixture(scope="module")
def olib():
    return ol.load()


# ---- positions, every one a move list that ends with a stone of the colour that is NOT to move --------------------------------------
def mv(sign, row, col):
    return sign | (row << 2) | (col << 9)


def interleave(cross, circle):
    """cross first, colours alternating; len(cross) - len(circle) in (0, 1)"""
    assert len(cross) - len(circle) in (0, 1)
    out = []
    for i, c in enumerate(cross):
        out.append(mv(1, *c))
        if i < len(circle):
            out.append(mv(2, *circle[i]))
    return out


CORNERS = [(0, 0), (0, 8), (8, 0), (8, 8), (4, 8), (8, 4)]   # lone stones, inside a 9x9 corner of any board


def open_four():
    """cross to move with an open four: the root is proven by the first step"""
    return interleave([(4, 2), (4, 3), (4, 4), (4, 5)], CORNERS[:4])


def four_three_against():
    """circle holds a four (one end blocked) and an open three on another line, cross is to move and loses"""
    return interleave([(2, 1)] + CORNERS, [(2, 2), (2, 3), (2, 4), (2, 5), (6, 3), (6, 4), (6, 5)])


def forced_defence():
    """circle holds a four with one end open and nothing else: cross has one move"""
    return interleave([(2, 1)] + CORNERS[:3], [(2, 2), (2, 3), (2, 4), (2, 5)])


def full_but_one(n):
    """every cell but one taken and no line longer than two: colour by (col + 2 row) mod 4"""
    cross = [(r, c) for r in range(n) for c in range(n) if (c + 2 * r) % 4 < 2]
    circle = [(r, c) for r in range(n) for c in range(n) if (c + 2 * r) % 4 >= 2]
    if len(cross) > len(circle):
        cross = cross[:-1]
    else:
        circle = circle[:-1]
    return interleave(cross, circle)


def oracle_game_moves(olib, rules, n, seed, sims=20):
    """the moves of one oracle self-play game, opening included (a cheap search: the game is only a source of positions)"""
    ocfg = ol.default_search_config(max_batch_size=BATCH, max_simulations=sims, table_entries=1 << 12)
    op = np.zeros(256, np.uint16)
    k = olib.ago_prepare_opening(rules, n, n, seed, ol.ptr(op))
    h = olib.ago_game_create_ex(rules, n, n, 0, ctypes.byref(ocfg))
    olib.ago_game_begin(h, ol.ptr(op), k)
    ev = _stand_in_evaluator(olib, n * n)
    moves = [int(x) for x in op[:k]]
    while olib.ago_game_outcome(h) == 0:
        f = np.zeros((BATCH, n * n), np.uint32)
        c = olib.ago_game_step_select(h, ol.ptr(f), BATCH)
        p, v = ev(f[:c])
        olib.ago_game_step_expand(h, ol.ptr(np.ascontiguousarray(p)), ol.ptr(np.ascontiguousarray(v)))
    for i in range(olib.ago_game_num_records(h)):
        moves.append(_oracle_record(olib, h, i)["move"])
    olib.ago_game_destroy(h)
    return k, moves


def positions_for(olib, rules, n):
    """the move lists of a case: prefixes of an oracle game every few plies, the empty board, the crafted boards"""
    k, game = oracle_game_moves(olib, rules, n, 2 if n == 20 else 1)
    if n == 15:
        assert len(game) >= 219
        cuts = [k + 5 * i for i in range(14)] + [100, 150, 200, len(game) - 1]
        assert max(c for c in cuts if c < 100) >= 70
        lists = [game[:c] for c in cuts] + [[], open_four(), four_three_against(), forced_defence(), full_but_one(n)]
        lists.append(oracle_game_moves(olib, rules, n, 3)[1][:40])
        assert len(lists) == 24
    elif n == 20:
        assert len(game) >= 300
        lists = [game[:c] for c in (k, 30, 60, 90, 135, 250)] + [[], open_four(), full_but_one(n)]
    else:
        lists = [game[:c] for c in (k, 12, 20, 30, 45, 60, len(game) - 1)] + [[], open_four(), four_three_against(), forced_defence(), full_but_one(n)]
    for m in lists:
        assert len({pref.move_cell(x, n) for x in m}) == len(m)
    return lists


def boards_and_signs(lists, n):
    boards = np.stack([pref.board_of(m, n) for m in lists]) if lists else np.zeros((0, n * n), np.uint8)
    signs = np.array([1 if not m else 3 - (m[-1] & 3) for m in lists], np.uint8)
    return boards, signs


# ---- the oracle's answer for a position -------------------------------------------------------------------------------------------------
def _oracle_record(olib, h, i):
    move, rv, rs = ctypes.c_uint16(), ctypes.c_int(), ctypes.c_uint16()
    rval = (ctypes.c_float * 2)()
    em, ev, ep, evl, es = np.zeros(512, np.uint16), np.zeros(512, np.int32), np.zeros(512, np.float32), np.zeros(1024, np.float32), np.zeros(512, np.uint16)
    n = olib.ago_game_record(h, i, ctypes.byref(move), ctypes.byref(rv), rval, ctypes.byref(rs), ol.ptr(em), ol.ptr(ev), ol.ptr(ep), ol.ptr(evl), ol.ptr(es), 512)
    assert n >= 0
    edges = [dict(move=int(em[j]), visits=int(ev[j]), prior=np.float32(ep[j]), win=np.float32(evl[2 * j]), draw=np.float32(evl[2 * j + 1]), score=int(es[j]))
             for j in range(n)]
    return dict(move=move.value, visits=rv.value, win=np.float32(rval[0]), draw=np.float32(rval[1]), score=rs.value, edges=edges)


def q_evaluator(base, hw):
    """test_engine_gpu.test_whole_games_with_action_values' stand-in for a 'pvq' network"""
    def evaluator(feats):
        pol, val = base(feats)
        h = (np.ascontiguousarray(feats, dtype=np.uint32).astype(np.uint64) * np.uint64(2654435761) + np.arange(hw, dtype=np.uint64) * np.uint64(40503)) % np.uint64(1 << 20)
        w = (h.astype(np.float32) / np.float32(1 << 20)) * np.float32(0.8)
        d = (np.float32(1.0) - w) * np.float32(0.25)
        return pol, val, np.stack([w, d], axis=2).astype(np.float32)
    return evaluator


def oracle_search(olib, rules, n, moves, serial, evaluator, opts, max_steps=None):
    """record 0 of a fresh game begun on `moves` (with max_steps: the root after that many steps, unless the move rule fired before)"""
    ocfg = ol.default_search_config(max_batch_size=opts.get("max_batch_size", BATCH), max_simulations=opts.get("max_simulations", SIMS), table_entries=TABLE,
                                    final_selector=opts.get("final_selector", 0), use_symmetries=opts.get("use_symmetries", 0),
                                    noise_type=opts.get("noise_type", 0) if opts.get("noise_weight", 0.0) > 0 else 0, noise_weight=opts.get("noise_weight", 0.0))
    batch = ocfg.max_batch_size
    h = olib.ago_game_create_ex(rules, n, n, 0, ctypes.byref(ocfg))
    olib.ago_game_set_serial(h, serial)
    olib.ago_game_begin(h, ol.ptr(np.array(list(moves) + [0], np.uint16)), len(moves))
    steps, moved = 0, 0
    while not moved and (max_steps is None or steps < max_steps):
        f = np.zeros((batch, n * n), np.uint32)
        c = olib.ago_game_step_select(h, ol.ptr(f), batch)
        out = evaluator(f[:c])
        if opts.get("action_values"):
            moved = olib.ago_game_step_expand_q(h, ol.ptr(np.ascontiguousarray(out[0])), ol.ptr(np.ascontiguousarray(out[1])), ol.ptr(np.ascontiguousarray(out[2])))
        else:
            moved = olib.ago_game_step_expand(h, ol.ptr(np.ascontiguousarray(out[0])), ol.ptr(np.ascontiguousarray(out[1])))
        steps += 1
        assert steps < 10000
    if moved:
        want = _oracle_record(olib, h, 0)
        want["flags"] = olib.ago_game_record_flags(h, 0)
    else:
        r = _oracle_root(olib, h)
        want = dict(move=None, flags=None, visits=r["visits"] if r["n"] else 0, win=r["win"], draw=r["draw"], score=r["score"],
                    edges=[dict(move=int(r["moves"][j]), visits=int(r["ev"][j]), prior=r["prior"][j], win=r["val"][2 * j], draw=r["val"][2 * j + 1], score=int(r["es"][j]))
                           for j in range(r["n"])])
    want["moved"], want["steps"] = bool(moved), steps
    olib.ago_game_destroy(h)
    return want


# ---- the device side ---------------------------------------------------------------------------------------------------------------------
def make_searcher(rules, n, slots, **opts):
    from alphagomoku_amd import search
    base = dict(rules=rules, board_size=n, draw_after=n * n, n_games=slots, max_batch_size=BATCH, max_simulations=SIMS, tss_table_entries=TABLE, tss_max_positions=100,
                node_capacity=4096, edge_capacity=65536 if n <= 15 else 131072)
    base.update(opts)
    if base.get("noise_weight", 0.0) <= 0:
        base.pop("noise_type", None)
    return search.PositionSearcher(**base)


def run_staged(ps, boards, signs, evaluator, serials=None, max_pv=8, max_steps=None, action_values=False, before_harvest=None, after_harvest=None, stage=None):
    """the job through the staged calls; evaluator(features) feeds the slots through provide() (stage: a callable instead, e.g. _evaluate(net))"""
    n = len(boards)
    ps.begin(boards, signs, serials=serials, max_pv=max_pv, max_steps=max_steps)
    hw = ps.board_size ** 2
    steps = 0
    while ps.finished() < n:
        ps.select_solve()
        if stage is not None:
            stage(ps)
        else:
            slots, feats = ps.scheduled()
            out = evaluator(feats) if len(slots) else (np.zeros((0, hw), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, hw, 2), np.float32))
            v3 = np.concatenate([out[1], 1 - out[1].sum(1, keepdims=True)], 1).astype(np.float32)
            ps.provide(slots, out[0], v3, np.ascontiguousarray(out[2], dtype=np.float32) if action_values else None)
        ps.expand()
        if before_harvest is not None:
            before_harvest(ps)
        ps.harvest()
        if after_harvest is not None:
            after_harvest(ps)
        steps += 1
        assert steps < 20000
    got = ps.results()
    got["steps"] = steps
    return got


def row_of(got, i):
    return {k: got[k][i] for k in OUTPUT_NAMES}


def compare_with_oracle(n, got, i, want, selector=0):
    """position i of a device run against the oracle's record (or root), bit for bit"""
    what = "position %d" % i
    root = got["root"][i]
    assert root[3] == len(want["edges"]), what
    if not want["edges"] and not want["moved"]:
        assert not root.any() and not got["root_value"][i].any() and got["best_move"][i] == 0 and (got["edge_index"][i] == -1).all(), what
        return
    assert root[0] == want["visits"] and root[1] == want["score"], (what, root, want["visits"], want["score"])
    assert got["root_value"][i][0] == want["win"] and got["root_value"][i][1] == want["draw"], what
    edges = pref.edges_from_rows(n, row_of(got, i))
    assert [e["cell"] for e in edges] == [pref.move_cell(e["move"], n) for e in want["edges"]], what                      # the root's own edge order
    for key in ("visits", "score"):
        assert [e[key] for e in edges] == [e[key] for e in want["edges"]], (what, key)
    for key in ("prior", "win", "draw"):
        assert np.array_equal(np.array([e[key] for e in edges], np.float32).view(np.uint32), np.array([e[key] for e in want["edges"]], np.float32).view(np.uint32)), (what, key)
    dense = pref.dense_rows(n, want["edges"])
    for key, row in dense.items():
        assert np.array_equal(np.ascontiguousarray(got[key][i]).view(np.uint8), np.ascontiguousarray(row).view(np.uint8)), (what, key)
    if want["moved"]:
        assert got["status"][i] == 0 and got["best_move"][i] == want["move"] and root[2] == want["flags"], (what, got["status"][i], got["best_move"][i], want["move"])
    if selector != 5:
        pick = pref.final_pick(selector, int(root[0]), want["edges"])
        assert got["best_move"][i] == (want["edges"][pick]["move"] if pick >= 0 else 0), what


def same_outputs(a, i, b, j, what, keys=OUTPUT_NAMES, steps_too=True):
    for k in keys:
        x, y = np.ascontiguousarray(a[k][i]), np.ascontiguousarray(b[k][j])
        if k == "info" and not steps_too:
            x, y = x[[0, 1, 3]], y[[0, 1, 3]]
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def parity_case(olib, rules, n, slots=5, serials=None, **opts):
    lists = positions_for(olib, rules, n)
    boards, signs = boards_and_signs(lists, n)
    base = _stand_in_evaluator(olib, n * n)
    evaluator = q_evaluator(base, n * n) if opts.get("action_values") else base
    loaded = []
    ps = make_searcher(rules, n, slots, **opts)
    got = run_staged(ps, boards, signs, evaluator, serials=serials, action_values=bool(opts.get("action_values")),
                     after_harvest=lambda s: loaded.append(s.slot_positions().copy()))
    stats = ps.stats()
    ps.close()
    assert stats["first_error"] == 0
    for i, moves in enumerate(lists):
        want = oracle_search(olib, rules, n, moves, 0 if serials is None else int(serials[i]), evaluator, opts)
        assert want["moved"]
        compare_with_oracle(n, got, i, want, opts.get("final_selector", 0))
        # as many steps as the oracle took (a solver launch that yields puts a batch off by a step: pacing, never another result)
        paced = opts.get("solver_yield_fraction", 0.0) > 0
        assert (got["info"][i][2] >= want["steps"] if paced else got["info"][i][2] == want["steps"]) and got["info"][i][3] == 0, (i, got["info"][i], want["steps"])
    # the slots freed up at different steps and took the next positions while the others searched on
    history = np.stack(loaded)
    assert len({tuple(np.flatnonzero(np.any(history[1:, s:s + 1] != history[:-1, s:s + 1], axis=1))) for s in range(slots)}) > 1
    if len(lists) >= 24:
        assert all(len(set(history[:, s]) - {-1}) >= 2 for s in range(slots))
    return got, lists


@pytest.mark.parametrize("speculative", [0, 1])
@pytest.mark.parametrize("rules,n", [(0, 15), (1, 15), (2, 15), (3, 20), (0, 9)])
def test_every_position_is_the_oracles_first_move(agx_lib, olib, rules, n, speculative):
    opts = dict(speculative_solver=1, solver_yield_fraction=0.5) if speculative else dict(speculative_solver=0)
    got, lists = parity_case(olib, rules, n, **opts)
    stones = [len(m) for m in lists]
    assert max(stones) >= (130 if n == 20 else 70) and 0 in stones and n * n - 1 in stones
    proven = [((int(s) >> 13) & 3) != 2 for s in got["root"][:, 1]]
    assert any(proven) and not all(proven)
    four = next(i for i, m in enumerate(lists) if m == open_four())
    assert got["info"][four][2] <= 2 and ((int(got["root"][four][1]) >> 13) & 3) == 3       # the open four: a proven win at once


@pytest.mark.parametrize("opts", [dict(max_batch_size=1), dict(max_batch_size=8), dict(final_selector=1), dict(final_selector=5),
                                  dict(noise_type=2, noise_weight=0.25), dict(use_symmetries=1), dict(action_values=1)],
                         ids=["batch1", "batch8", "max_visit", "lcb", "dirichlet", "symmetries", "action_values"])
def test_parity_under_other_settings(agx_lib, olib, opts):
    serials = (1000 + 7 * np.arange(24)).astype(np.int32) if ("noise_type" in opts or "use_symmetries" in opts) else None
    parity_case(olib, 0, 15, serials=serials, **opts)


def test_serials_key_the_noise_and_the_symmetries(agx_lib, olib):
    """the same board under two serials: other noise, other symmetries, other searches — and serial NULL is serial 0"""
    lists = positions_for(olib, 0, 15)[3:6]
    boards, signs = boards_and_signs(lists * 2, 15)
    ev = _stand_in_evaluator(olib)
    ps = make_searcher(0, 15, 3, noise_type=2, noise_weight=0.25, use_symmetries=1)
    got = run_staged(ps, boards, signs, ev, serials=np.array([0, 0, 0, 5, 6, 7], np.int32))
    plain = run_staged(ps, boards[:3], signs[:3], ev)
    ps.close()
    for i in range(3):
        same_outputs(got, i, plain, i, i)
    assert any(not np.array_equal(got["visits"][i], got["visits"][i + 3]) for i in range(3))


# ---- purity ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def purity_set(olib):
    lists = positions_for(olib, 1, 15)
    return [lists[i] for i in (0, 4, 9, 13, 15, 18, 19, 20, 21, 22)]


def test_a_slot_forgets_what_it_searched_before(agx_lib, olib, purity_set):
    a, b = purity_set[3], purity_set[0]           # 71 stones against 6: other stone counts, other trees
    boards, signs = boards_and_signs([a, b, a], 15)
    ps = make_searcher(1, 15, 1)
    got = run_staged(ps, boards, signs, _stand_in_evaluator(olib))
    ps.close()
    assert (got["status"] == 0).all() and got["info"][0][0] != got["info"][1][0]
    same_outputs(got, 0, got, 2, "A after B")


def test_order_and_slot_count_do_not_matter(agx_lib, olib, purity_set):
    ev = _stand_in_evaluator(olib)
    boards, signs = boards_and_signs(purity_set, 15)
    count = len(purity_set)
    runs = {}
    for slots, order in ((3, np.arange(count)), (3, np.arange(count)[::-1]), (3, np.random.default_rng(5).permutation(count)), (8, np.arange(count))):
        ps = make_searcher(1, 15, slots)
        runs[(slots, tuple(order))] = (order, run_staged(ps, boards[order], signs[order], ev))
        ps.close()
    (_, first), *others = runs.values()
    assert (first["status"] == 0).all()
    for order, got in others:
        for place, i in enumerate(order):
            same_outputs(got, place, first, int(i), (len(order), place))
    ps = make_searcher(1, 15, 5)                   # more slots than positions
    two = run_staged(ps, boards[[2, 7]], signs[[2, 7]], ev)
    assert (ps.slot_positions() == -1).all()
    ps.close()
    same_outputs(two, 0, first, 2, "2 on 5")
    same_outputs(two, 1, first, 7, "2 on 5")


def test_no_positions_is_a_no_op(agx_lib, olib):
    from alphagomoku_amd import _lib
    ps = make_searcher(0, 15, 2)
    out = _lib.AgxPositionSearchOutputs()
    assert agx_lib.agx_position_searcher_begin(ps.handle, 0, None, None, None, ctypes.byref(out), 8, 0, None) == 0
    assert ps.finished() == 0 and (ps.slot_positions() == -1).all()
    boards, signs = boards_and_signs([open_four()], 15)
    got = run_staged(ps, boards, signs, _stand_in_evaluator(olib))      # and the searcher is as good as new
    assert got["status"][0] == 0
    assert agx_lib.agx_position_searcher_begin(ps.handle, 0, None, None, None, ctypes.byref(out), 8, 0, None) == 0
    assert ps.finished() == 1                                           # (the finished job's count: nothing was touched)
    ps.close()


# ---- arenas ----------------------------------------------------------------------------------------------------------------------------
def test_trees_outgrow_their_arenas_and_hand_them_back(agx_lib, olib, purity_set):
    """class-0 arenas of 64 nodes: a search of 70 simulations outgrows them once (64 nodes + a batch of 4 against at most 70 + 2 x 4 nodes,
    which the next class — 128 nodes — holds; 32768 edges hold 80 nodes of at most 225 edges), and a finished position gives the larger
    bundle back before the slot takes the next one.  The reserve holds a class-1 bundle for every slot at once."""
    ev = _stand_in_evaluator(olib)
    boards, signs = boards_and_signs(purity_set, 15)
    big = make_searcher(1, 15, 4)
    want = run_staged(big, boards, signs, ev)
    assert big.stats()["arena_grows"] == 0
    big.close()
    ps = make_searcher(1, 15, 4, node_capacity=64, edge_capacity=32768, arena_reserve=4.0)
    got = run_staged(ps, boards, signs, ev)
    stats = ps.stats()
    assert stats["arena_grows"] > 0 and stats["arena_releases"] == stats["arena_grows"] and stats["arena_failures"] == 0 and stats["first_error"] == 0
    again = run_staged(ps, boards, signs, ev)
    stats = ps.stats()
    assert stats["arena_releases"] == stats["arena_grows"] and stats["arena_failures"] == 0
    ps.close()
    assert (want["status"] == 0).all()
    for i in range(len(purity_set)):
        same_outputs(got, i, want, i, i, steps_too=False)         # (a growth costs the slot one step)
        same_outputs(again, i, got, i, i)
    assert (got["info"][:, 2] > want["info"][:, 2]).any()


# ---- principal variation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_pv", [1, 8])
def test_principal_variation_is_the_engines_walk(agx_lib, olib, purity_set, max_pv):
    boards, signs = boards_and_signs(purity_set, 15)
    ps = make_searcher(1, 15, 3)
    expected = {}

    def before_harvest(s):
        for slot, position in enumerate(s.slot_positions()):
            if position < 0:
                continue
            info = s.engine.game_info(slot, with_edges=False)
            proven = ((info["root_score"] >> 13) & 3) != 2 and info["root_score"] not in (0, 0xFFFF)
            reduction = np.float32(max(0.0, min(1.0, (np.float32(info["root_draw"]) - np.float32(0.75)) / np.float32(0.25))))
            budget = int(np.float32(SIMS) - reduction * np.float32(SIMS - 50))
            if info["active"] and info["error"] == 0 and info["grow_pending"] == 0 and (proven or info["root_visits"] > budget):
                assert position not in expected
                expected[int(position)] = s.engine.principal_variation(slot, max_length=max_pv)["moves"]
    got = run_staged(ps, boards, signs, _stand_in_evaluator(olib), max_pv=max_pv, before_harvest=before_harvest)
    ps.close()
    assert sorted(expected) == list(range(len(purity_set)))
    assert got["pv"].shape == (len(purity_set), max_pv)
    for i, moves in expected.items():
        assert got["pv_length"][i] == len(moves) and got["pv"][i][:len(moves)].tolist() == moves and not got["pv"][i][len(moves):].any(), i
        assert not moves or moves[0] == got["best_move"][i]       # the "best" selector's first ply is the move
    assert min(max_pv, 2) <= max(len(m) for m in expected.values()) <= max_pv


# ---- step limit ------------------------------------------------------------------------------------------------------------------------
def test_step_limit_hands_over_the_root_as_it_stands(agx_lib, olib, purity_set):
    ev = _stand_in_evaluator(olib)
    boards, signs = boards_and_signs(purity_set, 15)
    ps = make_searcher(1, 15, 3)
    got = run_staged(ps, boards, signs, ev, max_steps=2)
    assert (ps.slot_positions() == -1).all()
    ps.close()
    assert 3 in got["status"] and 0 in got["status"]
    for i, moves in enumerate(purity_set):
        want = oracle_search(olib, 1, 15, moves, 0, ev, {}, max_steps=2)
        assert got["status"][i] == (0 if want["moved"] else 3), i
        assert got["info"][i][2] == want["steps"], i
        compare_with_oracle(15, got, i, want)


# ---- bad input, guard zones, optional outputs --------------------------------------------------------------------------------------------
def test_bad_positions_are_reported_and_skipped(agx_lib, olib, purity_set):
    ev = _stand_in_evaluator(olib)
    boards, signs = boards_and_signs(purity_set[:6], 15)
    ps = make_searcher(1, 15, 2)
    want = run_staged(ps, boards, signs, ev)
    bad_boards = np.insert(boards, [2, 4], 0, axis=0)
    bad_signs = np.insert(signs, [2, 4], 1)
    assert len(bad_boards) == 8
    bad_boards[2][17] = 3          # a cell of 3 ...
    bad_signs[5] = 0               # ... and a sign of 0, in the middle of the batch
    got = run_staged(ps, bad_boards, bad_signs, ev)
    ps.close()
    good = [0, 1, 3, 4, 6, 7]
    for place, i in enumerate(good):
        same_outputs(got, i, want, place, i)
    for i in (2, 5):
        assert got["status"][i] == 1 and (got["edge_index"][i] == -1).all(), i
        for k in OUTPUT_NAMES:
            if k not in ("status", "edge_index"):
                assert not got[k][i].any(), (i, k)


def _guarded_job(ps, boards, signs, shapes, leave_out=()):
    """device buffers with a sentinel-filled guard zone on both sides of every output"""
    from alphagomoku_amd import _lib
    from alphagomoku_amd.networks import DeviceBuffer
    guard, sentinel = 256, 0xA5
    n = len(boards)
    c_out, bufs, sizes = _lib.AgxPositionSearchOutputs(), {}, {}
    for k, (shape, dtype) in shapes.items():
        if k in leave_out:
            continue
        sizes[k] = n * int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        bufs[k] = DeviceBuffer(sizes[k] + 2 * guard)
        bufs[k].upload(np.full(sizes[k] + 2 * guard, sentinel, np.uint8))
        setattr(c_out, k, ctypes.c_void_p(bufs[k].ptr.value + guard))
    d_boards, d_signs = DeviceBuffer(boards.nbytes), DeviceBuffer(signs.nbytes)
    d_boards.upload(boards)
    d_signs.upload(signs)

    def read():
        out = {}
        for k, buf in bufs.items():
            raw = buf.download((sizes[k] + 2 * guard,), np.uint8)
            assert (raw[:guard] == sentinel).all() and (raw[guard + sizes[k]:] == sentinel).all(), "guard zone of %s overwritten" % k
            out[k] = raw[guard:guard + sizes[k]].copy().view(shapes[k][1]).reshape((n,) + shapes[k][0])
        for buf in list(bufs.values()) + [d_boards, d_signs]:
            buf.free()
        return out
    return c_out, d_boards, d_signs, read


def _run_raw(agx_lib, ps, c_out, d_boards, d_signs, n, evaluator, max_pv):
    from alphagomoku_amd._lib import check
    check(agx_lib.agx_position_searcher_begin(ps.handle, n, d_boards.ptr, d_signs.ptr, None, ctypes.byref(c_out), max_pv, 0, None))
    hw = ps.board_size ** 2
    for _ in range(20000):
        if ps.finished() == n:
            return
        ps.select_solve()
        slots, feats = ps.scheduled()
        pol, val = evaluator(feats) if len(slots) else (np.zeros((0, hw), np.float32), np.zeros((0, 2), np.float32))
        ps.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
        ps.expand()
        ps.harvest()
    raise AssertionError("the job did not finish")


def test_guard_zones_and_optional_outputs(agx_lib, olib, purity_set):
    ev = _stand_in_evaluator(olib)
    lists = [purity_set[1], [], purity_set[5], full_but_one(15), purity_set[2]]
    boards, signs = boards_and_signs(lists, 15)
    boards[2][3] = 7                                    # one bad position: its zero rows are written too
    ps = make_searcher(1, 15, 2)
    shapes = ps._shapes(5)
    c_out, d_boards, d_signs, read = _guarded_job(ps, boards, signs, shapes)
    _run_raw(agx_lib, ps, c_out, d_boards, d_signs, len(lists), ev, 5)
    want = read()
    assert want["status"].tolist() == [0, 0, 1, 0, 0] and want["root"][0][3] > 64 and want["root"][3][3] == 1     # more root edges than lanes; one
    for leave_out in [(k,) for k in OUTPUT_NAMES] + [tuple(OUTPUT_NAMES)]:
        c_out, d_boards, d_signs, read = _guarded_job(ps, boards, signs, shapes, leave_out)
        _run_raw(agx_lib, ps, c_out, d_boards, d_signs, len(lists), ev, 5)
        got = read()
        assert set(got) == set(OUTPUT_NAMES) - set(leave_out)
        for k in got:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (leave_out, k)
    ps.close()


# ---- end to end with the tower ---------------------------------------------------------------------------------------------------------
def _synthetic_net(n, seed=3):
    from alphagomoku_amd import synthetic
    from alphagomoku_amd.networks import AGNetwork
    desc = synthetic.net_desc(blocks=2, filters=64, rows=n, cols=n)
    blob, _ = synthetic.make_weights(desc, seed=seed)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    return net


@pytest.mark.parametrize("rules,n", [(1, 15), (3, 20)])
def test_search_with_the_tower_equals_the_staged_run(agx_lib, olib, rules, n):
    lists = positions_for(olib, rules, n)
    lists = lists[:9] if n == 20 else [lists[i] for i in (0, 3, 7, 11, 13, 14, 18, 19, 20, 21, 22, 23)]
    boards, signs = boards_and_signs(lists, n)
    net = _synthetic_net(n)
    ps = make_searcher(rules, n, 4)
    got = ps.search(boards, signs, net, max_pv=6)
    assert (ps.slot_positions() == -1).all() and ps.finished() == len(lists)
    again = ps.search(boards.reshape(-1, n, n), signs, net, max_pv=6)
    limited = ps.search(boards, signs, net, max_steps=2)           # the step limit ends the call
    assert set(limited["status"].tolist()) == {0, 3} and (limited["info"][:, 2] <= 2).all() and (ps.slot_positions() == -1).all()
    ps.close()
    staged = make_searcher(rules, n, 3)
    want = run_staged(staged, boards, signs, None, max_pv=6, stage=lambda s: s.evaluate(net))
    staged.close()
    net.close()
    assert (want["status"] == 0).all() and (want["root"][:, 0] > 0).all()
    for i in range(len(lists)):
        same_outputs(got, i, want, i, i)
        same_outputs(again, i, want, i, i)


def test_calls_on_two_streams_are_ordered_on_the_device(agx_lib, olib, purity_set):
    """the stages of a step alternate between two streams with nothing waited for in between: the searcher orders each behind the previous"""
    boards, signs = boards_and_signs(purity_set, 15)
    net = _synthetic_net(15)
    ps = make_searcher(1, 15, 4)
    want = ps.search(boards, signs, net)
    streams = []
    for _ in range(2):
        s = ctypes.c_void_p()
        assert agx_lib.agx_stream_create(ctypes.byref(s)) == 0
        streams.append(s)
    ps.begin(boards, signs, stream=streams[0])
    k = 0
    for step in range(20000):
        if step % 8 == 7 and ps.finished(streams[k % 2]) == len(purity_set):
            break
        for stage in (ps.select_solve, lambda stream: ps.evaluate(net, stream), ps.expand, ps.harvest):
            k += 1
            stage(streams[k % 2])
    got = ps.results(streams[k % 2])
    for i in range(len(purity_set)):
        same_outputs(got, i, want, i, i)
    other = ps.search(boards, signs, net, stream=streams[1])       # and a whole search on a stream of its own
    for i in range(len(purity_set)):
        same_outputs(other, i, want, i, i)
    ps.close()
    net.close()
    for s in streams:
        agx_lib.agx_stream_destroy(s)


def test_torch_tensors_on_a_torch_stream(agx_lib):
    """search.PositionSearcher.search with device torch tensors on a non-default torch stream, in a process of its own (the library has to
    share torch's HIP runtime from the start)"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "position_search_torch_main.py")], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0 and "ok:" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(agx_lib, olib):
    from alphagomoku_amd import _lib, selfplay
    from alphagomoku_amd.networks import DeviceBuffer
    INVALID, STATE, UNSUPPORTED = 1, 4, 3
    lib = agx_lib
    ps = make_searcher(0, 15, 2)
    boards, signs = boards_and_signs([[], open_four(), forced_defence()], 15)
    d_boards, d_signs = DeviceBuffer(boards.nbytes), DeviceBuffer(signs.nbytes)
    d_boards.upload(boards)
    d_signs.upload(signs)
    out = _lib.AgxPositionSearchOutputs()
    begin = lib.agx_position_searcher_begin
    assert begin(ps.handle, 3, d_boards.ptr, d_signs.ptr, None, None, 8, 0, None) == INVALID
    assert begin(ps.handle, -1, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), 8, 0, None) == INVALID
    assert begin(ps.handle, 3, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), -1, 0, None) == INVALID and b"max_pv" in lib.agx_last_error()
    assert begin(ps.handle, 3, None, d_signs.ptr, None, ctypes.byref(out), 8, 0, None) == INVALID
    assert begin(ps.handle, 3, d_boards.ptr, None, None, ctypes.byref(out), 8, 0, None) == INVALID
    assert lib.agx_position_searcher_search(ps.handle, None, 3, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), 8, 0, None) == INVALID
    assert lib.agx_position_searcher_evaluate(ps.handle, None, None) == INVALID
    assert lib.agx_position_searcher_slots(ps.handle, None, None) == INVALID and lib.agx_position_searcher_finished(ps.handle, None, None) == INVALID
    assert ps.finished() == 0 and (ps.slot_positions() == -1).all()                 # nothing of the above reached the device
    assert begin(ps.handle, 3, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), 8, 0, None) == 0
    assert begin(ps.handle, 3, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), 8, 0, None) == STATE and b"finished" in lib.agx_last_error()
    assert sorted(ps.slot_positions().tolist()) == [0, 1]
    ev = _stand_in_evaluator(olib)
    for _ in range(20000):
        if ps.finished() == 3:
            break
        ps.select_solve()
        slots, feats = ps.scheduled()
        pol, val = ev(feats) if len(slots) else (np.zeros((0, 225), np.float32), np.zeros((0, 2), np.float32))
        ps.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
        ps.expand()
        ps.harvest()
    assert begin(ps.handle, 3, d_boards.ptr, d_signs.ptr, None, ctypes.byref(out), 8, 0, None) == 0     # the job has finished: the next one is taken
    ps.close()
    d_boards.free()
    d_signs.free()
    handle = ctypes.c_void_p()
    for mode in (dict(match_mode=1), dict(search_threads=2, n_games=2), dict(search_buffers=2, n_games=2)):
        cfg = selfplay.default_config(**dict(dict(n_games=4), **mode))
        assert lib.agx_position_searcher_create(ctypes.byref(cfg), ctypes.byref(handle)) == UNSUPPORTED and not handle.value, mode
    cfg = selfplay.default_config(n_games=0)
    assert lib.agx_position_searcher_create(ctypes.byref(cfg), ctypes.byref(handle)) == INVALID and not handle.value
