"""Tree analysis on the device tree: Tree::getInfo(moves) for any move path (agx_engine_node_info), the principal variation of
SearchEngine::getSummary in one launch (agx_engine_principal_variation) and Tree::setBoard(..., forceRemoveRootNode = true)
(agx_engine_set_board_ex).  Nodes are compared field by field, floats bit for bit."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from alphagomoku_amd import synthetic
from alphagomoku_amd._lib import AgxError, check, lib
from test_engine_gpu import _best_edge, _oracle_root, _second_evaluator, _stand_in_evaluator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 15
HW = N * N


@pytest.fixture(scope="module")
def olib():
    return ol.load()


def _mv(r, c, sign=0):
    return sign | r << 2 | c << 9


def _cell(m):
    return (m >> 2 & 127) * N + (m >> 9 & 127)


def _provide(pool, ev):
    slots, feats = pool.scheduled()
    pol, val = ev(feats) if len(slots) else (np.zeros((0, HW), np.float32), np.zeros((0, 2), np.float32))
    pool.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
    return len(slots)


def _player_engine(rules=0, sims=200, speculative=0):
    """a one-game engine driven from outside (an evaluation Player's Tree / Search pair)"""
    from alphagomoku_amd import selfplay
    cfg = selfplay.default_config(rules=rules, n_games=1, max_batch_size=8, max_simulations=1 << 24, tss_table_entries=1 << 16, node_capacity=4096,
                                  edge_capacity=65536, force_expand_root=0, speculative_solver=speculative, speculative_waves=16)
    pool = selfplay.GeneratorPool(cfg)
    pool.begin(selfplay.pack_openings([[]]))
    pool.set_max_simulations(sims)
    return pool


def _search(pool, ev, board, sign, sims, force_remove_root=False):
    pool.set_board(0, board, sign, force_remove_root=force_remove_root)
    for _ in range(1000):
        info = pool.game_info(0, with_edges=False)
        proven = ((info["root_score"] >> 13) & 3) != 2 and info["root_score"] not in (0, 0xFFFF)
        if proven or info["root_visits"] >= sims:
            break
        pool.select_solve()
        _provide(pool, ev)
        pool.expand_only()
    assert pool.game_info(0, with_edges=False)["error"] == 0


def _start_board():
    board = np.zeros(HW, np.uint8)
    for r, c, s in [(7, 7, 1), (7, 8, 2), (8, 8, 1), (6, 6, 2)]:
        board[r * N + c] = s
    return board, 1


def _assert_node_is_root(node, info):
    """a node_info record against agx_engine_game_info's root of the same position"""
    if not node["found"]:
        assert info["root_visits"] == 0 and info["root_edges"] == 0
        return
    assert node["visits"] == info["root_visits"] and node["score"] == info["root_score"] and node["n_edges"] == info["root_edges"]
    assert np.float32(node["win"]) == np.float32(info["root_win"]) and np.float32(node["draw"]) == np.float32(info["root_draw"])
    assert np.float32(node["moves_left"]) == np.float32(info["root_moves_left"])
    assert node["edges"] == info["edges"]


def _same_node(a, b):
    assert a["found"] == b["found"]
    for k in ["visits", "score", "flags", "sign_to_move", "depth", "virtual_loss", "n_edges"]:
        assert a[k] == b[k], k
    for k in ["win", "draw", "moves_left"]:
        assert np.float32(a[k]) == np.float32(b[k]), k
    assert a["edges"] == b["edges"]


@pytest.mark.parametrize("rules,sims,speculative", [(0, 60, 0), (1, 60, 1), (2, 60, 0)])
def test_depth_two_lookup_matches_the_oracle(agx_lib, olib, rules, sims, speculative):
    """Two players, each a one-game engine, play a whole game like test_player_api_drives_a_game_from_outside; before a player's set-board its
    tree is asked for [its last move, the opponent's reply].  That node must be the oracle player's root after Tree::setBoard (take_turn) and
    the device root after the set-board, bit for bit (the root mark aside)."""
    from alphagomoku_amd import selfplay
    batch = 8
    evaluators = [_stand_in_evaluator(olib), _second_evaluator(olib)]
    ocfg = ol.default_search_config(max_batch_size=batch, max_simulations=sims, table_entries=1 << 16)
    op = np.zeros(64, np.uint16)
    k = olib.ago_prepare_opening(rules, N, N, 4242, ol.ptr(op))
    opening = [int(x) for x in op[:k]]
    pools, handles = [], []
    for _ in range(2):
        pools.append(_player_engine(rules, sims, speculative))
        h = olib.ago_game_create_ex(rules, N, N, 0, ctypes.byref(ocfg))
        olib.ago_game_set_force_expand_root(h, 0)
        olib.ago_game_match_begin(h, ol.ptr(np.array(opening + [0], np.uint16)), len(opening))
        handles.append(h)
    board = np.zeros(HW, np.uint8)
    for m in opening:
        board[_cell(m)] = m & 3
    sign = 1 if not opening else 3 - (opening[-1] & 3)
    who = 0 if sign == 1 else 1
    last = [None, None]
    plies = lookups = found = 0
    while True:
        pool, h = pools[who], handles[who]
        query = pool.node_info(0, [[last[who], last[1 - who]]])[0] if last[who] is not None else None
        pool.set_board(0, board, sign)
        olib.ago_game_take_turn(h)
        if query is not None:
            lookups += 1
            found += query["found"]
            _assert_node_is_root(query, pool.game_info(0))
            if query["found"]:
                root = pool.node_info(0, [[]])[0]
                assert root["flags"] == query["flags"] | 2
                query_unmarked = dict(query, flags=query["flags"] | 2)
                _same_node(root, query_unmarked)
            r = _oracle_root(olib, h)
            assert r["n"] == query["n_edges"] and r["visits"] == query["visits"], plies
            if query["found"]:
                e = query["edges"]
                assert np.float32(query["win"]) == r["win"] and np.float32(query["draw"]) == r["draw"] and query["score"] == r["score"], plies
                assert np.array_equal(np.array([x["move"] for x in e], np.uint16), r["moves"]), plies
                assert np.array_equal(np.array([x["visits"] for x in e], np.int32), r["ev"]), plies
                assert np.array_equal(np.array([x["prior"] for x in e], np.float32), r["prior"]), plies
                assert np.array_equal(np.array([[x["win"], x["draw"]] for x in e], np.float32).reshape(-1), r["val"]), plies
                assert np.array_equal(np.array([x["score"] for x in e], np.uint16), r["es"]), plies
        while True:
            pool.select_solve()
            slots, feats = pool.scheduled()
            f = np.zeros((batch, HW), np.uint32)
            c = olib.ago_game_step_select(h, ol.ptr(f), batch)
            assert c == len(slots) and np.array_equal(feats, f[:c]), plies
            pol, val = evaluators[who](feats) if c else (np.zeros((0, HW), np.float32), np.zeros((0, 2), np.float32))
            pool.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
            pool.expand_only()
            moved = olib.ago_game_step_expand(h, ol.ptr(np.ascontiguousarray(pol)), ol.ptr(np.ascontiguousarray(val)))
            info = pool.game_info(0)
            assert info["error"] == 0
            proven = ((info["root_score"] >> 13) & 3) != 2 and info["root_score"] not in (0, 0xFFFF)
            reduction = np.float32(max(0.0, min(1.0, (np.float32(info["root_draw"]) - np.float32(0.75)) / np.float32(0.25))))
            budget = int(np.float32(sims) - reduction * np.float32(sims - 50))
            over = proven or info["root_visits"] > budget
            assert over == bool(moved), plies
            if over:
                break
        mv = info["edges"][_best_edge(info["root_visits"], info["edges"])]["move"]
        assert mv == olib.ago_game_last_move(h), plies
        board[_cell(mv)] = mv & 3
        sign = 3 - (mv & 3)
        last[who] = mv
        olib.ago_game_external_move(handles[1 - who], mv)
        plies += 1
        if olib.ago_game_outcome(h) != 0:
            break
        who = 1 - who
    assert plies >= 10 and lookups >= 5 and found >= 1
    for pool in pools:
        pool.close()
    for h in handles:
        olib.ago_game_destroy(h)


def _step_selfplay(pool, ev, steps):
    for _ in range(steps):
        pool.select_solve()
        _provide(pool, ev)
        pool.expand_backup()


def test_empty_path_is_the_root(agx_lib, olib):
    """node_info(game, [[]]) is agx_engine_game_info's root: a self-play pool in mid-game (several games), a match pool, a tournament pool"""
    from alphagomoku_amd import selfplay
    ev = _stand_in_evaluator(olib)
    openings = []
    for g in range(4):
        op = np.zeros(64, np.uint16)
        k = olib.ago_prepare_opening(0, N, N, 300 + g, ol.ptr(op))
        openings.append([int(x) for x in op[:k]])
    configs = [dict(n_games=4), dict(n_games=4, match_mode=1), dict(n_games=2, search_threads=2)]
    for extra in configs:
        cfg = selfplay.default_config(rules=0, max_batch_size=4, max_simulations=60, tss_table_entries=1 << 14, node_capacity=4096, edge_capacity=65536, **extra)
        pool = selfplay.GeneratorPool(cfg)
        pool.begin(selfplay.pack_openings([[]] if extra.get("search_threads") else openings))
        games = [0] if extra.get("search_threads") else range(extra["n_games"])
        seen = 0
        for step in range(6):
            if extra.get("match_mode"):
                pool.select_solve_match()
                parts = [pool.scheduled_group(player, 2) for player in (0, 1)]
                slots, feats = np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])
                pol, val = ev(feats) if len(slots) else (np.zeros((0, HW), np.float32), np.zeros((0, 2), np.float32))
                pool.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
                pool.expand_backup_match()
            else:
                _step_selfplay(pool, ev, 1)
            for g in games:
                info = pool.game_info(g)
                if not info["active"]:
                    continue   # (a match tree waiting for its pair's next game holds no position)
                node = pool.node_info(g, [[]])[0]
                _assert_node_is_root(node, info)
                seen += node["found"]
        assert seen > 0, extra
        pool.close()


def test_depth_one_equals_the_root_after_set_board(agx_lib, olib):
    """every root child with a cached node: node_info([m]) on one engine equals the root a twin engine (same search) reads after a set-board
    to that child position"""
    ev = _stand_in_evaluator(olib)
    board, sign = _start_board()
    pool = _player_engine(sims=200)
    _search(pool, ev, board, sign, 200)
    root = pool.node_info(0, [[]])[0]
    children = pool.node_info(0, [[e["move"]] for e in root["edges"]])
    cached = [(e["move"], c) for e, c in zip(root["edges"], children) if c["found"]]
    assert len(cached) >= 2
    for m, child in cached[:6]:
        twin = _player_engine(sims=200)
        _search(twin, ev, board, sign, 200)
        b2 = board.copy()
        b2[_cell(m)] = sign
        twin.set_board(0, b2, 3 - sign)
        info = twin.game_info(0)
        _assert_node_is_root(child, info)
        assert twin.node_info(0, [[]])[0]["flags"] == child["flags"] | 2
        twin.close()
    pool.close()


def test_principal_variation_is_the_host_walk(agx_lib, olib):
    """the one-launch variation equals node_info + BestEdgeSelector ply by ply, move for move and edge for edge, from the root and from a path"""
    ev = _stand_in_evaluator(olib)
    board, sign = _start_board()
    pool = _player_engine(sims=400)
    _search(pool, ev, board, sign, 400)
    for start in ([], None):
        if start is None:
            start = [pool.principal_variation(0)["moves"][0]]
        pv = pool.principal_variation(0, start)
        path, moves, edges, nodes = list(start), [], [], []
        while True:
            node = pool.node_info(0, [path])[0]
            nodes.append(node)
            if not node["found"] or node["n_edges"] == 0:
                break
            e = node["edges"][_best_edge(node["visits"], node["edges"])]
            moves.append(e["move"])
            edges.append(e)
            path.append(e["move"])
        assert pv["moves"] == moves and pv["edges"] == edges and len(moves) >= 2
        assert len(pv["nodes"]) == len(nodes)
        for a, b in zip(pv["nodes"], nodes):
            _same_node(dict(a, edges=b["edges"]), b)
    # max_length cuts the walk
    short = pool.principal_variation(0, [], max_length=1)
    assert short["moves"] == pool.principal_variation(0)["moves"][:1] and len(short["nodes"]) == 2
    pool.close()


def test_principal_variation_starts_with_the_move_the_best_selector_plays(agx_lib, olib):
    """self-play pool with the 'best' final selector: the first move of every game's variation, read between the expand and the advance
    stage, is the move the advance stage plays"""
    from alphagomoku_amd import selfplay
    ev = _stand_in_evaluator(olib)
    games = 4
    openings = []
    for g in range(games):
        op = np.zeros(64, np.uint16)
        k = olib.ago_prepare_opening(0, N, N, 900 + g, ol.ptr(op))
        openings.append([int(x) for x in op[:k]])
    cfg = selfplay.default_config(rules=0, n_games=games, max_batch_size=4, max_simulations=60, tss_table_entries=1 << 14, node_capacity=4096,
                                  edge_capacity=65536, final_selector=0)
    pool = selfplay.GeneratorPool(cfg)
    pool.begin(selfplay.pack_openings(openings))
    checked, records_seen = 0, 0
    for step in range(120):
        pool.select_solve()
        _provide(pool, ev)
        check(lib.agx_engine_expand_group(pool._h, 0, 1, None))
        first = {g: pool.principal_variation(g, max_length=1)["moves"] for g in range(games)}
        check(lib.agx_engine_advance_group(pool._h, 0, 1, None))
        recs, _ = pool.records()
        for r in recs[records_seen:]:
            assert first[r.game_slot] == [r.move], (step, r.game_slot)
            checked += 1
        records_seen = len(recs)
    assert checked >= 8
    pool.close()


def test_paths_that_leave_the_tree(agx_lib, olib):
    """an occupied cell, an uncached position and a path deeper than the tree give found = 0; a cell off the board is an error"""
    ev = _stand_in_evaluator(olib)
    board, sign = _start_board()
    pool = _player_engine(sims=200)
    _search(pool, ev, board, sign, 200)
    root = pool.node_info(0, [[]])[0]
    unvisited = [e["move"] for e in root["edges"] if e["visits"] == 0]
    pv = pool.principal_variation(0)["moves"]
    corner = [_mv(0, 0), _mv(0, 14), _mv(14, 0), _mv(14, 14), _mv(0, 7), _mv(14, 7)]
    paths = [[_mv(7, 7)], [pv[0], _mv(8, 8)], [unvisited[0]] if unvisited else [_mv(0, 1)], pv + corner, [pv[0], pv[0]]]
    out = pool.node_info(0, paths)
    assert [o["found"] for o in out] == [0] * len(paths)
    assert all(o["n_edges"] == 0 and o["visits"] == 0 and o["edges"] == [] for o in out)
    assert pool.principal_variation(0, [_mv(7, 7)])["moves"] == []
    with pytest.raises(AgxError):
        pool.node_info(0, [[_mv(15, 3)]])
    with pytest.raises(AgxError):
        pool.principal_variation(0, [_mv(3, 15)])
    with pytest.raises(AgxError):
        pool.node_info(1, [[]])
    # edges_per_path below the edge count truncates the copy, n_edges stays
    few = pool.node_info(0, [[]], edges_per_path=3)[0]
    assert few["n_edges"] == root["n_edges"] and few["edges"] == root["edges"][:3]
    pool.close()


def test_forced_root_removal(agx_lib, olib):
    """set_board(force_remove_root=True) against a twin engine without it, both from the same search: forcing an uncached position changes
    nothing; forcing a cached one removes that node alone, and the next step hands the root to the network"""
    ev = _stand_in_evaluator(olib)
    board, sign = _start_board()
    forced, twin = _player_engine(sims=200), _player_engine(sims=200)
    for p in (forced, twin):
        _search(p, ev, board, sign, 200)
    # a position the trees do not hold: forcing is not forcing
    q = board.copy()
    q[0] = sign
    q[HW - 1] = 3 - sign
    assert forced.node_info(0, [[_mv(0, 0), _mv(14, 14)]])[0]["found"] == 0
    forced.set_board(0, q, sign, force_remove_root=True)
    twin.set_board(0, q, sign)
    a, b = forced.game_info(0), twin.game_info(0)
    assert a["n_nodes"] == b["n_nodes"] and a["n_edges"] == b["n_edges"] and a["root_visits"] == b["root_visits"] == 0
    for p in (forced, twin):
        _search(p, ev, q, sign, 150)
    a, b = forced.game_info(0), twin.game_info(0)
    assert a["n_nodes"] == b["n_nodes"] and a["root_visits"] == b["root_visits"] > 0 and a["edges"] == b["edges"]
    # the cached position q again: forced drops its node
    root = twin.node_info(0, [[]])[0]
    assert root["found"]
    forced.set_board(0, q, sign, force_remove_root=True)
    twin.set_board(0, q, sign)
    a, b = forced.game_info(0), twin.game_info(0)
    assert a["root_visits"] == 0 and a["root_edges"] == 0 and forced.node_info(0, [[]])[0]["found"] == 0
    assert a["n_nodes"] == b["n_nodes"] - 1 and a["n_edges"] == b["n_edges"] - root["n_edges"]
    paths = [[e["move"]] for e in root["edges"]]
    kids_forced, kids_twin = forced.node_info(0, paths), twin.node_info(0, paths)
    assert sum(k["found"] for k in kids_twin) >= 2
    for x, y in zip(kids_forced, kids_twin):
        _same_node(x, y)
    # the first step after the forced set-board evaluates the root itself
    forced.select_solve()
    slots, feats = forced.scheduled()
    assert len(slots) == 1
    pol, val = ev(feats)
    forced.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
    forced.expand_only()
    again = forced.node_info(0, [[]])[0]
    assert again["found"] and again["visits"] == 1 and again["n_edges"] > 0
    forced.close()
    twin.close()


def test_reference_boundary_walks_the_principal_variation(agx_lib, tmp_path):
    """a C++ program on the reference-named classes (libagx_ag.so): Tree::getInfo(pv) + the 'best' selector ply by ply equals the device's
    one-launch variation, and Tree::setBoard(board, sign, true) drops the root alone"""
    src = os.path.join(ROOT, "tests", "cpp", "tree_analysis_main.cpp")
    lib_dir = os.path.join(ROOT, "alphagomoku_amd")
    binary = str(tmp_path / "tree_analysis_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-o", binary, src, "-L" + lib_dir, "-lagx_ag", "-lagx", "-Wl,-rpath," + lib_dir, "-lpthread"])
    d = synthetic.net_desc(blocks=2, filters=64)
    blob, _ = synthetic.make_weights(d)
    net = tmp_path / "network.agxw"
    synthetic.save_weights(net, d, blob)
    p = subprocess.run([binary, str(net), "300"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:] + p.stdout[-2000:]
    line = json.loads([x for x in p.stdout.splitlines() if x.startswith('{"mode"')][0])
    assert line["root_visits"] >= 300 and line["pv_length"] >= 2
    assert line["pv_equal"] == 1 and line["tail_equal"] == 1
    assert line["occupied_edges"] == 0 and line["occupied_visits"] == 0
    assert line["nodes_after_force"] == line["nodes_before"] - 1 and line["root_visits_after_force"] == 0
    assert line["child_visits_after_force"] > 0
