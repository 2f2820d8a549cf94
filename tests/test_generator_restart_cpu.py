"""What an oracle generator carries from one game into the next (oracle only, no device): the facts tests/test_engine_restart_gpu.py rests on.

A pool slot's later games are played by the generator that played its earlier ones (tests/generator_restart_ref.py lists what
GameGenerator.cpp keeps and what it resets).  Here: every case of the GPU file holds a later game that a NEW generator would play
differently — so a device that started every game from scratch could not pass it — and each carried-over item is shown on its own."""
import ctypes

import numpy as np
import pytest

import generator_restart_ref as ref
import oracle_lib as ol


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@pytest.mark.parametrize("name", list(ref.CASES))
def test_every_gpu_case_holds_a_later_game_that_a_new_generator_plays_differently(olib, name):
    """the non-vacuity condition of the GPU cases: at least one game after a slot's first whose steps (leaf count, feature words, root
    moves-left, maximum depth) or records (move, root, edges) differ from the game a new generator plays from the same opening under the same
    serial.  A difference in the records' solved flags alone (nearly every later game has one: slot 0's "solved" flags are never reset)
    does not count."""
    case = ref.CASES[name]
    differences, steps = ref.later_game_differences(olib, case)
    for opening_id, (what, k) in differences:
        print("%s: opening %d (game %d of slot %d) differs from a new generator's game at %s %d" % (name, opening_id, opening_id // case["slots"], opening_id % case["slots"], what, k))
    print("%s: %d oracle steps over %d games" % (name, steps, case["slots"] * case["rounds"]))
    assert any(what in ("step", "records") for _, (what, _) in differences), differences


def test_a_slots_first_game_is_the_new_generators_game(olib):
    """... and the comparison itself is sound: the FIRST game of a slot is the game of a new generator, step for step and record for record"""
    case = ref.CASES["freestyle"]
    for slot in range(case["slots"]):
        assert ref.first_difference(ref.play_slot(olib, dict(case, rounds=1), slot)[0], ref.play_fresh(olib, case, slot)) is None


@pytest.mark.parametrize("name", ["freestyle", "renju", "tournament_two_buffers"])
def test_the_generation_runs_on_over_the_games(olib, name):
    """SharedHashTable::m_base_generation (SharedHashTable.hpp:126,153-156) is never reset: a game's first solve runs at the generation the
    previous games left plus one (every prepare_search increases it: once per game begun, once per move that does not end the game — as many
    as the game has records), modulo 64, while the cleared table's entries carry generation 0.  A new generator starts at 1."""
    case = ref.CASES[name]
    games = ref.play_slot(olib, case, 0)
    total = 0
    for k, game in enumerate(games):
        assert game["outcome"] != 0 and len(game["records"]) > 0
        assert game["generation_first"] == (total + 1) % 64, k
        total += len(game["records"])
        assert game["generation_last"] == total % 64, k
    assert games[1]["generation_first"] != 1 and ref.play_fresh(olib, case, games[1]["id"])["generation_first"] == 1


def test_every_search_thread_of_a_shared_tree_is_at_the_same_generation(olib):
    """a tournament search over several games: prepare_search raises the generation of EVERY thread's solver, once per game begun and once per
    move that does not end the game — the move that ends a game raises none.  (The device used to raise the threads behind the first, and the
    first thread's second task buffer, on that last move too: from the tree's second game on they solved one generation ahead.)"""
    case = ref.CASES["tournament_two_buffers"]
    g = ref.Generator(olib, case)
    expected = 0
    for opening_id in ref.slot_ids(case, 0):
        g.begin(opening_id)
        expected += 1
        while not g.over():
            records = olib.ago_game_num_records(g.h)
            g.step()
            expected += int(olib.ago_game_num_records(g.h) > records and not g.over())
            assert [ref.search_state(olib, g.h, lane)["generation"] for lane in range(case["threads"])] == [expected % 64] * case["threads"]
    g.close()


def _generation_only(olib, case, opening_id, generation):
    """a new generator whose solver generation is wound forward by beginning the game again and again (Game::begin clears the tree and the
    table, touches no task slot and increases the generation once): it differs from a new generator in the generation ALONE"""
    g = ref.Generator(olib, case)
    g.begin(opening_id)
    while ref.search_state(olib, g.h)["generation"] != (generation + 63) % 64:
        g.begin(opening_id)
    game = g.play(opening_id)
    g.close()
    return game


def test_the_generation_alone_changes_a_later_game(olib):
    """the table's replacement rule reads depth - (generation - entry's generation) (SharedHashTable.hpp:218) and an empty entry has
    generation 0: a generator that differs from a new one ONLY in its generation (no task slot touched) plays some opening differently"""
    found = []
    for name in ("format201", "freestyle", "renju"):
        case = ref.CASES[name]
        for slot in range(case["slots"]):
            for game in ref.play_slot(olib, case, slot)[1:]:
                wound = _generation_only(olib, case, game["id"], game["generation_first"])
                assert wound["generation_first"] == game["generation_first"]
                d = ref.first_difference(wound, ref.play_fresh(olib, case, game["id"]))
                if d is not None and d[0] != "flags":
                    found.append((name, game["id"], d))
    print("a generation-only generator differs from a new one:", found)
    assert found


def _step_watching_the_tasks(olib, g, dirty, residue):
    """one step of a generator; returns the proven-edge leaves (task slot, moves_left) that sat in a slot nothing has written in this game"""
    feats = np.zeros((g.width, g.hw), np.uint32)
    c = olib.ago_game_step_select(g.h, ol.ptr(feats), g.width)
    state = ref.search_state(olib, g.h)
    seen = []
    for k in range(state["stored"]):
        if state["flags"][k] & 1:        # REACHED_PROVEN_EDGE (Search.cpp:139-150): neither the solver nor the network writes this task
            if k not in dirty:
                seen.append((k, state["moves_left"][k]))
                assert state["moves_left"][k] == residue[k], (k, state["moves_left"][k], residue[k])
        else:
            dirty.add(k)                 # solved, or answered by the network: moves_left is overwritten (AlphaBetaSearch.cpp:114-139, NNEvaluator.cpp:263-286)
    pol, val = g.ev(feats[:c]) if c else (np.zeros((0, g.hw), np.float32), np.zeros((0, 2), np.float32))
    olib.ago_game_step_expand(g.h, ol.ptr(pol), ol.ptr(val))
    return seen


def test_a_proven_edge_leaf_backs_up_what_its_task_slot_held_in_the_previous_game(olib):
    """SearchTask::set (SearchTask.cpp:32-50) leaves moves_left alone and a generator's SearchTaskList outlives the game: a proven-edge leaf
    of a later game whose task slot has not been written in that game yet carries the moves_left the slot held when the previous game ended —
    not the 0 of a new generator's slot — into Tree::backup and so into the root's moves-left mean"""
    carried = []
    for name in ("freestyle", "standard", "renju", "caro5", "noise_custom", "board12"):
        case = ref.CASES[name]
        for slot in range(case["slots"]):
            g = ref.Generator(olib, case)
            for k, opening_id in enumerate(ref.slot_ids(case, slot)):
                residue = ref.search_state(olib, g.h)["moves_left"]      # what the slots hold as the game begins
                g.begin(opening_id)
                assert ref.search_state(olib, g.h)["moves_left"] == residue   # Game::begin touches no task slot
                dirty = set()
                while not g.over():
                    for slot_k, left in _step_watching_the_tasks(olib, g, dirty, residue):
                        if k > 0 and left != 0.0:
                            carried.append((name, opening_id, slot_k, float(left)))
            g.close()
    print("proven-edge leaves that backed up a previous game's moves_left (case, opening, task slot, moves_left):", carried[:12], len(carried))
    assert carried


def test_cleanup_cancels_both_task_buffers(olib):
    """Search::cleanup (Search.cpp:233-242) at every prepare_search: with two task buffers per search thread (the double-buffered
    tournament search) a move is made while the OTHER buffer's leaves are with the network; behind the step that made the move that buffer is
    empty in every thread and the new root's edges carry exactly the virtual losses of the leaves selected since — one per stored task —
    and none of the cancelled ones; the same holds across a game boundary (Game::begin)"""
    case = ref.CASES["tournament_two_buffers"]
    g = ref.Generator(olib, case)
    in_flight_dropped = moves_checked = 0
    for opening_id in ref.slot_ids(case, 0):
        g.begin(opening_id)
        assert all(ref.search_state(olib, g.h, lane)[key] == 0 for lane in range(case["threads"]) for key in ("stored", "other_stored"))
        while not g.over():
            records = olib.ago_game_num_records(g.h)
            other_before = sum(ref.search_state(olib, g.h, lane)["other_stored"] for lane in range(case["threads"]))
            feats = np.zeros((g.width, g.hw), np.uint32)
            c = olib.ago_game_async_step(g.h, ol.ptr(feats), g.width)
            if g.over():
                break
            states = [ref.search_state(olib, g.h, lane) for lane in range(case["threads"])]
            if olib.ago_game_num_records(g.h) > records:
                # the step made a move: prepare_search ran Search::cleanup on both buffers before the new leaves were selected
                assert all(s["other_stored"] == 0 for s in states)
                rv, rs = ctypes.c_int(), ctypes.c_uint16()
                rval = (ctypes.c_float * 2)()
                em, ev, ep, evl = np.zeros(512, np.uint16), np.zeros(512, np.int32), np.zeros(512, np.float32), np.zeros(1024, np.float32)
                es, ef = np.zeros(512, np.uint16), np.zeros(512, np.uint16)
                n = olib.ago_game_root(g.h, ctypes.byref(rv), rval, ctypes.byref(rs), ol.ptr(em), ol.ptr(ev), ol.ptr(ep), ol.ptr(evl), ol.ptr(es), ol.ptr(ef), 512)
                if n > 0:
                    assert int((ef[:n] & 0x7FFF).sum()) == sum(s["stored"] for s in states)
                    moves_checked += 1
                in_flight_dropped += int(other_before > 0)
            pol, val = g.ev(feats[:c]) if c else (np.zeros((0, g.hw), np.float32), np.zeros((0, 2), np.float32))
            olib.ago_game_async_provide(g.h, ol.ptr(pol), ol.ptr(val))
    g.close()
    assert in_flight_dropped > 0 and moves_checked > 0
