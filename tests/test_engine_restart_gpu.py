"""A pool slot's SECOND and later games against the oracle: one oracle generator per slot for the whole run.

Slot s of S plays openings s, s + S, s + 2 S, ... and nearly every game a long-running pool plays is a later game of its slot.  The restart is
the tail of agx_engine_advance_group: k_arena_service hands out the next opening and takes a grown arena bundle back, k_clear_tables(restart = 1)
clears tree and solver table and its last part begins the game (k_restart for a tournament search), begin_game keeps the solver's generation
and the task slots.  The oracle side is ONE generator per slot that goes on (tests/generator_restart_ref.py: what a GameGenerator keeps between
games); tests/test_generator_restart_cpu.py shows for every case below that a generator made anew for each game would play differently."""
import time

import numpy as np
import pytest

import generator_restart_ref as ref
import oracle_lib as ol
import test_engine_gpu as teg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def olib():
    return ol.load()


def _report(name, started, compared_by_round, stats):
    print("%s: roots compared per round %s, games finished %d, %.1f s" % (name, compared_by_round, stats["games_finished"], time.time() - started))


def _play_case(olib, name, **extra):
    case = ref.CASES[name]
    s = case["search"]
    started = time.time()
    compared, stats = teg._play_and_compare(olib, case["rules"], games=case["slots"], batch=case["batch"], sims=case["sims"], max_steps=6000,
                                            evaluator=teg._stand_in_evaluator(olib, case["n"] * case["n"]), n=case["n"], draw_after=case["draw_after"],
                                            rounds=case["rounds"], table_entries=s.get("table_entries", 1 << 16), use_symmetries=s.get("use_symmetries", 0),
                                            noise_weight=s.get("noise_weight", 0.0), noise_type=s.get("noise_type", 1), **case["device"], **extra)
    _report(name, started, stats["compared_by_round"], stats)
    assert stats["first_error"] == 0
    assert all(c > 0 for c in stats["compared_by_round"]), stats["compared_by_round"]     # every round was compared, the later ones too
    assert stats["games_finished"] == case["slots"] * case["rounds"]
    return stats


@pytest.mark.parametrize("name", ["freestyle", "standard", "renju", "caro5", "caro6", "board12", "spec_freestyle", "sliced", "symmetries", "noise_custom",
                                  "noise_dirichlet"])
def test_later_games_of_a_slot_match_the_generator_that_goes_on(agx_lib, olib, name):
    """every rule set on 15x15 with the serial solver, a 12x12 board (the run-time-size kernels), the speculative solver, the pool stepped as 4
    CU-masked slices the way bench.py steps it, input symmetries and root noise (their streams are keyed by the opening id and the move number: a
    later game must draw what the oracle draws under its new serial): scheduled leaves and features, root edges, visits, priors, values, scores,
    root moves-left, maximum depth, n_moves, opening_id and games_done after every step of every game, then every game's moves and root flags"""
    stats = _play_case(olib, name)
    if ref.CASES[name]["device"].get("speculative_solver"):
        assert stats["speculative_solves"] > 0


def test_format_201_samples_and_game_framing_over_all_rounds(agx_lib, olib):
    """record_format 3: every sample of every round byte for byte, game_slot / game_index of every record and every finished game's frame
    (GameDataStorage::serialize) — the record sink's framing of games after a slot's first"""
    _play_case(olib, "format201")


def test_a_grown_arena_bundle_is_taken_back_and_the_next_game_starts_small(agx_lib, olib):
    """node_capacity at an eighth of what a search needs: every game outgrows its class-0 arenas, a finished game's bundle is taken back by
    k_arena_service before the slot is handed its next opening, and the next game starts in class 0 again and grows anew"""
    case = ref.CASES["small_arenas"]
    stats = _play_case(olib, "small_arenas")
    assert stats["arena_failures"] == 0
    assert stats["arena_grows"] >= case["slots"] * case["rounds"]          # once per game or more
    assert stats["arena_releases"] >= case["slots"] * (case["rounds"] - 1)  # every game that was followed by another gave its bundle back


def test_slots_wait_for_openings_and_start_in_game_order(agx_lib, olib):
    """five openings for three slots and three rounds: slot 2 waits for its second opening, slots 0 and 1 for their third — idle (nothing
    scheduled, not active) until agx_engine_add_openings brings the rest, then every slot starts the game its number and its games_done name,
    in the step in which the oracle's generator begins it"""
    stats = _play_case(olib, "starved", n_openings=5)
    assert stats["idle_steps"] >= 3 and stats["openings_taken"] == 9


def test_restored_games_are_played_out_and_followed_by_the_slots_next_games(agx_lib, olib):
    """agx_engine_restore_game, then the restart: the saved games (an opening and six moves) go on as a new generator's would
    (GameGenerator::load makes a new AlphaBetaSearch: generation 1), and the slot's next games follow on the same generator"""
    case = ref.CASES["restored"]
    saved = []
    for g in range(case["slots"]):
        moves = ref.restored_moves(olib, case, g)
        saved.append(dict(game_slot=g, game_index=0, opening_id=g, sign_to_move=3 - (moves[-1] & 3), nn_queued=0, moves=moves))
    _play_case(olib, "restored", restore_from=saved)


def _device_records(pool):
    """opening id -> the pool's records of that game in ref.game_records' form"""
    recs, edges = pool.records()
    out = {}
    for r in sorted(recs, key=lambda x: (x.game_serial, x.move_number)):
        e = edges[r.edge_offset:r.edge_offset + r.n_edges]
        out.setdefault(r.game_serial, []).append((
            r.move, r.root_visits, np.float32(r.root_win).tobytes() + np.float32(r.root_draw).tobytes(), r.root_score, r.root_flags,
            np.array([x.move for x in e], np.uint16).tobytes(), np.array([x.visits for x in e], np.int32).tobytes(),
            np.array([x.prior for x in e], np.float32).tobytes(), np.array([[x.win, x.draw] for x in e], np.float32).tobytes(),
            np.array([x.score for x in e], np.uint16).tobytes()))
    return out


RECORD_FIELDS = ("move", "root visits", "root value", "root score", "root flags", "edge moves", "edge visits", "edge priors", "edge values", "edge scores")


def _assert_same_records(device, oracle, tag):
    assert device is not None and len(device) == len(oracle), (tag, None if device is None else len(device), len(oracle))
    for i, (d, o) in enumerate(zip(device, oracle)):
        assert d == o, (tag, "record", i, [name for name, x, y in zip(RECORD_FIELDS, d, o) if x != y])


def test_later_games_with_parked_solves(agx_lib, olib):
    """the speculative solver on renju with solver_yield_fraction 0.5: solves are parked at a launch's end and taken up by the next one, games sit
    steps out, and the slots restart in between — pacing only.  The pool is stepped to the end of 12 slots x 2 rounds without looking, then every
    record of every game (move, root visits, value, score, flags, every root edge's move, visits, prior, value, score) must be what the slot's ONE
    oracle generator produced.  (k_advance makes no move for a game whose batch is still pending, so no game ends WHILE one of its solves is
    parked; begin_game's park_forget_game clears what the finished batch left.)"""
    from alphagomoku_amd import selfplay
    case = ref.CASES["spec_renju_park"]
    started = time.time()
    slots, rounds, n = case["slots"], case["rounds"], case["n"]
    cfg = selfplay.default_config(rules=case["rules"], board_size=n, draw_after=case["draw_after"], n_games=slots, max_batch_size=case["batch"],
                                  max_simulations=case["sims"], tss_table_entries=case["search"]["table_entries"], node_capacity=4096, edge_capacity=65536,
                                  record_edge_capacity=slots * rounds * case["draw_after"] * n * n, **case["device"])
    pool = selfplay.GeneratorPool(cfg)
    ev = teg._stand_in_evaluator(olib, n * n)
    pool.begin(selfplay.pack_openings([ref.opening(olib, case, i) for i in range(slots * rounds)]))
    for _ in range(6000):
        pool.select_solve()
        picked, feats = pool.scheduled()
        if len(picked):
            p, v = ev(feats)
            pool.provide(picked, p, np.concatenate([v, 1 - v.sum(1, keepdims=True)], 1).astype(np.float32))
        pool.expand_backup()
        if pool.stats()["active_games"] == 0:
            break
    st = pool.stats()
    device = _device_records(pool)
    pool.close()
    assert st["first_error"] == 0 and st["games_finished"] == slots * rounds
    assert st["speculative_solves"] > 0 and st["speculative_parks"] > 0
    later = 0
    for slot in range(slots):
        for k, game in enumerate(ref.play_slot(olib, case, slot)):
            _assert_same_records(device.get(game["id"]), game["records"], (slot, k, game["id"]))
            later += len(game["records"]) if k > 0 else 0
    print("spec_renju_park: %d records of later games compared, %d solves parked, games finished %d, %.1f s" % (later, st["speculative_parks"], st["games_finished"],
                                                                                                               time.time() - started))
    assert later > 0


@pytest.mark.parametrize("name", ["tournament", "tournament_two_buffers"])
def test_next_game_on_a_shared_tree(agx_lib, olib, name):
    """a tournament search (three search threads on one tree, one or two task buffers each) over three games: the k_restart pair of
    agx_engine_advance_group.  The oracle's game goes on with its Search objects — every thread's solver generation and task slots — and is compared
    the way test_tournament_search_on_one_tree / test_double_buffered_tournament_search compare a first game: leaves and features of every
    step, the root after it, then every game's moves and root visits"""
    from alphagomoku_amd import selfplay
    case = ref.CASES[name]
    started = time.time()
    n, hw, threads, buffers, batch, rounds = case["n"], case["n"] * case["n"], case["threads"], case["buffers"], case["batch"], case["rounds"]
    cfg = selfplay.default_config(rules=case["rules"], draw_after=case["draw_after"], n_games=threads * buffers, search_threads=threads, search_buffers=buffers,
                                  max_batch_size=batch, max_simulations=case["sims"], tss_table_entries=1 << 16, node_capacity=4096, edge_capacity=65536)
    pool = selfplay.GeneratorPool(cfg)
    gen = ref.Generator(olib, case)
    h = gen.h
    openings = [ref.opening(olib, case, i) for i in range(rounds)]
    gen.begin(0)
    pool.begin(selfplay.pack_openings(openings))
    ev = teg._stand_in_evaluator(olib, hw)
    compared = [0] * rounds
    oracle_records = {}
    game = 0
    for step in range(6000):
        b = step % buffers
        if buffers == 2:
            pool.expand_backup_group(b, 2)
            pool.select_solve_group(b, 2)
            slots, feats = pool.scheduled_group(b, 2)
        else:
            pool.select_solve()
            slots, feats = pool.scheduled()
        order = np.argsort(slots)                       # thread-major, task order inside a thread: the oracle's queue order
        slots, feats = slots[order], feats[order]
        pol, val = ev(feats) if len(slots) else (np.zeros((0, hw), np.float32), np.zeros((0, 2), np.float32))
        pool.provide(slots, pol, np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32))
        f = np.zeros((threads * batch, hw), np.uint32)
        if buffers == 2:
            c = olib.ago_game_async_step(h, ol.ptr(f), threads * batch)
            if olib.ago_game_outcome(h) != 0:
                # the expand of this iteration ended the game: the device restarts inside the same advance stage and selects the next game's first
                # leaves in the same iteration — so does the generator (GAME_NOT_STARTED falls through to the select stage, GameGenerator.cpp:48-86)
                oracle_records[game] = ref.game_records(olib, h)
                game += 1
                if game == rounds:
                    assert len(slots) == 0, step
                    break
                gen.begin(game)
                c = olib.ago_game_async_step(h, ol.ptr(f), threads * batch)
        else:
            c = olib.ago_game_step_select(h, ol.ptr(f), threads * batch)
        assert c == len(slots), (step, game, c, len(slots))
        assert np.array_equal(feats, f[:c]), (step, game)
        if buffers == 2:
            olib.ago_game_async_provide(h, ol.ptr(np.ascontiguousarray(pol)), ol.ptr(np.ascontiguousarray(val)))
        else:
            olib.ago_game_step_expand(h, ol.ptr(np.ascontiguousarray(pol)), ol.ptr(np.ascontiguousarray(val)))
            pool.expand_backup()
            if olib.ago_game_outcome(h) != 0:
                oracle_records[game] = ref.game_records(olib, h)
                game += 1
                if game == rounds:
                    break
                gen.begin(game)
        info = pool.game_info(0)
        assert info["error"] == 0 and info["grow_pending"] == 0, step
        assert info["active"] and info["opening_id"] == game and info["games_done"] == game, (step, game, info["opening_id"], info["games_done"])
        assert info["n_moves"] == len(openings[game]) + olib.ago_game_num_records(h), (step, game)
        if info["root_edges"] == 0 and olib.ago_game_num_records(h) == 0:
            continue                                          # nothing expanded yet (the first iterations of a game)
        r = teg._oracle_root(olib, h)
        e = info["edges"]
        assert r["n"] == info["root_edges"] and r["visits"] == info["root_visits"], (step, game)
        assert np.array_equal(np.array([x["move"] for x in e], np.uint16), r["moves"]), (step, game)
        assert np.array_equal(np.array([x["visits"] for x in e], np.int32), r["ev"]), (step, game)
        assert np.array_equal(np.array([x["score"] for x in e], np.uint16), r["es"]), (step, game)
        assert np.array_equal(np.array([x["prior"] for x in e], np.float32), r["prior"]), (step, game)
        assert np.array_equal(np.array([[x["win"], x["draw"]] for x in e], np.float32).reshape(-1), r["val"]), (step, game)
        compared[game] += 1
    st = pool.stats()
    device = _device_records(pool)
    info = pool.game_info(0, with_edges=False)
    pool.close()
    gen.close()
    print("%s: roots compared per game %s, games finished %d, %.1f s" % (name, compared, st["games_finished"], time.time() - started))
    assert game == rounds and st["first_error"] == 0 and st["games_finished"] == rounds and info["games_done"] == rounds and not info["active"]
    assert all(c > 0 for c in compared), compared
    for k in range(rounds):
        _assert_same_records(device.get(k), oracle_records[k], k)
