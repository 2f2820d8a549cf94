"""Evaluation matches on the device between two players with search settings of their own (agx_engine_set_player_search), held against
the CPU oracle bit for bit: the oracle side is two handles per pair, each created from its own AgoSearchConfig (tests/match_players_ref.py).
Also: 'pv' against 'pvq' players, the defaults' identity, agx_engine_match_summary / evaluation.play_matches and the error behaviour."""
import ctypes

import numpy as np
import pytest

import match_players_ref as ref
import oracle_lib as ol
from alphagomoku_amd import synthetic

pytestmark = pytest.mark.gpu
N = 15
HW = N * N
PAIRS = 2


@pytest.fixture(scope="module")
def olib():
    return ol.load()


def _match_config(rules=0, pairs=PAIRS, **overrides):
    from alphagomoku_amd import selfplay
    base = dict(rules=rules, board_size=N, draw_after=60, n_games=2 * pairs, max_batch_size=ref.POOL_BATCH, max_simulations=60,
                tss_max_positions=ref.POOL_TSS, tss_table_entries=ref.TABLE_ENTRIES, node_capacity=4096, edge_capacity=65536, match_mode=1)
    base.update(overrides)
    return selfplay.default_config(**base)


def _same_settings(reported, wanted):
    return all(np.float32(reported[k]) == np.float32(v) for k, v in wanted.items())


def _play_and_compare(olib, rules, merged, speculative, settings, pool_action_values=0, max_steps=4000):
    """_play_matches_and_compare of tests/test_engine_gpu.py with a configuration per player: after every half-step the features of every
    scheduled leaf and the searching tree's root edges (moves, visits, scores, priors, values) are compared bit for bit.  Returns
    (roots compared, results, peak root visits per player of the compared roots that player's search has just grown, stats)."""
    from alphagomoku_amd import selfplay
    batch = ref.POOL_BATCH
    pool = selfplay.GeneratorPool(_match_config(rules, speculative_solver=speculative, action_values=pool_action_values))
    assert (pool.speculative_waves() > 0) == bool(speculative)
    for p in (0, 1):
        pool.set_player_search(p, **settings[p])
        assert _same_settings(pool.player_search(p), settings[p])
    openings = ref.prepare_openings(olib, rules, N, [500, 501])
    matches = ref.OracleMatches(olib, rules, N, 60, PAIRS, openings, settings)
    evaluators = [ref.first_evaluator(olib, HW), ref.second_evaluator(olib, HW)]
    pool.begin(selfplay.pack_openings(openings))
    matches.restart_waiting()
    compared, peak = 0, [0, 0]
    # merged: every stage one launch over both players' trees (agx_engine_step_match); else two group steps one after the other
    phases = [(0, 1)] if merged else [(0,), (1,)]
    for step in range(max_steps):
        for phase in phases:
            if merged:
                pool.select_solve_match()
            else:
                pool.select_solve_group(phase[0], 2)
            by_slot = {}
            all_slots, all_pol, all_val, all_q = [], [], [], []
            for player in phase:
                slots, feats = pool.scheduled_group(player, 2)
                pol, val = evaluators[player](feats[:len(slots)])
                q = ref.stand_in_q(feats[:len(slots)], HW)    # (also handed to a 'pv' player's slots: the device must not read it there)
                for i, sl in enumerate(slots):
                    assert (int(sl) // batch >= PAIRS) == (player == 1)      # each player's list holds only its own trees' leaves
                    by_slot[int(sl)] = (feats[i], pol[i], val[i], q[i])
                all_slots.append(slots)
                all_pol.append(pol)
                all_val.append(val)
                all_q.append(q)
            slots, pol, val, q = np.concatenate(all_slots), np.concatenate(all_pol), np.concatenate(all_val), np.concatenate(all_q)
            v3 = np.concatenate([val, 1 - val.sum(1, keepdims=True)], 1).astype(np.float32)
            pool.provide(slots, pol, v3, q if pool_action_values else None)
            seen = 0
            searched = [False] * PAIRS       # pairs whose tree to move searched in this half-step and goes on searching (it did not move)
            for m, who in enumerate(list(matches.mover)):
                if who is None or who not in phase:
                    continue
                tree = m + who * PAIRS
                c, f = matches.select(m, who)
                mine = sorted(sl for sl in by_slot if sl // batch == tree)    # (a player's leaves sit at the POOL's stride whatever its own batch size)
                assert c == len(mine) and c <= settings[who]["max_batch_size"], (step, phase, m)
                assert np.array_equal(np.array([by_slot[sl][0] for sl in mine], np.uint32).reshape(c, HW), f[:c]), (step, phase, m)
                seen += c
                moved = matches.expand(m, who, np.array([by_slot[sl][1] for sl in mine], np.float32).reshape(c, HW),
                                       np.array([by_slot[sl][2] for sl in mine], np.float32).reshape(c, 2),
                                       np.array([by_slot[sl][3] for sl in mine], np.float32).reshape(c, HW, 2))
                searched[m] = not moved
            assert seen == len(slots), (step, phase)      # idle trees schedule nothing
            if merged:
                pool.expand_backup_match()
            else:
                pool.expand_backup_group(phase[0], 2)
            if merged or phase[0] == 0:
                matches.restart_waiting()
            for m in range(PAIRS):
                who = matches.mover[m]
                infos = [pool.game_info(m), pool.game_info(m + PAIRS)]
                assert infos[0]["error"] == 0 and infos[1]["error"] == 0
                if who is None:
                    assert not infos[0]["active"] and not infos[1]["active"], (step, phase, m)
                    continue
                info = infos[who]
                assert info["active"] and not infos[1 - who]["active"], (step, phase, m)   # exactly the player to move searches
                assert info["opening_id"] == matches.opening_of[m] and info["games_done"] == matches.games_done[m], (step, phase, m)
                r = matches.root(m, who)
                e = info["edges"]
                assert r["n"] == info["root_edges"] and r["visits"] == info["root_visits"], (step, phase, m)
                assert np.array_equal(np.array([x["move"] for x in e], np.uint16), r["moves"]), (step, phase, m)
                assert np.array_equal(np.array([x["visits"] for x in e], np.int32), r["ev"]), (step, phase, m)
                assert np.array_equal(np.array([x["score"] for x in e], np.uint16), r["es"]), (step, phase, m)
                assert np.array_equal(np.array([x["prior"] for x in e], np.float32), r["prior"]), (step, phase, m)
                assert np.array_equal(np.array([[x["win"], x["draw"]] for x in e], np.float32).reshape(-1), r["val"]), (step, phase, m)
                # the budget shows in the roots a player's OWN search has grown, as in tests/test_match_players_cpu.py.  (A root that has just
                # received the opponent's move carries what earlier searches of this persistent tree left on that node — over several
                # searches, through transpositions, that can exceed one search's budget: 69 visits for a 60-playout player here, in the
                # oracle and on the device alike — and such a player moves at once without searching.  Those roots are compared, not counted.)
                if searched[m]:
                    peak[who] = max(peak[who], info["root_visits"])
                compared += 1
        if matches.all_played():
            break
    stats = pool.stats()
    summary = pool.match_summary()
    pool.close()
    results = list(matches.results)
    matches.close()
    # the pool's own score of the finished games is the oracle's: outcome 2 = cross won; the first player plays cross in a pair's even games
    first_won = sum(1 for _, _, k, outcome in results if outcome == (2 if k == 0 else 3))
    drawn = sum(1 for _, _, _, outcome in results if outcome == 1)
    assert summary == dict(wins=first_won, draws=drawn, losses=len(results) - first_won - drawn, games=len(results))
    return compared, results, peak, stats


@pytest.mark.parametrize("rules,merged,speculative,swapped", [(0, False, 0, False), (1, True, 1, False), (2, True, 0, False), (0, True, 1, True)])
def test_players_with_their_own_settings_bit_exact(agx_lib, olib, rules, merged, speculative, swapped):
    """player A (60 playouts, batch 4, the defaults) against player B (100 playouts, batch 8, c 0.8 + 0.25 log, init_to loss, leak threshold
    1, 20 children, solver budget 30, max_visit, temperature 0.5), each tree against an oracle player of ITS configuration: group-stepped
    (the host writes the player's values into the launch's arguments) and merged (the kernels choose by tree), serial and speculative
    solver, and with the roles swapped.

    Every root is compared bit for bit.  The two visit bounds (B reaches >= 90, A stays <= 60 + 4) are taken over the roots a player's own
    search has just grown — the roots tests/test_match_players_cpu.py measures on the oracle alone.  A root that has just received the
    opponent's move is left out of the bounds: it carries what earlier searches of the persistent tree left on that node, which through
    transpositions can exceed one search's budget (69 visits for the 60-playout player in the standard-rules case, in the oracle and on
    the device alike; such a player moves at once without searching)."""
    settings = [ref.PLAYER_B, ref.PLAYER_A] if swapped else [ref.PLAYER_A, ref.PLAYER_B]
    compared, results, peak, stats = _play_and_compare(olib, rules, merged, speculative, settings)
    a, b = (1, 0) if swapped else (0, 1)
    print("rules %d merged %d speculative %d swapped %d: %d roots compared, peak root visits A %d B %d" % (rules, merged, speculative, swapped, compared, peak[a], peak[b]))
    assert len(results) == 4 and stats["games_finished"] == 4          # 2 openings x 2 colour assignments
    assert compared > 100
    assert peak[b] >= 90                                               # B's trees really search with B's budget ...
    assert peak[a] <= ref.PLAYER_A["max_simulations"] + ref.PLAYER_A["max_batch_size"]   # ... and A's with A's


def test_pv_player_against_pvq_player(agx_lib, olib):
    """a pool with the action-values exchange buffer whose first player is a 'pv' player (new edges start at (0, 0), the oracle's
    ago_game_step_expand) and whose second is a 'pvq' player (ago_game_step_expand_q); then the same with two real networks: the 'pv'
    network is accepted for the player that asks for no head and refused for the one that does"""
    from alphagomoku_amd import selfplay, AgxError
    from alphagomoku_amd.networks import AGNetwork
    settings = [dict(ref.PLAYER_A, action_values=0), dict(ref.PLAYER_A, max_simulations=80, max_batch_size=8, action_values=1)]
    compared, results, peak, stats = _play_and_compare(olib, 0, True, 0, settings, pool_action_values=1)
    assert len(results) == 4 and compared > 100 and peak[0] <= 64 < peak[1]

    d = synthetic.net_desc(blocks=2, filters=64, action_values=1)
    blob, _ = synthetic.make_weights(d)
    pvq = AGNetwork(d)
    pvq.loadWeights(blob)
    pv = AGNetwork(synthetic.net_desc(blocks=2, filters=64))
    pv.loadWeights(blob[:pv.blobFloats()])
    pool = selfplay.GeneratorPool(_match_config(0, action_values=1, max_simulations=50))
    assert pool.player_search(0)["action_values"] == 1 and pool.player_search(1)["action_values"] == 1   # the pool's configuration
    pool.set_player_search(0, action_values=0)
    pool.begin(selfplay.pack_openings(synthetic.make_openings(15, 2, seed0=3)))
    for _ in range(30):
        pool.step_match(pv, pvq)
    with pytest.raises(AgxError, match="agx error 1: .*action-values head"):
        pool.step_match(pvq, pv)                 # the second player asks for the head, this network has none
    seeded = False
    for _ in range(200):                         # until a second player's tree shows a root: its unvisited edges start from the 'q' output
        pool.step_match(pv, pvq)
        roots = [pool.game_info(g) for g in range(PAIRS, 2 * PAIRS)]
        seeded = any(e["visits"] == 0 and e["win"] != 0.0 for r in roots if r["active"] for e in r["edges"])
        if seeded:
            break
    assert seeded
    stats = pool.stats()
    assert stats["first_error"] == 0 and stats["moves_played"] > 0
    pool.close()
    pv.close()
    pvq.close()


def _two_networks():
    from alphagomoku_amd import networks
    nets = []
    for seed in (1234, 4321):
        d = synthetic.net_desc(blocks=2, filters=64)
        net = networks.AGNetwork(d)
        net.loadWeights(synthetic.make_weights(d, seed=seed)[0])
        nets.append(net)
    return nets


def _agx_openings(agx_lib, count, seed0=900):
    from alphagomoku_amd import selfplay
    openings = []
    for g in range(count):
        op = np.zeros(selfplay.OPENING_CAP, np.uint16)
        agx_lib.agx_make_opening(0, N, seed0 + g, op.ctypes.data_as(ctypes.c_void_p))
        openings.append([int(x) for x in op[1:1 + int(op[0])]])
    return openings


def test_setting_the_reported_values_changes_nothing(agx_lib):
    """both players set to what player_search reports: records, match results and statistics of 200 merged steps are those of an
    untouched pool"""
    from alphagomoku_amd import selfplay
    nets = _two_networks()
    openings = _agx_openings(agx_lib, 8)

    def run(touch):
        pool = selfplay.GeneratorPool(_match_config(0, pairs=4, max_simulations=50, max_children=30, final_selector=1, policy_temperature=0.75))
        before = [pool.player_search(p) for p in (0, 1)]
        assert before[0] == before[1] and before[0]["max_simulations"] == 50 and before[0]["max_batch_size"] == ref.POOL_BATCH
        assert before[0]["max_children"] == 30 and before[0]["final_selector"] == 1 and before[0]["policy_temperature"] == 0.75
        if touch:
            for p in (0, 1):
                pool.set_player_search(p, **before[p])
            assert [pool.player_search(p) for p in (0, 1)] == before
        pool.begin(selfplay.pack_openings(openings))
        for _ in range(200):
            pool.step_match(nets[0], nets[1])
        recs, edges = pool.records()
        # (the trees append their records in the order their workgroups get to it: a record is identified by tree, game and move number)
        moves = sorted((r.game_slot, r.game_index, r.move_number, r.game_serial, r.move, r.root_score, r.root_visits, r.root_win, r.root_draw, r.root_flags,
                        r.outcome, b"".join(bytes(e) for e in edges[r.edge_offset:r.edge_offset + r.n_edges])) for r in recs)
        out = (moves, pool.match_results().tolist(), pool.stats())
        pool.close()
        return out
    plain, touched = run(False), run(True)
    assert len(plain[0]) > 8 and plain[2]["moves_played"] == len(plain[0])
    assert plain == touched
    for net in nets:
        net.close()


def test_match_summary_and_play_matches(agx_lib):
    """agx_engine_match_summary == the column sums of match_results at three points of a run of two networks; evaluation.play_matches on
    the same inputs returns those totals"""
    from alphagomoku_amd import selfplay, evaluation
    pairs, n_openings = 8, 8
    nets = _two_networks()
    openings = _agx_openings(agx_lib, n_openings)
    cfg = _match_config(0, pairs=pairs, max_simulations=50)
    pool = selfplay.GeneratorPool(cfg)
    pool.begin(selfplay.pack_openings(openings))
    assert pool.match_summary() == dict(wins=0, draws=0, losses=0, games=0)
    checked, partly, final = 0, 0, None
    for step in range(1, 6001):
        pool.step_match(nets[0], nets[1])
        if step % 50 == 0:
            summary, res = pool.match_summary(), pool.match_results()
            assert [summary["wins"], summary["draws"], summary["losses"], summary["games"]] == [int(x) for x in res.sum(0)], step
            checked += 1
            partly += 1 if 0 < summary["games"] < 2 * n_openings else 0
            if summary["games"] == 2 * n_openings:
                final = summary
                break
    assert checked >= 3 and partly >= 1 and final is not None      # (also at points where some pairs have finished games and others have not)
    assert final["wins"] + final["draws"] + final["losses"] == final["games"]
    pool.close()
    out = evaluation.play_matches(cfg, nets[0], nets[1], openings)
    assert {k: out[k] for k in ("wins", "draws", "losses", "games")} == final and out["games"] == 2 * n_openings
    assert out["players"][0] == out["players"][1] and out["players"][0]["max_simulations"] == 50
    assert out["score"] == (final["wins"] + 0.5 * final["draws"]) / final["games"] and out["elo_low"] <= out["elo"] <= out["elo_high"]
    # ... and with settings of their own the players are the ones asked for
    out = evaluation.play_matches(cfg, nets[0], nets[0], openings[:1], first=dict(max_simulations=50, max_batch_size=4),
                                  second=dict(max_simulations=100, exploration_constant=0.8))
    assert out["games"] == 2 and out["players"][0]["max_batch_size"] == 4 and out["players"][1]["max_simulations"] == 100
    assert out["players"][1]["exploration_constant"] == np.float32(0.8) and out["players"][0]["exploration_constant"] == 1.25
    for net in nets:
        net.close()


BAD_SETTINGS = [(dict(max_simulations=49), "max_simulations"), (dict(max_batch_size=0), "max_batch_size"), (dict(max_batch_size=ref.POOL_BATCH + 1), "max_batch_size"),
                (dict(init_to=-1), "init_to"), (dict(init_to=4), "init_to"), (dict(tss_max_positions=0), "tss_max_positions"),
                (dict(tss_max_positions=ref.POOL_TSS + 1), "tss_max_positions"), (dict(final_selector=-1), "final_selector"), (dict(final_selector=6), "final_selector"),
                (dict(policy_temperature=-0.5), "policy_temperature"), (dict(action_values=2), "action_values"), (dict(action_values=-1), "action_values"),
                (dict(action_values=1), "action_values")]   # (the pool below has no action-values exchange buffer)


def test_player_search_errors(agx_lib):
    """every range of AgxPlayerSearch, the player index, null arguments and a pool without match_mode: a status and a message that names the
    field; nothing changes and the pool steps on"""
    from alphagomoku_amd import selfplay, AgxError
    from alphagomoku_amd._lib import AgxPlayerSearch
    nets = _two_networks()
    pool = selfplay.GeneratorPool(_match_config(0, max_simulations=50))
    pool.set_player_search(1, **ref.PLAYER_B)
    before = [pool.player_search(0), pool.player_search(1)]
    with pytest.raises(AgxError, match="agx error 4"):
        pool.match_summary()                                   # before begin()
    pool.begin(selfplay.pack_openings(_agx_openings(agx_lib, 2)))

    def still_fine():
        assert [pool.player_search(0), pool.player_search(1)] == before
        pool.step_match(nets[0], nets[1])
        pool.step_match_groups(nets[0], nets[1])
    for fields, name in BAD_SETTINGS:
        for player in (0, 1):
            with pytest.raises(AgxError, match="agx error 1: agx_engine_set_player_search: .*" + name):
                pool.set_player_search(player, **fields)
        still_fine()
    for player in (-1, 2):
        with pytest.raises(AgxError, match="agx error 1: .*player must be 0"):
            pool.player_search(player)
        with pytest.raises(AgxError, match="agx error 1: .*player must be 0"):
            pool.set_player_search(player, max_simulations=80)
    with pytest.raises(KeyError):
        pool.set_player_search(0, noise_weight=0.25)           # pool-wide by decision: not a player's field
    p = AgxPlayerSearch()
    assert agx_lib.agx_engine_player_search(pool._h, 0, None) == 1 and agx_lib.agx_engine_set_player_search(pool._h, 0, None) == 1
    assert agx_lib.agx_engine_player_search(None, 0, ctypes.byref(p)) == 1 and agx_lib.agx_engine_match_summary(pool._h, None, None) == 1
    still_fine()
    # the pool-wide setters keep their meaning: both players, the last call wins
    pool.set_max_simulations(70)
    pool.set_batch_size(2)
    assert [pool.player_search(q)["max_simulations"] for q in (0, 1)] == [70, 70] and [pool.player_search(q)["max_batch_size"] for q in (0, 1)] == [2, 2]
    pool.set_player_search(1, max_simulations=90)
    assert [pool.player_search(q)["max_simulations"] for q in (0, 1)] == [70, 90]
    pool.step_match(nets[0], nets[1])
    assert pool.stats()["first_error"] == 0
    pool.close()

    plain = selfplay.GeneratorPool(selfplay.default_config(n_games=4, max_simulations=50, tss_table_entries=1 << 12, node_capacity=1024, edge_capacity=16384))
    plain.begin(selfplay.pack_openings([[], [], [], []]))
    for call in (lambda: plain.player_search(0), lambda: plain.set_player_search(0, max_simulations=80), lambda: plain.match_summary()):
        with pytest.raises(AgxError, match="agx error 4: .*match_mode"):
            call()
    plain.step(nets[0])                                        # a self-play pool is what it was
    assert plain.stats()["first_error"] == 0
    plain.close()
    for net in nets:
        net.close()
