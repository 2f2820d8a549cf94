"""The pair log of a match pool (agx_engine_match_track_pairs / agx_engine_match_pair_results, k_match_pair_log) against the pool's own move
records, and what is built on it: evaluation.play_matches(stop=...) and tuning.tune.

Shape: freestyle 15x15, 3 pairs, 6 openings (two rounds: every pair logs twice, the rounds interleave across pairs), draw_after 40, a 1x64
synthetic network for both players.  The two players differ so that not every opening ends 2-2: 50 playouts (the pool's) against 100 playouts
with exploration constant 0.5 — on these openings the six results are 1, 1, 2, 3, 1, 2 points.  Budgets below 50 cannot be used: with a drawish root the move rule then asks for more visits than select ever reaches and the
game never moves (agx.h, AgxEngineConfig.max_simulations — a pool configured for 24 playouts finished 5 of the 12 games in 40 000 steps),
and agx_engine_set_player_search refuses them."""
import functools

import numpy as np
import pytest

from alphagomoku_amd import synthetic

pytestmark = pytest.mark.gpu
N = 15
PAIRS = 3
OPENINGS = 6
GAMES = 2 * OPENINGS
MAX_STEPS = 40000
SECOND_PLAYER = dict(max_simulations=100, exploration_constant=0.5)


def _config(**overrides):
    from alphagomoku_amd import selfplay
    base = dict(rules=0, board_size=N, draw_after=40, n_games=2 * PAIRS, max_batch_size=4, max_simulations=50, tss_max_positions=30,
                tss_table_entries=1 << 16, node_capacity=4096, edge_capacity=65536, match_mode=1)
    base.update(overrides)
    return selfplay.default_config(**base)


@functools.lru_cache(maxsize=None)
def _net():
    from alphagomoku_amd.networks import AGNetwork
    d = synthetic.net_desc(blocks=1, filters=64)
    net = AGNetwork(d)
    net.loadWeights(synthetic.make_weights(d, seed=1234)[0])
    return net


@functools.lru_cache(maxsize=None)
def _openings():
    return tuple(tuple(o) for o in synthetic.make_openings(N, OPENINGS, seed0=912))


def _points(outcome, game_index):
    """the first player's points of one game: it plays cross in a pair's even games (outcome 1 draw, 2 cross won, 3 circle won)"""
    if outcome == 1:
        return 1
    return 2 if outcome == (2 if game_index % 2 == 0 else 3) else 0


@functools.lru_cache(maxsize=None)
def _run(merged, speculative, capacity):
    """all 12 games on one pool (capacity 0: no tracking): the move records, the summary, the per-pair results and the pair log"""
    from alphagomoku_amd import selfplay
    net = _net()
    pool = selfplay.GeneratorPool(_config(speculative_solver=speculative))
    pool.set_player_search(1, **SECOND_PLAYER)
    if capacity:
        pool.track_pairs(capacity)
    pool.begin(selfplay.pack_openings([list(o) for o in _openings()]))
    steps = 0
    while steps < MAX_STEPS:
        for _ in range(25):
            if merged:
                pool.step_match(net, net)
            else:
                pool.step_match_groups(net, net)
        steps += 25
        if pool.match_summary()["games"] >= GAMES:
            break
    out = dict(steps=steps, summary=pool.match_summary(), results=pool.match_results().tolist(), stats=pool.stats())
    recs, edges = pool.records()
    out["records"] = sorted((r.game_slot, r.game_index, r.move_number, r.game_serial, r.move, r.root_score, r.root_visits, r.root_win, r.root_draw, r.root_flags,
                             r.outcome, b"".join(bytes(e) for e in edges[r.edge_offset:r.edge_offset + r.n_edges])) for r in recs)
    if capacity:
        entries, totals = pool.pair_results()
        out["log"] = [tuple(int(x) for x in e) for e in entries]          # (pair, round, points, launch)
        out["totals"] = totals
        out["beyond"] = len(pool.pair_results(first=OPENINGS - 1 if capacity < OPENINGS else OPENINGS)[0])
        out["direct"] = [_direct_read(pool, first, 4) for first in (OPENINGS - 1, OPENINGS, OPENINGS + 1)]
    pool.close()
    return out


def _direct_read(pool, first, room):
    """agx_engine_match_pair_results with a buffer of `room` entries from `first` on, past the wrapper's own clamping: the buffer (filled
    with -1 beforehand) as tuples"""
    import ctypes
    from alphagomoku_amd import selfplay, lib, check
    out = np.zeros(room, selfplay.PAIR_RESULT_DTYPE)
    for name in out.dtype.names:
        out[name] = -1
    totals = (ctypes.c_longlong * 8)()
    check(lib.agx_engine_match_pair_results(pool._h, first, out.ctypes.data_as(ctypes.c_void_p), room, totals, None))
    return [tuple(int(x) for x in e) for e in out]


def _points_from_records(records):
    points = {}
    for slot, game_index, _, _, _, _, _, _, _, _, outcome, _ in records:
        if outcome != 0:
            key = (slot % PAIRS, game_index // 2)
            points.setdefault(key, []).append(_points(outcome, game_index))
    assert all(len(v) == 2 for v in points.values())                      # one last move per game, two games per opening
    return {k: sum(v) for k, v in points.items()}


@pytest.mark.parametrize("merged,speculative", [(True, 0), (True, 1), (False, 0), (False, 1)])
def test_log_against_the_records(agx_lib, merged, speculative):
    """every (pair, round)'s points in the log are what the last moves of its two games say; the log is sorted by (launch, pair) and a
    pair's rounds ascend; histogram, count, flags and the per-pair sums agree with match_results"""
    run = _run(merged, speculative, 16)
    assert run["summary"]["games"] == GAMES and run["stats"]["first_error"] == 0, run["steps"]
    want = _points_from_records(run["records"])
    log = run["log"]
    print("merged %d speculative %d: %d steps, log %s" % (merged, speculative, run["steps"], log))
    assert len(want) == OPENINGS and {(p, r): pts for p, r, pts, _ in log} == want and len(log) == OPENINGS
    assert [(e[3], e[0]) for e in log] == sorted((e[3], e[0]) for e in log)
    for pair in range(PAIRS):
        assert [e[1] for e in log if e[0] == pair] == [0, 1]
        won, drawn, lost, done = run["results"][pair]
        assert sum(e[2] for e in log if e[0] == pair) == 2 * won + drawn and done == 4 and won + drawn + lost == 4
    totals = run["totals"]
    assert totals["histogram"] == [sum(1 for e in log if e[2] == k) for k in range(5)] and totals["results"] == OPENINGS and totals["flags"] == 0
    # one log launch per advance launch: one per merged step, two per group-stepped one; an entry's launch is one of them
    assert totals["launches"] == run["steps"] * (1 if merged else 2) and all(0 <= e[3] < totals["launches"] for e in log)
    assert run["beyond"] == 0
    # the C call with room for 4 entries: from the last entry on it writes that one, from the log's end on nothing at all
    untouched = (-1, -1, -1, -1)
    assert run["direct"][0] == [log[-1]] + [untouched] * 3 and run["direct"][1] == [untouched] * 4 and run["direct"][2] == [untouched] * 4
    assert any(pts != 2 for pts in want.values())                         # the players differ: not every opening is shared 2-2


@pytest.mark.parametrize("merged", [True, False])
def test_tracking_changes_nothing_else(agx_lib, merged):
    """merged: one log launch per step; group-stepped: two"""
    tracked, plain = _run(merged, 0, 16), _run(merged, 0, 0)
    assert len(plain["records"]) > GAMES and plain["records"] == tracked["records"]
    assert plain["summary"] == tracked["summary"] and plain["results"] == tracked["results"] and plain["steps"] == tracked["steps"]


def test_overflow(agx_lib):
    full, short = _run(True, 0, 16), _run(True, 0, 1)
    assert short["log"] == full["log"][:1]
    assert short["totals"]["results"] == OPENINGS and short["totals"]["histogram"] == full["totals"]["histogram"] and short["totals"]["flags"] == 1
    assert short["beyond"] == 0 and short["records"] == full["records"]
    assert short["direct"] == [[(-1, -1, -1, -1)] * 4] * 3                 # (first 5, 6, 7 on a log of one entry)


def test_life_cycle(agx_lib):
    from alphagomoku_amd import selfplay, AgxError
    net = _net()
    packed = selfplay.pack_openings([list(o) for o in _openings()])
    plain = selfplay.GeneratorPool(selfplay.default_config(n_games=4, max_simulations=50, tss_table_entries=1 << 12, node_capacity=1024, edge_capacity=16384))
    with pytest.raises(AgxError, match="agx error 4: .*match_mode"):
        plain.track_pairs(8)
    plain.begin(selfplay.pack_openings([[], [], [], []]))
    with pytest.raises(AgxError, match="agx error 4: .*match_mode"):
        plain.pair_results()
    plain.close()

    untracked = selfplay.GeneratorPool(_config())
    untracked.begin(packed)
    with pytest.raises(AgxError, match="agx error 4: .*track"):
        untracked.pair_results()
    with pytest.raises(AgxError, match="agx error 4: .*before agx_engine_begin"):
        untracked.track_pairs(8)
    untracked.close()

    pool = selfplay.GeneratorPool(_config())
    for capacity in (0, -3):
        with pytest.raises(AgxError, match="agx error 1: .*capacity"):
            pool.track_pairs(capacity)
    pool.track_pairs(8)
    with pytest.raises(AgxError, match="agx error 4: .*already"):
        pool.track_pairs(8)
    with pytest.raises(AgxError, match="agx error 4: .*agx_engine_begin"):
        pool.pair_results()
    pool.begin(packed)
    with pytest.raises(AgxError, match="agx error 1"):
        pool.pair_results(first=-1)
    entries, totals = pool.pair_results()
    assert len(entries) == 0 and totals == dict(histogram=[0] * 5, results=0, flags=0, launches=0)
    steps = 0
    while steps < MAX_STEPS and totals["results"] == 0:
        for _ in range(25):
            pool.step_match(net, net)
        steps += 25
        entries, totals = pool.pair_results()
    assert totals["results"] >= 1 and len(entries) == totals["results"] and totals["launches"] == steps
    pool.begin(packed)                                                     # a second begin: an empty log, the totals at zero
    entries, totals = pool.pair_results()
    assert len(entries) == 0 and totals == dict(histogram=[0] * 5, results=0, flags=0, launches=0)
    for _ in range(10):
        pool.step_match(net, net)
    assert pool.pair_results()[1]["launches"] == 10 and pool.stats()["first_error"] == 0
    pool.close()


class _AfterTwo:
    """decides once it has seen two results; remembers what it was fed"""

    def __init__(self):
        self.status, self.seen = -1, []

    def add_result(self, points):
        self.seen.append(points)
        if len(self.seen) >= 2:
            self.status = 1


def test_play_matches_with_a_stop_rule(agx_lib):
    from alphagomoku_amd import evaluation
    from alphagomoku_amd.tuning import GSPRT
    net, openings = _net(), [list(o) for o in _openings()]
    full = _run(True, 0, 16)                                               # the same pool stepped the same way: its log is the whole sequence
    sequence = [e[2] for e in full["log"]]
    rule, poll = _AfterTwo(), 20
    out = evaluation.play_matches(_config(), net, net, openings, second=SECOND_PLAYER, stop=rule, poll_every=poll, max_steps=MAX_STEPS)
    second_launch = full["log"][1][3]                                      # (merged stepping: log launch k is step k + 1's)
    assert out["steps"] == poll * (second_launch // poll + 1)              # the first poll that had two results
    assert rule.seen == out["pair_sequence"] == sequence[:len(rule.seen)] and 2 <= len(rule.seen) < OPENINGS
    assert out["status"] == 1 and out["stopped_early"] and out["games"] < GAMES and "llr" not in out
    assert out["pair_histogram"] == [rule.seen.count(k) for k in range(5)]

    out = evaluation.play_matches(_config(), net, net, openings, second=SECOND_PLAYER, stop=GSPRT(), poll_every=poll, max_steps=MAX_STEPS)
    fresh = GSPRT()
    for points in out["pair_sequence"]:
        fresh.add_result(points)
    assert out["pair_sequence"] == sequence and out["llr"] == fresh.llr and out["status"] == fresh.status == -1 and not out["stopped_early"]
    assert {k: out[k] for k in ("wins", "draws", "losses", "games")} == full["summary"]

    out = evaluation.play_matches(_config(), net, net, openings, second=SECOND_PLAYER, poll_every=poll, max_steps=MAX_STEPS)
    assert set(out) == {"wins", "draws", "losses", "games", "steps", "players", "score", "elo", "elo_low", "elo_high"}
    assert {k: out[k] for k in ("wins", "draws", "losses", "games")} == full["summary"]


def test_tune(agx_lib):
    """two SPSA iterations on exploration_constant, two pairs each: the history obeys the update formula with the gradient of the observed
    histograms, and a second run with the same seed repeats it exactly (the pool plays the same games run to run)"""
    from alphagomoku_amd import tuning
    net, openings = _net(), [list(o) for o in _openings()]
    parameter = tuning.Parameter("exploration_constant", 0.5, 2.5)

    def run():
        return tuning.tune(_config(), net, [parameter], openings, iterations=2, pairs_per_iteration=2, seed=7, poll_every=20,
                           max_steps=MAX_STEPS)
    out = run()
    theta = [0.5]
    for k, h in enumerate(out["history"]):
        c_k, a_k = 0.1 / (k + 1) ** 0.101, 1.1 / (k + 1 + 2 / 10.0) ** 0.602
        assert h["theta"] == theta and h["c_k"] == c_k and h["a_k"] == a_k and h["delta"] in ([1.0], [-1.0])
        assert sum(h["histogram"]) == 2 and h["g"] == tuning.gradient_of(h["histogram"])
        plus, minus = min(1.0, theta[0] + c_k * h["delta"][0]), max(0.0, theta[0] - c_k * h["delta"][0])
        assert h["first"]["exploration_constant"] == parameter.value(plus) and h["second"]["exploration_constant"] == parameter.value(minus)
        theta = [float(np.clip(theta[0] + a_k * h["g"] / (2.0 * c_k * h["delta"][0]), 0.0, 1.0))]
        assert h["theta_after"] == pytest.approx(theta, rel=1e-15)
        theta = h["theta_after"]
    assert len(out["history"]) == 2 and out["theta"] == theta and out["settings"] == dict(exploration_constant=parameter.value(theta[0]))
    print("tune:", [(h["histogram"], h["g"], h["theta_after"]) for h in out["history"]])
    again = run()
    assert again["history"] == out["history"] and again["theta"] == out["theta"]
