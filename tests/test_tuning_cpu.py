"""alphagomoku_amd.tuning (GSPRT, SPSA, Parameter) against their formulas, evaluated independently here in float64, and the host logic of
evaluation.play_matches(stop=...) / evaluation.gate on a stub pool.  No device."""
import math

import numpy as np
import pytest

from alphagomoku_amd import evaluation, selfplay, tuning
from alphagomoku_amd.tuning import GSPRT, SPSA, Parameter

LN10 = math.log(10.0)


def _llr(r, elo0, elo1):
    """the specification, written out on its own"""
    n = float(sum(r))
    p = [max(1e-3, float(x)) / n for x in r]
    s = [i / 4.0 for i in range(5)]
    mu = sum(s[i] * p[i] for i in range(5))
    var = sum(p[i] * (s[i] - mu) ** 2 for i in range(5))
    t = (mu - 0.5) / math.sqrt(2.0 * var)
    t0, t1 = elo0 * LN10 / 800.0, elo1 * LN10 / 800.0
    return n * math.log((1.0 + (t - t0) ** 2) / (1.0 + (t - t1) ** 2))


def _feed(test, histogram):
    for points, count in enumerate(histogram):
        for _ in range(count):
            test.add_result(points)
    return test


HISTOGRAMS = [[5, 0, 0, 0, 0], [0, 0, 7, 0, 0], [0, 0, 0, 0, 9], [1, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 3, 0, 4, 0], [2, 0, 5, 0, 1], [0, 1, 10, 3, 0],
              [4, 9, 30, 12, 6], [120, 410, 900, 455, 140]]


@pytest.mark.parametrize("histogram", HISTOGRAMS)
@pytest.mark.parametrize("elos", [(0.0, 5.0), (-3.0, 12.0)])
def test_llr_is_the_stated_expression(histogram, elos):
    """all in one bin, a single result, zeros lifted by the 1e-3 floor, and filled histograms: the same float64 expression on both sides,
    so the two agree to the bit"""
    got = _feed(GSPRT(elos[0], elos[1]), histogram)
    want = _llr(histogram, *elos)
    assert got.results == histogram and math.isfinite(want)
    assert got.llr == want
    assert tuning.pair_llr(histogram, *elos) == want


@pytest.mark.parametrize("histogram", [[1, 1, 1, 1, 1], [2, 5, 11, 5, 2], [7, 3, 20, 3, 7], [120, 400, 900, 400, 120]])
def test_symmetric_histograms(histogram):
    """mean exactly 1/2, t = 0: n ln((1 + t0^2) / (1 + t1^2)) exactly.  (Every bin filled: an empty bin is lifted to 1e-3 results without
    the others giving anything up, so the p_i then add up to more than 1 and the mean of a symmetric histogram is 1/2 of that sum, not 1/2.)"""
    n = sum(histogram)
    for elo0, elo1 in [(0.0, 5.0), (-2.0, 8.0)]:
        t0, t1 = elo0 * LN10 / 800.0, elo1 * LN10 / 800.0
        assert _feed(GSPRT(elo0, elo1), histogram).llr == n * math.log((1.0 + t0 ** 2) / (1.0 + t1 ** 2))


def test_bounds():
    for alpha, beta in [(0.05, 0.05), (0.01, 0.1)]:
        lower, upper = GSPRT(alpha=alpha, beta=beta).bounds()
        assert lower == math.log(beta / (1.0 - alpha)) and upper == math.log((1.0 - beta) / alpha)
    lower, upper = GSPRT().bounds()
    assert abs(lower + math.log(19.0)) < 1e-12 and abs(upper - math.log(19.0)) < 1e-12
    for bad in (dict(alpha=0.0), dict(beta=1.0), dict(alpha=0.6, beta=0.5), dict(elo0=5.0, elo1=5.0)):
        with pytest.raises(ValueError):
            GSPRT(**bad)
    with pytest.raises(ValueError):
        GSPRT().add_result(5)


def test_overshoot_terms_replayed_by_hand():
    sequence = [3, 2, 4, 1, 0, 2, 1, 0, 3, 4, 4, 3]
    test = GSPRT(0.0, 40.0)
    r, hi, lo, sq1, sq0, o1, o0 = [0] * 5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    new_max = new_min = 0
    for points in sequence:
        r[points] += 1
        llr = _llr(r, 0.0, 40.0)
        if llr > hi:
            sq1 += (llr - hi) ** 2
            hi = llr
            o1 = sq1 / (2.0 * llr)
            new_max += 1
        if llr < lo:
            sq0 += (llr - lo) ** 2
            lo = llr
            o0 = -sq0 / (2.0 * llr)
            new_min += 1
        test.add_result(points)
        assert (test.sq1, test.sq0, test.o1, test.o0) == pytest.approx((sq1, sq0, o1, o0), rel=1e-12, abs=0.0)
        assert test.bounds() == pytest.approx((math.log(0.05 / 0.95) + o0, math.log(0.95 / 0.05) - o1), rel=1e-12)
    assert new_max >= 2 and new_min >= 2 and o1 > 0.0 and o0 > 0.0      # both corrections were exercised; both narrow the bounds


def test_a_decision_is_never_overwritten():
    test = GSPRT(0.0, 100.0)
    for k in range(40):
        test.add_result(3 if k % 2 == 0 else 2)
        if test.status >= 0:
            break
    assert test.status == 1 and test.llr > test.bounds()[1]
    decided_at = sum(test.results)
    for _ in range(200):
        test.add_result(0)                                         # evidence for the other side, enough to cross the lower bound
    assert test.llr < test.bounds()[0] and test.status == 1 and sum(test.results) == decided_at + 200


P_ELO0 = [0.05, 0.2, 0.5, 0.2, 0.05]
P_ELO1 = [0.045450058844668254, 0.2, 0.5, 0.2, 0.054549941155331746]     # normalised Elo 5
STREAM_SEED, STREAM_LENGTH = 0, 20000


def _normalised_elo(p):
    mu = sum(i / 4.0 * p[i] for i in range(5))
    var = sum(p[i] * (i / 4.0 - mu) ** 2 for i in range(5))
    return (mu - 0.5) / math.sqrt(2.0 * var) * 800.0 / LN10


def _stream(p):
    rng = np.random.default_rng(STREAM_SEED)
    return np.searchsorted(np.cumsum(p), rng.random(STREAM_LENGTH), side="right").clip(0, 4)


def test_seeded_streams_end_where_they_were_drawn():
    assert abs(_normalised_elo(P_ELO1) - 5.0) < 1e-9 and _normalised_elo(P_ELO0) == 0.0
    for p, decision in ((P_ELO1, 1), (P_ELO0, 0)):
        test, used = GSPRT(0.0, 5.0, 0.05, 0.05), 0
        for points in _stream(p):
            used += 1
            if test.add_result(int(points)) >= 0:
                break
        assert test.status == decision and 1000 < used < STREAM_LENGTH


# ---- SPSA ----
def test_two_steps_against_the_formulas():
    target = np.array([0.8, 0.3, 0.55])

    def f(theta):
        return -float(((theta - target) ** 2).sum())
    opt = SPSA(3, seed=11)
    check_rng = np.random.default_rng(11)
    deltas = np.array([2.0 * check_rng.integers(0, 2, 3) - 1.0 for _ in range(2)])
    theta = np.full(3, 0.5)
    for k in range(2):
        c_k = 0.1 / (k + 1) ** 0.101
        a_k = 1.1 / (k + 1 + 40 / 10.0) ** 0.602
        plus, minus = np.clip(theta + c_k * deltas[k], 0, 1), np.clip(theta - c_k * deltas[k], 0, 1)
        g = f(plus) - f(minus)
        got = opt.step(lambda p, m: f(p) - f(m), 40)
        theta = np.clip(theta + a_k * g / (2.0 * c_k * deltas[k]), 0, 1)
        assert got == g and opt.last["c_k"] == c_k and opt.last["a_k"] == a_k and np.array_equal(opt.last["delta"], deltas[k])
        assert np.array_equal(opt.last["theta_plus"], plus) and np.array_equal(opt.last["theta_minus"], minus)
        assert np.allclose(opt.theta, theta, rtol=1e-15, atol=0.0)
    assert set(np.abs(deltas).ravel()) == {1.0} and opt.step_count == 2


def test_clipping_at_0_and_1():
    opt = SPSA(2, theta=[0.02, 0.97], seed=3)
    seen = {}

    def gradient(plus, minus):
        seen.update(plus=plus.copy(), minus=minus.copy())
        return 50.0
    opt.step(gradient, 10)
    for v in (seen["plus"], seen["minus"], opt.theta):
        assert v.min() >= 0.0 and v.max() <= 1.0
    delta = opt.last["delta"]
    assert seen["plus"][1] == (1.0 if delta[1] > 0 else 0.97 - opt.last["c_k"]) and seen["minus"][0] == (0.0 if delta[0] > 0 else 0.02 + opt.last["c_k"])
    assert all(opt.theta[i] == (1.0 if delta[i] > 0 else 0.0) for i in range(2))       # a gradient of 50 leaves the cube in one step
    assert np.array_equal(SPSA(2, theta=[-1.0, 3.0]).theta, [0.0, 1.0])


def test_state_round_trip_and_seed():
    def gradient(plus, minus):
        return float(minus.sum() - plus.sum()) + 0.1

    def run(opt, steps):
        return [(opt.step(gradient, 30), opt.theta.tolist(), opt.last["delta"].tolist()) for _ in range(steps)]
    whole = run(SPSA(4, seed=5), 6)
    first = SPSA(4, seed=5)
    head = run(first, 3)
    state = first.state()
    assert set(state) == {"a", "c", "alpha", "gamma", "step", "theta", "rng"} and state["step"] == 3
    import json
    resumed = SPSA.from_state(json.loads(json.dumps(state)))      # plain values: survives a file
    assert head + run(resumed, 3) == whole                        # bit-identical continuation
    assert run(SPSA(4, seed=5), 6) == whole and run(SPSA(4, seed=6), 6) != whole
    with pytest.raises(ValueError):
        SPSA(0)
    with pytest.raises(ValueError):
        SPSA(2, theta=[0.5])


# ---- Parameter ----
def test_parameter_maps():
    lin = Parameter("exploration_constant", 0.5, 2.5)
    assert [lin.value(t) for t in (0.0, 0.5, 1.0)] == [0.5, 1.5, 2.5]
    log = Parameter("policy_expansion_threshold", 1e-5, 1e-1, log=True)
    assert log.value(0.0) == 1e-5 and log.value(1.0) == pytest.approx(1e-1, rel=1e-12) and log.value(0.5) == pytest.approx(1e-3, rel=1e-12)
    integer = Parameter("max_children", 10, 35, integer=True)
    assert [integer.value(t) for t in (0.0, 0.5, 1.0)] == [10, 23, 35] and isinstance(integer.value(0.5), int)      # 22.5 rounds to 23
    both = Parameter("tss_max_positions", 10, 1000, integer=True, log=True)
    assert [both.value(t) for t in (0.0, 0.5, 1.0)] == [10, 100, 1000]
    assert lin.value(-0.3) == 0.5 and lin.value(1.7) == 2.5
    assert tuning.settings_of([lin, integer], [0.5, 1.0]) == dict(exploration_constant=1.5, max_children=35)


def test_parameter_refusals():
    with pytest.raises(ValueError, match="noise_weight"):
        Parameter("noise_weight", 0.0, 1.0)                       # pool-wide, not a player's field
    with pytest.raises(ValueError):
        Parameter("exploration_constant", 2.0, 2.0)
    with pytest.raises(ValueError):
        Parameter("exploration_constant", 0.0, 2.0, log=True)
    assert tuning.gradient_of([0, 0, 0, 0, 3]) == 1.0 and tuning.gradient_of([2, 0, 0, 0, 0]) == -1.0 and tuning.gradient_of([1, 0, 2, 0, 1]) == 0.0
    assert tuning.gradient_of([0, 1, 1, 2, 0]) == 2.0 * (1 + 2 + 6) / 16.0 - 1.0
    with pytest.raises(ValueError):
        tuning.gradient_of([0, 0, 0, 0, 0])


# ---- play_matches / gate on a stub pool ----
GAMES_OF_POINTS = {4: (2, 0, 0), 3: (1, 1, 0), 2: (1, 0, 1), 1: (0, 1, 1), 0: (0, 0, 2)}


class StubPool:
    """a pool that finishes one opening every `every` steps with the next of `script`'s points"""
    script, every, flags, made = [], 3, 0, []

    def __init__(self, cfg):
        self.steps, self.capacity, self.reads = 0, None, []
        StubPool.made.append(self)

    def set_player_search(self, player, **fields):
        pass

    def player_search(self, player):
        return {}

    def track_pairs(self, capacity):
        self.capacity = capacity

    def begin(self, openings, stream=None):
        self.openings = len(openings)

    def step_match(self, first_net, second_net, stream=None):
        self.steps += 1

    def _finished(self):
        return min(self.steps // self.every, self.openings, len(self.script))

    def pair_results(self, first=0, stream=None):
        assert self.capacity is not None
        n = self._finished()
        self.reads.append((first, n))
        out = np.zeros(max(n - first, 0), selfplay.PAIR_RESULT_DTYPE)
        out["points"] = self.script[first:n]
        hist = [self.script[:n].count(k) for k in range(5)]
        return out, dict(histogram=hist, results=n, flags=self.flags, launches=self.steps)

    def match_summary(self, stream=None):
        won = [sum(GAMES_OF_POINTS[p][k] for p in self.script[:self._finished()]) for k in range(3)]
        return dict(wins=won[0], draws=won[1], losses=won[2], games=2 * self._finished())

    def stats(self):
        return dict(first_error=0)

    def close(self):
        pass


@pytest.fixture
def stub_pool(monkeypatch):
    monkeypatch.setattr(selfplay, "GeneratorPool", StubPool)
    StubPool.made = []
    StubPool.flags = 0
    return StubPool


def _config(match_mode=1):
    class Config:
        pass
    cfg = Config()
    cfg.match_mode = match_mode
    return cfg


def test_play_matches_arguments():
    with pytest.raises(ValueError, match="match_mode"):
        evaluation.play_matches(_config(0), None, None, [[1]], stop=GSPRT())
    with pytest.raises(ValueError, match="opening"):
        evaluation.play_matches(_config(1), None, None, [], stop=GSPRT())
    with pytest.raises(ValueError, match="add_result"):
        evaluation.play_matches(_config(1), None, None, [[1]], stop=object())
    with pytest.raises(ValueError, match="pair_capacity"):
        evaluation.play_matches(_config(1), None, None, [[1]], pair_capacity=4)


def test_stop_rule_sees_every_entry_once_in_order(stub_pool):
    stub_pool.script = [3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 3, 2, 4, 4, 4, 4]
    rule = GSPRT(0.0, 100.0)
    out = evaluation.play_matches(_config(), None, None, [[1]] * 16, stop=rule, poll_every=4)
    pool = stub_pool.made[-1]
    assert pool.capacity == 32
    fresh = GSPRT(0.0, 100.0)
    for points in out["pair_sequence"]:
        fresh.add_result(points)
    assert out["pair_sequence"] == stub_pool.script[:len(out["pair_sequence"])] and out["llr"] == fresh.llr == rule.llr and out["status"] == fresh.status == 1
    assert out["stopped_early"] and out["games"] == 2 * len(out["pair_sequence"]) < 32 and out["pair_histogram"] == rule.results
    assert [r[0] for r in pool.reads] == [0] + [n for _, n in pool.reads[:-1]]          # every read starts where the previous one ended
    assert out["steps"] % 4 == 0 and pool.reads[-1][1] == len(out["pair_sequence"])       # the loop ended at the poll that decided
    # without a rule the pool is not asked to track anything and the result has the old keys
    out = evaluation.play_matches(_config(), None, None, [[1]] * 4, poll_every=4)
    assert stub_pool.made[-1].capacity is None and stub_pool.made[-1].reads == []
    assert set(out) == {"wins", "draws", "losses", "games", "steps", "players", "score", "elo", "elo_low", "elo_high"} and out["games"] == 8
    # a run that max_steps cut off has not stopped early: nothing was decided
    out = evaluation.play_matches(_config(), None, None, [[1]] * 16, stop=GSPRT(), poll_every=4, max_steps=10)
    assert out["steps"] == 10 and out["status"] == -1 and 0 < out["games"] < 32 and out["stopped_early"] is False
    # a raised flag is an error, not a result
    from alphagomoku_amd import AgxError
    stub_pool.flags = 2
    with pytest.raises(AgxError, match="flags 2"):
        evaluation.play_matches(_config(), None, None, [[1]] * 4, stop=GSPRT(), poll_every=4)


@pytest.mark.parametrize("script,elo1,status,passed", [
    ([3, 2] * 8, 100.0, 1, True),            # the test accepts H1
    ([1, 2] * 8, 100.0, 0, False),           # the test accepts H0
    ([4, 3, 2, 2], 5.0, -1, True),           # undecided, score 11/16
    ([2, 2, 2, 2], 5.0, -1, False),          # undecided, score exactly 1/2: not above
    ([0, 1, 2, 2], 5.0, -1, False),          # undecided, score below
    ([4, 4, 4, 4], 5.0, -1, True)])          # every point taken and still undecided at elo1 = 5: the score decides
def test_gate_rule(stub_pool, script, elo1, status, passed):
    stub_pool.script = list(script)
    out = evaluation.gate(_config(), None, None, [[1]] * len(script), elo1=elo1, poll_every=3)
    assert out["status"] == status and out["passed"] is passed
    assert out["stopped_early"] == (status >= 0 and out["games"] < 2 * len(script))
    if status < 0:
        assert out["games"] == 2 * len(script) and (out["score"] > 0.5) == passed


def test_gate_status_beats_score(stub_pool):
    """H0 accepted while the score over the games played is above 1/2 (nearly all 2-2, a few 3-1, against elo1 = 100): not passed"""
    stub_pool.script = ([3] + [2] * 39) * 6
    out = evaluation.gate(_config(), None, None, [[1]] * len(stub_pool.script), elo1=100.0, poll_every=30, max_steps=2000)
    assert out["status"] == 0 and out["score"] > 0.5 and out["stopped_early"]
    assert out["passed"] is False
