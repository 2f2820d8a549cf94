"""The two sequential procedures around evaluation matches, and the tuning run built on them.

`GSPRT` is a generalised sequential probability ratio test on PAIR RESULTS (the first player's points over one opening played twice with the
colours swapped, 0..4 — what a match pool logs, selfplay.GeneratorPool.pair_results): it stops a match as soon as "the new player is at
least elo1 stronger" or "it is at most elo0 stronger" is decided.  `SPSA` is simultaneous-perturbation stochastic approximation on the unit
cube.  Both stand in for the reference's src/tuning (GSPRT.cpp, SPSA.cpp) and are written from their formulas (which also
records where GSPRT deviates from GSPRT.cpp as written).  `tune` moves AgxPlayerSearch fields with them: every iteration is one match of the
theta+ settings against the theta- settings on one network.  Host arithmetic only; the matches run on the device (evaluation.play_matches)."""
import math

import numpy as np

LN10_OVER_800 = math.log(10.0) / 800.0   # normalised Elo -> the t of the pentanomial model
PDF_FLOOR = 1.0e-3                        # an empty bin counts as this many results


def pair_llr(results, elo0, elo1):
    """n ln((1 + (t - t0)^2) / (1 + (t - t1)^2)) of a histogram r[0..4] of pair results: p_i = max(1e-3, r_i) / n, s_i = i / 4, mean and
    variance of s under p, t = (mean - 1/2) / sqrt(2 variance), t0 / t1 = elo0 / elo1 * ln 10 / 800"""
    n = float(sum(results))
    p = [max(PDF_FLOOR, float(r)) / n for r in results]
    mean = sum(0.25 * i * p[i] for i in range(5))
    variance = sum(p[i] * (0.25 * i - mean) ** 2 for i in range(5))
    t = (mean - 0.5) / math.sqrt(2.0 * variance)
    t0, t1 = elo0 * LN10_OVER_800, elo1 * LN10_OVER_800
    return n * math.log((1.0 + (t - t0) ** 2) / (1.0 + (t - t1) ** 2))


class GSPRT:
    """add_result(points) one pair result at a time; `status` -1 undecided, 0 H0 (elo0) accepted, 1 H1 (elo1) accepted; `llr` the current
    log-likelihood ratio, `results` the histogram.  The bounds ln(beta / (1 - alpha)) and ln((1 - beta) / alpha) are corrected for the
    overshoot of the steps that set a new maximum / minimum of the ratio.  The first decision is final: later results still move `llr` and
    `results`, `status` stays."""

    def __init__(self, elo0=0.0, elo1=5.0, alpha=0.05, beta=0.05):
        if not (0.0 < alpha < 1.0 and 0.0 < beta < 1.0 and alpha + beta < 1.0):
            raise ValueError("GSPRT needs error rates in (0, 1) whose sum is below 1 (alpha %r, beta %r)" % (alpha, beta))
        if not elo0 < elo1:
            raise ValueError("GSPRT needs elo0 < elo1 (%r, %r)" % (elo0, elo1))
        self.elo0, self.elo1 = float(elo0), float(elo1)
        self.lower = math.log(beta / (1.0 - alpha))
        self.upper = math.log((1.0 - beta) / alpha)
        self.results = [0, 0, 0, 0, 0]
        self.llr = 0.0
        self.status = -1
        self.max_llr = self.min_llr = 0.0
        self.sq0 = self.sq1 = 0.0
        self.o0 = self.o1 = 0.0

    def bounds(self):
        """(lower, upper) as they stand now: H0 is accepted below lower, H1 above upper"""
        return self.lower + self.o0, self.upper - self.o1

    def add_result(self, points):
        if points not in (0, 1, 2, 3, 4):
            raise ValueError("a pair result is 0..4 points, not %r" % (points,))
        self.results[points] += 1
        self.llr = pair_llr(self.results, self.elo0, self.elo1)
        if self.llr > self.max_llr:
            self.sq1 += (self.llr - self.max_llr) ** 2
            self.max_llr = self.llr
            self.o1 = self.sq1 / (2.0 * self.llr)
        if self.llr < self.min_llr:
            self.sq0 += (self.llr - self.min_llr) ** 2
            self.min_llr = self.llr
            self.o0 = -self.sq0 / (2.0 * self.llr)
        if self.status < 0:
            lower, upper = self.bounds()
            if self.llr > upper:
                self.status = 1
            elif self.llr < lower:
                self.status = 0
        return self.status


class SPSA:
    """theta in [0, 1]^dim, started at 0.5.  step(gradient_function, max_iterations): c_k = c / (k + 1)^gamma, a_k = a / (k + 1 + A)^alpha
    with A = max_iterations / 10, delta_i = +-1 from the seeded generator, g = gradient_function(clip(theta + c_k delta), clip(theta - c_k
    delta)) (a scalar: how much better the first argument did), theta <- clip(theta + a_k g / (2 c_k delta)).  Returns g; `last` keeps what
    the step used."""

    def __init__(self, dim, a=1.1, c=0.1, alpha=0.602, gamma=0.101, theta=None, seed=0):
        if dim < 1:
            raise ValueError("SPSA needs at least one dimension")
        self.a, self.c, self.alpha, self.gamma = float(a), float(c), float(alpha), float(gamma)
        self.step_count = 0
        self.theta = np.full(dim, 0.5) if theta is None else np.clip(np.asarray(theta, np.float64), 0.0, 1.0)
        if self.theta.shape != (dim,):
            raise ValueError("theta must have %d entries" % dim)
        self._rng = np.random.default_rng(seed)
        self.last = None

    def step(self, gradient_function, max_iterations):
        k = self.step_count
        big_a = max_iterations / 10.0
        c_k = self.c / (k + 1) ** self.gamma
        a_k = self.a / (k + 1 + big_a) ** self.alpha
        delta = 2.0 * self._rng.integers(0, 2, self.theta.size) - 1.0
        plus = np.clip(self.theta + c_k * delta, 0.0, 1.0)
        minus = np.clip(self.theta - c_k * delta, 0.0, 1.0)
        g = float(gradient_function(plus, minus))
        before = self.theta
        self.theta = np.clip(before + a_k * (g / (2.0 * c_k * delta)), 0.0, 1.0)
        self.step_count = k + 1
        self.last = dict(step=k, theta=before, delta=delta, c_k=c_k, a_k=a_k, theta_plus=plus, theta_minus=minus, g=g)
        return g

    def state(self):
        """the reference's progress keys (a, c, alpha, gamma, step, theta) plus the generator's state: plain Python values"""
        return dict(a=self.a, c=self.c, alpha=self.alpha, gamma=self.gamma, step=self.step_count, theta=[float(x) for x in self.theta],
                    rng=self._rng.bit_generator.state)

    @classmethod
    def from_state(cls, state):
        out = cls(len(state["theta"]), state["a"], state["c"], state["alpha"], state["gamma"], theta=state["theta"])
        out.step_count = int(state["step"])
        out._rng.bit_generator.state = state["rng"]
        return out


class Parameter:
    """One tuned AgxPlayerSearch field: value(theta) maps [0, 1] to [low, high], linearly or (log=True) as low (high / low)^theta; integer
    fields are rounded to nearest."""

    def __init__(self, name, low, high, integer=False, log=False):
        from .selfplay import PLAYER_SEARCH_FIELDS
        if name not in PLAYER_SEARCH_FIELDS:
            raise ValueError("%r is not a field of AgxPlayerSearch (%s)" % (name, ", ".join(PLAYER_SEARCH_FIELDS)))
        if not low < high:
            raise ValueError("parameter %s needs low < high (%r, %r)" % (name, low, high))
        if log and low <= 0:
            raise ValueError("parameter %s: a log scale needs low > 0 (%r)" % (name, low))
        self.name, self.low, self.high, self.integer, self.log = name, low, high, bool(integer), bool(log)

    def value(self, theta):
        theta = min(1.0, max(0.0, float(theta)))
        v = self.low * (self.high / self.low) ** theta if self.log else self.low + (self.high - self.low) * theta
        return int(math.floor(v + 0.5)) if self.integer else float(v)


def settings_of(parameters, theta):
    return {p.name: p.value(t) for p, t in zip(parameters, theta)}


def gradient_of(histogram):
    """2 s - 1 with s = sum k hist[k] / (4 sum hist): +1 when the first player took every point, -1 when the second did"""
    n = sum(histogram)
    if n <= 0:
        raise ValueError("no pair result to take a gradient from")
    return 2.0 * sum(k * h for k, h in enumerate(histogram)) / (4.0 * n) - 1.0


def tune(config, net, parameters, openings, iterations, pairs_per_iteration, base=None, spsa=None, seed=0, **match_args):
    """SPSA over `parameters` (Parameter objects).  One iteration = one match on a fresh match_mode pool (evaluation.play_matches with pair
    tracking): the theta+ settings are the first player, the theta- settings the second, both on top of `base` (a dict of AgxPlayerSearch
    fields) and on `net`, over the next `pairs_per_iteration` openings — `openings` is a list taken in consecutive chunks that wrap round, or
    a callable iteration -> list.  The gradient is gradient_of(the match's pair histogram).  `spsa`: an SPSA to continue (its dimension must
    match), else SPSA(len(parameters), seed=seed).  Returns dict(settings = base + the final values, theta, spsa = the optimiser, history =
    per iteration: theta before the step, delta, c_k, a_k, first / second settings, histogram, g, theta_after)."""
    from . import evaluation
    if len(parameters) == 0:
        raise ValueError("tune needs at least one parameter")
    if iterations < 1 or pairs_per_iteration < 1:
        raise ValueError("tune needs iterations >= 1 and pairs_per_iteration >= 1")
    if not callable(openings) and len(openings) == 0:
        raise ValueError("tune needs at least one opening")
    spsa = SPSA(len(parameters), seed=seed) if spsa is None else spsa
    if spsa.theta.size != len(parameters):
        raise ValueError("the SPSA state has %d dimensions for %d parameters" % (spsa.theta.size, len(parameters)))
    base = dict(base or {})
    history = []
    for it in range(iterations):
        if callable(openings):
            chunk = list(openings(it))
        else:
            chunk = [openings[(it * pairs_per_iteration + j) % len(openings)] for j in range(pairs_per_iteration)]
        played = {}

        def gradient(plus, minus):
            first, second = dict(base, **settings_of(parameters, plus)), dict(base, **settings_of(parameters, minus))
            out = evaluation.play_matches(config, net, net, chunk, first=first, second=second, stop=_NeverStops(), **match_args)
            played.update(first=first, second=second, histogram=list(out["pair_histogram"]))
            return gradient_of(out["pair_histogram"])
        spsa.step(gradient, iterations)
        last = spsa.last
        history.append(dict(theta=last["theta"].tolist(), delta=last["delta"].tolist(), c_k=last["c_k"], a_k=last["a_k"], g=last["g"],
                            theta_after=spsa.theta.tolist(), **played))
    return dict(settings=dict(base, **settings_of(parameters, spsa.theta)), theta=spsa.theta.tolist(), spsa=spsa, history=history)


class _NeverStops:
    """a stop rule that only listens: tune plays every opening of an iteration"""
    status = -1

    def add_result(self, points):
        pass
