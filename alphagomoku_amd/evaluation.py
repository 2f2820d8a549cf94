"""Evaluation matches on the device between two players with search settings of their own, and the rating difference their score stands for.

`play_matches` is the counterpart of the reference's base-against-tested run (tuning_launcher plays base_player_config against
tested_player_config on one network; evaluation/EvaluationManager plays two networks): one match_mode pool, the two players' settings
applied with GeneratorPool.set_player_search, stepped with step_match until every opening has been played with both colour assignments —
or, under a sequential stop rule fed from the pool's pair log (tuning.GSPRT), until the result is decided.  `gate` is that run as the
accept / reject decision on a new network (TrainingManager::gating)."""
import math

from . import selfplay
from ._lib import AgxError


def _elo_of(score):
    if score <= 0.0:
        return -math.inf
    if score >= 1.0:
        return math.inf
    return 400.0 * math.log10(score / (1.0 - score))


def elo(wins, draws, losses):
    """dict(score, elo, elo_low, elo_high) of a match result from the first player's point of view: score s = (W + D/2) / n, elo =
    400 log10(s / (1 - s)); the 95 % interval is s -+ 1.96 sqrt(var / n) mapped through the same formula, with the per-game variance
    var = (W (1 - s)^2 + D (1/2 - s)^2 + L s^2) / n.  A score of 0 or 1 gives -inf / +inf; n = 0 raises ValueError."""
    n = wins + draws + losses
    if n <= 0 or min(wins, draws, losses) < 0:
        raise ValueError("elo needs at least one game and no negative count (wins %r, draws %r, losses %r)" % (wins, draws, losses))
    s = (wins + 0.5 * draws) / n
    var = (wins * (1.0 - s) ** 2 + draws * (0.5 - s) ** 2 + losses * s ** 2) / n
    half = 1.96 * math.sqrt(var / n)
    return dict(score=s, elo=_elo_of(s), elo_low=_elo_of(s - half), elo_high=_elo_of(s + half))


def play_matches(config, first_net, second_net, openings, first=None, second=None, max_steps=100000, poll_every=50, stream=None, stop=None,
                 pair_capacity=None):
    """Plays every opening twice (colours swapped) between the first player (first_net, settings `first`) and the second (second_net,
    `second`) on a match_mode pool created from `config` (an AgxEngineConfig, selfplay.default_config(match_mode=1, ...)).  `first` /
    `second`: dicts of AgxPlayerSearch fields, the fields not named stay the pool's.  `openings`: lists of Move::toShort words.  The loop
    steps the pool and reads match_summary() every `poll_every` steps.  Returns the summary (wins, draws, losses, games from the first
    player's point of view) plus steps, elo(...)'s fields when a game was finished, and each player's settings as played.

    `stop`: a sequential rule — anything with add_result(points) and status, e.g. tuning.GSPRT.  The pool then logs its pair results on the
    device (GeneratorPool.track_pairs, `pair_capacity` entries, 2 len(openings) unless given); every poll feeds the rule the new log
    entries one by one in log order, and the loop ends at the first poll that leaves status >= 0, or when every opening is played.  The
    result gains pair_histogram, pair_sequence (the points in the order the rule saw them), status, llr (when the rule has one) and
    stopped_early (the rule decided before every opening was played; a run cut off by max_steps is not one); the summary then counts the
    games finished when the loop ended.  A flag of the log (full, skipped opening, inconsistent scores) raises AgxError."""
    if not config.match_mode:
        raise ValueError("play_matches needs a match_mode configuration")
    if len(openings) == 0:
        raise ValueError("play_matches needs at least one opening")
    if stop is None and pair_capacity is not None:
        raise ValueError("pair_capacity belongs to a stop rule")
    if stop is not None and not (hasattr(stop, "add_result") and hasattr(stop, "status")):
        raise ValueError("a stop rule has add_result(points) and status")
    pool = selfplay.GeneratorPool(config)
    try:
        if first:
            pool.set_player_search(0, **first)
        if second:
            pool.set_player_search(1, **second)
        settings = [pool.player_search(0), pool.player_search(1)]
        if stop is not None:
            pool.track_pairs(2 * len(openings) if pair_capacity is None else pair_capacity)
        pool.begin(selfplay.pack_openings(openings), stream)
        summary, steps, sequence, totals = None, 0, [], None

        def poll():
            """the summary; with a stop rule, the new log entries go to it first.  True: the loop is over"""
            nonlocal summary, totals
            if stop is not None:
                entries, totals = pool.pair_results(len(sequence), stream)
                if totals["flags"] != 0:
                    raise AgxError("the match pool's pair log raised flags %d (1 full, 2 skipped opening, 4 inconsistent scores)" % totals["flags"])
                for points in entries["points"]:
                    sequence.append(int(points))
                    stop.add_result(int(points))
            summary = pool.match_summary(stream)
            return summary["games"] >= 2 * len(openings) or (stop is not None and stop.status >= 0)
        done = False
        while steps < max_steps and not done:
            pool.step_match(first_net, second_net, stream)
            steps += 1
            if steps % poll_every == 0:
                done = poll()
        if summary is None or steps % poll_every != 0:
            poll()
        stats = pool.stats()
        if stats["first_error"] != 0:
            raise AgxError("a game of the match pool stopped with engine error %d" % stats["first_error"])
    finally:
        pool.close()
    out = dict(summary, steps=steps, players=settings)
    if summary["wins"] + summary["draws"] + summary["losses"] > 0:
        out.update(elo(summary["wins"], summary["draws"], summary["losses"]))
    if stop is not None:
        out.update(pair_histogram=totals["histogram"], pair_sequence=sequence, status=stop.status,
                   stopped_early=stop.status >= 0 and summary["games"] < 2 * len(openings))
        if hasattr(stop, "llr"):
            out["llr"] = stop.llr
    return out


def gate(config, new_net, best_net, openings, elo0=0.0, elo1=5.0, alpha=0.05, beta=0.05, **match_args):
    """Does `new_net` replace `best_net`?  play_matches(new first, best second) under tuning.GSPRT(elo0, elo1, alpha, beta): the match ends
    as soon as the test decides.  Returns play_matches' result plus `passed`: status == 1 when the test decided; when the openings ran out
    first, the reference's gating rule (TrainingManager::gating) — the new network's score over all games played is above 0.5."""
    from .tuning import GSPRT
    out = play_matches(config, new_net, best_net, openings, stop=GSPRT(elo0, elo1, alpha, beta), **match_args)
    out["passed"] = (out["status"] == 1) if out["status"] >= 0 else (out.get("score", 0.0) > 0.5)
    return out
