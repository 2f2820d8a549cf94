"""Evaluation matches on the device between two players with search settings of their own, and the rating difference their score stands for.

`play_matches` is the counterpart of the reference's base-against-tested run (tuning_launcher plays base_player_config against
tested_player_config on one network; evaluation/EvaluationManager plays two networks): one match_mode pool, the two players' settings
applied with GeneratorPool.set_player_search, stepped with step_match until every opening has been played with both colour assignments."""
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


def play_matches(config, first_net, second_net, openings, first=None, second=None, max_steps=100000, poll_every=50, stream=None):
    """Plays every opening twice (colours swapped) between the first player (first_net, settings `first`) and the second (second_net,
    `second`) on a match_mode pool created from `config` (an AgxEngineConfig, selfplay.default_config(match_mode=1, ...)).  `first` /
    `second`: dicts of AgxPlayerSearch fields, the fields not named stay the pool's.  `openings`: lists of Move::toShort words.  The loop
    steps the pool and reads match_summary() every `poll_every` steps.  Returns the summary (wins, draws, losses, games from the first
    player's point of view) plus steps, elo(...)'s fields when a game was finished, and each player's settings as played."""
    if not config.match_mode:
        raise ValueError("play_matches needs a match_mode configuration")
    if len(openings) == 0:
        raise ValueError("play_matches needs at least one opening")
    pool = selfplay.GeneratorPool(config)
    try:
        if first:
            pool.set_player_search(0, **first)
        if second:
            pool.set_player_search(1, **second)
        settings = [pool.player_search(0), pool.player_search(1)]
        pool.begin(selfplay.pack_openings(openings), stream)
        summary, steps = None, 0
        while steps < max_steps:
            pool.step_match(first_net, second_net, stream)
            steps += 1
            if steps % poll_every == 0:
                summary = pool.match_summary(stream)
                if summary["games"] >= 2 * len(openings):
                    break
        if summary is None or steps % poll_every != 0:
            summary = pool.match_summary(stream)
        stats = pool.stats()
        if stats["first_error"] != 0:
            raise AgxError("a game of the match pool stopped with engine error %d" % stats["first_error"])
    finally:
        pool.close()
    out = dict(summary, steps=steps, players=settings)
    if summary["wins"] + summary["draws"] + summary["losses"] > 0:
        out.update(elo(summary["wins"], summary["draws"], summary["losses"]))
    return out

