"""CPU side of the matches between players with search settings of their own: the conditions the device test relies on, shown on the
oracle alone (tests/match_players_ref.py), and the rating arithmetic of alphagomoku_amd.evaluation (no GPU)."""
import math

import pytest

import match_players_ref as ref
import oracle_lib as ol


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@pytest.mark.parametrize("rules", [0, 1, 2])
def test_oracle_players_with_their_own_settings_differ_and_finish(olib, rules):
    """player A (60 playouts, batch 4, defaults) against player B (100 playouts, batch 8, c 0.8 + 0.25 log, init_to loss, no leak repair, 20
    children, solver budget 30, max_visit, temperature 0.5) on openings 500 and 501, draw_after 60: every game ends, the two players'
    roots show their own playout budgets and B's max_children — what tests/test_match_players_gpu.py counts on to be a real comparison"""
    out = ref.play_alone(olib, rules, seeds=[500, 501], draw_after=60, settings=[ref.PLAYER_A, ref.PLAYER_B])
    print("rules %d: longest game %d half-steps, peak root visits %s, peak root edges %s, results %s" % (
        rules, out["half_steps"], out["peak_visits"], out["peak_edges"], out["results"]))
    assert out["all_played"] and len(out["results"]) == 4                       # 2 openings x 2 colour assignments
    assert sorted((oid, k) for _, oid, k, _ in out["results"]) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert 0 < out["half_steps"] <= 1500
    assert out["peak_visits"][0] <= ref.PLAYER_A["max_simulations"] + ref.PLAYER_A["max_batch_size"]
    assert out["peak_visits"][1] >= 90
    assert out["peak_edges"][1] < out["peak_edges"][0]


def test_elo_of_a_match_score():
    from alphagomoku_amd.evaluation import elo
    even = elo(10, 5, 10)
    assert even["score"] == 0.5 and even["elo"] == 0.0 and even["elo_low"] < 0.0 < even["elo_high"]
    r = elo(75, 0, 25)
    assert abs(r["elo"] - 400.0 * math.log10(3.0)) < 1e-9 and r["score"] == 0.75
    # the variance of a 75 : 25 score without draws is s (1 - s): the interval by hand
    half = 1.96 * math.sqrt(0.75 * 0.25 / 100)
    assert abs(r["elo_low"] - 400.0 * math.log10((0.75 - half) / (0.25 + half))) < 1e-9
    assert abs(r["elo_high"] - 400.0 * math.log10((0.75 + half) / (0.25 - half))) < 1e-9
    s = elo(25, 0, 75)
    assert abs(s["elo"] + r["elo"]) < 1e-9 and abs(s["elo_low"] + r["elo_high"]) < 1e-9 and abs(s["elo_high"] + r["elo_low"]) < 1e-9
    d = elo(30, 40, 30)
    assert d["elo"] == 0.0 and d["elo_high"] < elo(50, 0, 50)["elo_high"]       # draws carry less variance than decided games
    widths = []
    for n in (1, 4, 16, 64):
        x = elo(6 * n, 2 * n, 2 * n)
        assert x["elo_low"] < x["elo"] < x["elo_high"] and abs(x["score"] - 0.7) < 1e-12
        widths.append(x["elo_high"] - x["elo_low"])
    assert all(a > b for a, b in zip(widths, widths[1:]))                       # more games at the same ratio: a narrower interval
    w = elo(12, 0, 0)
    assert w["score"] == 1.0 and w["elo"] == math.inf and w["elo_low"] == math.inf and w["elo_high"] == math.inf
    assert elo(0, 0, 7)["elo"] == -math.inf
    with pytest.raises(ValueError):
        elo(0, 0, 0)
