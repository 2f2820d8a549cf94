"""Evaluation matches between two players with search settings of their own, played by the CPU oracle alone (helper, no test).

The loop is the one of tests/test_oracle_match.py's first test with a configuration per player: two oracle handles per pair, each created
from its own AgoSearchConfig (and policy temperature), openings from ago_prepare_opening, every opening played twice with the colours
swapped, the pairs restarted the way the device pool restarts them (pair m plays openings m, m + pairs, ...).  OracleMatches keeps that
bookkeeping for tests/test_match_players_gpu.py, which holds the device against it half-step by half-step; play_alone() drives it with the
stand-in evaluators only (tests/test_match_players_cpu.py)."""
import ctypes

import numpy as np

import oracle_lib as ol

# the AgxPlayerSearch fields of the two players the tests use; PLAYER_A is the pools' configuration apart from max_simulations / max_batch_size
PLAYER_A = dict(max_simulations=60, max_batch_size=4, exploration_constant=1.25, exploration_scaling=0.0, init_to=0, information_leak_threshold=0.01,
                max_children=0, policy_expansion_threshold=1.0e-4, policy_temperature=1.0, tss_max_positions=100, final_selector=0, action_values=0)
PLAYER_B = dict(max_simulations=100, max_batch_size=8, exploration_constant=0.8, exploration_scaling=0.25, init_to=3, information_leak_threshold=1.0,
                max_children=20, policy_expansion_threshold=1.0e-4, policy_temperature=0.5, tss_max_positions=30, final_selector=1, action_values=0)
POOL_BATCH = 8      # the largest batch of the two: the pools' max_batch_size, the stride of the task buffers
POOL_TSS = 100      # ... and the largest solver budget: the pools' tss_max_positions
TABLE_ENTRIES = 1 << 16


def oracle_config(settings):
    """the AgoSearchConfig of a player with these AgxPlayerSearch fields (the temperature is set on the handle)"""
    cfg = ol.default_search_config(max_batch_size=settings["max_batch_size"], max_simulations=settings["max_simulations"], table_entries=TABLE_ENTRIES,
                                   final_selector=settings["final_selector"])
    cfg.exploration_constant = settings["exploration_constant"]
    cfg.exploration_scaling = settings["exploration_scaling"]
    cfg.init_to = settings["init_to"]
    cfg.information_leak_threshold = settings["information_leak_threshold"]
    cfg.max_children = settings["max_children"] if settings["max_children"] > 0 else 2 ** 31 - 1
    cfg.policy_expansion_threshold = settings["policy_expansion_threshold"]
    cfg.tss_max_positions = settings["tss_max_positions"]
    return cfg


def prepare_openings(olib, rules, n, seeds):
    out = []
    for seed in seeds:
        op = np.zeros(64, np.uint16)
        k = olib.ago_prepare_opening(rules, n, n, seed, ol.ptr(op))
        out.append([int(x) for x in op[:k]])
    return out


def first_evaluator(olib, hw):
    def f(feats):
        feats = np.ascontiguousarray(feats, dtype=np.uint32)
        pol = np.zeros((len(feats), hw), np.float32)
        val = np.zeros((len(feats), 2), np.float32)
        if len(feats):
            olib.ago_fake_eval(len(feats), hw, ol.ptr(feats), ol.ptr(pol), ol.ptr(val))
        return pol, val
    return f


def second_evaluator(olib, hw):
    """a different deterministic 'network' for the second player: sharper policy, shifted value"""
    base = first_evaluator(olib, hw)

    def f(feats):
        pol, val = base(feats)
        pol = (pol * pol).astype(np.float32)
        s = pol.sum(1, keepdims=True, dtype=np.float32)
        pol = np.where(s > 0, pol / np.where(s > 0, s, 1), np.float32(1.0 / hw)).astype(np.float32)
        val = np.stack([np.float32(0.9) * val[:, 0] + np.float32(0.05), np.float32(0.5) * val[:, 1]], 1).astype(np.float32)
        return pol, val
    return f


def stand_in_q(feats, hw):
    """a deterministic stand-in for the 'q' output: (win, draw) per cell, a hash of the cell's feature word"""
    f = np.ascontiguousarray(feats, dtype=np.uint32).reshape(-1, hw)
    h = (f.astype(np.uint64) * np.uint64(2654435761) + np.arange(hw, dtype=np.uint64) * np.uint64(40503)) % np.uint64(1 << 20)
    w = (h.astype(np.float32) / np.float32(1 << 20)) * np.float32(0.8)
    d = (np.float32(1.0) - w) * np.float32(0.25)
    return np.stack([w, d], axis=2).astype(np.float32)


def oracle_root(olib, h):
    rv, rs = ctypes.c_int(), ctypes.c_uint16()
    rval = (ctypes.c_float * 2)()
    em, ev, ep, evl, es, ef = (np.zeros(512, np.uint16), np.zeros(512, np.int32), np.zeros(512, np.float32), np.zeros(1024, np.float32),
                               np.zeros(512, np.uint16), np.zeros(512, np.uint16))
    n = olib.ago_game_root(h, ctypes.byref(rv), rval, ctypes.byref(rs), ol.ptr(em), ol.ptr(ev), ol.ptr(ep), ol.ptr(evl), ol.ptr(es), ol.ptr(ef), 512)
    return dict(n=n, visits=rv.value, moves=em[:n].copy(), ev=ev[:n].copy(), prior=ep[:n].copy(), val=evl[:2 * n].copy(), es=es[:n].copy())


class OracleMatches:
    """`pairs` pairs of oracle players, player 0 / 1 of every pair created from settings[0] / settings[1]"""

    def __init__(self, olib, rules, n, draw_after, pairs, openings, settings):
        self.olib, self.n, self.hw, self.pairs, self.openings, self.settings = olib, n, n * n, pairs, openings, settings
        self.players = []       # [pair][0 first / 1 second player]
        for _ in range(pairs):
            hs = []
            for s in settings:
                cfg = oracle_config(s)
                h = olib.ago_game_create_ex(rules, n, n, draw_after, ctypes.byref(cfg))
                olib.ago_game_set_force_expand_root(h, 0)   # Player::setBoard builds UnifiedGenerator without forceExpandRoot
                olib.ago_game_set_policy_temperature(h, s["policy_temperature"])
                hs.append(h)
            self.players.append(hs)
        self.games_done = [0] * pairs
        self.mover = [None] * pairs      # 0 / 1: whose turn; None: the pair waits for an opening
        self.opening_of = [None] * pairs
        self.results = []                # (pair, opening, 0 / 1 colours swapped, outcome)

    def start_game(self, m, oid):
        olib = self.olib
        self.opening_of[m] = oid
        op = np.array(self.openings[oid] + [0], np.uint16)
        first_sign = 1 if self.games_done[m] % 2 == 0 else 2      # EvaluationGame.cpp:59-71
        for h in self.players[m]:
            olib.ago_game_set_serial(h, oid)
            olib.ago_game_match_begin(h, ol.ptr(op), len(self.openings[oid]))
        self.mover[m] = 0 if olib.ago_game_sign_to_move(self.players[m][0]) == first_sign else 1
        olib.ago_game_take_turn(self.players[m][self.mover[m]])

    def restart_waiting(self):
        """a pair that finished a game plays its opening again with the colours swapped, then its next opening: m, m + pairs, ..."""
        for m in range(self.pairs):
            if self.mover[m] is None:
                if self.games_done[m] % 2 == 1:
                    self.start_game(m, self.opening_of[m])
                elif m + self.pairs * (self.games_done[m] // 2) < len(self.openings):
                    self.start_game(m, m + self.pairs * (self.games_done[m] // 2))

    def select(self, m, who):
        """the select stage of pair m's player `who`: (count, features uint32 [POOL_BATCH][hw])"""
        f = np.zeros((POOL_BATCH, self.hw), np.uint32)
        c = self.olib.ago_game_step_select(self.players[m][who], ol.ptr(f), POOL_BATCH)
        return c, f

    def expand(self, m, who, policy, value, q=None):
        """the expand stage with the network's answers; the move, if one is played, goes to the partner.  Returns True when the player moved."""
        olib, h = self.olib, self.players[m][who]
        policy, value = np.ascontiguousarray(policy, np.float32), np.ascontiguousarray(value, np.float32)
        if self.settings[who]["action_values"]:
            moved = olib.ago_game_step_expand_q(h, ol.ptr(policy), ol.ptr(value), ol.ptr(np.ascontiguousarray(q, np.float32)))
        else:
            moved = olib.ago_game_step_expand(h, ol.ptr(policy), ol.ptr(value))
        if moved:
            other = self.players[m][1 - who]
            olib.ago_game_external_move(other, olib.ago_game_last_move(h))
            assert olib.ago_game_outcome(other) == olib.ago_game_outcome(h)
            if olib.ago_game_outcome(h) != 0:
                self.results.append((m, self.opening_of[m], self.games_done[m] % 2, olib.ago_game_outcome(h)))
                self.games_done[m] += 1
                self.mover[m] = None
            else:
                olib.ago_game_take_turn(other)
                self.mover[m] = 1 - who
        return bool(moved)

    def root(self, m, who):
        return oracle_root(self.olib, self.players[m][who])

    def all_played(self):
        return all(x is None for x in self.mover) and all(d % 2 == 0 and m + self.pairs * (d // 2) >= len(self.openings) for m, d in enumerate(self.games_done))

    def close(self):
        for hs in self.players:
            for h in hs:
                self.olib.ago_game_destroy(h)


def play_alone(olib, rules, seeds, draw_after, settings, n=15, max_half_steps=4000):
    """One pair per opening, every pair plays its opening twice.  Returns dict(results, half_steps = the longest game's half-steps (select +
    expand of the player to move), peak_visits[player], peak_edges[player]) of the roots seen after every half-step."""
    openings = prepare_openings(olib, rules, n, seeds)
    matches = OracleMatches(olib, rules, n, draw_after, len(openings), openings, settings)
    evaluators = [first_evaluator(olib, n * n), second_evaluator(olib, n * n)]
    peak_visits, peak_edges, longest = [0, 0], [0, 0], 0
    length = [0] * matches.pairs
    matches.restart_waiting()
    for _ in range(max_half_steps):
        for m in range(matches.pairs):
            who = matches.mover[m]
            if who is None:
                continue
            c, f = matches.select(m, who)
            pol, val = evaluators[who](f[:c])
            q = stand_in_q(f[:c], n * n) if settings[who]["action_values"] else None
            length[m] += 1
            if not matches.expand(m, who, pol, val, q):
                r = matches.root(m, who)
                peak_visits[who] = max(peak_visits[who], r["visits"])
                peak_edges[who] = max(peak_edges[who], r["n"])
            elif matches.mover[m] is None:
                longest = max(longest, length[m])
                length[m] = 0
        matches.restart_waiting()
        if matches.all_played():
            break
    out = dict(results=list(matches.results), half_steps=longest, peak_visits=peak_visits, peak_edges=peak_edges, all_played=matches.all_played())
    matches.close()
    return out
