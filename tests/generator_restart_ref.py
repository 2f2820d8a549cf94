"""A pool slot's SEQUENCE of games on ONE oracle generator (oracle only, no device).

Slot s of S plays openings s, s + S, s + 2 S, ... (assign_openings, csrc/engine.hip).  The reference plays them with one GameGenerator per slot,
and a generator is not made anew between games.  What selfplay/GameGenerator.cpp does at GAME_NOT_STARTED (:48-77), read against
Game::begin / Game::prepare_search of oracle/ag_mcts.cpp:

  reset for every game
    Game::beginGame, GameDataStorage::clear                   GameGenerator.cpp:50-51   board, moves, records, outcome
    Tree::clear -> NodeCache::clear                           GameGenerator.cpp:52, Tree.cpp:124-127, NodeCache.cpp:204-218   every node and edge
    AlphaBetaSearch::clear -> SharedHashTable::clear          GameGenerator.cpp:53, AlphaBetaSearch.cpp:69-72, SharedHashTable.hpp:149-152
                                                              every bucket becomes Bucket(): key 0, generation 0, depth 0
    prepare_search (GameGenerator.cpp:75 -> :174-185):
      Search::cleanup                                         Search.cpp:233-242   BOTH task buffers: virtual losses cancelled, buffers emptied
                                                              (a generator's buffers are empty at a game's end: Search::backup clears the one
                                                              it uses, :231, and it never switches to the other)
      Tree::setBoard: base board, move number, max_depth = 0  Tree.cpp:128-151
      Search::setBoard -> increaseGeneration                  Search.cpp:113-116
      a fresh EdgeSelector (the root noise of the move) and EdgeGenerator   GameGenerator.cpp:180-184
  kept from game to game
    the Search object and its two SearchTaskLists             GameGenerator.hpp (member `search`), Search.cpp:84-91.  SearchTask::set
                                                              (SearchTask.cpp:32-50) does not touch moves_left or the two "solved" flags, so
                                                              a task slot holds them until a solve or a network answer overwrites them — a
                                                              proven-edge leaf (Search.cpp:139-150) backs up the moves_left its slot held
    SharedHashTable::m_base_generation                        SharedHashTable.hpp:126,153-156   runs on modulo 64 over all games, while cleared
                                                              entries carry generation 0: their age depth - (base - 0) (:218) differs from
                                                              game to game, and with it which entry of a full bucket is replaced
    Search::current_task_buffer                               Search.cpp:233-251   (1 after the first cleanup, for good: one buffer is used)
    the NodeCache's freed entries and its bin count           NodeCache.cpp:204-218   (memory reuse only: look-ups go by hash and board)
    SearchStats, NodeCacheStats, the OpeningGenerator's queue counters and openings not played yet; not part of any compared value

oracle/ag_mcts.cpp keeps and resets the same things (Game::begin clears the tree and the tables and keeps Search, the tasks and
Solver::generation), so a game after the first is NOT the game a new generator would play from the same opening: tests/test_generator_restart_cpu.py
shows where they part, tests/test_engine_restart_gpu.py holds the device to the generator that goes on."""
import ctypes

import numpy as np

import oracle_lib as ol

SEED0 = 100   # opening id -> ago_prepare_opening seed SEED0 + id (what _play_and_compare of tests/test_engine_gpu.py uses)

# The cases of tests/test_engine_restart_gpu.py; tests/test_generator_restart_cpu.py requires of each that some later game differs from the
# game a new generator plays.  `search`: what reaches the oracle's search as well; `device`: further options of _play_and_compare / the engine.
CASES = {
    "freestyle":       dict(rules=0, n=15, batch=8, sims=100, draw_after=40),
    "standard":        dict(rules=1, n=15, batch=4, sims=100, draw_after=40),
    "renju":           dict(rules=2, n=15, batch=4, sims=100, draw_after=40),
    "caro5":           dict(rules=3, n=15, batch=8, sims=60, draw_after=40),
    "caro6":           dict(rules=4, n=15, batch=4, sims=100, draw_after=40),
    "board12":         dict(rules=0, n=12, batch=8, sims=60, draw_after=40),
    "spec_freestyle":  dict(rules=0, n=15, batch=8, sims=100, draw_after=40, device=dict(speculative_solver=1, speculative_waves=48)),
    "spec_renju_park": dict(rules=2, n=15, batch=8, sims=60, draw_after=60, slots=12, rounds=2, kind="parked", search=dict(table_entries=1 << 12),
                            device=dict(speculative_solver=1, speculative_waves=48, solver_yield_fraction=0.5)),
    "sliced":          dict(rules=0, n=15, batch=8, sims=60, draw_after=50, slots=8, rounds=2,
                            device=dict(groups=4, speculative_solver=1, speculative_waves=96)),
    "format201":       dict(rules=2, n=15, batch=8, sims=60, draw_after=60, device=dict(record_format=3)),
    "symmetries":      dict(rules=1, n=15, batch=4, sims=100, draw_after=40, search=dict(use_symmetries=1)),
    "noise_custom":    dict(rules=0, n=15, batch=4, sims=60, draw_after=40, search=dict(noise_weight=0.25, noise_type=1)),
    "noise_dirichlet": dict(rules=2, n=15, batch=4, sims=100, draw_after=40, search=dict(noise_weight=0.25, noise_type=2)),
    "small_arenas":    dict(rules=0, n=15, batch=8, sims=100, draw_after=40, device=dict(node_capacity=64, edge_capacity=1024, arena_reserve=60.0)),
    "starved":         dict(rules=0, n=15, batch=8, sims=100, draw_after=40, kind="starved"),
    "tournament":      dict(rules=0, n=15, batch=4, sims=100, draw_after=60, slots=1, rounds=3, kind="tournament", threads=3, buffers=1),
    "tournament_two_buffers": dict(rules=2, n=15, batch=8, sims=200, draw_after=40, slots=1, rounds=3, kind="tournament", threads=3, buffers=2),
    "restored":        dict(rules=1, n=15, batch=4, sims=100, draw_after=40, kind="restored"),
}
for _case in CASES.values():
    _case.setdefault("slots", 3)
    _case.setdefault("rounds", 3)
    _case.setdefault("kind", "pool")
    _case.setdefault("search", {})
    _case.setdefault("device", {})
    _case.setdefault("threads", 1)
    _case.setdefault("buffers", 1)


def search_config(case):
    s = case["search"]
    cfg = ol.default_search_config(max_batch_size=case["batch"], max_simulations=case["sims"], table_entries=s.get("table_entries", 1 << 16),
                                   use_symmetries=s.get("use_symmetries", 0), noise_type=s.get("noise_type", 1) if s.get("noise_weight", 0.0) > 0 else 0,
                                   noise_weight=s.get("noise_weight", 0.0))
    return cfg


def opening(olib, case, opening_id):
    op = np.zeros(256, np.uint16)
    k = olib.ago_prepare_opening(case["rules"], case["n"], case["n"], SEED0 + opening_id, ol.ptr(op))
    return [int(x) for x in op[:k]]


def stand_in_evaluator(olib, hw):
    def f(feats):
        feats = np.ascontiguousarray(feats, dtype=np.uint32)
        pol = np.zeros((len(feats), hw), np.float32)
        val = np.zeros((len(feats), 2), np.float32)
        olib.ago_fake_eval(len(feats), hw, ol.ptr(feats), ol.ptr(pol), ol.ptr(val))
        return pol, val
    return f


def search_state(olib, h, lane=0, capacity=16):
    """dict(generation, stored, other_stored, flags[k], moves_left[k]) of one Search of the generator (ago_game_search_state)"""
    out_i, flags, left = np.zeros(4, np.int32), np.zeros(capacity, np.int32), np.zeros(capacity, np.float32)
    olib.ago_game_search_state(h, lane, ol.ptr(out_i), ol.ptr(flags), ol.ptr(left), capacity)
    slots = min(capacity, int(out_i[3]))
    return dict(generation=int(out_i[0]), stored=int(out_i[1]), other_stored=int(out_i[2]), flags=[int(x) for x in flags[:slots]],
                moves_left=[np.float32(x) for x in left[:slots]])


def game_records(olib, h):
    """every record of the generator's current game as a comparable tuple (move, root visits, value, score, flags, the root's edges)"""
    out = []
    for i in range(olib.ago_game_num_records(h)):
        mv, rv, rs = ctypes.c_uint16(), ctypes.c_int(), ctypes.c_uint16()
        rval = (ctypes.c_float * 2)()
        em, ev, ep = np.zeros(512, np.uint16), np.zeros(512, np.int32), np.zeros(512, np.float32)
        evl, es = np.zeros(1024, np.float32), np.zeros(512, np.uint16)
        ne = olib.ago_game_record(h, i, ctypes.byref(mv), ctypes.byref(rv), rval, ctypes.byref(rs), ol.ptr(em), ol.ptr(ev), ol.ptr(ep), ol.ptr(evl), ol.ptr(es), 512)
        out.append((mv.value, rv.value, np.float32(rval[0]).tobytes() + np.float32(rval[1]).tobytes(), rs.value, olib.ago_game_record_flags(h, i),
                    em[:ne].tobytes(), ev[:ne].tobytes(), ep[:ne].tobytes(), evl[:2 * ne].tobytes(), es[:ne].tobytes()))
    return out


class Generator:
    """one oracle handle that plays game after game, as a GameGenerator does"""

    def __init__(self, olib, case):
        self.olib, self.case = olib, case
        self.hw = case["n"] * case["n"]
        self.cfg = search_config(case)
        self.h = olib.ago_game_create_ex(case["rules"], case["n"], case["n"], case["draw_after"], ctypes.byref(self.cfg))
        if case["threads"] > 1:
            olib.ago_game_set_search_threads(self.h, case["threads"])
        self.ev = stand_in_evaluator(olib, self.hw)
        self.width = case["batch"] * case["threads"]

    def begin(self, opening_id, moves=None):
        """GAME_NOT_STARTED -> loadOpening -> prepare_search on the SAME generator; moves: a saved game's moves instead of the opening"""
        moves = opening(self.olib, self.case, opening_id) if moves is None else moves
        op = np.array(list(moves) + [0], np.uint16)
        self.olib.ago_game_set_serial(self.h, opening_id)
        self.olib.ago_game_begin(self.h, ol.ptr(op), len(moves))
        return moves

    def over(self):
        return self.olib.ago_game_outcome(self.h) != 0

    def tree_info(self):
        f, i = np.zeros(1, np.float32), np.zeros(5, np.int32)
        self.olib.ago_game_tree_info(self.h, ol.ptr(f), ol.ptr(i))
        return f[0].tobytes(), int(i[0])

    def step(self):
        """one step of the generator: (leaf count, feature words, root moves-left, maximum depth) behind its expand + backup"""
        feats = np.zeros((self.width, self.hw), np.uint32)
        if self.case["buffers"] == 2:
            c = self.olib.ago_game_async_step(self.h, ol.ptr(feats), self.width)
            if not self.over():
                pol, val = self.ev(feats[:c]) if c else (np.zeros((0, self.hw), np.float32), np.zeros((0, 2), np.float32))
                self.olib.ago_game_async_provide(self.h, ol.ptr(pol), ol.ptr(val))
        else:
            c = self.olib.ago_game_step_select(self.h, ol.ptr(feats), self.width)
            pol, val = self.ev(feats[:c]) if c else (np.zeros((0, self.hw), np.float32), np.zeros((0, 2), np.float32))
            self.olib.ago_game_step_expand(self.h, ol.ptr(pol), ol.ptr(val))
        return (c, feats[:c].tobytes()) + self.tree_info()

    def play(self, opening_id, moves=None, max_steps=20000):
        """a whole game: dict(id, opening, trace = step tuples, records, outcome, generation at its start and at its end)"""
        start = self.begin(opening_id, moves)
        first = search_state(self.olib, self.h)
        trace = []
        while not self.over():
            trace.append(self.step())
            assert len(trace) < max_steps
        return dict(id=opening_id, opening=start, trace=trace, records=game_records(self.olib, self.h), outcome=self.olib.ago_game_outcome(self.h),
                    generation_first=first["generation"], generation_last=search_state(self.olib, self.h)["generation"])

    def close(self):
        self.olib.ago_game_destroy(self.h)


def restored_moves(olib, case, slot, plies=6):
    """the "saved game" of the restored case: opening `slot` and the first `plies` moves a new generator plays from it"""
    g = Generator(olib, case)
    start = g.begin(slot)
    while olib.ago_game_num_records(g.h) < plies and not g.over():
        g.step()
    moves = start + [r[0] for r in game_records(olib, g.h)[:plies]]
    g.close()
    return moves


def slot_ids(case, slot):
    return [slot + case["slots"] * k for k in range(case["rounds"])]


def first_moves(olib, case, slot):
    """what the slot's first game starts from: its opening, or (restored case) the saved game"""
    return restored_moves(olib, case, slot) if case["kind"] == "restored" else None


def play_slot(olib, case, slot):
    """the slot's games, one after the other on one generator"""
    g = Generator(olib, case)
    games = [g.play(i, first_moves(olib, case, slot) if k == 0 else None) for k, i in enumerate(slot_ids(case, slot))]
    g.close()
    return games


def play_fresh(olib, case, opening_id):
    """the game a NEW generator plays from the same opening under the same serial"""
    g = Generator(olib, case)
    game = g.play(opening_id)
    g.close()
    return game


def first_difference(a, b):
    """where two games part: ("step", k) for the first step whose leaf count, features, root moves-left or maximum depth differ,
    ("records", k) for the first record that differs in its move, its root or its edges when every step agrees, ("flags", k) when only the
    solved / must-defend flags of record k differ (a task slot's two "solved" flags are never reset), None when the games are the same"""
    for k, (x, y) in enumerate(zip(a["trace"], b["trace"])):
        if x != y:
            return ("step", k)
    if len(a["trace"]) != len(b["trace"]):
        return ("step", min(len(a["trace"]), len(b["trace"])))
    for k, (x, y) in enumerate(zip(a["records"], b["records"])):
        if x[:4] + x[5:] != y[:4] + y[5:]:
            return ("records", k)
    if len(a["records"]) != len(b["records"]):
        return ("records", min(len(a["records"]), len(b["records"])))
    for k, (x, y) in enumerate(zip(a["records"], b["records"])):
        if x[4] != y[4]:
            return ("flags", k)
    return None


def later_game_differences(olib, case):
    """[(opening id, first_difference)] over every later game of every slot that differs from its fresh counterpart, and the oracle steps played"""
    out, steps = [], 0
    for slot in range(case["slots"]):
        games = play_slot(olib, case, slot)
        steps += sum(len(g["trace"]) for g in games)
        for g in games[1:]:
            d = first_difference(g, play_fresh(olib, case, g["id"]))
            if d is not None:
                out.append((g["id"], d))
    return out, steps
