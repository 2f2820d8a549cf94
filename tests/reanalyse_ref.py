"""numpy restatement of the sample sink of the position searcher (csrc/engine.hip: position_write_sample; agx.h: AgxPositionSampleSink):
the dense per-cell rows of one harvested root -> the bytes of SearchDataStorage_v201::loadFrom + serialize (csrc/sample_v201.hpp), in
float32, one operation after the other.  Held against the oracle's ago_sample_v201_pack in tests/test_reanalyse_cpu.py."""
import numpy as np

F32 = np.float32
UNKNOWN_SCORE = (2 << 13) | 4000   # Score(): what SearchDataPack::clear leaves on a cell without an edge


def _bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def _pow2(e):
    return np.array([(127 + e) << 23], np.uint32).view(F32)[0]


class SmallFloat:
    """LowFP<S, E, M, B> (utils/low_precision.hpp): to_lowp rounds by adding one half before truncation and saturates the mantissa"""

    def __init__(self, s, e, m, b):
        self.s, self.e, self.m, self.b = s, e, m, b
        self.bits, self.exp_min, self.exp_max = s + e + m, b, (1 << e) - 1 + b

    def encode(self, x):
        x = F32(x)
        raw = _bits(x)
        sign = ((raw & 0x80000000) >> (32 - self.bits)) if self.s == 1 else 0
        e = min(max(((raw >> 23) & 255) - 127, self.exp_min), self.exp_max)
        sub = 1 if e == self.exp_min else 0
        magnitude = x if sign == 0 else F32(-x)
        frac = F32(F32(F32(magnitude * _pow2(-(e + sub))) + F32(sub)) - F32(1.0))
        m = min(int(F32(F32(frac * F32(1 << self.m)) + F32(0.5))), (1 << self.m) - 1)
        return sign | ((e - self.b) << self.m) | m

    def decode(self, code):
        negative = self.s == 1 and ((code >> (self.e + self.m)) & 1)
        e = ((code >> self.m) & ((1 << self.e) - 1)) + self.b
        frac = F32(F32(code & ((1 << self.m) - 1)) / F32(1 << self.m))
        sub = 1 if e == self.exp_min else 0
        return F32(F32(F32(-1.0 if negative else 1.0) * F32(F32(1 - sub) + frac)) / _pow2(-(e + sub)))

    def largest(self):
        return self.decode((1 << self.bits) - 1 if self.s == 0 else (1 << (self.bits - 1)) - 1)


SCORE, VISIT, PRIOR, SCALE = SmallFloat(1, 3, 2, -8), SmallFloat(0, 3, 5, -8), SmallFloat(0, 4, 4, -16), SmallFloat(0, 5, 11, -16)


def proven(score):
    """Score::isProven on the raw bits"""
    return ((score >> 13) & 3) != 2 and score not in (0, 0xFFFF)


def score_code(score):
    """score_to_int8 (SearchDataStorage.cpp:24-31)"""
    pv, evaluation = (score >> 13) & 3, (score & 8191) - 4000
    if proven(score):
        distance = -evaluation if pv == 3 else evaluation
        return (pv << 6) | min(max(distance, 0), 63)
    return ((pv << 6) | SCORE.encode(F32(evaluation) / F32(1000.0))) & 255


def sample_bytes(n, rows, root_score, stones, flags):
    """rows: visits [cells], prior [cells], q [cells][2], score [cells], edge_index [cells] (-1: the root has no edge there) of one position
    (AgxPositionSearchOutputs) -> uint8 array: header (three scales, root score, move number = stones, flags, entry count), then an entry for
    every cell whose edge has visits or a proven score, and for every cell 255 or more past the previous entry (the first counts from 0)"""
    cells = n * n
    visits, prior, q, score, edge = (np.asarray(rows[k]) for k in ("visits", "prior", "q", "score", "edge_index"))
    has = edge >= 0
    max_prior = max([F32(p) for p in prior[has] if p > 0] + [F32(0.0)])
    max_value = max([max(F32(w), F32(d)) for w, d in q[has] if max(w, d) > 0] + [F32(0.0)])
    max_visits = max([int(v) for v in visits[has]] + [0])
    prior_scale = F32(1.0) if max_prior == 0 else F32(max_prior / PRIOR.largest())
    value_scale = F32(1.0) if max_value == 0 else F32(max_value / PRIOR.largest())
    visit_scale = F32(F32(max(1, max_visits)) / VISIT.largest())
    entries, last = [], 0
    for c in range(cells):
        natural = bool(has[c]) and (int(visits[c]) > 0 or proven(int(score[c])))
        if natural or c - last >= 255:
            v, p, w, d, s = (int(visits[c]), F32(prior[c]), F32(q[c][0]), F32(q[c][1]), int(score[c])) if has[c] else (0, F32(0), F32(0), F32(0), UNKNOWN_SCORE)
            entries.append([c - last, VISIT.encode(F32(F32(v) / visit_scale)), PRIOR.encode(F32(p / prior_scale)), score_code(s),
                            PRIOR.encode(F32(w / value_scale)), PRIOR.encode(F32(d / value_scale))])
            last = c
    header = np.array([SCALE.encode(value_scale), SCALE.encode(prior_scale), SCALE.encode(visit_scale), root_score, stones, flags], np.uint16).view(np.uint8)
    return np.concatenate([header, np.array([len(entries)], np.uint32).view(np.uint8), np.array(entries, np.uint8).reshape(-1)])


def sample_of_position(n, got, i, stones):
    """sample_bytes of position i of a searcher's output dict (root [n][4] = visits, score bits, flags, edges)"""
    rows = {k: got[k][i] for k in ("visits", "prior", "q", "score", "edge_index")}
    return sample_bytes(n, rows, int(got["root"][i][1]) & 0xFFFF, stones, int(got["root"][i][2]))


def has_filler(sample):
    """a cell that got its entry only for lying 255 cells past the previous one: location_delta 255, no visit, no proven score"""
    entries = np.asarray(sample[16:], np.uint8).reshape(-1, 6)
    return bool(((entries[:, 0] == 255) & (entries[:, 1] == 0) & ((entries[:, 3] >> 6) == 2)).any())
