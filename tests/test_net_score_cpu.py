"""The network score without a GPU: the numpy reference (tests/net_score_ref.py) against hand-computed values, its top-k rule against a
line-by-line transcription of the reference's getAccuracy (NaNs included), and the names of the new C ABI entry points."""
import ctypes
import math
import os
import re

import numpy as np

import net_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)


def test_reference_on_a_2x2_toy_by_hand():
    """every number is a power of two, so the float32 inputs are exact and the sums can be written down"""
    policy = np.array([0.5, 0.25, 0.125, 0.125], np.float32)
    target = np.array([0.0, 0.75, 0.25, 0.0], np.float32)
    value, value_target = np.array([0.5, 0.25, 0.25], np.float32), np.array([1.0, 0.0, 0.0], np.float32)
    q = np.array([[0.125, 0.125], [0.5, 0.25], [0.25, 0.25], [1.0, 0.0]], np.float32)
    q_target = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], np.float32)   # rows 0 and 3 are filler: no edge there
    s = ref.sample_score(policy, value, target, value_target, q, q_target)
    assert abs(s["policy_ce"] - (0.75 * 2 * LN2 + 0.25 * 3 * LN2)) < 1e-15
    assert abs(s["value_ce"] - LN2) < 1e-15
    assert abs(s["q_ce"] - ((0.5 * LN2 + 0.5 * 2 * LN2) + LN2)) < 1e-15 and s["q_cells"] == 2
    # correct = cell 1; the outputs rank cell 0 first, cell 1 second, then the tie 2 before 3
    assert s["topk_hit"] == [0, 1, 1, 1]
    without = ref.sample_score(policy, value, target, value_target)
    assert without["q_ce"] == 0.0 and without["q_cells"] == 0 and without["policy_ce"] == s["policy_ce"]
    records, total = ref.batch_score(np.stack([policy, policy]), np.stack([value, value]), np.stack([target, target]), np.stack([value_target, value_target]),
                                     np.stack([q, q]), np.stack([q_target, q_target]))
    assert total["samples"] == 2 and total["q_cells"] == 4 and total["topk_hit"] == [0, 2, 2, 2] and total["policy_ce"] == 2 * s["policy_ce"]


def test_reference_floor_and_zeroed_cells_by_hand():
    """an output of exactly 0 under a positive target costs -log(FLT_MIN); with only zeros left the first maximum stays on cell 0, so a
    correct move on cell 0 is counted at every rank"""
    zeros, one_hot = np.zeros(4, np.float32), np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    s = ref.sample_score(zeros, np.array([0.0, 1.0, 0.0], np.float32), one_hot, np.array([0.5, 0.5, 0.0], np.float32))
    assert abs(s["policy_ce"] - 126 * LN2) < 1e-12          # FLT_MIN = 2^-126
    assert abs(s["value_ce"] - 0.5 * 126 * LN2) < 1e-12     # 0.5 * -log(FLT_MIN) + 0.5 * -log(1)
    assert s["topk_hit"] == [1, 2, 3, 4]
    assert ref.topk_hits(np.full(4, 0.25, np.float32), np.array([0, 0, 1, 0], np.float32)) == [0, 0, 1, 1]   # ties: 0, 1, 2, 3 in turn


def test_topk_rule_against_the_transcription():
    rng = np.random.default_rng(3)
    rows, cols = 3, 4
    outputs, targets = [], []
    for i in range(300):
        kind = i % 6
        out = rng.dirichlet(np.ones(12)).astype(np.float32)
        tgt = rng.dirichlet(np.ones(12)).astype(np.float32)
        if kind == 1:      # ties among the outputs and the targets
            out = (rng.integers(0, 3, 12) / 4).astype(np.float32)
            tgt = (rng.integers(0, 2, 12)).astype(np.float32)
        elif kind == 2:    # fewer than four non-zero outputs: the zeroed-cell behaviour
            out = np.zeros(12, np.float32)
            out[rng.integers(0, 12, rng.integers(0, 3))] = 0.5
            tgt = np.zeros(12, np.float32)
            tgt[rng.integers(0, 2)] = 1.0
        elif kind == 3:    # all equal
            out = np.full(12, 1 / 12, np.float32)
        elif kind == 4:    # signed zeros compare equal
            out = np.where(rng.random(12) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            tgt = np.zeros(12, np.float32)
        elif kind == 5:    # NaNs: one on cell 0 stays the maximum, one anywhere else never becomes it
            out[rng.integers(0, 12, 2)] = np.nan
            tgt[rng.integers(0, 12, 2)] = np.nan
            if i % 12 == 5:
                out[0] = np.nan
            if i % 18 == 5:
                tgt[0] = np.nan
        outputs.append(out)
        targets.append(tgt)
    for top_k in (1, 4):
        want = ref.get_accuracy_transcribed(len(outputs), outputs, targets, rows, cols, top_k)
        got = np.sum([ref.topk_hits(o, t, top_k) for o, t in zip(outputs, targets)], axis=0)
        assert want[0] == len(outputs) and [int(x) for x in want[1:]] == [int(x) for x in got]
    four = np.sum([ref.topk_hits(o, t, 4) for o, t in zip(outputs, targets)], axis=0)
    nan_rows = [(o, t) for o, t in zip(outputs, targets) if np.isnan(o).any()]
    assert any(np.isnan(o[0]) for o, _ in nan_rows) and any(np.isnan(t[0]) for _, t in nan_rows) and any(not np.isnan(o[0]) for o, _ in nan_rows)
    assert any(ref.first_max(o) != int(np.argmax(o)) for o, _ in nan_rows)   # (np.argmax alone would disagree)
    assert four[3] > four[0] > 0 and any(ref.topk_hits(o, t)[3] > 1 for o, t in zip(outputs, targets))   # (not vacuous: a sample counted twice occurs)


def test_entry_points_are_declared_and_exported(agx_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "agx.h")).read(), flags=re.S)
    from alphagomoku_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("agx_net_score_clear", "agx_net_score_outputs", "agx_net_score_dataset"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(cdll, name), name
    assert "AgxSampleScore" in text and "AgxNetScore" in text
    assert ctypes.sizeof(_lib.AgxSampleScore) == ref.SAMPLE_DTYPE.itemsize == 48 and ctypes.sizeof(_lib.AgxNetScore) == ref.TOTAL_DTYPE.itemsize == 72
    for struct, dtype in ((_lib.AgxSampleScore, ref.SAMPLE_DTYPE), (_lib.AgxNetScore, ref.TOTAL_DTYPE)):
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]
