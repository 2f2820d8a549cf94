"""The combine rules behind the solver (tests/position_solve_ref.py, which tests/test_position_solve_gpu.py holds the device against) on
cases computed by hand, and the refusals of agx_position_solver_* that are decided before a device is touched.  No GPU needed."""
import ctypes

import numpy as np

import position_solve_ref as sref
from position_eval_ref import MASK_FORBIDDEN, RENORMALISE

F32 = np.float32
N = 3   # a 3x3 board keeps the hand computation short; the rules do not depend on the size
UNKNOWN = (2 << 13) | 4000


def move(sign, cell):
    return sign | ((cell // N) << 2) | ((cell % N) << 9)


def win_in(k):
    return (3 << 13) | (4000 - k)


def loss_in(k):
    return (0 << 13) | (4000 + k)


def draw_in(k):
    return (1 << 13) | (4000 + k)


ROW = np.array([0.1, 0.2, 0.3, 0.05, 0.05, 0.1, 0.1, 0.05, 0.05], F32)
VALUE = np.array([[0.5, 0.25, 0.25]], F32)
BOARD = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 2]], np.uint8)


def solved(flags, top_k, score, cells, scores, board=BOARD, features=None, **status):
    return sref.combine_solved(N, board, 0x01, flags, top_k, ROW[None], VALUE, None, features, score, [move(1, c) for c in cells], scores, **status)


def test_score_classes():
    assert sref.is_proven(win_in(3)) and sref.is_proven(loss_in(4)) and sref.is_proven(draw_in(0))
    assert not sref.is_proven(UNKNOWN) and not sref.is_proven(0) and not sref.is_proven(0xFFFF)
    assert sref.score_value(win_in(1)).tolist() == [1, 0, 0] and sref.score_value(draw_in(2)).tolist() == [0, 1, 0]
    assert sref.score_value(loss_in(2)).tolist() == [0, 0, 1] and sref.score_value(UNKNOWN).tolist() == [0, 0, 0]
    assert sref.move_cell(move(2, 7), N) == 7


def test_unproven_policy_lives_on_the_action_list_only():
    out = solved(0, 4, UNKNOWN, [5, 1, 2], [UNKNOWN] * 3)
    assert out["policy"].tolist() == [0, F32(0.2), F32(0.3), 0, 0, F32(0.1), 0, 0, 0]
    assert np.array_equal(out["value"], VALUE[0])
    assert out["top_cells"].tolist() == [2, 1, 5, -1] and out["top_probs"].tolist() == [F32(0.3), F32(0.2), F32(0.1), 0]
    assert out["status"] == 0


def test_unproven_policy_renormalised_over_what_is_left():
    out = solved(RENORMALISE, 1, UNKNOWN, [5, 1, 2], [UNKNOWN] * 3)
    total = F32(F32(F32(0.2) + F32(0.3)) + F32(0.1))   # cell order, one float32 addition after the other
    scale = F32(F32(1.0) / total)
    assert out["policy"].tolist() == [0, F32(F32(0.2) * scale), F32(F32(0.3) * scale), 0, 0, F32(F32(0.1) * scale), 0, 0, 0]
    assert out["top_cells"].tolist() == [2] and out["top_probs"][0] == F32(F32(0.3) * scale)


def test_the_masks_of_the_evaluator_still_hold_on_the_list():
    """an occupied cell in the list (cell 0) and a forbidden one (cell 2, bit 6 of its feature word) carry no policy and are not picked"""
    features = np.zeros(9, np.uint32)
    features[2] = 1 << 6
    out = solved(MASK_FORBIDDEN, 3, UNKNOWN, [0, 1, 2], [UNKNOWN] * 3, features=features)
    assert out["policy"].tolist() == [0, F32(0.2), 0, 0, 0, 0, 0, 0, 0]
    assert out["top_cells"].tolist() == [1, -1, -1]


def test_proven_position_splits_over_the_equal_best_scores():
    out = solved(RENORMALISE, 4, win_in(3), [7, 4, 1, 5], [win_in(3), UNKNOWN, win_in(3), win_in(5)])
    assert out["policy"].tolist() == [0, 0.5, 0, 0, 0, 0, 0, 0.5, 0]           # win in 3 beats win in 5: the larger 16-bit value
    assert out["value"].tolist() == [1, 0, 0]
    assert out["top_cells"].tolist() == [1, 7, 4, 5] and out["top_probs"].tolist() == [0.5, 0.5, 0, 0]   # then the rest of the list, lowest cell first
    lost = solved(0, 1, loss_in(4), [3, 6, 1], [loss_in(4)] * 3)
    third = F32(F32(1.0) / F32(3.0))
    assert lost["policy"].tolist() == [0, third, 0, third, 0, 0, third, 0, 0] and lost["value"].tolist() == [0, 0, 1]
    assert lost["top_cells"].tolist() == [1]
    single = solved(0, 0, win_in(1), [4], [win_in(1)])
    assert single["policy"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]


def test_empty_action_list():
    full = np.array([[1, 2, 1], [2, 1, 2], [2, 1, 2]], np.uint8)
    out = solved(RENORMALISE, 2, draw_in(0), [], [], board=full)
    assert not out["policy"].any() and out["value"].tolist() == [0, 1, 0] and out["top_cells"].tolist() == [-1, -1] and not out["top_probs"].any()
    quiet = solved(RENORMALISE, 2, UNKNOWN, [], [])
    assert not quiet["policy"].any() and np.array_equal(quiet["value"], VALUE[0]) and quiet["top_cells"].tolist() == [-1, -1]   # a sum of 0.0f: no NaN


def test_status_words_combine_as_their_maximum():
    bad = solved(0, 2, win_in(1), [4], [win_in(1)], status_solver=1, status_eval=1)
    assert bad["status"] == 1 and not bad["policy"].any() and not bad["value"].any() and bad["top_cells"].tolist() == [-1, -1]
    assert solved(0, 0, UNKNOWN, [4], [UNKNOWN], status_solver=1)["status"] == 1
    doubtful = solved(0, 0, UNKNOWN, [4], [UNKNOWN], status_solver=2)
    assert doubtful["status"] == 2 and doubtful["policy"][4] == F32(0.05)
    assert solved(0, 0, UNKNOWN, [4], [UNKNOWN], status_eval=2)["status"] == 2


def test_expected_flags():
    assert sref.expected_flags(dict(must_defend=True, nodes=1, score=UNKNOWN)) == 1 | 4 | 16
    assert sref.expected_flags(dict(must_defend=False, nodes=57, score=win_in(5))) == 4 | 32


def test_refusals_that_need_no_device(agx_lib):
    """argument checks come before the first HIP call: they give their code on a machine without a GPU, and *out stays NULL"""
    INVALID, UNSUPPORTED = 1, 3
    lib, handle = agx_lib, ctypes.c_void_p()
    create = lib.agx_position_solver_create
    assert create(0, 15, 4, 100, 1 << 12, 1, None) == INVALID and b"null" in lib.agx_last_error()
    for size in (4, 21, 0, -3):
        assert create(0, size, 4, 100, 1 << 12, 1, ctypes.byref(handle)) == UNSUPPORTED and not handle.value, size
    for budget in (0, 1001, -1):
        assert create(0, 15, 4, budget, 1 << 12, 1, ctypes.byref(handle)) == UNSUPPORTED and not handle.value, budget
    assert b"max_positions" in lib.agx_last_error()
    for rules in (-1, 5):
        assert create(rules, 15, 4, 100, 1 << 12, 1, ctypes.byref(handle)) == INVALID and not handle.value
    for capacity in (0, -1, (1 << 20) + 1):
        assert create(0, 15, capacity, 100, 1 << 12, 1, ctypes.byref(handle)) == INVALID and not handle.value
    assert create(0, 15, 4, 100, (1 << 32) + 1, 1, ctypes.byref(handle)) == INVALID and not handle.value and b"table" in lib.agx_last_error()
    from alphagomoku_amd import _lib
    assert lib.agx_position_solver_solve(None, 1, None, None, ctypes.byref(_lib.AgxSolvedPositions()), None) == INVALID
    assert lib.agx_position_solver_info(None, None, None, None) == INVALID
    assert lib.agx_position_solver_destroy(None) == 0
    assert lib.agx_position_evaluator_evaluate_solved(None, None, None, 1, None, None, 1, 0, 0, None, None, None) == INVALID
