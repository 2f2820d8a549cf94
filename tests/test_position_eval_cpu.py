"""tests/position_eval_ref.py, the numpy restatement of the combine step of csrc/position_eval.hip, against values worked out by hand on a
5x5 toy board, and its symmetry maps against the oracle's ago_apply_symmetry.  (The device kernel is compared with the restatement, on
the bits, in tests/test_position_eval_gpu.py.)"""
import numpy as np
import pytest

import oracle_lib as ol
import position_eval_ref as ref

N, HW = 5, 25
F32 = np.float32


def rows_with(entries, rows=1):
    out = np.zeros((rows, HW), F32)
    for (j, cell), v in entries.items():
        out[j, cell] = v
    return out


def test_no_flags_masks_the_occupied_cells_only():
    board = np.zeros((N, N), np.uint8)
    board[1, 2] = 1                                                    # cell 7
    rows = rows_with({(0, 7): 0.5, (0, 8): 0.25, (0, 24): 0.125})
    out = ref.combine(N, board, 0x01, 0, 2, rows, [[0.5, 0.25, 0.25]])
    want = np.zeros(HW, F32)
    want[8], want[24] = 0.25, 0.125                                    # the stone's 0.5 is gone, nothing is rescaled
    assert np.array_equal(out["policy"], want) and np.array_equal(out["value"], np.array([0.5, 0.25, 0.25], F32))
    assert out["top_cells"].tolist() == [8, 24] and out["top_probs"].tolist() == [0.25, 0.125]


def test_two_symmetries_are_added_in_ascending_order_and_divided():
    """identity and FLIP_VERTICALLY (row r shows row 4 - r): cell (1, 2) = 7 lies at (3, 2) = 17 in the flipped row"""
    board = np.zeros((N, N), np.uint8)
    rows = rows_with({(0, 7): 0.5, (1, 17): 0.25, (1, 7): 1.0}, rows=2)
    values = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.0]]
    q = np.zeros((2, HW, 2), F32)
    q[0, 7], q[1, 17] = (0.5, 0.25), (0.25, 0.25)
    out = ref.combine(N, board, 0x03, 0, 0, rows, values, q_rows=q)
    assert out["policy"][7] == F32(0.375)                              # (0.5 + 0.25) * 0.5
    assert out["policy"][17] == F32(0.5)                               # the flipped row's cell 7 is the board's cell 17: (0 + 1.0) * 0.5
    assert np.array_equal(out["value"], np.array([0.75, 0.25, 0.0], F32))
    assert out["action_values"][7].tolist() == [0.375, 0.25]


@pytest.mark.parametrize("s,row_cell", [(1, 21), (2, 3), (3, 23), (4, 5), (5, 19), (6, 15), (7, 9)])
def test_one_symmetry_is_mapped_back_in_the_right_direction(s, row_cell):
    """cell (0, 1) = 1 of the board, by hand from utils/augmentations.hpp (cell (r, c) of the transformed board shows ...):
    1 FLIP_VERTICALLY (4 - r, c): seen at (4, 1) = 21;  2 FLIP_HORIZONTALLY (r, 4 - c): (0, 3) = 3;  3 ROTATE_180: (4, 3) = 23;
    4 FLIP_DIAGONALLY (c, r): (1, 0) = 5;  5 FLIP_ANTIDIAGONALLY (4 - c, 4 - r): (3, 4) = 19;  6 ROTATE_90 (c, 4 - r): (3, 0) = 15;
    7 ROTATE_270 (4 - c, r): (1, 4) = 9"""
    out = ref.combine(N, np.zeros((N, N), np.uint8), 1 << s, 0, 1, rows_with({(0, row_cell): 1.0}), [[0.0, 0.0, 1.0]])
    assert out["policy"][1] == F32(1.0) and out["top_cells"].tolist() == [1]


def test_forbidden_flag_takes_the_foul_out_of_the_policy_and_the_picks():
    board = np.zeros((N, N), np.uint8)
    features = np.full(HW, 1 | 8 | 16, np.uint32)
    features[3] |= 1 << 6
    rows = rows_with({(0, 3): 0.5, (0, 4): 0.25})
    plain = ref.combine(N, board, 0x01, 0, 1, rows, [[0, 0, 1]], feature_row0=features)
    assert plain["policy"][3] == F32(0.5) and plain["top_cells"].tolist() == [3]
    out = ref.combine(N, board, 0x01, ref.MASK_FORBIDDEN, 2, rows, [[0, 0, 1]], feature_row0=features)
    assert out["policy"][3] == 0.0 and out["policy"][4] == F32(0.25)
    assert out["top_cells"].tolist() == [4, 0] and out["top_probs"].tolist() == [0.25, 0.0]   # then the lowest legal cell: 3 is never picked


def test_renormalise_scales_the_survivors_and_a_tie_goes_to_the_lower_cell():
    board = np.zeros((N, N), np.uint8)
    board[0, 2] = 2
    rows = rows_with({(0, 0): 0.25, (0, 1): 0.25, (0, 2): 0.5})
    out = ref.combine(N, board, 0x01, ref.RENORMALISE, 3, rows, [[0, 0, 1]])
    want = np.zeros(HW, F32)
    want[0] = want[1] = 0.5                                            # sum 0.5, every value * (1 / 0.5)
    assert np.array_equal(out["policy"], want)
    assert out["top_cells"].tolist() == [0, 1, 3] and out["top_probs"].tolist() == [0.5, 0.5, 0.0]   # cell 2 holds a stone


def test_renormalise_with_a_zero_sum_leaves_zeros():
    board = np.zeros((N, N), np.uint8)
    board[0, 0] = 1
    out = ref.combine(N, board, 0x01, ref.RENORMALISE, 2, rows_with({(0, 0): 1.0}), [[0, 0, 1]])
    assert not np.isnan(out["policy"]).any() and not out["policy"].any()
    assert out["top_cells"].tolist() == [1, 2] and out["top_probs"].tolist() == [0.0, 0.0]


def test_fewer_legal_cells_than_picks():
    board = np.ones((N, N), np.uint8)
    board[2, 2] = board[4, 0] = 0                                      # cells 12 and 20
    out = ref.combine(N, board, 0x01, 0, 4, rows_with({(0, 20): 0.75, (0, 12): 0.125, (0, 0): 0.125}), [[0, 0, 1]])
    assert out["top_cells"].tolist() == [20, 12, -1, -1] and out["top_probs"].tolist() == [0.75, 0.125, 0.0, 0.0]
    full = ref.combine(N, np.ones((N, N), np.uint8), 0x01, ref.RENORMALISE, 1, rows_with({(0, 0): 1.0}), [[0, 0, 1]])
    assert full["top_cells"].tolist() == [-1] and not full["policy"].any()


def test_bad_input_gives_zero_outputs():
    out = ref.combine(N, np.zeros((N, N), np.uint8), 0x01, 0, 2, rows_with({(0, 0): 1.0}), [[1, 0, 0]], status=ref.STATUS_BAD_INPUT)
    assert not out["policy"].any() and not out["value"].any() and out["top_cells"].tolist() == [-1, -1]


def test_ordered_sum_is_sequential_float32():
    values = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24], F32)
    assert ref.ordered_sum(values) == F32(1.0)                         # each small addend is lost on its own; a pairwise sum would keep them
    assert ref.ordered_sum(values[::-1]) > F32(1.0)


@pytest.mark.parametrize("n", [15, 20])
def test_symmetry_maps_against_the_oracle(n):
    olib = ol.load()
    cells = np.arange(n * n, dtype=np.uint32)
    for s in range(8):
        shown = np.zeros(n * n, np.uint32)
        olib.ago_apply_symmetry(n, s, 0, ol.ptr(cells), ol.ptr(shown))   # shown[i]: the board's cell that cell i of the transformed board shows
        image = ref.image_map(s, n)
        assert np.array_equal(image[shown], np.arange(n * n)), s
        assert np.array_equal(ref.transform_board(cells.reshape(n, n), s).reshape(-1), shown), s
    assert ref.symmetries_of(0x24) == [2, 5] and ref.symmetries_of(0xFF) == list(range(8))
