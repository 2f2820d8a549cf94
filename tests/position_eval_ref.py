"""numpy float32 restatement of the combine step of csrc/position_eval.hip (agx.h: agx_position_evaluator_*), for the tests.  Not a test.

Rows are the tower's outputs for the (position, symmetry) rows p * S + j, j the rank of symmetry s in the mask.  Everything below is done
in float32 in the order the kernel uses: ascending s from 0.0f, then * (1.0f / S); the renormalising sum in cell order, one addition after
the other; the top-k by (value, lowest cell index)."""
import numpy as np

MASK_FORBIDDEN, RENORMALISE = 1, 2
STATUS_BAD_INPUT = 1
F32 = np.float32


def symmetry_source(s, n, r, c):
    """utils/augmentations.hpp for square boards: the cell of the board that cell (r, c) of the board under symmetry s shows"""
    last = n - 1
    return [(r, c), (last - r, c), (r, last - c), (last - r, last - c), (c, r), (last - c, last - r), (c, last - r), (last - c, r)][s]


def symmetries_of(mask):
    return [s for s in range(8) if (mask >> s) & 1]


def image_map(s, n):
    """image[c]: the cell of the board under symmetry s that shows cell c of the untransformed board"""
    image = np.zeros(n * n, np.int64)
    for i in range(n * n):
        sr, sc = symmetry_source(s, n, i // n, i % n)
        image[sr * n + sc] = i
    return image


def transform_board(board, s):
    """the board under symmetry s (what ago_apply_symmetry gives)"""
    b = np.asarray(board)
    n = b.shape[0]
    out = np.empty_like(b)
    for r in range(n):
        for c in range(n):
            out[r, c] = b[symmetry_source(s, n, r, c)]
    return out


def ordered_sum(values):
    """float32 sum in index order, one addition after the other, from 0.0f"""
    total = F32(0.0)
    for v in np.asarray(values, F32).reshape(-1):
        total = F32(total + v)
    return total


def combine(n, board, mask, flags, top_k, policy_rows, value_rows, q_rows=None, feature_row0=None, status=0):
    """one position: board [n, n] of 0 / 1 / 2; policy_rows [S, n * n], value_rows [S, 3], q_rows [S, n * n, 2] or None; feature_row0 the
    identity row's feature words (needed with MASK_FORBIDDEN).  Returns policy [n * n], value [3], action_values [n * n, 2] or None,
    top_cells [top_k] int32, top_probs [top_k]."""
    hw = n * n
    syms = symmetries_of(mask)
    S = len(syms)
    if status & STATUS_BAD_INPUT:
        return dict(policy=np.zeros(hw, F32), value=np.zeros(3, F32), action_values=None if q_rows is None else np.zeros((hw, 2), F32),
                    top_cells=np.full(top_k, -1, np.int32), top_probs=np.zeros(top_k, F32))
    policy_rows = np.asarray(policy_rows, F32).reshape(S, hw)
    value_rows = np.asarray(value_rows, F32).reshape(S, 3)
    inv = F32(F32(1.0) / F32(S))
    policy, value = np.zeros(hw, F32), np.zeros(3, F32)
    q = None if q_rows is None else np.zeros((hw, 2), F32)
    for j, s in enumerate(syms):
        image = image_map(s, n)
        policy = (policy + policy_rows[j][image]).astype(F32)
        value = (value + value_rows[j]).astype(F32)
        if q is not None:
            q = (q + np.asarray(q_rows, F32).reshape(S, hw, 2)[j][image]).astype(F32)
    policy, value = (policy * inv).astype(F32), (value * inv).astype(F32)
    if q is not None:
        q = (q * inv).astype(F32)
    legal = np.asarray(board).reshape(hw) == 0
    if flags & MASK_FORBIDDEN:
        assert 0 in syms
        legal &= ((np.asarray(feature_row0, np.uint32).reshape(hw) >> 6) & 1) == 0
    policy[~legal] = F32(0.0)
    if flags & RENORMALISE:
        total = ordered_sum(policy)
        if total != F32(0.0):
            policy = (policy * F32(F32(1.0) / total)).astype(F32)
    top_cells, top_probs = np.full(top_k, -1, np.int32), np.zeros(top_k, F32)
    key = np.where(np.isnan(policy), F32(-np.inf), policy)
    left = legal.copy()
    for k in range(top_k):
        cells = np.flatnonzero(left)
        if cells.size == 0:
            break
        best = cells[int(np.argmax(key[cells]))]   # argmax: the first of equal maxima, i.e. the lowest cell index
        top_cells[k], top_probs[k] = best, policy[best]
        left[best] = False
    return dict(policy=policy, value=value, action_values=q, top_cells=top_cells, top_probs=top_probs)
