"""numpy float32 restatement of the combine step behind the solver (csrc/position_eval.hip: k_combine_solved_positions, agx.h:
agx_position_evaluator_evaluate_solved), and the oracle's threat solver on a fresh solver per position.  For the tests; not a test.

The sums over the symmetries, the masks, the renormalising sum and the top-k order are those of tests/position_eval_ref.py.  On top:
  unproven score   policy 0.0f outside the solver's action list; RENORMALISE by its rule over what is left; value: the network's
  proven score     value = (win, draw, loss) of the score; policy = 1.0f / k on the k actions whose 16-bit score is the largest in the
                   list, 0.0f elsewhere, not renormalised, no mask applied
  top_k picks      among the cells of the action list that are legal by the evaluator's rule (empty; not forbidden with MASK_FORBIDDEN)
  status           the larger of the solver's and the evaluator's word; either one's "bad input" zeroes everything"""
import ctypes

import numpy as np

import position_eval_ref as ref

F32 = np.float32
STATUS_BAD_INPUT, STATUS_SOLVER_ERROR = 1, 2
TF_MUST_DEFEND, TF_BY_SOLVER, TF_STATICALLY_SOLVED, TF_RECURSIVELY_SOLVED = 1, 4, 16, 32


def is_proven(score):
    """Score::isProven on the raw 16 bits: a proven-value class other than UNKNOWN (2) and neither infinity"""
    score = int(score)
    return ((score >> 13) & 3) != 2 and score not in (0, 0xFFFF)


def score_value(score):
    """(win, draw, loss) of a proven score, zeros when unproven"""
    out = np.zeros(3, F32)
    if is_proven(score):
        out[{3: 0, 1: 1, 0: 2}[(int(score) >> 13) & 3]] = F32(1.0)
    return out


def move_cell(move, n):
    """Move::toShort -> row * n + col"""
    return ((int(move) >> 2) & 127) * n + ((int(move) >> 9) & 127)


def combine_solved(n, board, mask, flags, top_k, policy_rows, value_rows, q_rows, feature_row0, score, moves, move_scores, status_eval=0, status_solver=0):
    """one position; `moves` / `move_scores` the solver's action list (its first n_actions entries).  Returns what position_eval_ref.combine
    returns, plus status."""
    hw = n * n
    status = max(int(status_eval), int(status_solver))
    if (status_eval & ref.STATUS_BAD_INPUT) or status_solver == STATUS_BAD_INPUT:
        out = ref.combine(n, board, mask, flags, top_k, policy_rows, value_rows, q_rows, feature_row0, ref.STATUS_BAD_INPUT)
        return dict(out, status=status)
    # the network's part: sums over the symmetries, masks; neither renormalised nor picked from yet
    base = ref.combine(n, board, mask, flags & ref.MASK_FORBIDDEN, 0, policy_rows, value_rows, q_rows, feature_row0, 0)
    legal = np.asarray(board).reshape(hw) == 0
    if flags & ref.MASK_FORBIDDEN:
        legal &= ((np.asarray(feature_row0, np.uint32).reshape(hw) >> 6) & 1) == 0
    cells = [move_cell(m, n) for m in moves]
    listed = np.zeros(hw, bool)
    listed[cells] = True
    policy, value = base["policy"].copy(), base["value"]
    if is_proven(score):
        value = score_value(score)
        policy = np.zeros(hw, F32)
        if len(cells):
            best = max(int(s) for s in move_scores)
            best_cells = [c for c, s in zip(cells, move_scores) if int(s) == best]
            policy[best_cells] = F32(F32(1.0) / F32(len(best_cells)))
    else:
        policy[~listed] = F32(0.0)
        if flags & ref.RENORMALISE:
            total = ref.ordered_sum(policy)
            if total != F32(0.0):
                policy = (policy * F32(F32(1.0) / total)).astype(F32)
    top_cells, top_probs = np.full(top_k, -1, np.int32), np.zeros(top_k, F32)
    key = np.where(np.isnan(policy), F32(-np.inf), policy)
    left = legal & listed
    for k in range(top_k):
        candidates = np.flatnonzero(left)
        if candidates.size == 0:
            break
        pick = candidates[int(np.argmax(key[candidates]))]   # the first of equal maxima: the lowest cell index
        top_cells[k], top_probs[k] = pick, policy[pick]
        left[pick] = False
    return dict(policy=policy, value=value, action_values=base["action_values"], top_cells=top_cells, top_probs=top_probs, status=status)


def oracle_solve(olib, rules, n, board, sign, max_positions, table_entries, zobrist_seed, keep=None):
    """ago_solver_solve on a new ago_solver_create(...) — or, with `keep` (a handle from ago_solver_create), on that solver and its table as
    it stands.  -> dict(n_actions, moves, move_scores, score, must_defend, nodes)"""
    import oracle_lib as ol
    hw = n * n
    handle = keep if keep is not None else olib.ago_solver_create(rules, n, n, table_entries, zobrist_seed, max_positions)
    b = np.ascontiguousarray(np.asarray(board, np.uint8).reshape(hw))
    feat, mv, sc = np.zeros(hw, np.uint32), np.zeros(hw, np.uint16), np.zeros(hw, np.uint16)
    fl, rs, nodes = ctypes.c_int(), ctypes.c_uint16(), ctypes.c_int()
    count = olib.ago_solver_solve(handle, ol.ptr(b), int(sign), ol.ptr(feat), ol.ptr(mv), ol.ptr(sc), ctypes.byref(fl), ctypes.byref(rs), ctypes.byref(nodes))
    if keep is None:
        olib.ago_solver_destroy(handle)
    return dict(n_actions=count, moves=mv[:count].copy(), move_scores=sc[:count].copy(), score=rs.value, must_defend=bool(fl.value & 1), nodes=nodes.value)


def expected_flags(result):
    """the task flags of a solve: processed by the solver; must defend; statically solved = at most one node; recursively solved = proven"""
    return (TF_BY_SOLVER | (TF_MUST_DEFEND if result["must_defend"] else 0) | (TF_STATICALLY_SOLVED if result["nodes"] <= 1 else 0)
            | (TF_RECURSIVELY_SOLVED if is_proven(result["score"]) else 0))
