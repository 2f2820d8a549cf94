"""float64 numpy restatement of the training loss of the heads and its logit gradients (include/agx.h: agx_head_loss_grad) for the
tests.  It takes the float32 arrays the device sees; every exponential, logarithm, product and sum is formed in float64 from them."""
import numpy as np

from net_score_ref import SAMPLE_DTYPE, TOTAL_DTYPE  # noqa: F401  (the record layouts are net_score's)


def head(logits, target):
    """one softmax over the 1-D `logits`: (sum over target > 0 of target * (lse - z), p * T - t with the targets that do not count as 0)"""
    z = np.asarray(logits, np.float32).astype(np.float64).reshape(-1)
    t = np.asarray(target, np.float32).reshape(-1)
    t = np.where(t > 0, t, np.float32(0.0)).astype(np.float64)      # selected, never multiplied: a NaN does not count
    m = z.max()
    lse = m + np.log(np.exp(z - m).sum())
    on = t > 0
    return float((t[on] * (lse - z[on])).sum()), np.exp(z - lse) * t.sum() - t


def spread(logits):
    """R of the tolerance: the largest |lse - z| of a head is below zmax - zmin + log(cells) <= zmax - zmin + 6"""
    z = np.asarray(logits, np.float64)
    return float(z.max() - z.min() + 6.0) if z.size else 6.0


def sample_loss(policy, value, policy_target, value_target, q=None, q_target=None):
    """policy [HW], value [3], q [HW, 3] logits or None; targets [HW], [3], [HW, 3].  Returns (record, gradients, spreads): gradients without
    the scale, spreads = R per head"""
    pt = np.asarray(policy_target, np.float32).reshape(-1)
    policy_ce, policy_grad = head(policy, pt)
    value_ce, value_grad = head(value, value_target)
    record = dict(policy_ce=policy_ce, value_ce=value_ce, q_ce=0.0, q_cells=0, topk_hit=[0, 0, 0, 0])
    grads = dict(policy=policy_grad, value=value_grad, q=None)
    spreads = dict(policy_ce=spread(policy), value_ce=spread(value), q_ce=6.0)
    if q is not None:
        q = np.asarray(q, np.float32).reshape(-1, 3)
        qt = np.asarray(q_target, np.float32).reshape(-1, 3)
        grads["q"] = np.zeros(q.shape, np.float64)                    # exactly 0 on the cells without an edge
        for cell in np.flatnonzero(pt > 0):
            ce, g = head(q[cell], qt[cell])
            record["q_ce"] += ce
            grads["q"][cell] = g
            spreads["q_ce"] = max(spreads["q_ce"], spread(q[cell]))
        record["q_cells"] = int((pt > 0).sum())
    return record, grads, spreads


def batch_loss(policy, value, policy_target, value_target, q=None, q_target=None):
    """(per-sample records, total, gradients, per-sample spreads) of a batch: arrays with a leading sample axis; gradients without the scale"""
    n = len(policy)
    out = [sample_loss(policy[b], value[b], policy_target[b], value_target[b], None if q is None else q[b], None if q is None else q_target[b]) for b in range(n)]
    records, grads, spreads = [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]
    total = dict(samples=n, policy_ce=0.0, value_ce=0.0, q_ce=0.0, q_cells=0, topk_hit=[0, 0, 0, 0])
    for r in records:
        for k in ("policy_ce", "value_ce", "q_ce", "q_cells"):
            total[k] += r[k]
    stacked = {k: None if grads[0][k] is None else np.stack([g[k] for g in grads]) for k in ("policy", "value", "q")}
    return records, total, stacked, spreads
