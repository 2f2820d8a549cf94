"""float64 numpy restatement of the network score (include/agx.h: agx_net_score_*) for the tests.  It takes the float32 arrays the
device sees: every product and logarithm is formed in float64 from them — only the loss class of the action-value OUTPUT is the float32
expression 1.0f - win - draw, which is part of the definition."""
import numpy as np

FLT_MIN = np.float64(np.finfo(np.float32).tiny)

SAMPLE_DTYPE = np.dtype([("policy_ce", "<f8"), ("value_ce", "<f8"), ("q_ce", "<f8"), ("q_cells", "<i4"), ("topk_hit", "<i4", (4,)), ("reserved", "<i4")])
TOTAL_DTYPE = np.dtype([("samples", "<i8"), ("policy_ce", "<f8"), ("value_ce", "<f8"), ("q_ce", "<f8"), ("q_cells", "<i8"), ("topk_hit", "<i8", (4,))])
assert SAMPLE_DTYPE.itemsize == 48 and TOTAL_DTYPE.itemsize == 72


def cross_entropy(target, output):
    """- sum over the entries with target > 0 of target * log(max(output, FLT_MIN))"""
    t, p = np.asarray(target, np.float32).reshape(-1), np.asarray(output, np.float32).reshape(-1)
    on = t > 0
    return float(-(t[on].astype(np.float64) * np.log(np.maximum(p[on].astype(np.float64), FLT_MIN))).sum())


def first_max(values):
    """std::max_element: the first of the largest values.  It compares with <, which is false for a NaN on either side, so a NaN on cell 0
    stays the maximum and a NaN anywhere else never becomes it (np.argmax alone would pick a NaN wherever it is)."""
    v = np.asarray(values, np.float32).reshape(-1)
    if np.isnan(v[0]):
        return 0
    return int(np.argmax(np.where(np.isnan(v), -np.inf, v)))


def topk_hits(output, target, top_k=4):
    """getAccuracy's inner loop for one sample: cumulative hits per rank"""
    out = np.array(output, np.float32).reshape(-1)
    correct = first_max(target)
    hits = [0] * top_k
    for rank in range(top_k):
        best = first_max(out)
        if best == correct:
            for m in range(rank, top_k):
                hits[m] += 1
        out[best] = 0.0
    return hits


def get_accuracy_transcribed(batch_size, outputs, targets, rows, cols, top_k):
    """NetworkDataPack.cpp:321-345 and misc.cpp:79-83, statement by statement, on Python lists of numpy.float32"""
    def max_element(m):
        largest = 0
        for it in range(1, len(m)):
            if m[largest] < m[it]:
                largest = it
        return largest

    def pick_move(m):
        idx = max_element(m)
        return (idx // cols, idx % cols)

    result = [0.0] * (1 + top_k)
    for b in range(batch_size):
        output = [np.float32(x) for x in outputs[b]]
        answer = [np.float32(x) for x in targets[b]]
        correct = pick_move(answer)
        for l in range(top_k):   # noqa: E741
            best = pick_move(output)
            if correct == best:
                for m in range(l, top_k):
                    result[1 + m] += 1
            output[best[0] * cols + best[1]] = np.float32(0.0)
        result[0] += 1
    return result


def sample_score(policy, value, policy_target, value_target, q=None, q_target=None):
    """policy [HW], value [3], q [HW, 2] = (win, draw) or None; targets [HW], [3], [HW, 3]"""
    pt = np.asarray(policy_target, np.float32).reshape(-1)
    out = dict(policy_ce=cross_entropy(pt, policy), value_ce=cross_entropy(value_target, value), q_ce=0.0, q_cells=0, topk_hit=topk_hits(policy, pt))
    if q is not None:
        q = np.asarray(q, np.float32).reshape(-1, 2)
        qt = np.asarray(q_target, np.float32).reshape(-1, 3)
        edge = pt > 0
        loss = np.float32(1.0) - q[:, 0] - q[:, 1]                       # float32, left to right: Value::loss_rate
        classes = np.stack([q[:, 0], q[:, 1], loss], axis=1)[edge].astype(np.float64)
        out["q_ce"] = float(-(qt[edge].astype(np.float64) * np.log(np.maximum(classes, FLT_MIN))).sum())
        out["q_cells"] = int(edge.sum())
    return out


def batch_score(policy, value, policy_target, value_target, q=None, q_target=None):
    """(per-sample records, total) of a batch: arrays with a leading sample axis"""
    n = len(policy)
    records = [sample_score(policy[b], value[b], policy_target[b], value_target[b], None if q is None else q[b], None if q is None else q_target[b]) for b in range(n)]
    total = dict(samples=n, policy_ce=0.0, value_ce=0.0, q_ce=0.0, q_cells=0, topk_hit=[0, 0, 0, 0])
    for r in records:
        for k in ("policy_ce", "value_ce", "q_ce", "q_cells"):
            total[k] += r[k]
        total["topk_hit"] = [a + b for a, b in zip(total["topk_hit"], r["topk_hit"])]
    return records, total
