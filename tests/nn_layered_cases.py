"""Cases, networks and the storage-rounding restatement of the layered-tower tests (helper module of test_nn_layered_cpu.py /
test_nn_layered_gpu.py).

The exact-arithmetic machinery is nn_exact.py's, unchanged and generic in the filter count: exact_weights(), reference(), check_exact().
The boards are nn_any_board.py's (directed_boards for any shape: corners, edges, both sides of every 16-position tile seam)."""
import functools

import numpy as np

import nn_any_board as ab
import nn_exact as nx
from alphagomoku_amd import synthetic

WIDE = [192, 256, 320, 384, 448, 512]
KINDS = ["pv", "raw", "pvq"]
HEADS = ["random", "transparent"]
# 5x5: smaller than one 16-position tile per row, two tiles in all; 7x9: rows != cols, a position chunk and a half; 15x15; 20x20: the most
# tiles (F <= 256 and at most one block there: the numpy reference stays short).  192: six 32-channel k-chunks, three 64-channel wave tiles,
# no power of two; 256; 512: the maximum, on the two small boards
SHAPES = {192: [(5, 5), (7, 9), (15, 15), (20, 20)], 256: [(5, 5), (7, 9), (15, 15), (20, 20)], 512: [(5, 5), (7, 9)]}
SEED = 1
# where check_exact refuses seed 1 for a (rows, cols, filters, kind, blocks, heads), another seed goes here, the check unchanged (none so far)
OTHER_SEED = {}


def make_desc(rows, cols, filters, kind, blocks):
    return ab.make_desc(rows, cols, filters, kind, blocks)


def network_cases():
    """(rows, cols, filters, kind, blocks, heads) of every network the GPU file compares exactly: every (width, board) with 0, 1 and 2 blocks
    and both kinds of heads, the network kinds rotating so that every width sees every kind with every kind of heads"""
    cases, k = [], 0
    for filters, shapes in SHAPES.items():
        for rows, cols in shapes:
            for blocks in ((0, 1) if rows * cols == 400 else (0, 1, 2)):
                for heads in HEADS:
                    cases.append((rows, cols, filters, KINDS[k % 3], blocks, heads))
                    k += 1
            k += 1
    return cases


@functools.lru_cache(maxsize=4)
def weights(rows, cols, filters, kind, blocks, heads):
    desc = make_desc(rows, cols, filters, kind, blocks)
    return desc, nx.exact_weights(desc, OTHER_SEED.get((rows, cols, filters, kind, blocks, heads), SEED), heads)


BATCHES = ["random", "directed"]
# a launch longer than the activation planes hold (3799 boards at 192 filters on 5x5): the network, the boards, and the ones looked at exactly
SLICE_CASE = (5, 5, 192, "pvq", 1, "random")
SLICE_BOARDS, SLICE_SEAM = 4100, slice(3790, 3810)


@functools.lru_cache(maxsize=None)
def slice_pool():
    f = synthetic.random_features(SLICE_BOARDS, 5, 5, seed=77)
    f.setflags(write=False)
    return f


def feature_batch(rows, cols, kind):
    """nn_any_board.feature_batch ("random" | "directed" | "pool"), and "slice seam": the boards of slice_pool() on both sides of the seam"""
    return slice_pool()[SLICE_SEAM] if kind == "slice seam" else ab.feature_batch(rows, cols, kind)


# the launch-shape cases: (rows, cols, filters, kind) of 1-block networks with random heads on nn_any_board's 600-board pool
POOL_NETWORK = (1, "random")
SHAPE_NETWORKS = [(7, 9, 192, "pvq"), (7, 9, 256, "raw")]
# AGX_NN_LAYERED=1 against the default kernels: nn_exact's square networks and boards (seed 1) and one rectangle of nn_any_board's
SWITCH_CASES = [(15, 15, 64, "pvq"), (15, 15, 128, "raw"), (20, 20, 128, "pvq"), (20, 20, 64, "pv"), (7, 9, 128, "pvq"), (7, 9, 64, "raw")]


def exact_pairs():
    """every (network, inputs) pair of the GPU file: ((rows, cols, filters, kind, blocks, heads), batch name)"""
    pairs = [(case, batch) for case in network_cases() for batch in BATCHES]
    pairs += [((r, c, f, k) + POOL_NETWORK, "pool") for r, c, f, k in SHAPE_NETWORKS]
    pairs += [((r, c, f, k) + POOL_NETWORK, batch) for r, c, f, k in SWITCH_CASES for batch in BATCHES]
    pairs += [(SLICE_CASE, "slice seam")]
    return pairs


# ---------------------------------------------------------------------------------------------------------------------- He-init networks

HE_INIT_CASES = [(15, 15, 2, 192, "pvq"), (15, 15, 2, 256, "pv")]   # rows, cols, blocks, filters, kind
HE_INIT_RESIDUAL_GAIN = 0.5      # activations of order one like a trained tower's (synthetic.make_weights)
BASE_TOLERANCE = 1.0e-3          # the project's bound on softmax outputs (tests/test_nn_gpu.py)


def restatement(desc, blob, features, backwards=False):
    """oracle.nn_ref.forward(storage="fp16") restated with fp32 sums whose order can be turned round -> (policy [B, HW], value [B, 3]
    [, q [B, HW, 2]]), float64: weights that feed the matrix cores and every stored activation rounded to fp16, every channel / tap sum in
    fp32 (backwards: in the opposite order), bias and residual added behind it, the last 1x1 of policy / q, the value head's last dense
    layer and all biases unrounded."""
    rows, cols, F = desc["rows"], desc["cols"], desc["filters"]
    B, HW = len(features), rows * cols
    fp16 = lambda name: name.endswith((".w1", ".w2", "conv_in.w")) and name not in ("policy.w2", "q.w2")
    w = {k: (v.astype(np.float16).astype(np.float64) if fp16(k) else v) for k, v in nx.split(desc, blob).items()}
    flip = (lambda a, axis: np.flip(a, axis)) if backwards else (lambda a, axis: a)

    def store(a):
        return a.astype(np.float16).astype(np.float64)

    def lin(x, wt):
        return (np.ascontiguousarray(flip(x, -1)).astype(np.float32) @ np.ascontiguousarray(flip(wt, 0)).astype(np.float32)).astype(np.float64)

    def conv(x, wt, b, extra=None):
        k = wt.shape[0]
        xp = np.zeros((B, rows + k - 1, cols + k - 1, x.shape[-1]))
        xp[:, k // 2:k // 2 + rows, k // 2:k // 2 + cols] = x
        patches = np.concatenate([xp[:, dy:dy + rows, dx:dx + cols] for dy in range(k) for dx in range(k)], axis=-1)
        return lin(patches, wt.reshape(-1, wt.shape[-1])) + b + (0.0 if extra is None else extra)

    f = np.asarray(features, dtype=np.uint32).reshape(B, rows, cols, 1)
    C = desc["in_channels"]
    x = ((f >> np.arange(C, dtype=np.uint32).reshape(1, 1, 1, C)) & np.uint32(1)).astype(np.float64)
    x = store(np.maximum(conv(x, w["conv_in.w"], w["conv_in.b"]), 0.0))
    for i in range(desc["blocks"]):
        n = "block%d" % i
        y = store(np.maximum(conv(x, w[n + ".w1"], w[n + ".b1"]), 0.0))
        x = store(np.maximum(conv(y, w[n + ".w2"], w[n + ".b2"], extra=x), 0.0))
    p = store(np.maximum(conv(x, w["policy.w1"], w["policy.b1"]), 0.0))
    policy = (lin(p, w["policy.w2"].reshape(F, 1)) + w["policy.b2"][0]).reshape(B, HW)
    v = store(np.maximum(lin(x, w["value.w1"]) + w["value.b1"], 0.0)).reshape(B, HW * 4)
    h = np.maximum(lin(v, w["value.w2"]) + w["value.b2"], 0.0)
    value = lin(h, w["value.w3"]) + w["value.b3"]
    out = (nx.softmax(policy), nx.softmax(value))
    if desc.get("action_values", 0):
        t = store(np.tanh(conv(x, w["q.w1"], w["q.b1"])))
        q = (lin(t, w["q.w2"]) + w["q.b2"]).reshape(B, HW, 3)
        out = out + (nx.softmax(q)[:, :, :2],)
    return out


def tolerance(desc, blob, features, forwards=None):
    """-> (bounds, gaps) per output (policy, value[, q]), the derivation of nn_bottleneck_ref.tolerance: the gap is the largest difference
    between the restatement with every sum taken forwards and the same taken backwards — the restatement's own error on this network and
    these boards, measured on the CPU; the bound is BASE_TOLERANCE, or 4 x the gap where that is larger.  Never a value read off the device."""
    forwards = restatement(desc, blob, features) if forwards is None else forwards
    gaps = [float(np.abs(a - b).max()) for a, b in zip(forwards, restatement(desc, blob, features, backwards=True))]
    return [max(BASE_TOLERANCE, 4.0 * g) for g in gaps], gaps


def he_init_case(rows, cols, blocks, filters, kind):
    desc = make_desc(rows, cols, filters, kind, blocks)
    blob, _ = synthetic.make_weights(desc, residual_gain=HE_INIT_RESIDUAL_GAIN)
    return desc, blob, synthetic.random_features(4, rows, cols, seed=7)
