"""References, exact networks and cases of the bottleneck network tests (helper module of test_nn_bottleneck_cpu.py / test_nn_bottleneck_gpu.py).

BottleneckPV / BottleneckPVraw / BottleneckPVQ (the bottleneck block of csrc/nn_any_board.hip) are the residual networks with another block (blob layout of
include/agx.h):

    y = relu(W1 . x + b1)   1x1, F -> F/2      y = relu(W2 * y + b2)   3x3, F/2 -> F/2      x = relu(x + W3 * y + b3)   3x3, F/2 -> F

  * reference(): float64, written like nn_exact.reference (its convolution, its input block and heads word for word: with blocks = 0 the two
    agree bit for bit on any blob, which test_nn_bottleneck_cpu.py asserts);
  * exact_weights(): nn_exact.exact_weights' input block and heads around blocks that round nowhere: W1 and W2 sparse in {-1, 0, +1}, W3
    non-positive with a bias in 1..3 (a block adds at most 3); check_exact() holds nn_exact's conditions for all three layers of a block;
  * restatement(): what the kernel stores — fp16 weights for the matrix cores, fp16 activations behind ReLU / tanh — with fp32 sums, taken
    forwards or backwards; tolerance() is the bound of DESIGN 3.13 from the gap between the two.
"""
import functools

import numpy as np

import nn_any_board as ab
import nn_exact as nx
from alphagomoku_amd import synthetic

K1, K2 = nx.K1, nx.K2


# ------------------------------------------------------------------------------------------------------------------------ weights

def part_names(desc):
    names = ["conv_in.w", "conv_in.b"]
    for i in range(desc["blocks"]):
        names += ["block%d.%s" % (i, p) for p in ("w1", "b1", "w2", "b2", "w3", "b3")]
    names += ["policy.w1", "policy.b1", "policy.w2", "policy.b2", "value.w1", "value.b1", "value.w2", "value.b2", "value.w3", "value.b3"]
    if desc.get("action_values", 0):
        names += ["q.w1", "q.b1", "q.w2", "q.b2"]
    return names


def part_shapes(desc):
    """the blob layout of include/agx.h for AGX_ARCH_BOTTLENECK"""
    F, C, HW, D = desc["filters"], desc["in_channels"], desc["rows"] * desc["cols"], desc["value_hidden"]
    H = F // 2
    shapes = [(5, 5, C, F), (F,)]
    for _ in range(desc["blocks"]):
        shapes += [(F, H), (H,), (3, 3, H, H), (H,), (3, 3, H, F), (F,)]
    shapes += [(3, 3, F, F), (F,), (F,), (1,), (F, 4), (4,), (HW * 4, D), (D,), (D, 3), (3,)]
    if desc.get("action_values", 0):
        shapes += [(3, 3, F, F), (F,), (F, 3), (3,)]
    return shapes


def blob_floats(desc):
    return sum(int(np.prod(s)) for s in part_shapes(desc))


def split(desc, blob):
    """blob -> {name: float64 array}"""
    out, pos = {}, 0
    blob = np.asarray(blob)
    for name, shape in zip(part_names(desc), part_shapes(desc)):
        n = int(np.prod(shape))
        out[name] = blob[pos:pos + n].astype(np.float64).reshape(shape)
        pos += n
    assert pos == blob.size, "blob size does not fit the description"
    return out


def is_fp16_weight(name):
    """the weights that feed the matrix cores"""
    return name.endswith((".w1", ".w2", ".w3")) and name not in ("policy.w2", "q.w2", "value.w3") or name == "conv_in.w"


def resnet_desc(desc):
    """the residual description with the same input block and heads and no block"""
    return synthetic.net_desc(desc["rows"], desc["cols"], 0, desc["filters"], desc["in_channels"], desc.get("action_values", 0))


def exact_weights(desc, seed, heads="random"):
    """fp32 blob of a bottleneck network whose forward pass is exact in fp16 storage / fp32 accumulation: the input block and the heads are
    nn_exact.exact_weights' of the same description without blocks (q's first layer in multiples of 8 among them)"""
    F = desc["filters"]
    H = F // 2
    outer = nx.exact_weights(resnet_desc(desc), seed, heads)
    n_in = 25 * desc["in_channels"] * F + F
    rng = np.random.default_rng([seed, desc["rows"], desc["cols"], F, desc["blocks"], 77])

    def sparse(shape, k, values):
        fan_in, units = int(np.prod(shape[:-1])), shape[-1]
        w = np.zeros((fan_in, units))
        rows = rng.integers(0, fan_in, size=(k, units))
        w[rows, np.arange(units)[None, :]] = rng.choice(values, size=(k, units))
        return w.reshape(shape)

    def ints(n, lo, hi):
        return rng.integers(lo, hi + 1, size=n).astype(np.float64)

    parts = [outer[:n_in]]
    for _ in range(desc["blocks"]):
        parts += [sparse((F, H), K1, [-1.0, 1.0]), ints(H, 0, 2), sparse((3, 3, H, H), K1, [-1.0, 1.0]), ints(H, 0, 2),
                  sparse((3, 3, H, F), K2, [-1.0]), ints(F, 1, 3)]
    parts.append(outer[n_in:])
    blob = np.concatenate([np.asarray(p).reshape(-1) for p in parts]).astype(np.float32)
    assert blob.size == blob_floats(desc)
    return blob


def head_grids(desc, blob):
    w = split(desc, blob)
    g = {"policy": nx.dyadic_grid(w["policy.w2"], w["policy.b2"]), "value": nx.dyadic_grid(w["value.w3"], w["value.b3"])}
    if desc.get("action_values", 0):
        g["q"] = nx.dyadic_grid(w["q.w2"], w["q.b2"])
    return g


# ---------------------------------------------------------------------------------------------------------------------- reference

def reference(desc, blob, features, hook=None, stats=True):
    """float64 forward pass up to the logits -> nn_exact.Reference(policy [B, HW], value [B, 3], q [B, HW, 3] or None, per-layer stats).
    nn_exact.reference with the bottleneck block; stored outputs a hook sees: "conv_in", "block<i>.y1", "block<i>.y2", "block<i>",
    "policy.p", "q.t", "value.v", "value.h"."""
    rows, cols, HW = desc["rows"], desc["cols"], desc["rows"] * desc["cols"]
    w = split(desc, blob)
    if hook is None:
        def hook(name, array):
            return array
    collected = []

    def layer(name, out, terms):
        if stats:
            collected.append(nx.LayerStats(name, float(np.abs(out).max()), float((out > 0).mean()), float(terms().max())))
        return hook(name, out)

    def logits_stats(name, out, terms):
        if stats:
            collected.append(nx.LayerStats(name, float(np.abs(out).max()), 1.0, float(terms.max())))

    def per_channel(b):
        return b.reshape(-1, 1, 1, 1)

    def kernel(wname):
        a = w[wname]
        return a.reshape((1, 1) + a.shape) if a.ndim == 2 else a   # a 1x1 convolution [cin][cout]

    def conv(x, wname, bname):
        return nx._conv_same(x, kernel(wname)) + per_channel(w[bname])

    def conv_terms(x, wname, bname, extra=0.0):
        return lambda: nx._conv_same(np.abs(x), np.abs(kernel(wname))) + per_channel(np.abs(w[bname])) + extra

    def mix(x, m):
        return np.tensordot(x, m, axes=([0], [0]))

    f = np.asarray(features, dtype=np.uint32).reshape(-1, rows, cols)
    C = desc["in_channels"]
    bits = ((f[None] >> np.arange(C, dtype=np.uint32).reshape(C, 1, 1, 1)) & np.uint32(1)).astype(np.float64)
    xp = np.zeros((C, f.shape[0], rows + 4, cols + 4))
    xp[:, :, 2:2 + rows, 2:2 + cols] = bits
    x = layer("conv_in", np.maximum(nx._conv_padded(xp, w["conv_in.w"], rows, cols) + per_channel(w["conv_in.b"]), 0.0),
              lambda: nx._conv_padded(np.abs(xp), np.abs(w["conv_in.w"]), rows, cols) + per_channel(np.abs(w["conv_in.b"])))
    for i in range(desc["blocks"]):
        n = "block%d" % i
        y = layer(n + ".y1", np.maximum(conv(x, n + ".w1", n + ".b1"), 0.0), conv_terms(x, n + ".w1", n + ".b1"))
        y = layer(n + ".y2", np.maximum(conv(y, n + ".w2", n + ".b2"), 0.0), conv_terms(y, n + ".w2", n + ".b2"))
        x = layer(n, np.maximum(x + conv(y, n + ".w3", n + ".b3"), 0.0), conv_terms(y, n + ".w3", n + ".b3", np.abs(x)))
    p = layer("policy.p", np.maximum(conv(x, "policy.w1", "policy.b1"), 0.0), conv_terms(x, "policy.w1", "policy.b1"))
    policy = (mix(p, w["policy.w2"]) + w["policy.b2"][0]).reshape(-1, HW)
    logits_stats("policy.logits", policy, mix(np.abs(p), np.abs(w["policy.w2"])) + abs(w["policy.b2"][0]))
    v = layer("value.v", np.maximum(mix(x, w["value.w1"]) + w["value.b1"], 0.0).reshape(-1, HW, 4),
              lambda: mix(np.abs(x), np.abs(w["value.w1"])) + np.abs(w["value.b1"]))
    v = v.reshape(-1, HW * 4)
    h = layer("value.h", np.maximum(v.dot(w["value.w2"]) + w["value.b2"], 0.0), lambda: np.abs(v).dot(np.abs(w["value.w2"])) + np.abs(w["value.b2"]))
    value = h.dot(w["value.w3"]) + w["value.b3"]
    logits_stats("value.logits", value, np.abs(h).dot(np.abs(w["value.w3"])) + np.abs(w["value.b3"]))
    q = None
    if desc.get("action_values", 0):
        pre = conv(x, "q.w1", "q.b1")
        t = layer("q.t", np.tanh(pre), conv_terms(x, "q.w1", "q.b1"))
        q = (mix(t, w["q.w2"]) + w["q.b2"]).reshape(-1, HW, 3)
        if stats:
            collected.append(nx.LayerStats("q.pre", float(np.abs(pre).max()), float((pre > 0).mean()), 0.0))
        logits_stats("q.logits", q, mix(np.abs(t), np.abs(w["q.w2"])) + np.abs(w["q.b2"]))
    return nx.Reference(policy, value, q, collected)


def check_exact(desc, blob, features):
    """nn_exact.check_exact for a bottleneck network: the comparison of a device forward pass with reference() on these inputs is exact up
    to the softmax and not vacuous — every weight is an fp16 number, every stored activation (all three layers of a block included) an
    integer of at most 2048, every accumulation's sum of absolute terms below 2^24 units of the finest head grid, the logit spans bounded.
    Returns the Reference."""
    w = split(desc, blob)
    for name, a in w.items():
        assert np.array_equal(a.astype(np.float16).astype(np.float64), a), name
    grids = head_grids(desc, blob)
    seen = {}

    def keep(name, a):
        seen[name] = a
        return a
    ref = reference(desc, blob, features, hook=keep)
    names = [s.name for s in ref.stats]
    for i in range(desc["blocks"]):
        assert all("block%d%s" % (i, suffix) in names for suffix in (".y1", ".y2", ""))
    for s in ref.stats:
        where = "%s of %s" % (s.name, describe(desc))
        assert s.max_abs_sum < nx.MAX_ABS_SUM * min(grids.values()), where
        if s.name.endswith((".logits", ".pre")):
            continue
        assert s.max_abs <= nx.MAX_ACTIVATION, where
        if s.name != "q.t":
            assert s.positive_share >= nx.MIN_POSITIVE_SHARE, "%s: %.3f of the activations positive" % (where, s.positive_share)
    for name, a in seen.items():
        if name == "q.t":
            assert np.abs(a - np.round(a)).max() < 2.5e-7, name
        else:
            assert np.array_equal(a, np.round(a)), name
    span = ref.policy.max(axis=1) - ref.policy.min(axis=1)
    assert span.max() <= nx.MAX_SPAN, "policy logit span %.2f" % span.max()
    assert span.min() > 0.0 or desc["blocks"] == 0, "a constant policy"
    vspan = ref.value.max(axis=1) - ref.value.min(axis=1)
    assert vspan.max() <= nx.MAX_SPAN, "value logit span %.2f" % vspan.max()
    if ref.q is not None:
        qspan = ref.q.max(axis=2) - ref.q.min(axis=2)
        assert qspan.max() <= nx.MAX_Q_SPAN, "q logit span %.2f" % qspan.max()
        assert nx.softmax(ref.q).min() > 5.0e-3
    live = (nx.softmax(ref.value).min(axis=1) > nx.MIN_VALUE_PROBABILITY).mean()
    assert live >= 0.5, "value head saturated on %.0f %% of the boards" % (100.0 * (1.0 - live))
    return ref


# -------------------------------------------------------------------------------------------------------------------- restatement

BASE_TOLERANCE = 1.0e-3          # the project's bound on softmax outputs (tests/test_nn_gpu.py)


def restatement(desc, blob, features, backwards=False):
    """The storage-rounding restatement -> the outputs the device returns (policy [B, HW], value [B, 3][, q [B, HW, 2]]), float64: weights
    that feed the matrix cores and every stored activation (behind ReLU / tanh) rounded to fp16, sums in fp32 starting from nothing with the
    bias (and the residual) added in float64 behind them, the last 1x1 of policy / q, the value head's last dense layer and all biases in
    fp32 / float64.  backwards: every channel / tap sum taken in the opposite order."""
    rows, cols, F = desc["rows"], desc["cols"], desc["filters"]
    B, HW = len(features), rows * cols
    w = {k: (v.astype(np.float16).astype(np.float64) if is_fp16_weight(k) else v) for k, v in split(desc, blob).items()}
    flip = (lambda a, axis: np.flip(a, axis)) if backwards else (lambda a, axis: a)

    def store(a):
        return a.astype(np.float16).astype(np.float64)

    def lin(x, wt):
        return (np.ascontiguousarray(flip(x, -1)).astype(np.float32) @ np.ascontiguousarray(flip(wt, 0)).astype(np.float32)).astype(np.float64)

    def conv(x, wt, b, extra=None):
        """x [B, rows, cols, cin] (*) wt [k, k, cin, cout] or [cin, cout] + b (+ extra)"""
        if wt.ndim == 2:
            y = lin(x, wt)
        else:
            k = wt.shape[0]
            xp = np.zeros((B, rows + k - 1, cols + k - 1, x.shape[-1]))
            xp[:, k // 2:k // 2 + rows, k // 2:k // 2 + cols] = x
            patches = np.concatenate([xp[:, dy:dy + rows, dx:dx + cols] for dy in range(k) for dx in range(k)], axis=-1)
            y = lin(patches, wt.reshape(-1, wt.shape[-1]))
        return y + b + (0.0 if extra is None else extra)

    f = np.asarray(features, dtype=np.uint32).reshape(B, rows, cols, 1)
    C = desc["in_channels"]
    x = ((f >> np.arange(C, dtype=np.uint32).reshape(1, 1, 1, C)) & np.uint32(1)).astype(np.float64)
    x = store(np.maximum(conv(x, w["conv_in.w"], w["conv_in.b"]), 0.0))
    for i in range(desc["blocks"]):
        n = "block%d" % i
        y = store(np.maximum(conv(x, w[n + ".w1"], w[n + ".b1"]), 0.0))
        y = store(np.maximum(conv(y, w[n + ".w2"], w[n + ".b2"]), 0.0))
        x = store(np.maximum(conv(y, w[n + ".w3"], w[n + ".b3"], extra=x), 0.0))
    p = store(np.maximum(conv(x, w["policy.w1"], w["policy.b1"]), 0.0))
    policy = (lin(p, w["policy.w2"].reshape(F, 1)) + w["policy.b2"][0]).reshape(B, HW)
    v = store(np.maximum(conv(x, w["value.w1"], w["value.b1"]), 0.0)).reshape(B, HW * 4)
    h = np.maximum(lin(v, w["value.w2"]) + w["value.b2"], 0.0)
    value = lin(h, w["value.w3"]) + w["value.b3"]
    out = (nx.softmax(policy), nx.softmax(value))
    if desc.get("action_values", 0):
        t = store(np.tanh(conv(x, w["q.w1"], w["q.b1"])))
        q = (lin(t, w["q.w2"]) + w["q.b2"]).reshape(B, HW, 3)
        out = out + (nx.softmax(q)[:, :, :2],)
    return out


def tolerance(desc, blob, features, forwards=None):
    """-> (bounds, gaps) per output (policy, value[, q]): the gap is the largest difference between the restatement with every channel / tap
    sum taken forwards and the same taken backwards — the restatement's own error on this network and these boards, measured on the CPU;
    the bound is BASE_TOLERANCE, or 4 x the gap where that is larger.  Never a value read off the device."""
    forwards = restatement(desc, blob, features) if forwards is None else forwards
    gaps = [float(np.abs(a - b).max()) for a, b in zip(forwards, restatement(desc, blob, features, backwards=True))]
    return [max(BASE_TOLERANCE, 4.0 * g) for g in gaps], gaps


# --------------------------------------------------------------------------------------------------------------------------- cases

KINDS = ["pv", "raw", "pvq"]
# 5x5: waves without tiles; 8x8 with F = 64: one tile per wave in the full-width layers (the MFMA-settle case); 6x20 and 20x6: rows != cols both
# ways, one side at the maximum; 7x19: odd x odd; 15x15; 20x20 with F = 128: full accumulators, the largest plane
SHAPES = [(5, 5), (8, 8), (6, 20), (20, 6), (7, 19), (15, 15), (20, 20)]
HE_INIT_CASES = [(15, 15, 6, 128, "pvq"), (20, 20, 6, 128, "pv"), (9, 9, 2, 64, "raw")]   # rows, cols, blocks, filters, kind
HE_INIT_RESIDUAL_GAIN = 0.5      # activations of order one like a trained tower's (synthetic.make_weights)


def make_desc(rows, cols, filters, kind, blocks):
    return synthetic.bottleneck_desc(rows=rows, cols=cols, blocks=blocks, filters=filters, in_channels=8 if kind == "raw" else 32,
                                     action_values=1 if kind == "pvq" else 0)


def describe(desc):
    return "bottleneck %dx%d %dx%d cin %d%s" % (desc["rows"], desc["cols"], desc["blocks"], desc["filters"], desc["in_channels"],
                                                " +q" if desc.get("action_values", 0) else "")


# check_exact refuses seed 1 (and, at F = 64, seed 2) for the 3-block networks on 20x20 — 12.0 % of block 0's / 9.1 % of block 2's activations
# positive on the directed boards, the floor is 15 % —: another seed, the check unchanged (as nn_any_board.OTHER_SEED)
OTHER_SEED = {(20, 20, 64): 3, (20, 20, 128): 2}


def network_cases():
    """(rows, cols, filters, kind, blocks, heads, seed) of every network the GPU file compares exactly: every shape class with both filter
    counts as a 1-block network with random heads and as a 3-block network with transparent heads (every (cell, channel) of the last block's
    output observable), the kinds rotating; networks without a block; a second seed for the random heads"""
    cases = []
    for i, (r, c) in enumerate(SHAPES):
        for j, f in enumerate((64, 128)):
            cases.append((r, c, f, KINDS[(i + j) % 3], 1, "random", 1))
            cases.append((r, c, f, KINDS[(i + j + 1) % 3], 3, "transparent", OTHER_SEED.get((r, c, f), 1)))
    cases += [(8, 8, 64, "pvq", 0, "random", 1), (20, 20, 128, "pv", 0, "transparent", 1), (15, 15, 128, "raw", 0, "random", 2),
              (8, 8, 64, "pv", 1, "random", 2), (20, 20, 128, "pvq", 3, "random", 2), (7, 19, 64, "pvq", 3, "random", 2)]
    return cases


ENTRY_POINT_CASES = [(8, 16, 64, "pvq", 1, "random", 1), (8, 16, 128, "pvq", 1, "random", 1), (8, 16, 64, "pv", 1, "random", 1)]
BATCHES = ab.BATCHES                                            # "random", "directed": nn_any_board.feature_batch


@functools.lru_cache(maxsize=None)
def cached_weights(rows, cols, filters, kind, blocks, heads, seed):
    desc = make_desc(rows, cols, filters, kind, blocks)
    return desc, exact_weights(desc, seed, heads)


def features_of(rows, cols):
    """the directed boards (a stone in every corner and on every border column, every tile seam) and the random ones"""
    return np.concatenate([ab.feature_batch(rows, cols, kind) for kind in BATCHES])


@functools.lru_cache(maxsize=None)
def cached_reference(rows, cols, filters, kind, blocks, heads, seed):
    """computed once, shared by the tests that need it (check_exact included: the CPU file proves what the GPU file relies on)"""
    desc, blob = cached_weights(rows, cols, filters, kind, blocks, heads, seed)
    return check_exact(desc, blob, features_of(rows, cols))
