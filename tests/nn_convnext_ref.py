"""References, exact networks and inputs of the ConvNeXt network tests (helper module of test_nn_convnext_cpu.py / test_nn_convnext_gpu.py).

reference(desc, blob, features) is the graph of include/agx.h (ConvNextPVQraw / PVQMraw, batch norms folded) in float64, logits out.
With storage="fp16" it is the restatement of what csrc/nn_convnext.hip stores: activations rounded to fp16 where the kernel stores them
(the input conv's output, the depthwise output, relu(y1), the gated block output, every head's hidden 1x1 activation), fp16 weights where
the kernel uses them (input conv, depthwise, every 1x1 with F inputs), everything else - the pooled means, the SE layers, the dense layers
of the value and moves-left heads, the final 1x1 of the policy and q heads, all biases - unrounded.  acc=np.float32 carries every
accumulation in fp32 as the kernel does; backwards=True takes every channel / tap sum in the opposite order (the reference's own
sensitivity to the order of summation, from which the tolerance of the GPU test is derived).

Exact networks (exact_weights): weights in {-1, 0, +1} and sparse, biases small integers, the second 1x1 of a block non-positive (the
ReLU-less residual stream stays bounded), head weights on a dyadic grid, and squeeze-and-excitation gates that are 0.5, 1 or 0:
  "constant"  Ws2 = 0, bs2 in {0, +64, -64}: the same gates on any board.
  "live"      on boards whose cell count is a power of two the pooled means are exact; a live channel has bs2 = -64 and one weight 2^20 on
              a hidden unit that is 0 or at least 2^-11 (the grid of the means), so every pre-sigmoid is 0, -64 or >= 64 and the gate
              depends on the board.
sigmoid(64) is 1 in float64 and in fp32; sigmoid(-64) is 1.6e-28, and x * 1.6e-28 is stored as 0 by the kernel and differs from 0 by less
than 1e-20 in the float64 reference: check_exact allows a stored activation that much distance from an fp16 number, nothing more.
"""
import functools
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphagomoku_amd import synthetic  # noqa: E402

ML_FILTERS, ML_HIDDEN, VALUE_HIDDEN = 32, 128, 256
FP16_WEIGHTS = ("conv_in.w", ".wd", ".w1")          # + a block's .w2 (the heads' .w2 are fp32)
HEAD_GRID = 1.0 / 64.0
SIGMOID_TAIL = 1.0e-20
BIG = 2.0 ** 20


def part_shapes(desc):
    """[(name, shape)] in blob order"""
    F, HW = desc["filters"], desc["rows"] * desc["cols"]
    out = [("conv_in.w", (5, 5, 8, F)), ("conv_in.b", (F,))]
    for i in range(desc["blocks"]):
        out += [("block%d.wd" % i, (7, 7, F)), ("block%d.bd" % i, (F,)), ("block%d.w1" % i, (F, F)), ("block%d.b1" % i, (F,)),
                ("block%d.w2" % i, (F, F)), ("block%d.b2" % i, (F,)), ("block%d.ws1" % i, (F, F)), ("block%d.bs1" % i, (F,)),
                ("block%d.ws2" % i, (F, F)), ("block%d.bs2" % i, (F,))]
    out += [("policy.w1", (F, F)), ("policy.b1", (F,)), ("policy.w2", (F,)), ("policy.b2", (1,))]
    out += [("value.w1", (F, F)), ("value.b1", (F,)), ("value.w2", (F, VALUE_HIDDEN)), ("value.b2", (VALUE_HIDDEN,)),
            ("value.w3", (VALUE_HIDDEN, 3)), ("value.b3", (3,))]
    out += [("q.w1", (F, F)), ("q.b1", (F,)), ("q.w2", (F, 3)), ("q.b2", (3,))]
    if desc.get("moves_left", 0):
        out += [("m.w1", (F, ML_FILTERS)), ("m.b1", (ML_FILTERS,)), ("m.w2", (ML_FILTERS, ML_HIDDEN)), ("m.b2", (ML_HIDDEN,)),
                ("m.w3", (ML_HIDDEN, HW)), ("m.b3", (HW,))]
    return out


def blob_floats(desc):
    return sum(int(np.prod(s)) for _, s in part_shapes(desc))


def split(desc, blob):
    w, at = {}, 0
    for name, shape in part_shapes(desc):
        n = int(np.prod(shape))
        w[name] = np.asarray(blob[at:at + n], dtype=np.float64).reshape(shape)
        at += n
    assert at == len(blob)
    return w


def join(desc, w):
    return np.concatenate([np.asarray(w[name], dtype=np.float32).reshape(-1) for name, _ in part_shapes(desc)])


def is_fp16_weight(name):
    return name.endswith(FP16_WEIGHTS) or (name.startswith("block") and name.endswith(".w2"))


def unpack_low_byte(features, rows, cols):
    f = np.asarray(features, dtype=np.uint32)
    return ((f[:, :, None] >> np.arange(8, dtype=np.uint32)) & 1).astype(np.float64).reshape(len(f), rows, cols, 8)


def lowest_bit(a):
    """the largest power of two that divides every element of a (inf for an all-zero array)"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    a = a[a != 0]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(np.abs(a))
    ints = (m * 2.0 ** 53).astype(np.int64)
    return float(np.min((ints & -ints).astype(np.float64) * np.exp2(e.astype(np.float64) - 53)))


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def reference(desc, blob, features, storage=None, acc=np.float64, backwards=False, hook=None, stats=None):
    """-> namespace(policy [B, HW], value [B, 3], q [B, HW, 3], m [B, HW] or None): logits, float64.
    hook(name, array): called with every STORED activation before it is rounded.  stats: a dict that receives, per accumulation, the
    largest sum of absolute terms and the grid (power of two) its terms lie on - what check_exact asserts on."""
    rows, cols, F, B = desc["rows"], desc["cols"], desc["filters"], len(features)
    HW = rows * cols
    w = split(desc, blob)
    if storage == "fp16":
        w = {k: (v.astype(np.float16).astype(np.float64) if is_fp16_weight(k) else v) for k, v in w.items()}
    flip = (lambda a, axis: np.flip(a, axis)) if backwards else (lambda a, axis: a)

    def store(name, a):
        if hook is not None:
            hook(name, a)
        return a.astype(np.float16).astype(np.float64) if storage == "fp16" else a

    def grid(a):                                                # (x * sigmoid(-64) counts as the 0 the kernel stores)
        return lowest_bit(np.where(np.abs(a) <= SIGMOID_TAIL, 0.0, a))

    def note(name, x, wt, b, out_terms):
        if stats is not None:
            stats[name] = (float(out_terms.max()), min(grid(x) * lowest_bit(wt), grid(b)))

    def lin(name, x, wt, b, extra=None):
        """x [..., in] . wt [in, out] + b (+ extra)"""
        y = (flip(x, -1).astype(acc) @ flip(wt, 0).astype(acc)).astype(np.float64) + b
        if extra is not None:
            y = y + extra
        if stats is not None:
            note(name, x, wt, b if extra is None else np.concatenate([np.ravel(b), np.ravel(extra)]),
                 np.abs(x) @ np.abs(wt) + np.abs(b) + (0.0 if extra is None else np.abs(extra)))
        return y

    def depthwise(name, x, wd, bd):
        xp = np.zeros((B, rows + 6, cols + 6, F))
        xp[:, 3:3 + rows, 3:3 + cols] = x
        y = np.zeros((B, rows, cols, F), dtype=acc)
        terms = np.zeros((B, rows, cols, F)) + np.abs(bd)
        taps = [(dy, dx) for dy in range(7) for dx in range(7)]
        for dy, dx in (taps[::-1] if backwards else taps):
            y += (xp[:, dy:dy + rows, dx:dx + cols] * wd[dy, dx]).astype(acc)
            if stats is not None:
                terms += np.abs(xp[:, dy:dy + rows, dx:dx + cols] * wd[dy, dx])
        note(name, x, wd, bd, terms)
        return y.astype(np.float64) + bd

    x = unpack_low_byte(features, rows, cols)
    xp = np.zeros((B, rows + 4, cols + 4, 8))
    xp[:, 2:2 + rows, 2:2 + cols] = x
    patches = np.concatenate([xp[:, dy:dy + rows, dx:dx + cols] for dy in range(5) for dx in range(5)], axis=-1)
    x = store("conv_in", np.maximum(lin("conv_in", patches, w["conv_in.w"].reshape(200, F), w["conv_in.b"]), 0.0))
    gates = []
    for i in range(desc["blocks"]):
        n = "block%d" % i
        y = store(n + ".y", depthwise(n + ".y", x, w[n + ".wd"], w[n + ".bd"]))
        y = store(n + ".y1", np.maximum(lin(n + ".y1", y, w[n + ".w1"], w[n + ".b1"]), 0.0))
        x = lin(n + ".x", y, w[n + ".w2"], w[n + ".b2"], extra=x)
        mean = flip(x.reshape(B, HW, F), 1).astype(acc).sum(axis=1).astype(np.float64) / HW
        if stats is not None:
            stats[n + ".mean"] = (float(np.abs(x).reshape(B, HW, F).sum(axis=1).max()), grid(x))
        h = np.maximum(lin(n + ".se1", mean, w[n + ".ws1"], w[n + ".bs1"]), 0.0)
        saved, stats = stats, None                              # (the gate layer need not be exact: only which side of 0 / +-64 it lands on matters)
        z = lin(n + ".se2", h, w[n + ".ws2"], w[n + ".bs2"])
        stats = saved
        gates.append(z)
        x = store(n + ".x", x * sigmoid(z)[:, None, None, :])
    x = x.reshape(B, HW, F)
    out = types.SimpleNamespace(gates=gates, m=None)
    h = store("policy.h", np.maximum(lin("policy.h", x, w["policy.w1"], w["policy.b1"]), 0.0))
    out.policy = lin("policy.logits", h, w["policy.w2"].reshape(F, 1), w["policy.b2"])[:, :, 0]
    h = store("value.h", np.maximum(lin("value.h", x, w["value.w1"], w["value.b1"]), 0.0))
    mean = flip(h, 1).astype(acc).sum(axis=1).astype(np.float64) / HW
    if stats is not None:
        stats["value.mean"] = (float(np.abs(h).sum(axis=1).max()), grid(h))
    h = np.maximum(lin("value.hidden", mean, w["value.w2"], w["value.b2"]), 0.0)
    out.value = lin("value.logits", h, w["value.w3"], w["value.b3"])
    h = store("q.h", np.maximum(lin("q.h", x, w["q.w1"], w["q.b1"]), 0.0))
    out.q = lin("q.logits", h, w["q.w2"], w["q.b2"])
    if desc.get("moves_left", 0):
        h = store("m.h", np.maximum(lin("m.h", x, w["m.w1"], w["m.b1"]), 0.0))
        mean = flip(h, 1).astype(acc).sum(axis=1).astype(np.float64) / HW
        if stats is not None:
            stats["m.mean"] = (float(np.abs(h).sum(axis=1).max()), grid(h))
        h = np.maximum(lin("m.hidden", mean, w["m.w2"], w["m.b2"]), 0.0)
        out.m = lin("m.logits", h, w["m.w3"], w["m.b3"])
    return out


def softmax(logits, axis=-1):
    z = logits - logits.max(axis=axis, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=axis, keepdims=True)


def reference_outputs(ref):
    """what the device returns for these logits, in float64: policy, value, q (win, draw)[, moves_left]"""
    out = (softmax(ref.policy), softmax(ref.value), softmax(ref.q)[:, :, :2])
    return out if ref.m is None else out + (softmax(ref.m),)


BASE_TOLERANCE = 1.0e-3          # the project's bound on softmax outputs (tests/test_nn_gpu.py)


def restatement(desc, blob, features, backwards=False):
    """the storage-rounding restatement with fp32 accumulation -> the outputs the device returns"""
    return reference_outputs(reference(desc, blob, features, storage="fp16", acc=np.float32, backwards=backwards))


def tolerance(desc, blob, features, forwards=None):
    """-> (bounds, gaps) per output (policy, value, q[, m]): the gap is the largest difference between the restatement with every channel /
    tap sum taken forwards and the same taken backwards - the reference's own error on this network and these boards, measured on the
    CPU; the bound is BASE_TOLERANCE, or 4 x the gap where that is larger.  Never a value read off the device."""
    forwards = restatement(desc, blob, features) if forwards is None else forwards
    gaps = [float(np.abs(a - b).max()) for a, b in zip(forwards, restatement(desc, blob, features, backwards=True))]
    return [max(BASE_TOLERANCE, 4.0 * g) for g in gaps], gaps


# ----------------------------------------------------------------------------------------------------------------- exact networks

def exact_weights(desc, seed, se="constant"):
    """-> blob (fp32) of a network whose forward pass rounds nowhere before the softmax (module docstring); check_exact proves it"""
    rng = np.random.default_rng(seed)
    F = desc["filters"]

    def sparse(shape, k, values, scale=1.0):
        """k non-zero entries per output (last axis), the rest zero"""
        a = np.zeros((int(np.prod(shape[:-1])), shape[-1]))
        for o in range(shape[-1]):
            idx = rng.choice(a.shape[0], size=min(k, a.shape[0]), replace=False)
            a[idx, o] = rng.choice(values, size=len(idx)) * scale
        return a.reshape(shape)

    def ints(n, lo, hi, scale=1.0):
        return rng.integers(lo, hi + 1, size=n).astype(np.float64) * scale

    w = {"conv_in.w": sparse((5, 5, 8, F), 6, [-1.0, 1.0, 1.0]), "conv_in.b": ints(F, 0, 2)}
    for i in range(desc["blocks"]):
        n = "block%d" % i
        w[n + ".wd"] = sparse((7, 7, F), 2, [-1.0, 1.0])
        w[n + ".bd"] = ints(F, -1, 1)
        w[n + ".w1"] = sparse((F, F), 2, [-1.0, 1.0])
        w[n + ".b1"] = ints(F, 0, 2)
        w[n + ".w2"] = sparse((F, F), 1, [-1.0])
        w[n + ".b2"] = ints(F, 0, 3)
        w[n + ".ws1"] = sparse((F, F), 4, [-1.0, 1.0])
        w[n + ".bs1"] = ints(F, -2, 2)
        w[n + ".ws2"] = np.zeros((F, F))
        kind = rng.choice(3, size=F, p=[0.25, 0.55, 0.20])    # gate 0.5, 1, 0
        w[n + ".bs2"] = np.choose(kind, [0.0, 64.0, -64.0])
        if se == "live":
            for c in np.flatnonzero(kind == 2):                 # 0 or 1, by whether one hidden unit is positive on this board
                w[n + ".ws2"][rng.integers(F), c] = BIG
    g = HEAD_GRID
    w["policy.w1"], w["policy.b1"] = sparse((F, F), 3, [-1.0, 1.0]), ints(F, 0, 1)
    w["policy.w2"], w["policy.b2"] = sparse((F, 1), 8, [-2.0, -1.0, 1.0, 2.0], g).reshape(F), ints(1, -8, 8, g)
    w["value.w1"], w["value.b1"] = sparse((F, F), 3, [-1.0, 1.0]), ints(F, 0, 1)
    w["value.w2"], w["value.b2"] = sparse((F, VALUE_HIDDEN), 3, [-1.0, 1.0], 0.125), ints(VALUE_HIDDEN, 0, 2, 0.125)
    w["value.w3"], w["value.b3"] = sparse((VALUE_HIDDEN, 3), 8, [-1.0, 1.0], 0.125), ints(3, -4, 4, 0.125)
    w["q.w1"], w["q.b1"] = sparse((F, F), 3, [-1.0, 1.0]), ints(F, 0, 1)
    w["q.w2"], w["q.b2"] = sparse((F, 3), 4, [-1.0, 1.0], g), ints(3, -8, 8, g)
    if desc.get("moves_left", 0):
        HW = desc["rows"] * desc["cols"]
        w["m.w1"], w["m.b1"] = sparse((F, ML_FILTERS), 3, [-1.0, 1.0]), ints(ML_FILTERS, 0, 1)
        w["m.w2"], w["m.b2"] = sparse((ML_FILTERS, ML_HIDDEN), 3, [-1.0, 1.0], 0.125), ints(ML_HIDDEN, 0, 2, 0.125)
        w["m.w3"], w["m.b3"] = sparse((ML_HIDDEN, HW), 4, [-1.0, 1.0], 0.125), ints(HW, -4, 4, 0.125)
    return join(desc, w)


MAX_ABS_SUM = 2.0 ** 24          # fp32 adds multiples of one power of two exactly below 2^24 units
MAX_SPAN = 16.0                  # exp(-16) / cells stays a normal fp32 number: no cell is ever left out of a comparison
MAX_Q_SPAN = 4.0                 # the third q probability is 1 - win - draw, which cancels in fp32


def check_exact(desc, blob, features, se="constant", pooled_heads=True):
    """Asserts on the float64 reference that a device forward pass of these inputs rounds nowhere before the softmax and that the
    comparison is not vacuous: every stored activation is an fp16 number (up to SIGMOID_TAIL), every accumulation's sum of absolute terms
    stays below 2^24 units of the grid its terms lie on, every gate pre-sigmoid is 0 or at least 64 in magnitude, logit spans are small.
    pooled_heads=False (boards whose cell count is no power of two, constant gates): the value and moves-left heads pool over a
    non-dyadic count and are not part of the exact comparison - their statistics are skipped.  Returns the reference."""
    w = split(desc, blob)
    for name, a in w.items():
        if is_fp16_weight(name):
            assert np.array_equal(a.astype(np.float16).astype(np.float64), a), name
    seen, stats = {}, {}
    ref = reference(desc, blob, features, hook=lambda name, a: seen.__setitem__(name, a), stats=stats)
    for name, a in seen.items():
        if not pooled_heads and name.startswith(("value.", "m.")):
            continue
        assert np.abs(a - a.astype(np.float16).astype(np.float64)).max() <= SIGMOID_TAIL, "%s is not stored exactly" % name
        assert np.abs(a).max() <= 2048.0, name
    for name, (abs_sum, grid) in stats.items():
        pooled = name.startswith(("value.", "m.")) and not name.endswith(".h")
        se_layer = name.endswith((".mean", ".se1"))
        if (pooled and not pooled_heads) or (se_layer and se == "constant"):
            continue                                            # (constant gates: Ws2 = 0, whatever the SE layers compute is multiplied by 0)
        assert abs_sum < MAX_ABS_SUM * grid, "%s: sum of absolute terms %.3g on a grid of %.3g" % (name, abs_sum, grid)
    for z in ref.gates:
        assert ((z == 0) | (np.abs(z) >= 64.0)).all()
    if desc["blocks"]:
        kinds = {0.5 if v == 0 else (1.0 if v > 0 else 0.0) for v in np.unique(np.sign(np.concatenate([z.reshape(-1) for z in ref.gates])))}
        assert kinds == {0.0, 0.5, 1.0}, kinds
        if se == "live":                                        # some gate is 0 on one board and 1 on another
            assert any(((z >= 64).any(axis=0) & (z <= -64).any(axis=0)).any() for z in ref.gates), "no gate depends on the board"
    span = ref.policy.max(axis=1) - ref.policy.min(axis=1)
    assert span.max() <= MAX_SPAN, "policy logit span %.2f" % span.max()
    assert span.min() > 0.0 or desc["blocks"] == 0, "a constant policy"
    qspan = ref.q.max(axis=2) - ref.q.min(axis=2)
    assert qspan.max() <= MAX_Q_SPAN and softmax(ref.q).min() > 5.0e-3, "q logit span %.2f" % qspan.max()
    if pooled_heads:
        assert (ref.value.max(axis=1) - ref.value.min(axis=1)).max() <= MAX_SPAN
        if ref.m is not None:
            mspan = ref.m.max(axis=1) - ref.m.min(axis=1)
            assert 0.0 < mspan.max() <= MAX_SPAN, "moves-left logit span %.2f" % mspan.max()
    return ref


# -------------------------------------------------------------------------------------------------------------------------- inputs

def directed_boards(rows, cols):
    """feature words (low byte) with a stone in every corner, on every border column and row, and the plain cases -> uint32 [N, HW]"""
    EMPTY, OWN, OPP, ALWAYS = 1, 2, 4, 8
    empty = np.full((rows, cols), EMPTY | ALWAYS | 16, np.uint32)
    boards = [np.zeros((rows, cols), np.uint32), np.full((rows, cols), 0xFFFFFFFF, np.uint32), empty]
    corners = empty.copy()
    for k, (r, c) in enumerate([(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)]):
        corners[r, c] = (OWN if k % 2 == 0 else OPP) | ALWAYS | 32
    boards.append(corners)
    for c in range(cols):                                       # a stone on every border column: top and bottom row, alternating
        b = empty.copy()
        b[0 if c % 2 == 0 else rows - 1, c] = OWN | ALWAYS | 32 | 0xA5A5A500
        b[rows // 2, c] = OPP | ALWAYS | 16
        boards.append(b)
    for r in (0, rows // 2, rows - 1):                          # and on the left and right border
        b = empty.copy()
        b[r, 0] = OWN | ALWAYS | 32
        b[r, cols - 1] = OPP | ALWAYS | 32
        boards.append(b)
    frame = empty.copy()
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = OWN | ALWAYS | 16 | 0xFF00FF00
    boards.append(frame)
    return np.stack([b.reshape(-1) for b in boards])


@functools.lru_cache(maxsize=None)
def feature_batch(rows, cols, kind, seed=0):
    if kind == "random":
        f = synthetic.random_features(6, rows, cols, seed=300 + seed)
    elif kind == "directed":
        f = directed_boards(rows, cols)
    elif kind == "mixed":                                       # the random boards and the directed ones in one batch
        f = np.concatenate([synthetic.random_features(6, rows, cols, seed=300 + seed), directed_boards(rows, cols)])
    else:
        raise ValueError(kind)
    f.setflags(write=False)
    return f


# --------------------------------------------------------------------------------------------------------------------------- cases

LIVE_BOARDS = [(8, 8), (8, 16), (16, 16)]
CONSTANT_BOARDS = [(5, 5), (6, 20), (15, 15), (20, 20), (7, 19)]
FILTERS = [64, 128]
LIVE_BLOCKS = [0, 1, 3]
SEED = {}                                                        # (rows, cols, filters, blocks, moves_left, se) -> seed, where 1 does not pass check_exact


def make_desc(rows, cols, filters, blocks, moves_left):
    return synthetic.convnext_desc(rows, cols, blocks, filters, moves_left)


def describe(desc):
    return "%dx%d %dx%d %s" % (desc["rows"], desc["cols"], desc["blocks"], desc["filters"], "pvqm" if desc.get("moves_left", 0) else "pvq")


def live_cases():
    return [(r, c, f, b, m) for r, c in LIVE_BOARDS for f in FILTERS for b in LIVE_BLOCKS for m in (0, 1)]


def constant_cases():
    return [(r, c, f, 2, m) for (r, c), m in zip(CONSTANT_BOARDS, (1, 0, 1, 1, 0)) for f in FILTERS]


@functools.lru_cache(maxsize=None)
def cached_weights(rows, cols, filters, blocks, moves_left, se):
    desc = make_desc(rows, cols, filters, blocks, moves_left)
    blob = exact_weights(desc, SEED.get((rows, cols, filters, blocks, moves_left, se), 1), se)
    blob.setflags(write=False)
    return desc, blob


@functools.lru_cache(maxsize=None)
def cached_reference(rows, cols, filters, blocks, moves_left, se):
    desc, blob = cached_weights(rows, cols, filters, blocks, moves_left, se)
    return reference(desc, blob, feature_batch(rows, cols, "mixed"))
