"""Networks whose arithmetic is exact, and a float64 reference for them (helper module of test_nn_exact_cpu.py / test_nn_exact_gpu.py).

The tolerance tests of test_nn_gpu.py compare softmax outputs of He-init networks within 1e-3 ... 3e-2: a kernel that is wrong at one
cell, one border column or one 16-channel tile passes them.  The networks built here are chosen so that NOTHING rounds before the softmax,
whatever the order of additions and whichever storage precision is used:

  * input bits are 0 / 1; the weights of every layer that feeds the matrix cores are in {-1, 0, +1} and sparse (K1 non-zeros per output
    unit); biases are small integers;
  * the second convolution of every residual block has only non-positive weights (K2 of them, -1) and a bias in 0 ... 3, so
    x <- relu(x + y) grows by at most 3 per block: after ten blocks activations stay below 2048 (fp16 holds those integers exactly) and
    every accumulation's sum of absolute terms stays below 2^24 (fp32 adds those exactly in any order);
  * the small fp32 head weights (policy.w2, value.w3, q.w2) and their biases are multiples of a power of two g, so logits sit on a grid
    of spacing g;
  * q.w1 / q.b1 are multiples of 8: the pre-activation of the action-values head is 0 or at least 8 in magnitude, where tanh is 0 or
    rounds to +-1 in fp16 (and is within 2.3e-7 of +-1 in fp32).

The device's pre-softmax logits must then EQUAL the float64 reference, at every cell of every board; what is left for a tolerance is one
__expf and one division (about 1e-6), against a grid spacing of 2^-6 ... 2^-10.  check_exact() asserts the conditions under which that
argument holds for a given (network, inputs); logit_deviation() recovers logit differences from softmax outputs.

heads="transparent": the policy convolution is the identity and policy.w2 one constant, so the logit of a cell is the scaled sum of the
last tower plane's channels at that cell: every (cell, channel) of the tower output is observable (through random sparse heads a single
wrong (cell, channel) of the last tower layer is invisible in about a quarter of the trials).
"""
import functools
from collections import namedtuple

import numpy as np

from alphagomoku_amd import synthetic

K1 = 6   # non-zeros per output unit of a {-1, 0, +1} layer
K2 = 3   # non-zeros (-1) per output unit of a residual block's second convolution
HEAD_GRID = 1.0 / 64.0
TRANSPARENT_POLICY_W2 = 1.0 / 128.0
TRANSPARENT_VALUE_GRID = 1.0 / 256.0

Reference = namedtuple("Reference", "policy value q stats")
LayerStats = namedtuple("LayerStats", "name max_abs positive_share max_abs_sum")


# ------------------------------------------------------------------------------------------------------------------------ weights

def part_names(desc):
    names = ["conv_in.w", "conv_in.b"]
    for i in range(desc["blocks"]):
        names += ["block%d.w1" % i, "block%d.b1" % i, "block%d.w2" % i, "block%d.b2" % i]
    names += ["policy.w1", "policy.b1", "policy.w2", "policy.b2", "value.w1", "value.b1", "value.w2", "value.b2", "value.w3", "value.b3"]
    if desc.get("action_values", 0):
        names += ["q.w1", "q.b1", "q.w2", "q.b2"]
    return names


def part_shapes(desc):
    """the blob layout of include/agx.h"""
    F, C, HW, D = desc["filters"], desc["in_channels"], desc["rows"] * desc["cols"], desc["value_hidden"]
    shapes = [(5, 5, C, F), (F,)]
    for _ in range(desc["blocks"]):
        shapes += [(3, 3, F, F), (F,), (3, 3, F, F), (F,)]
    shapes += [(3, 3, F, F), (F,), (F,), (1,), (F, 4), (4,), (HW * 4, D), (D,), (D, 3), (3,)]
    if desc.get("action_values", 0):
        shapes += [(3, 3, F, F), (F,), (F, 3), (3,)]
    return shapes


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


def exact_weights(desc, seed, heads="random"):
    """fp32 blob (layout of include/agx.h) of a network whose forward pass is exact in fp16 storage / fp32 accumulation"""
    assert heads in ("random", "transparent")
    rng = np.random.default_rng([seed, desc["rows"], desc["filters"], desc["blocks"], desc["in_channels"]])
    F, C, HW, D = desc["filters"], desc["in_channels"], desc["rows"] * desc["cols"], desc["value_hidden"]

    def sparse(shape, k, values, scale=1.0):
        """k entries per output unit (last axis) drawn from `values`, the rest zero"""
        fan_in, units = int(np.prod(shape[:-1])), shape[-1]
        w = np.zeros((fan_in, units))
        rows = rng.integers(0, fan_in, size=(k, units))
        w[rows, np.arange(units)[None, :]] = rng.choice(values, size=(k, units))
        return (w * scale).reshape(shape)

    def ints(n, lo, hi, scale=1.0):
        return rng.integers(lo, hi + 1, size=n).astype(np.float64) * scale

    def input_conv():
        # the dense planes of a feature word are its low bits (stones, legality, colour); the threat bits above them are set on ~3 % of
        # the cells.  Two of the K1 taps of every unit read a low plane so that the first layer is not constant over the board.
        w = sparse((5, 5, C, F), K1 - 2, [-1.0, 1.0]).reshape(25, C, F)
        taps, low = rng.integers(0, 25, size=(2, F)), rng.integers(0, min(C, 6), size=(2, F))
        w[taps, low, np.arange(F)[None, :]] = rng.choice([-1.0, 1.0], size=(2, F))
        return w.reshape(5, 5, C, F)

    parts = [input_conv(), ints(F, 0, 2)]
    for _ in range(desc["blocks"]):
        parts += [sparse((3, 3, F, F), K1, [-1.0, 1.0]), ints(F, 0, 2), sparse((3, 3, F, F), K2, [-1.0]), ints(F, 1, 3)]
    if heads == "random":
        parts += [sparse((3, 3, F, F), K1, [-1.0, 1.0]), ints(F, 0, 2), sparse((F, 1), 12, [-2.0, -1.0, 1.0, 2.0], HEAD_GRID).reshape(F), ints(1, -4, 4, HEAD_GRID)]
        parts += [sparse((F, 4), K1, [-1.0, 1.0]), ints(4, 2, 4)]        # only four planes: a bias that keeps each of them alive
        value_grid = HEAD_GRID
    else:
        identity = np.zeros((3, 3, F, F))
        identity[1, 1] = np.eye(F)
        parts += [identity, np.zeros(F), np.full(F, TRANSPARENT_POLICY_W2), np.zeros(1)]
        route = np.zeros((F, 4))
        route[np.arange(F), np.arange(F) % 4] = 1.0          # channel c feeds value plane c mod 4
        parts += [route, np.zeros(4)]
        value_grid = TRANSPARENT_VALUE_GRID
    parts += [sparse((HW * 4, D), K1, [-1.0, 1.0]), ints(D, 0, 2), sparse((D, 3), 16, [-2.0, -1.0, 1.0, 2.0], value_grid), ints(3, -4, 4, value_grid)]
    if desc.get("action_values", 0):
        parts += [sparse((3, 3, F, F), K1, [-8.0, 8.0]), ints(F, -1, 1, 8.0), sparse((F, 3), 8, [-2.0, -1.0, 1.0, 2.0], HEAD_GRID), ints(3, -4, 4, HEAD_GRID)]
    for p, s in zip(parts, part_shapes(desc)):
        assert p.shape == s
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)


def dyadic_grid(*arrays):
    """the largest power of two of which every value is a multiple: integer combinations of the values lie on that grid"""
    v = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays])
    for k in range(0, 31):
        if np.array_equal(np.round(v * 2.0 ** k), v * 2.0 ** k):
            return 2.0 ** -k
    raise AssertionError("not multiples of a power of two down to 2^-30")


def head_grids(desc, blob):
    """grid spacing of the policy / value / q logits of an exact network (the activations they weigh are integers)"""
    w = split(desc, blob)
    g = {"policy": dyadic_grid(w["policy.w2"], w["policy.b2"]), "value": dyadic_grid(w["value.w3"], w["value.b3"])}
    if desc.get("action_values", 0):
        g["q"] = dyadic_grid(w["q.w2"], w["q.b2"])
    return g


# ---------------------------------------------------------------------------------------------------------------------- reference

def _conv_same(x, w):
    """x [Cin, B, H, W] (*) w [kh, kw, Cin, Cout] -> [Cout, B, H, W]: cross-correlation, zero padding, float64"""
    cin, B, H, W = x.shape
    kh, kw = w.shape[:2]
    xp = np.zeros((cin, B, H + kh - 1, W + kw - 1))
    xp[:, :, kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = x
    return _conv_padded(xp, w, H, W)


def _conv_padded(xp, w, H, W):
    kh, kw, cin, cout = w.shape
    _, B, Hp, Wp = xp.shape
    taps = np.nonzero(w)
    if 20 * taps[0].size < w.size:
        # sparse weights (the exact networks: K1 of 1152 entries per unit): one scaled add per non-zero.  The planes are flattened over
        # (board, padded row, padded column): a tap is then an offset into one contiguous vector, and the positions that run over a
        # row's or a board's end fall on outputs outside H x W, which are cropped
        xc = xp.reshape(cin, -1)
        n = B * Hp * Wp - (kh - 1) * Wp - (kw - 1)
        out = np.zeros((cout, B * Hp * Wp))
        for i, j, c, o in zip(*taps):
            out[o, :n] += w[i, j, c, o] * xc[c, i * Wp + j:i * Wp + j + n]
        return np.ascontiguousarray(out.reshape(cout, B, Hp, Wp)[:, :, :H, :W])
    out = np.zeros((cout, B, H, W))
    for i in range(kh):
        for j in range(kw):
            out += np.tensordot(w[i, j], xp[:, :, i:i + H, j:j + W], axes=([0], [0]))
    return out


def reference(desc, blob, features, hook=None, stats=True):
    """float64 forward pass up to the logits, written from the layer definitions (reference src/networks/blocks.cpp:32-127, the
    conventions of include/agx.h): -> Reference(policy logits [B, HW], value logits [B, 3], q logits [B, HW, 3] or None, per-layer stats).

    Activation planes are held channel-first, [C, B, H, W].  hook(name, array) -> array may replace any weight ("w:<part name>"), the
    padded input plane ("input_padded", [C, B, H + 4, W + 4]), a layer's stored output ("conv_in", "block<i>.y", "block<i>", "policy.p",
    "q.t": [F, B, H, W]; "value.v": [B, HW, 4]; "value.h": [B, D]) or a block's residual input ("block<i>.res"): the bug models of the
    sensitivity test."""
    rows, cols, HW = desc["rows"], desc["cols"], desc["rows"] * desc["cols"]
    w = split(desc, blob)
    if hook is None:
        def hook(name, array):
            return array
    w = {name: hook("w:" + name, a) for name, a in w.items()}
    collected = []

    def layer(name, out, terms):
        """terms: the sum of absolute terms behind every output element (what bounds the error of an fp32 accumulation in any order)"""
        if stats:
            collected.append(LayerStats(name, float(np.abs(out).max()), float((out > 0).mean()), float(terms().max())))
        return hook(name, out)

    def logits_stats(name, out, terms):
        if stats:
            collected.append(LayerStats(name, float(np.abs(out).max()), 1.0, float(terms.max())))

    def per_channel(b):
        return b.reshape(-1, 1, 1, 1)

    def conv(x, wname, bname):
        return _conv_same(x, w[wname]) + per_channel(w[bname])

    def conv_terms(x, wname, bname, extra=0.0):
        return lambda: _conv_same(np.abs(x), np.abs(w[wname])) + per_channel(np.abs(w[bname])) + extra

    def mix(x, m):
        """1x1 convolution: x [C, B, H, W], m [C, K] -> [B, H, W, K]"""
        return np.tensordot(x, m, axes=([0], [0]))

    f = np.asarray(features, dtype=np.uint32).reshape(-1, rows, cols)
    C = desc["in_channels"]
    bits = ((f[None] >> np.arange(C, dtype=np.uint32).reshape(C, 1, 1, 1)) & np.uint32(1)).astype(np.float64)   # bit c of the word -> channel c
    xp = np.zeros((C, f.shape[0], rows + 4, cols + 4))
    xp[:, :, 2:2 + rows, 2:2 + cols] = bits
    xp = hook("input_padded", xp)
    x = layer("conv_in", np.maximum(_conv_padded(xp, w["conv_in.w"], rows, cols) + per_channel(w["conv_in.b"]), 0.0),
              lambda: _conv_padded(np.abs(xp), np.abs(w["conv_in.w"]), rows, cols) + per_channel(np.abs(w["conv_in.b"])))
    for i in range(desc["blocks"]):
        n = "block%d" % i
        y = layer(n + ".y", np.maximum(conv(x, n + ".w1", n + ".b1"), 0.0), conv_terms(x, n + ".w1", n + ".b1"))
        res = hook(n + ".res", x)
        x = layer(n, np.maximum(res + conv(y, n + ".w2", n + ".b2"), 0.0), conv_terms(y, n + ".w2", n + ".b2", np.abs(res)))
    p = layer("policy.p", np.maximum(conv(x, "policy.w1", "policy.b1"), 0.0), conv_terms(x, "policy.w1", "policy.b1"))
    policy = (mix(p, w["policy.w2"]) + w["policy.b2"][0]).reshape(-1, HW)
    logits_stats("policy.logits", policy, mix(np.abs(p), np.abs(w["policy.w2"])) + abs(w["policy.b2"][0]))
    v = layer("value.v", np.maximum(mix(x, w["value.w1"]) + w["value.b1"], 0.0).reshape(-1, HW, 4),
              lambda: mix(np.abs(x), np.abs(w["value.w1"])) + np.abs(w["value.b1"]))
    v = v.reshape(-1, HW * 4)                                     # NHWC flatten: index = (row * cols + col) * 4 + c
    h = layer("value.h", np.maximum(v.dot(w["value.w2"]) + w["value.b2"], 0.0), lambda: np.abs(v).dot(np.abs(w["value.w2"])) + np.abs(w["value.b2"]))
    value = h.dot(w["value.w3"]) + w["value.b3"]
    logits_stats("value.logits", value, np.abs(h).dot(np.abs(w["value.w3"])) + np.abs(w["value.b3"]))
    q = None
    if desc.get("action_values", 0):
        pre = conv(x, "q.w1", "q.b1")
        t = layer("q.t", np.tanh(pre), conv_terms(x, "q.w1", "q.b1"))
        q = (mix(t, w["q.w2"]) + w["q.b2"]).reshape(-1, HW, 3)
        if stats:
            collected.append(LayerStats("q.pre", float(np.abs(pre).max()), float((pre > 0).mean()), 0.0))
        logits_stats("q.logits", q, mix(np.abs(t), np.abs(w["q.w2"])) + np.abs(w["q.b2"]))
    return Reference(policy, value, q, collected)


def reference_in_chunks(desc, blob, features, boards=100):
    """reference() without statistics for a large batch, a few boards at a time (a 900-board plane of a 20x20 128-filter layer is 370 MB)"""
    parts = [reference(desc, blob, features[i:i + boards], stats=False) for i in range(0, len(features), boards)]
    return Reference(np.concatenate([p.policy for p in parts]), np.concatenate([p.value for p in parts]),
                     None if parts[0].q is None else np.concatenate([p.q for p in parts]), [])


def softmax(logits, axis=-1):
    z = logits - logits.max(axis=axis, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=axis, keepdims=True)


def reference_outputs(ref):
    """what the device returns for these logits, in float64: policy [B, HW], value [B, 3], q [B, HW, 2] = (win, draw) or None"""
    return softmax(ref.policy), softmax(ref.value), None if ref.q is None else softmax(ref.q)[:, :, :2]


# ----------------------------------------------------------------------------------------------------------------------- checking

MIN_POSITIVE_SHARE = 0.15
MAX_ACTIVATION = 2048.0          # fp16 holds every integer up to 2048
MAX_ABS_SUM = 2.0 ** 24          # fp32 adds integers (and multiples of one power of two) exactly below 2^24 units
MAX_SPAN = 16.0                  # exp(-16) / cells stays a normal fp32 number: no cell is ever left out of a comparison
MAX_Q_SPAN = 4.0                 # the third q probability is 1 - win - draw, which cancels in fp32: span <= 4 keeps it above 5e-3
MIN_VALUE_PROBABILITY = 1.0e-6


def check_exact(desc, blob, features):
    """Asserts that the comparison of a device forward pass with reference() on these inputs is exact up to the softmax, and not vacuous.
    Returns the Reference."""
    w = split(desc, blob)
    tower = [n for n in w if n.endswith((".w1", ".w2")) and n not in ("policy.w2", "q.w2")] + ["conv_in.w"]
    for name in tower:                                        # the fp16-stored weights
        assert np.array_equal(w[name].astype(np.float16).astype(np.float64), w[name]), name
    for name, a in w.items():                                 # whole-graph fp16 conversion (nn_ref storage="fp16_all") rounds the rest as well
        assert np.array_equal(a.astype(np.float16).astype(np.float64), a), name
    grids = head_grids(desc, blob)
    seen = {}

    def keep(name, a):
        if not name.startswith("w:") and not name.endswith(".res") and name != "input_padded":
            seen[name] = a
        return a
    ref = reference(desc, blob, features, hook=keep)
    for s in ref.stats:
        where = "%s of %s" % (s.name, describe(desc))
        assert s.max_abs_sum < MAX_ABS_SUM * min(grids.values()), where     # in units of the finest grid in use
        if s.name.endswith((".logits", ".pre")):
            continue
        assert s.max_abs <= MAX_ACTIVATION, where
        if s.name != "q.t":
            assert s.positive_share >= MIN_POSITIVE_SHARE, "%s: %.3f of the activations positive" % (where, s.positive_share)
    for name, a in seen.items():                              # every stored activation is an integer
        if name == "q.t":
            # tanh of 0 or of a multiple of 8: within 2.3e-7 of {-1, 0, +1}, which is what fp16 storage rounds it to
            assert np.abs(a - np.round(a)).max() < 2.5e-7, name
        else:
            assert np.array_equal(a, np.round(a)), name
    span = ref.policy.max(axis=1) - ref.policy.min(axis=1)
    assert span.max() <= MAX_SPAN, "policy logit span %.2f" % span.max()
    assert span.min() > 0.0 or desc["blocks"] == 0, "a constant policy"
    vspan = ref.value.max(axis=1) - ref.value.min(axis=1)
    assert vspan.max() <= MAX_SPAN, "value logit span %.2f" % vspan.max()
    if ref.q is not None:
        qspan = ref.q.max(axis=2) - ref.q.min(axis=2)
        assert qspan.max() <= MAX_Q_SPAN, "q logit span %.2f" % qspan.max()
        assert softmax(ref.q).min() > 5.0e-3
    # the value output is not a saturated softmax (every value assertion on such a network would be vacuous)
    live = (softmax(ref.value).min(axis=1) > MIN_VALUE_PROBABILITY).mean()
    assert live >= 0.5, "value head saturated on %.0f %% of the boards" % (100.0 * (1.0 - live))
    return ref


def logit_deviation(probabilities, logits):
    """Largest |(log p_i - log p_j) - (l_i - l_j)| of every board, j the arg-max of the logits, in float64 -> [B].
    For the action values (probabilities [B, HW, 2] = (win, draw) of the three, logits [B, HW, 3]): per cell log(win / draw) against
    l_win - l_draw and log((1 - win - draw) / win) against l_loss - l_win, so that the third logit is pinned too."""
    p = np.asarray(probabilities, dtype=np.float64)
    l = np.asarray(logits, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if l.ndim == 3:
            assert p.shape == l.shape[:2] + (2,)
            win, draw = p[:, :, 0], p[:, :, 1]
            a = np.log(win / draw) - (l[:, :, 0] - l[:, :, 1])
            b = np.log((1.0 - win - draw) / win) - (l[:, :, 2] - l[:, :, 0])
            d = np.maximum(np.abs(a), np.abs(b)).max(axis=1)
        else:
            assert p.shape == l.shape
            top = l.argmax(axis=1)[:, None]
            d = np.abs((np.log(p) - np.log(np.take_along_axis(p, top, 1))) - (l - np.take_along_axis(l, top, 1))).max(axis=1)
    return np.where(np.isfinite(d), d, np.inf)                  # a zero or negative probability is an infinite deviation, never a skipped cell


# -------------------------------------------------------------------------------------------------------------------------- inputs

def directed_boards(rows, cols):
    """feature words of boards that aim at the edges of the kernels' tiling -> (uint32 [N, HW], names)"""
    EMPTY, OWN, OPP, ALWAYS = 1, 2, 4, 8                       # bits 0-3 of a feature word (synthetic.random_features)
    empty = np.full((rows, cols), EMPTY | ALWAYS | 16, np.uint32)
    boards, names = [], []

    def add(name, b):
        boards.append(np.asarray(b, np.uint32).reshape(-1))
        names.append(name)

    add("zero words", np.zeros((rows, cols)))
    add("all bits", np.full((rows, cols), 0xFFFFFFFF))
    add("empty", empty)
    full = np.where((np.add.outer(np.arange(rows), np.arange(cols)) // 2) % 2 == 0, OWN, OPP) | ALWAYS | 32
    add("full", full)
    mid_r, mid_c = rows // 2, cols // 2
    seams = [13, 14] if cols == 15 else [14, 15, 16, 19]
    stones = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (0, mid_c), (rows - 1, mid_c), (mid_r, 0), (mid_r, cols - 1)]
    stones += [(r, c) for c in seams for r in (0, mid_r, rows - 1)]
    for k, (r, c) in enumerate(dict.fromkeys(stones)):
        b = empty.copy()
        b[r, c] = (OWN if k % 2 == 0 else OPP) | ALWAYS | 16 | (0xA5A5A500 if k % 3 == 0 else 0)
        add("stone %d,%d" % (r, c), b)
    frame = empty.copy()
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = OWN | ALWAYS | 16 | 0xFF00FF00
    add("border frame", frame)
    return np.stack(boards), names


@functools.lru_cache(maxsize=None)
def feature_batch(rows, kind, seed=0):
    """the feature batches of the parametrised cases (cached: shared between the CPU and the GPU file and between cases)"""
    if kind == "random":
        f = synthetic.random_features(6, rows, rows, seed=100 + seed)
    elif kind == "directed":
        f = directed_boards(rows, rows)[0]
    elif kind == "pool":                                        # boards for the batch-shape, launch-width and slot-list cases
        f = synthetic.random_features(900, rows, rows, seed=200 + seed)
    elif kind == "high bits":                                   # raw networks read the low byte only: the upper 24 bits set must not matter
        f = synthetic.random_features(6, rows, rows, seed=100 + seed) | np.uint32(0xFFFFFF00)
    else:
        raise ValueError(kind)
    f.setflags(write=False)
    return f


# --------------------------------------------------------------------------------------------------------------------------- cases

GEOMETRIES = [(15, "0"), (15, "1"), (20, "0")]                 # (board size, AGX_NN_SINGLE_PLANE): two-plane, single-plane, 20x20 (always single-plane)
FILTERS = [64, 128]
KINDS = ["pv", "raw", "pvq"]                                     # 32 input channels, 8 input channels, 32 channels with the action-values head
BLOCKS = [0, 1, 10]
HEADS = ["random", "transparent"]
SEEDS = [1, 2]


def make_desc(rows, filters, kind, blocks):
    return synthetic.net_desc(rows=rows, cols=rows, blocks=blocks, filters=filters, in_channels=8 if kind == "raw" else 32,
                              action_values=1 if kind == "pvq" else 0)


def describe(desc):
    return "%dx%d %dx%d cin %d%s" % (desc["rows"], desc["cols"], desc["blocks"], desc["filters"], desc["in_channels"], " +q" if desc.get("action_values", 0) else "")


def instantiations():
    """the tower kernel's template combinations the dispatch can launch: (filters, board, in place, q head, raw input)"""
    return [(filters, rows, rows == 20 or single == "1", kind == "pvq", kind == "raw") for rows, single in GEOMETRIES for filters in FILTERS for kind in KINDS]


def network_cases():
    """(rows, single, filters, kind, blocks, heads, seed) of every network the GPU file evaluates"""
    return [(rows, single, filters, kind, blocks, heads, seed) for rows, single in GEOMETRIES for filters in FILTERS for kind in KINDS
            for blocks in BLOCKS for heads in HEADS for seed in SEEDS]


def batches_of(kind, seed):
    """the feature batches a network case is evaluated on"""
    return ["random", "directed"] + (["high bits"] if kind == "raw" and seed == 1 else [])


def distinct_networks():
    """network_cases() without the launch geometry (the two 15x15 kernels evaluate the same networks): what the CPU file checks"""
    return sorted({(rows, filters, kind, blocks, heads, seed) for rows, _, filters, kind, blocks, heads, seed in network_cases()})


@functools.lru_cache(maxsize=8)
def cached_weights(rows, filters, kind, blocks, heads, seed):
    desc = make_desc(rows, filters, kind, blocks)
    return desc, exact_weights(desc, seed, heads)


POOL_NETWORK = (1, "random", 1)                                  # (blocks, heads, seed) of the networks of the batch-shape / launch-width / slot-list cases


def dispatch_table():
    """the template combinations launch_forward() can launch, read from the dispatch macros of csrc/nn_forward.hip:
    (filters, board, in place, q head, raw input)"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphagomoku_amd", "csrc", "nn_forward.hip")
    with open(path) as f:
        source = f.read()
    flag = {"true": True, "false": False}
    geometries = {(int(f), int(n), flag[ip]) for f, n, ip in re.findall(r"AGX_LAUNCH_HEADS\((\d+), (\d+), (true|false)\);", source)}
    heads = {(flag[q], flag[r]) for q, r in re.findall(r"AGX_LAUNCH_TOWER\(FF, NN, IP, (true|false), (true|false)\)", source)}
    return sorted((f, n, ip, q, r) for f, n, ip in geometries for q, r in heads)
