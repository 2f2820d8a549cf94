"""CPU side of the exact-arithmetic network tests (nn_exact.py): the float64 reference is cross-checked against the numpy oracle and
torch, every (network, feature batch) the GPU file evaluates is proved exact (check_exact, and nn_ref.forward bit-identical in its three
storage modes: nothing rounds), and every modelled kernel bug moves the outputs by more than the GPU file's threshold."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import nn_exact as nx
from alphagomoku_amd import synthetic
from oracle import nn_ref


# ------------------------------------------------------------------------------------------------- the reference against others

@pytest.mark.parametrize("rows,blocks,filters,kind", [(15, 2, 64, "pv"), (20, 1, 64, "raw"), (15, 1, 128, "pvq")])
def test_reference_matches_the_numpy_oracle(rows, blocks, filters, kind):
    """dense He-init weights (the other convolution path of the reference): softmax of the float64 logits against the fp32 oracle, within
    the bounds test_nn_oracle.py uses between the oracle and torch"""
    d = nx.make_desc(rows, filters, kind, blocks)
    blob, _ = synthetic.make_weights(d, seed=7)
    f = synthetic.random_features(3, rows, rows, seed=11)
    out = nn_ref.forward(d, blob, f)
    p, v, q = nx.reference_outputs(nx.reference(d, blob, f))
    assert np.abs(p - out[0]).max() < 1e-6
    assert np.abs(v - out[1]).max() < 1e-5
    if kind == "pvq":
        assert np.abs(q - out[2]).max() < 1e-5


def torch_logits(d, blob, f):
    """the same layers on torch's float64 conv2d"""
    w = {k: torch.from_numpy(a) for k, a in nx.split(d, blob).items()}
    rows, cols = d["rows"], d["cols"]

    def conv3(x, wname, bname):
        return Fn.conv2d(x, w[wname].permute(3, 2, 0, 1), w[bname], padding=1)

    x = torch.from_numpy(nn_ref.unpack_input(f, rows, cols, d["in_channels"]).astype(np.float64)).permute(0, 3, 1, 2)
    x = torch.relu(Fn.conv2d(x, w["conv_in.w"].permute(3, 2, 0, 1), w["conv_in.b"], padding=2))
    for i in range(d["blocks"]):
        n = "block%d" % i
        x = torch.relu(x + conv3(torch.relu(conv3(x, n + ".w1", n + ".b1")), n + ".w2", n + ".b2"))
    p = torch.relu(conv3(x, "policy.w1", "policy.b1")).permute(0, 2, 3, 1) @ w["policy.w2"] + w["policy.b2"][0]
    v = torch.relu(x.permute(0, 2, 3, 1) @ w["value.w1"] + w["value.b1"]).reshape(x.shape[0], -1)
    value = torch.relu(v @ w["value.w2"] + w["value.b2"]) @ w["value.w3"] + w["value.b3"]
    q = None
    if d.get("action_values", 0):
        q = (torch.tanh(conv3(x, "q.w1", "q.b1")).permute(0, 2, 3, 1) @ w["q.w2"] + w["q.b2"]).reshape(x.shape[0], -1, 3).numpy()
    return p.reshape(p.shape[0], -1).numpy(), value.numpy(), q


@pytest.mark.parametrize("kind", ["raw", "pvq"])
@pytest.mark.parametrize("exact", [False, True])
def test_reference_matches_torch_float64(kind, exact):
    d = nx.make_desc(15, 64, kind, 2)
    blob = nx.exact_weights(d, 3) if exact else synthetic.make_weights(d, seed=8)[0]
    f = synthetic.random_features(3, 15, 15, seed=12)
    ref = nx.reference(d, blob, f)
    p, v, q = torch_logits(d, blob, f)
    tol = 0.0 if exact else 1e-11                                # integers: both must be exact; He-init: float64 rounding in another order
    assert np.abs(ref.policy - p).max() <= tol and np.abs(ref.value - v).max() <= tol
    if kind == "pvq":
        assert np.abs(ref.q - q).max() <= max(tol, 1e-15)


def test_logit_deviation_recovers_logit_differences():
    rng = np.random.default_rng(0)
    l = rng.integers(-200, 200, size=(4, 225)) / 64.0
    p = nx.softmax(l).astype(np.float32)
    assert nx.logit_deviation(p, l).max() < 2e-6
    m = l.copy()
    m[2, 17] += 1.0 / 64.0
    d = nx.logit_deviation(nx.softmax(m).astype(np.float32), l)
    assert abs(d[2] - 1.0 / 64.0) < 2e-6 and d[[0, 1, 3]].max() < 2e-6
    z = p.copy()
    z[1, 5] = 0.0                                                # a zero probability is an infinite deviation, not a skipped cell
    assert np.isinf(nx.logit_deviation(z, l)[1])
    lq = rng.integers(-64, 64, size=(2, 225, 3)) / 64.0
    pq = nx.softmax(lq).astype(np.float32)[:, :, :2]
    assert nx.logit_deviation(pq, lq).max() < 1e-4
    mq = lq.copy()
    mq[1, 100, 2] += 1.0 / 64.0                                  # the logit the device does not store
    assert abs(nx.logit_deviation(nx.softmax(mq).astype(np.float32)[:, :, :2], lq)[1] - 1.0 / 64.0) < 1e-4


def test_the_cases_cover_the_dispatch_table():
    inst = nx.instantiations()
    assert len(inst) == 18 and set(inst) == set(nx.dispatch_table())
    assert len(nx.network_cases()) == 18 * len(nx.BLOCKS) * len(nx.HEADS) * len(nx.SEEDS)


# ---------------------------------------------------------------------------------------------------- every case is exact

@pytest.mark.parametrize("rows,filters,kind,blocks,heads,seed", nx.distinct_networks())
def test_case_is_exact(rows, filters, kind, blocks, heads, seed):
    """check_exact on every feature batch the GPU file uses for this network, and the CPU-side proof that nothing rounds: the oracle's
    fp32, fp16-storage and whole-graph-fp16 modes give bit-identical policy and value"""
    desc, blob = nx.cached_weights(rows, filters, kind, blocks, heads, seed)
    batches = [nx.feature_batch(rows, b, seed) for b in nx.batches_of(kind, seed)]
    for f in batches:
        nx.check_exact(desc, blob, f)
    f = np.concatenate(batches)
    out = [nn_ref.forward(desc, blob, f, storage=s) for s in ("fp32", "fp16", "fp16_all")]
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and np.array_equal(out[0][1], other[1])
        if kind == "pvq":
            assert np.abs(out[0][2] - other[2]).max() < 1e-6      # tanh(+-8 k) is +-1 only after fp16 rounding
    ref = nx.reference(desc, blob, f, stats=False)
    p, v, q = nx.reference_outputs(ref)
    assert np.abs(p - out[0][0]).max() < 1e-6 and np.abs(v - out[0][1]).max() < 1e-6
    g = nx.head_grids(desc, blob)
    assert nx.logit_deviation(out[0][0], ref.policy).max() < g["policy"] / 64 and nx.logit_deviation(out[0][1], ref.value).max() < g["value"] / 64


@pytest.mark.parametrize("kind", nx.KINDS)
@pytest.mark.parametrize("filters", nx.FILTERS)
@pytest.mark.parametrize("rows", [15, 20])
def test_pool_boards_are_exact(rows, filters, kind):
    """the 900 boards the batch-shape, launch-width and slot-list cases of the GPU file draw from, a hundred at a time"""
    desc, blob = nx.cached_weights(rows, filters, kind, *nx.POOL_NETWORK)
    pool = nx.feature_batch(rows, "pool", nx.POOL_NETWORK[2])
    for i in range(0, len(pool), 100):
        nx.check_exact(desc, blob, pool[i:i + 100])
    assert nx.reference_in_chunks(desc, blob, pool[:150]).policy.shape == (150, rows * rows)


# ------------------------------------------------------------------------------------------------------------ sensitivity

def bug_models(desc):
    """name -> hook factory; every hook edits what reference() hands it the way the modelled kernel bug would"""
    rows, cols, blocks, F = desc["rows"], desc["cols"], desc["blocks"], desc["filters"]
    mid, last = "block%d" % (blocks // 2), "block%d" % (blocks - 1)
    models = {}

    def on(layer, edit):
        def hook(name, a):
            if name == layer:
                a = a.copy()
                edit(a)
            return a
        return hook

    def zero_tile(a):
        a[16:32, :, rows - 1, cols - 1] = 0.0
    models["corner tile zero in a middle layer"] = on(mid + ".y", zero_tile)
    for c in ([14] if cols == 15 else [15, 16, 19]):
        def zero_column(a, c=c):
            a[5, :, :, c] = 0.0
        models["column %d of one channel zero" % c] = on(mid, zero_column)

    def plus_one(a):
        a[3, :, rows // 2, cols - 1] += 1.0
    models["one cell of one channel +1 in the first layer"] = on("conv_in", plus_one)
    models["one cell of one channel +1 in the last tower layer"] = on(last, plus_one)

    def swap_out_tile(a):
        a[0, 0, :, 16:32], a[2, 1, :, 16:32] = a[2, 1, :, 16:32].copy(), a[0, 0, :, 16:32].copy()
    models["two taps swapped for a 16-channel output tile"] = on("w:" + mid + ".w1", swap_out_tile)

    def swap_in_group(a):
        a[0, 0, 8:16, :], a[2, 1, 8:16, :] = a[2, 1, 8:16, :].copy(), a[0, 0, 8:16, :].copy()
    models["two taps swapped for an 8-channel input group"] = on("w:" + mid + ".w2", swap_in_group)

    def wrap(a):
        # the padded plane's column just right of the board (the 16th of a 15-column row tile) holds the next row's first cell
        a[:, :, 2:1 + rows, 2 + cols] = a[:, :, 3:2 + rows, 2]
    models["5x5 input conv wraps into the next row"] = on("input_padded", wrap)

    def shift_plane(a):
        a[:, 1:, 2] = a[:, :-1, 2].copy()
    models["a value plane shifted by one cell"] = on("value.v", shift_plane)

    kept = {}

    def stale_residual(name, a):
        if name == "block%d.res" % (blocks // 2 - 1):
            kept["x"] = a
        if name == mid + ".res":
            return kept["x"]
        return a
    models["residual input taken from the previous block"] = stale_residual
    return models


def detected(desc, blob, f, hook):
    """the GPU file's comparison, applied to the mutant's softmax outputs (as float32, like the device's) against the clean logits"""
    g = nx.head_grids(desc, blob)
    clean = nx.reference(desc, blob, f, stats=False)
    p, v, q = nx.reference_outputs(nx.reference(desc, blob, f, hook=hook, stats=False))
    hit = (nx.logit_deviation(p.astype(np.float32), clean.policy) > g["policy"] / 4) | (nx.logit_deviation(v.astype(np.float32), clean.value) > g["value"] / 4)
    if q is not None:
        hit |= nx.logit_deviation(q.astype(np.float32), clean.q) > g["q"] / 4
    return int(hit.sum())


SENSITIVITY_NETWORKS = [(15, 128, "pv", 10), (20, 128, "pv", 10), (20, 64, "pvq", 10), (15, 64, "raw", 10)]


@pytest.mark.parametrize("rows,filters,kind,blocks", SENSITIVITY_NETWORKS)
def test_every_bug_model_is_detected(rows, filters, kind, blocks):
    """each bug model, applied to the reference, must push at least one board of the parametrised set over the GPU test's threshold; the
    models that edit the last tower layer need the transparent heads (which is what those are for)"""
    assert all((rows, filters, kind, blocks, heads, seed) in nx.distinct_networks() for heads in nx.HEADS for seed in nx.SEEDS)
    missed = []
    for name in bug_models(nx.make_desc(rows, filters, kind, blocks)):
        boards = 0
        for heads in (["transparent"] if "last tower layer" in name else nx.HEADS):
            for seed in nx.SEEDS:
                desc, blob = nx.cached_weights(rows, filters, kind, blocks, heads, seed)
                for b in nx.batches_of(kind, seed):
                    boards += detected(desc, blob, nx.feature_batch(rows, b, seed), bug_models(desc)[name])
                if boards:
                    break
            if boards:
                break
        print("%-55s %s: %d boards over the threshold" % (name, nx.describe(desc), boards))
        if not boards:
            missed.append(name)
    assert not missed, missed
