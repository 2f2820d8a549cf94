"""The weighted forms of the training loss and of the network score on the device (agx.h: agx_head_loss_grad_weighted,
agx_net_score_outputs_weighted) against float64 restatements fed the same float32 arrays.  The crafted tensors, the staging inside guard zones
and the bars are those of tests/test_head_loss_gpu.py and tests/test_net_score_gpu.py: a weighted cell contributes w * ce with w <= 1, so
every error term of the unweighted derivation is scaled down by w and the float64 product adds nothing visible; the gradient carries one more
float32 multiplication (q_scale * w, relative 6e-8), far inside 2e-6 * scale."""
import ctypes

import numpy as np
import pytest

import head_loss_ref as ref
import net_score_ref as score_ref
import test_head_loss_gpu as hl
import test_net_score_gpu as ns

pytestmark = pytest.mark.gpu

BOARDS = [(5, 5), (15, 15), (20, 20), (7, 12)]


def make_weights(batch, n, hw, rng, targets_key="q_target"):
    """weights like visits / sum of visits: sparse rows that sum to 1.  Sample 1 has no weight at all, sample 2 a single positive cell, the
    last one (the partial chunk).  On the cells that do not count, some weights are NaN or negative and the action-value targets are NaN;
    the targets of the cells that count are finite whatever the policy target says there."""
    w = rng.random((n, hw)) * (rng.random((n, hw)) < 0.25)
    w[np.arange(n), rng.integers(0, hw, n)] += 0.05
    if n > 1:
        w[1] = 0.0
    if n > 2:
        w[2] = 0.0
        w[2, hw - 1] = 1.0
    sums = w.sum(axis=1, keepdims=True)
    w = (w / np.where(sums > 0, sums, 1.0)).astype(np.float32)
    dead = ~(w > 0)
    wd = rng.dirichlet(np.ones(3), (n, hw))[:, :, :2].astype(np.float32)
    target = np.concatenate([wd, (np.float32(1.0) - (wd[:, :, 0] + wd[:, :, 1]))[:, :, None]], axis=2).astype(np.float32)
    target[dead & (rng.random((n, hw)) < 0.6)] = np.nan
    w[dead & (rng.random((n, hw)) < 0.2)] = np.nan
    w[dead & ~np.isnan(w) & (rng.random((n, hw)) < 0.2)] = -0.5
    batch[targets_key] = target
    batch["q_weight"] = w
    return w


def weighted_q_loss(q, q_target, w):
    """float64: per sample (sum over the cells with w > 0 of w * ce, the number of those cells), the gradients w * (p * T - t) without the
    scale, the spread R per sample"""
    n, hw = w.shape
    ce, cells, grads, spreads = np.zeros(n), np.zeros(n, np.int64), np.zeros(q.shape, np.float64), np.full(n, 6.0)
    for b in range(n):
        for cell in np.flatnonzero(w[b] > 0):
            one, g = ref.head(q[b, cell], q_target[b, cell])
            ce[b] += float(w[b, cell]) * one
            grads[b, cell] = float(w[b, cell]) * g
            spreads[b] = max(spreads[b], ref.spread(q[b, cell]))
        cells[b] = int((w[b] > 0).sum())
    return ce, cells, grads, spreads


class StagedLoss(hl.Staged):
    def __init__(self, batch, n, grads=True):
        from alphagomoku_amd.networks import DeviceBuffer
        super().__init__(batch, n, grads)
        self.bufs["q_weight"] = DeviceBuffer(batch["q_weight"].nbytes)
        self.bufs["q_weight"].upload(batch["q_weight"])

    def run(self, lib, rows, cols, first=0, count=None, stream=None, scales=hl.SCALES, weighted=True):
        from alphagomoku_amd import check
        count = self.n - first if count is None else count
        a = lambda k: self.address(k, first)   # noqa: E731
        check(lib.agx_head_loss_grad_weighted(rows, cols, count, a("policy"), a("value"), a("q"), a("policy_target"), a("value_target"), a("q_target"),
                                              a("q_weight") if weighted else None, scales[0], scales[1], scales[2], a("policy_grad"), a("value_grad"), a("q_grad"),
                                              a("records"), a("total"), stream))


def loss_batch(rows, cols, n, seed):
    batch = hl.make_batch(rows, cols, n, True, seed)
    w = make_weights(batch, n, rows * cols, np.random.default_rng(seed + 1))
    return batch, w


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("rows,cols", BOARDS)
def test_weighted_losses_and_gradients(agx_lib, rows, cols, n):
    batch, w = loss_batch(rows, cols, n, seed=rows * 1000 + cols * 10 + n)
    dead = ~(w > 0)
    assert np.isnan(w[dead]).any() and np.isnan(batch["q_target"][dead]).any() and not np.isnan(batch["q_target"][~dead]).any()
    plain_records, plain, plain_grads, spreads = ref.batch_loss(batch["policy"], batch["value"], batch["policy_target"], batch["value_target"])
    q_ce, q_cells, q_grads, q_spreads = weighted_q_loss(batch["q"], batch["q_target"], w)
    staged = StagedLoss(batch, n)
    staged.run(agx_lib, rows, cols)
    got = staged.results()
    staged.free()
    worst = 0.0
    for b, r in enumerate(got["records"]):
        assert int(r["q_cells"]) == q_cells[b] and [int(x) for x in r["topk_hit"]] == [0, 0, 0, 0] and int(r["reserved"]) == 0, (b, r)
        for k, want, spread in (("policy_ce", plain_records[b]["policy_ce"], spreads[b]["policy_ce"]), ("value_ce", plain_records[b]["value_ce"], spreads[b]["value_ce"]),
                                ("q_ce", q_ce[b], q_spreads[b])):
            bar = hl.loss_bar(want, spread)
            worst = max(worst, abs(float(r[k]) - want) / bar)
            assert np.isfinite(r[k]) and abs(float(r[k]) - want) <= bar, (b, k, float(r[k]), want, bar)
    print("%dx%d n=%d: largest deviation of a per-sample loss, as a fraction of its bar: %.3g" % (rows, cols, n, worst))
    if n > 1:
        assert q_cells[1] == 0 and float(got["records"][1]["q_ce"]) == 0.0
    if n > 2:
        assert q_cells[2] == 1 and float(got["records"][2]["q_ce"]) > 0.0
    t = got["total"].view(ref.TOTAL_DTYPE)[0]
    assert int(t["samples"]) == n and int(t["q_cells"]) == int(q_cells.sum())
    for k, want, spread in (("policy_ce", plain["policy_ce"], max(s["policy_ce"] for s in spreads)), ("value_ce", plain["value_ce"], max(s["value_ce"] for s in spreads)),
                            ("q_ce", float(q_ce.sum()), float(q_spreads.max()))):
        print("%dx%d n=%d total %s: device %.17g reference %.17g (bar %.3g)" % (rows, cols, n, k, t[k], want, hl.loss_bar(want, spread)))
        assert abs(float(t[k]) - want) <= hl.loss_bar(want, spread), k
    for i, (k, want) in enumerate((("policy", plain_grads["policy"]), ("value", plain_grads["value"]), ("q", q_grads))):
        deviation = float(np.abs(got[k + "_grad"].astype(np.float64) / hl.SCALES[i] - want.reshape(got[k + "_grad"].shape)).max())
        print("%dx%d n=%d: largest deviation of the %s gradient / scale: %.3g (bar %g)" % (rows, cols, n, k, deviation, hl.GRAD_TOL))
        assert deviation <= hl.GRAD_TOL, k
    assert (got["q_grad"][dead].view(np.uint32) == 0).all()          # exactly 0.0f, NaN weight, NaN targets or not
    assert np.abs(got["q_grad"][~dead]).max() > 0


def test_null_weight_gives_the_bits_of_the_unweighted_call(agx_lib):
    batch = hl.make_batch(15, 15, 70, True, seed=5)
    old = hl.Staged(batch, 70)
    old.run(agx_lib, 15, 15)
    want = old.results()
    old.free()
    make = dict(batch)
    make["q_weight"] = np.full((70, 225), np.nan, np.float32)      # uploaded, never read
    new = StagedLoss(make, 70)
    new.run(agx_lib, 15, 15, weighted=False)
    got = new.results()
    new.free()
    for k in want:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k


def test_weight_one_gives_the_bits_of_the_unweighted_gradient(agx_lib):
    """the rounding order stated in agx.h: (q_scale * w) * (p * T - t) — with w == 1.0f on exactly the cells that had an edge these are the
    unweighted call's gradients and cell counts"""
    batch = hl.make_batch(7, 12, 70, True, seed=6)
    old = hl.Staged(batch, 70)
    old.run(agx_lib, 7, 12)
    want = old.results()
    old.free()
    make = dict(batch)
    make["q_weight"] = (batch["policy_target"] > 0).astype(np.float32)
    new = StagedLoss(make, 70)
    new.run(agx_lib, 7, 12)
    got = new.results()
    new.free()
    assert np.array_equal(got["q_grad"].view(np.uint32), want["q_grad"].view(np.uint32))
    assert np.array_equal(got["records"]["q_cells"], want["records"]["q_cells"])


def test_weighted_chaining_and_determinism(agx_lib):
    """70 samples as one call, as 7 calls of 10 accumulated into one total, and without gradients: the same 72 bytes, the same records"""
    batch, _ = loss_batch(15, 15, 70, seed=78)
    runs = {}
    whole = StagedLoss(batch, 70)
    whole.run(agx_lib, 15, 15)
    runs["one call"] = whole.results()
    whole.free()
    parts = StagedLoss(batch, 70)
    for first in range(0, 70, 10):
        parts.run(agx_lib, 15, 15, first, 10)
    runs["7 x 10"] = parts.results()
    parts.free()
    bare = StagedLoss(batch, 70, grads=False)
    bare.run(agx_lib, 15, 15)
    runs["losses only"] = bare.results()
    bare.free()
    for k, got in runs.items():
        assert np.array_equal(got["total"], runs["one call"]["total"]), k
        assert np.array_equal(got["records"].view(np.uint8), runs["one call"]["records"].view(np.uint8)), k
        if k != "losses only":
            for g in ("policy_grad", "value_grad", "q_grad"):
                assert np.array_equal(got[g].view(np.uint32), runs["one call"][g].view(np.uint32)), (k, g)


def test_weighted_refusals(agx_lib):
    p, f = ctypes.c_void_p(16), ctypes.c_float(1.0)   # never dereferenced: the arguments are refused first
    assert agx_lib.agx_head_loss_grad_weighted(15, 15, 4, p, p, None, p, p, None, p, f, f, f, None, None, None, p, p, None) == 1
    assert b"a weight without action values" in agx_lib.agx_last_error()
    assert agx_lib.agx_net_score_outputs_weighted(15, 15, 4, p, p, None, p, p, None, p, None, p, None) == 1
    assert b"a weight without action values" in agx_lib.agx_last_error()


# ---------------------------------------------------------------- agx_net_score_outputs_weighted ----------------------------------------------------------------
class StagedScore(ns.Staged):
    def __init__(self, batch, n, records=True):
        from alphagomoku_amd.networks import DeviceBuffer
        super().__init__(batch, n, records)
        self.bufs["q_weight"] = DeviceBuffer(batch["q_weight"].nbytes)
        self.bufs["q_weight"].upload(batch["q_weight"])

    def score(self, rows, cols, first=0, count=None, stream=None, weighted=True):
        from alphagomoku_amd.networks import score_outputs
        count = self.n - first if count is None else count
        score_outputs(rows, cols, count, self.address("policy", first), self.address("value", first), self.address("policy_target", first),
                      self.address("value_target", first), self.address("q", first), self.address("q_target", first),
                      sample_scores=None if self.records is None else self.records.ptr.value + ns.GUARD + 48 * first,
                      total=self.total.ptr.value + ns.GUARD, stream=stream, action_values_weight=self.address("q_weight", first) if weighted else None)


def weighted_q_score(q, q_target, w):
    """float64: per sample the sum over the cells with w > 0 of w * (- sum over the 3 classes of t * log(max(output, FLT_MIN)))"""
    n = len(w)
    out = np.zeros(n)
    for b in range(n):
        on = w[b] > 0
        loss = np.float32(1.0) - q[b, :, 0] - q[b, :, 1]                 # float32, left to right: Value::loss_rate
        classes = np.stack([q[b, :, 0], q[b, :, 1], loss], axis=1)[on].astype(np.float64)
        ce = -(q_target[b][on].astype(np.float64) * np.log(np.maximum(classes, score_ref.FLT_MIN))).sum(axis=1)
        out[b] = float((w[b][on].astype(np.float64) * ce).sum())
    return out


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("rows,cols", BOARDS)
def test_weighted_score_outputs(agx_lib, rows, cols, n):
    batch = ns.make_batch(rows, cols, n, True, seed=rows * 1000 + cols * 10 + n)
    w = make_weights(batch, n, rows * cols, np.random.default_rng(n + rows))
    plain_records, plain = score_ref.batch_score(batch["policy"], batch["value"], batch["policy_target"], batch["value_target"])
    q_ce = weighted_q_score(batch["q"], batch["q_target"], w)
    for with_records in (True, False):
        staged = StagedScore(batch, n, records=with_records)
        staged.score(rows, cols)
        records, total = staged.results()
        staged.free()
        t = total.view(score_ref.TOTAL_DTYPE)[0]
        assert int(t["samples"]) == n and int(t["q_cells"]) == int((w > 0).sum()) and [int(x) for x in t["topk_hit"]] == plain["topk_hit"]
        for k, want in (("policy_ce", plain["policy_ce"]), ("value_ce", plain["value_ce"]), ("q_ce", float(q_ce.sum()))):
            print("%dx%d n=%d total %s: device %.17g reference %.17g" % (rows, cols, n, k, t[k], want))
            assert ns.close(float(t[k]), want), k
        if records is not None:
            for b, r in enumerate(records):
                assert int(r["q_cells"]) == int((w[b] > 0).sum()) and ns.close(float(r["q_ce"]), q_ce[b]) and ns.close(float(r["policy_ce"]), plain_records[b]["policy_ce"]), b
            first = total
        else:
            assert np.array_equal(total, first)      # the one-workgroup form: the same bits


def test_weighted_score_null_weight_and_chaining(agx_lib):
    batch = ns.make_batch(15, 15, 70, True, seed=9)
    old = ns.Staged(batch, 70)
    old.score(15, 15)
    want_records, want_total = old.results()
    old.free()
    make_weights(batch, 70, 225, np.random.default_rng(10), targets_key="unused")
    null = StagedScore(batch, 70)
    null.score(15, 15, weighted=False)
    records, total = null.results()
    null.free()
    assert np.array_equal(total, want_total) and np.array_equal(records.view(np.uint8), want_records.view(np.uint8))
    whole = StagedScore(batch, 70)
    whole.score(15, 15)
    one_records, one_total = whole.results()
    whole.free()
    parts = StagedScore(batch, 70)
    for first in range(0, 70, 10):
        parts.score(15, 15, first, 10)
    records, total = parts.results()
    parts.free()
    assert np.array_equal(total, one_total) and np.array_equal(records.view(np.uint8), one_records.view(np.uint8))
    assert not np.array_equal(one_total, want_total)
