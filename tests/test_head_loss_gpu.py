"""The training loss of the heads on the device (csrc/head_loss.hip; agx.h: agx_head_loss_grad) against the float64 numpy restatement in
tests/head_loss_ref.py, fed the same float32 arrays.  ctypes and numpy only.

Tolerances.  Losses, per sample and in total: |got - ref| <= 1e-5 * |ref| + 2^-20 * max(16, R), R = zmax - zmin + 6 of that head
(the total takes the largest R among its samples): lse and lse - z are float32 values of magnitude up to R, so the error is a handful of
half-ulps there, about R * 2^-22; the bar leaves 4 x.  Gradients: 2e-6 * scale absolute: p <= 1 carries expf's 2 ulp, a divide and a
multiply-subtract, about 2.4e-7.  Counts are exact."""
import ctypes

import numpy as np
import pytest

import head_loss_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes before and after every output
SENTINEL = 0x5A
BOARDS = [(5, 5), (15, 15), (20, 20), (7, 12)]
SCALES = (0.5, 0.25, 0.05)
GRAD_TOL = 2e-6


def loss_bar(want, spread):
    return 1e-5 * abs(want) + 2.0 ** -20 * max(16.0, spread)


def make_batch(rows, cols, n, with_q, seed):
    """normal logits of a few units and sparse targets like visit counts; from sample 0 on, as far as n reaches, the rows built to hit the
    edges.  With action values every second sample carries NaN as the target filler of the cells without an edge."""
    rng = np.random.default_rng(seed)
    hw = rows * cols
    policy = (3.0 * rng.standard_normal((n, hw))).astype(np.float32)
    target = rng.dirichlet(np.full(hw, 0.3), n) * (rng.random((n, hw)) < 0.3)
    target[np.arange(n), rng.integers(0, hw, n)] += 0.1          # at least one edge
    target = (target / target.sum(axis=1, keepdims=True)).astype(np.float32)
    value = (2.0 * rng.standard_normal((n, 3))).astype(np.float32)
    value_target = np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)]
    value_target[::5] = rng.dirichlet(np.ones(3), len(value_target[::5])).astype(np.float32)
    q = q_target = None
    if with_q:
        q = (2.0 * rng.standard_normal((n, hw, 3))).astype(np.float32)
        wd = rng.dirichlet(np.ones(3), (n, hw))[:, :, :2].astype(np.float32)
        q_target = np.concatenate([wd, (np.float32(1.0) - (wd[:, :, 0] + wd[:, :, 1]))[:, :, None]], axis=2).astype(np.float32)   # as the loader writes it
    one_hot = lambda c: np.eye(hw, dtype=np.float32)[c]   # noqa: E731
    edits = []

    def edit(fn):
        edits.append(fn)

    @edit
    def all_equal_logits(b):
        policy[b] = np.float32(0.75)
        value[b] = np.float32(-1.5)
        if with_q:
            q[b] = np.float32(0.25)

    @edit
    def one_cell_ahead_by_80(b):         # the others' probabilities vanish beside it; their edges still cost t * (lse - z), a finite loss
        policy[b] = np.float32(-40.0)
        policy[b, hw // 3] = np.float32(40.0)
        target[b, (hw // 3 + 1) % hw] = max(target[b, (hw // 3 + 1) % hw], np.float32(0.05))
        value[b] = (-40.0, 40.0, -40.0)
        value_target[b] = (0.25, 0.5, 0.25)
        if with_q:
            cell = int(np.argmax(target[b]))
            q[b, cell] = (40.0, -40.0, -40.0)
            q_target[b, cell] = (0.25, 0.5, 0.25)

    @edit
    def one_hot_target(b):
        target[b] = one_hot(int(rng.integers(0, hw)))

    @edit
    def single_edge(b):                  # one cell with an edge, the last one (the partial chunk): q_cells == 1
        target[b] = 0.0
        target[b, hw - 1] = 1.0

    @edit
    def targets_sum_to_half(b):          # the T factor of the gradient
        target[b] *= np.float32(0.5)
        value_target[b] = (0.25, 0.125, 0.125)

    @edit
    def targets_sum_to_two(b):
        target[b] *= np.float32(2.0)
        value_target[b] = (1.0, 0.5, 0.5)
        if with_q:
            q_target[b] *= np.float32(2.0)

    for b, fn in enumerate(edits[:n]):
        fn(b)
    if with_q:
        filler = (target <= 0)
        filler[1::2] = False
        q_target[filler] = np.nan
    return dict(policy=policy, value=value, policy_target=target, value_target=value_target, q=q, q_target=q_target, edge_rows=min(n, len(edits)))


OUTPUTS = ("policy_grad", "value_grad", "q_grad", "records", "total")


class Staged:
    """the six inputs in device memory; every output inside guard zones, filled with the sentinel like memory from torch.empty"""

    def __init__(self, batch, n, grads=True):
        from alphagomoku_amd.networks import DeviceBuffer
        self.n, self.batch, self.bufs = n, batch, {}
        for k in ("policy", "value", "policy_target", "value_target", "q", "q_target"):
            if batch[k] is not None:
                self.bufs[k] = DeviceBuffer(batch[k].nbytes)
                self.bufs[k].upload(batch[k])
        self.sizes = dict(records=48 * n, total=72)
        if grads:
            self.sizes.update(policy_grad=batch["policy"].nbytes, value_grad=batch["value"].nbytes)
            if batch["q"] is not None:
                self.sizes["q_grad"] = batch["q"].nbytes
        self.out = {}
        for k, nbytes in self.sizes.items():
            self.out[k] = DeviceBuffer(nbytes + 2 * GUARD)
            fill = np.full(nbytes + 2 * GUARD, SENTINEL, np.uint8)
            if k == "total":
                fill[GUARD:GUARD + 72] = 0
            self.out[k].upload(fill)

    def address(self, k, first=0):
        if k in self.bufs:
            return ctypes.c_void_p(self.bufs[k].ptr.value + first * self.batch[k][0].nbytes)
        if k in self.out:
            item = dict(policy_grad="policy", value_grad="value", q_grad="q").get(k)
            step = 48 if k == "records" else (0 if k == "total" else self.batch[item][0].nbytes)
            return ctypes.c_void_p(self.out[k].ptr.value + GUARD + first * step)
        return None

    def run(self, lib, rows, cols, first=0, count=None, stream=None, scales=SCALES):
        from alphagomoku_amd import check
        count = self.n - first if count is None else count
        a = lambda k: self.address(k, first)   # noqa: E731
        check(lib.agx_head_loss_grad(rows, cols, count, a("policy"), a("value"), a("q"), a("policy_target"), a("value_target"), a("q_target"),
                                     scales[0], scales[1], scales[2], a("policy_grad"), a("value_grad"), a("q_grad"), a("records"), a("total"), stream))

    def results(self):
        from alphagomoku_amd import check, lib
        check(lib.agx_device_synchronize())
        got = {}
        for k, nbytes in self.sizes.items():
            raw = self.out[k].download((nbytes + 2 * GUARD,), np.uint8)
            assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), "guard zone of %s overwritten" % k
            got[k] = raw[GUARD:GUARD + nbytes].copy()
        for k, buf in self.bufs.items():   # the caller's buffers are only read
            assert np.array_equal(buf.download(self.batch[k].shape, np.uint32), self.batch[k].view(np.uint32)), "%s was changed" % k
        got["records"] = got["records"].view(ref.SAMPLE_DTYPE)
        for k, item in (("policy_grad", "policy"), ("value_grad", "value"), ("q_grad", "q")):
            if k in got:
                got[k] = got[k].view(np.float32).reshape(self.batch[item].shape)
        return got

    def free(self):
        for buf in list(self.bufs.values()) + list(self.out.values()):
            buf.free()


def compare_total(total, want, spreads, what=""):
    t = total.view(ref.TOTAL_DTYPE)[0]
    assert int(t["samples"]) == want["samples"] and int(t["q_cells"]) == want["q_cells"] and [int(x) for x in t["topk_hit"]] == [0, 0, 0, 0], (what, t, want)
    for k in ("policy_ce", "value_ce", "q_ce"):
        bar = loss_bar(want[k], max(s[k] for s in spreads))
        print("%s total %s: device %.17g reference %.17g deviation %.3g (bar %.3g)" % (what, k, t[k], want[k], abs(t[k] - want[k]), bar))
        assert np.isfinite(t[k]) and abs(float(t[k]) - want[k]) <= bar, (what, k, float(t[k]), want[k])


@pytest.mark.parametrize("with_q", [True, False], ids=["q", "no_q"])
@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("rows,cols", BOARDS)
def test_losses_and_gradients_on_crafted_tensors(agx_lib, rows, cols, n, with_q):
    batch = make_batch(rows, cols, n, with_q, seed=rows * 1000 + cols * 10 + n)
    assert n < 70 or batch["edge_rows"] == 6
    want_records, want, want_grads, spreads = ref.batch_loss(batch["policy"], batch["value"], batch["policy_target"], batch["value_target"], batch["q"], batch["q_target"])
    staged = Staged(batch, n)
    staged.run(agx_lib, rows, cols)
    got = staged.results()
    staged.free()
    worst = dict(policy_ce=0.0, value_ce=0.0, q_ce=0.0)
    failures = []
    for b, (r, w, s) in enumerate(zip(got["records"], want_records, spreads)):
        assert int(r["q_cells"]) == w["q_cells"] and [int(x) for x in r["topk_hit"]] == [0, 0, 0, 0] and int(r["reserved"]) == 0, (b, r, w)
        for k in worst:
            assert np.isfinite(r[k]), (b, k, r[k])
            deviation = abs(float(r[k]) - w[k])
            worst[k] = max(worst[k], deviation / loss_bar(w[k], s[k]))
            if deviation > loss_bar(w[k], s[k]):
                failures.append((b, k, float(r[k]), w[k]))
    print("%dx%d n=%d q=%s: largest deviation of a per-sample loss, as a fraction of its bar: %s" % (rows, cols, n, with_q, worst))
    grad_worst = {}
    for i, k in enumerate(("policy", "value", "q")):
        if want_grads[k] is None:
            assert k + "_grad" not in got
            continue
        g = got[k + "_grad"].astype(np.float64)
        grad_worst[k] = float(np.abs(g / SCALES[i] - want_grads[k].reshape(g.shape)).max())
    print("%dx%d n=%d q=%s: largest gradient deviation / scale: %s (bar %g)" % (rows, cols, n, with_q, grad_worst, GRAD_TOL))
    assert not failures, failures
    compare_total(got["total"], want, spreads, "%dx%d n=%d" % (rows, cols, n))
    for k, dev in grad_worst.items():
        assert dev <= GRAD_TOL, (k, dev)      # (a NaN fails too)
    if with_q:   # exactly 0.0f on the cells without an edge, NaN filler or not
        no_edge = ~(batch["policy_target"] > 0)
        assert np.isnan(batch["q_target"][no_edge]).any()
        assert (got["q_grad"][no_edge].view(np.uint32) == 0).all()
    if n == 70:   # the crafted rows did what they were built for
        assert abs(want_records[0]["policy_ce"] - np.log(rows * cols) * float(batch["policy_target"][0].astype(np.float64).sum())) < 1e-9
        assert want_records[1]["policy_ce"] > 80 * 0.05 * 0.99 and want_records[1]["value_ce"] > 39.0
        assert not with_q or want_records[3]["q_cells"] == 1
        assert abs(float(batch["policy_target"][4].astype(np.float64).sum()) - 0.5) < 1e-6 and abs(float(batch["policy_target"][5].astype(np.float64).sum()) - 2.0) < 1e-6
        assert with_q or want["q_cells"] == 0 and want["q_ce"] == 0.0


def test_chaining_and_determinism(agx_lib):
    """the same 70 samples as one call, as 7 calls of 10 accumulated into one total, on a stream confined to 8 compute units, and without
    gradients: the 72 bytes of the total and the records are identical"""
    from alphagomoku_amd import check, lib, selfplay
    batch = make_batch(15, 15, 70, True, seed=77)
    _, want, _, spreads = ref.batch_loss(batch["policy"], batch["value"], batch["policy_target"], batch["value_target"], batch["q"], batch["q_target"])
    runs = {}
    whole = Staged(batch, 70)
    whole.run(agx_lib, 15, 15)
    runs["one call"] = whole.results()
    whole.free()
    parts = Staged(batch, 70)
    for first in range(0, 70, 10):
        parts.run(agx_lib, 15, 15, first, 10)
    runs["7 x 10"] = parts.results()
    parts.free()
    masked = Staged(batch, 70)
    stream = selfplay.cu_mask_stream(0, 8)
    check(lib.agx_device_synchronize())
    masked.run(agx_lib, 15, 15, stream=stream)
    check(lib.agx_stream_synchronize(stream))
    runs["8 compute units"] = masked.results()
    masked.free()
    bare = Staged(batch, 70, grads=False)
    bare.run(agx_lib, 15, 15)
    runs["losses only"] = bare.results()
    bare.free()
    compare_total(runs["one call"]["total"], want, spreads, "one call")
    for k, got in runs.items():
        assert np.array_equal(got["total"], runs["one call"]["total"]), k
        assert np.array_equal(got["records"].view(np.uint8), runs["one call"]["records"].view(np.uint8)), k
        if k != "losses only":
            for g in ("policy_grad", "value_grad", "q_grad"):
                assert np.array_equal(got[g].view(np.uint32), runs["one call"][g].view(np.uint32)), (k, g)


def test_refusals(agx_lib):
    p = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first
    f = ctypes.c_float(1.0)

    def call(rows=15, cols=15, n=4, policy=p, value=p, q=None, pt=p, vt=p, qt=None, pg=None, vg=None, qg=None, records=p, total=p):
        return agx_lib.agx_head_loss_grad(rows, cols, n, policy, value, q, pt, vt, qt, f, f, f, pg, vg, qg, records, total, None)

    for name in ("policy", "value", "pt", "vt", "records", "total"):
        assert call(**{name: None}) == 1, name
        assert b"null argument" in agx_lib.agx_last_error()
    assert call(n=0) == 1 and call(n=-3) == 1
    for rows, cols in ((4, 15), (15, 4), (21, 15), (15, 21)):
        assert call(rows=rows, cols=cols) == 1
    assert call(q=p) == 1 and call(qt=p) == 1                       # action values given in part
    assert call(pg=p) == 1 and call(vg=p) == 1 and call(qg=p) == 1  # gradients given in part
    assert call(pg=p, vg=p, qg=p) == 1                              # a gradient for a head without logits
    assert call(q=p, qt=p, pg=p, vg=p) == 1                         # no gradient for a head with logits
