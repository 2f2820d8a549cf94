"""The network score on the device (csrc/net_score.hip; agx.h: agx_net_score_*) against the float64 numpy restatement in
tests/net_score_ref.py, fed the same float32 arrays.  Counts are compared exactly, losses within relative 1e-5: all addends of a sum have one
sign, and each carries at most logf's 2 ulp plus one float32 multiply (<= 2^-21, about 4.8e-7, relative); the bar leaves 20 x over that."""
import ctypes
import subprocess

import numpy as np
import pytest

import net_score_ref as ref
import oracle_lib as ol
import training_batch_ref as tb

pytestmark = pytest.mark.gpu

REL = 1e-5
GUARD = 256          # bytes before and after the per-sample records and the total
SENTINEL = 0x5A
BOARDS = [(5, 5), (15, 15), (20, 20), (7, 12)]


def close(got, want):
    return abs(got - want) <= REL * abs(want)


def make_batch(rows, cols, n, with_q, seed):
    """Dirichlet outputs and targets (the policy targets sparse, like visit counts); from sample 0 on, as far as n reaches, the rows built to
    hit the edges"""
    rng = np.random.default_rng(seed)
    hw = rows * cols
    policy = rng.dirichlet(np.full(hw, 0.3), n).astype(np.float32)
    target = rng.dirichlet(np.full(hw, 0.3), n) * (rng.random((n, hw)) < 0.3)
    target[np.arange(n), rng.integers(0, hw, n)] += 0.1          # at least one edge
    target = (target / target.sum(axis=1, keepdims=True)).astype(np.float32)
    value = rng.dirichlet(np.ones(3), n).astype(np.float32)
    value_target = np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)]
    value_target[::5] = rng.dirichlet(np.ones(3), len(value_target[::5])).astype(np.float32)
    q = q_target = None
    if with_q:
        q = np.ascontiguousarray(rng.dirichlet(np.ones(3), (n, hw))[:, :, :2], dtype=np.float32)
        wd = rng.dirichlet(np.ones(3), (n, hw))[:, :, :2].astype(np.float32)
        q_target = np.concatenate([wd, (np.float32(1.0) - (wd[:, :, 0] + wd[:, :, 1]))[:, :, None]], axis=2).astype(np.float32)   # Value::loss_rate, as the loader writes it
    one_hot = lambda c: np.eye(hw, dtype=np.float32)[c]   # noqa: E731
    ranked = lambda b, k: int(np.argsort(-policy[b], kind="stable")[k])   # noqa: E731
    edits = []

    def edit(fn):
        edits.append(fn)

    @edit
    def all_equal_correct_first(b):      # ties go to cell 0 ...
        policy[b] = np.float32(1.0 / hw)
        target[b] = one_hot(0)

    @edit
    def all_equal_correct_third(b):      # ... then cells 1, 2, 3 once cell 0 is zeroed
        policy[b] = np.float32(1.0 / hw)
        target[b] = one_hot(2)

    @edit
    def all_zero_outputs(b):             # only zeros: `best` stays on cell 0, which is correct here: counted at every rank; and the FLT_MIN floor
        policy[b] = 0.0
        target[b] = one_hot(0)

    @edit
    def two_outputs_then_zeros(b):       # two non-zero outputs, then the zeroed-cell behaviour with the correct move elsewhere
        policy[b] = 0.0
        policy[b, [hw - 1, hw // 2]] = (0.75, 0.25)
        target[b] = one_hot(1)

    for k in (0, 1, 3, 4):               # the correct move ranked exactly 1st, 2nd, 4th and 5th
        def ranked_k(b, k=k):
            assert len(set(np.sort(policy[b])[-6:])) == 6
            target[b] = 0.0
            target[b, ranked(b, k)] = 0.5
            target[b, [ranked(b, 7), ranked(b, 8)]] = (0.25, 0.25)
        edits.append(ranked_k)

    @edit
    def zero_output_under_an_edge(b):    # the FLT_MIN floor inside an ordinary sample
        policy[b, int(np.argmax(target[b]))] = 0.0

    @edit
    def one_hot_target(b):
        target[b] = one_hot(int(rng.integers(0, hw)))

    @edit
    def single_edge(b):                  # one cell with an edge: q_cells == 1
        target[b] = 0.0
        target[b, hw - 1] = 1.0
        if with_q:
            q[b, hw - 1] = (0.7, 0.3000001)   # win + draw above 1: the output's loss class is negative, floored

    @edit
    def last_cell_wins(b):               # the maximum in the last (partial) chunk
        policy[b, hw - 1] = 2.0
        target[b] = one_hot(hw - 1)

    for b, fn in enumerate(edits[:n]):
        fn(b)
    return dict(policy=policy, value=value, policy_target=target, value_target=value_target, q=q, q_target=q_target, edge_rows=min(n, len(edits)))


class Staged:
    """the six inputs in device memory; the records and the total inside guard zones"""

    def __init__(self, batch, n, records=True):
        from alphagomoku_amd.networks import DeviceBuffer
        self.n, self.batch, self.bufs = n, batch, {}
        for k in ("policy", "value", "policy_target", "value_target", "q", "q_target"):
            if batch[k] is not None:
                self.bufs[k] = DeviceBuffer(batch[k].nbytes)
                self.bufs[k].upload(batch[k])
        self.records = self._guarded(48 * n) if records else None
        self.total = self._guarded(72)
        zeroed = np.full(2 * GUARD + 72, SENTINEL, np.uint8)
        zeroed[GUARD:GUARD + 72] = 0
        self.total.upload(zeroed)

    @staticmethod
    def _guarded(nbytes):
        from alphagomoku_amd.networks import DeviceBuffer
        buf = DeviceBuffer(nbytes + 2 * GUARD)
        buf.upload(np.full(nbytes + 2 * GUARD, SENTINEL, np.uint8))
        return buf

    def address(self, k, first=0):
        if k not in self.bufs:
            return None
        return self.bufs[k].ptr.value + first * self.batch[k][0].nbytes

    def score(self, rows, cols, first=0, count=None, stream=None):
        from alphagomoku_amd.networks import score_outputs
        count = self.n - first if count is None else count
        score_outputs(rows, cols, count, self.address("policy", first), self.address("value", first), self.address("policy_target", first),
                      self.address("value_target", first), self.address("q", first), self.address("q_target", first),
                      sample_scores=None if self.records is None else self.records.ptr.value + GUARD + 48 * first,
                      total=self.total.ptr.value + GUARD, stream=stream)

    def read(self, buf, nbytes, what):
        raw = buf.download((nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all(), "guard zone of %s overwritten" % what
        return raw[GUARD:GUARD + nbytes].copy()

    def results(self):
        from alphagomoku_amd import check, lib
        check(lib.agx_device_synchronize())
        total = self.read(self.total, 72, "the total")
        records = None if self.records is None else self.read(self.records, 48 * self.n, "the records").view(ref.SAMPLE_DTYPE)
        for k, buf in self.bufs.items():   # the caller's buffers are only read
            assert np.array_equal(buf.download(self.batch[k].shape, np.uint32), self.batch[k].view(np.uint32)), "%s was changed" % k
        return records, total

    def free(self):
        for buf in list(self.bufs.values()) + [self.total] + ([self.records] if self.records is not None else []):
            buf.free()


def compare_total(total, want, what=""):
    t = total.view(ref.TOTAL_DTYPE)[0]
    assert int(t["samples"]) == want["samples"] and int(t["q_cells"]) == want["q_cells"] and [int(x) for x in t["topk_hit"]] == want["topk_hit"], (what, t, want)
    for k in ("policy_ce", "value_ce", "q_ce"):
        print("%s total %s: device %.17g reference %.17g relative %.3g" % (what, k, t[k], want[k], abs(t[k] - want[k]) / max(abs(want[k]), 1e-300)))
        assert close(float(t[k]), want[k]), (what, k, float(t[k]), want[k])


@pytest.mark.parametrize("with_q", [True, False], ids=["q", "no_q"])
@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("rows,cols", BOARDS)
def test_score_outputs_on_crafted_tensors(agx_lib, rows, cols, n, with_q):
    batch = make_batch(rows, cols, n, with_q, seed=rows * 1000 + cols * 10 + n)
    assert n < 70 or batch["edge_rows"] == 12
    want_records, want = ref.batch_score(batch["policy"], batch["value"], batch["policy_target"], batch["value_target"], batch["q"], batch["q_target"])
    staged = Staged(batch, n)
    staged.score(rows, cols)
    records, total = staged.results()
    staged.free()
    worst = 0.0
    for b, (got, w) in enumerate(zip(records, want_records)):
        assert int(got["q_cells"]) == w["q_cells"] and [int(x) for x in got["topk_hit"]] == w["topk_hit"] and int(got["reserved"]) == 0, (b, got, w)
        for k in ("policy_ce", "value_ce", "q_ce"):
            worst = max(worst, abs(got[k] - w[k]) / abs(w[k]) if w[k] != 0 else 0.0)
            assert close(float(got[k]), w[k]), (b, k, float(got[k]), w[k])
    print("%dx%d n=%d q=%s: largest relative deviation of a per-sample loss %.3g" % (rows, cols, n, with_q, worst))
    compare_total(total, want, "%dx%d n=%d" % (rows, cols, n))
    if n == 70:   # the crafted rows did what they were built for
        hits = [r["topk_hit"] for r in want_records]
        assert hits[0] == [1, 1, 1, 1] and hits[1] == [0, 0, 1, 1] and hits[2] == [1, 2, 3, 4] and hits[3] == [0, 0, 0, 0]
        assert hits[4:8] == [[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 1], [0, 0, 0, 0]]
        assert abs(want_records[2]["policy_ce"] + np.log(ref.FLT_MIN)) < 1e-9
        assert not with_q or want_records[10]["q_cells"] == 1
        assert with_q or want["q_cells"] == 0 and want["q_ce"] == 0.0


def test_nan_follows_max_element(agx_lib):
    """std::max_element compares with <, false for a NaN on either side: a NaN on cell 0 stays the maximum, a NaN anywhere else never becomes
    it (agx.h).  15x15 rows with NaNs among the outputs and the targets (never an output NaN under a positive target, so the losses stay
    defined), against the transcription of getAccuracy and the numpy reference"""
    rows = cols = 15
    hw, n = rows * cols, 7
    batch = {k: None if v is None else v[12:].copy() for k, v in make_batch(rows, cols, 12 + n, False, seed=404).items() if k != "edge_rows"}   # ordinary rows
    policy, target = batch["policy"], batch["policy_target"]
    policy[:, 0] = np.maximum(policy[:, 0], np.float32(1e-6))
    target[:, 0] = 0.0
    top = lambda b, k=0: int(np.argsort(-policy[b], kind="stable")[k])   # noqa: E731
    one_hot = lambda c: np.eye(hw, dtype=np.float32)[c]   # noqa: E731
    # 0: an output NaN on cell 0 is the first `best`; the correct move is the largest number, found second
    target[0] = one_hot(top(0) if top(0) != 0 else top(0, 1))
    policy[0, 0] = np.nan
    # 1: a target NaN on cell 0 makes cell 0 the correct move, whatever else the target holds
    target[1, 0] = np.nan
    policy[1, 0] = 2.0
    # 2: output NaNs elsewhere (cells of one lane, 36 / 100 / 164) are never `best`; np.argmax would take them
    c = [k for k in range(4) if top(2, k) not in (0, 36, 100, 164)][0]
    target[2] = one_hot(top(2, c))
    policy[2, [36, 100, 164]] = np.nan
    # 3: a target NaN elsewhere is never the correct move
    target[3] = 0.0
    target[3, [5, 9]] = (0.75, 0.25)
    target[3, 7] = np.nan
    policy[3, 5] = 2.0
    # 4: NaNs on the last cell (the partial chunk) and on cell 64 (lane 0's second cell)
    target[4] = one_hot(hw - 2)
    policy[4, hw - 2] = 2.0
    policy[4, [64, hw - 1]] = np.nan
    # 5: only NaNs among the outputs: `best` stays on cell 0, the correct move (a target NaN on cell 0), counted at every rank
    policy[5] = np.nan
    target[5] = 0.0
    target[5, 0] = np.nan
    target[5, 3] = 1.0
    policy[5, 3] = 0.0
    # 6: only NaNs but one number on the correct move: `best` is cell 0 first, and once that is zeroed it compares again, so the number is second
    policy[6] = np.nan
    target[6] = one_hot(9)
    policy[6, 9] = 0.25
    assert not np.isnan(policy[target > 0]).any()
    want_records, want = ref.batch_score(policy, batch["value"], target, batch["value_target"])
    transcribed = [[int(x) for x in ref.get_accuracy_transcribed(1, [policy[b]], [target[b]], rows, cols, 4)[1:]] for b in range(n)]
    assert transcribed == [r["topk_hit"] for r in want_records]
    assert transcribed[0] == [0, 1, 1, 1] and transcribed[1] == [1, 1, 1, 1] and transcribed[2][3] == 1 and transcribed[3] == [1, 1, 1, 1]
    assert transcribed[4] == [1, 1, 1, 1] and transcribed[5] == [1, 2, 3, 4] and transcribed[6] == [0, 1, 1, 1]
    staged = Staged(batch, n)
    staged.score(rows, cols)
    records, total = staged.results()
    staged.free()
    for b, (got, w) in enumerate(zip(records, want_records)):
        assert [int(x) for x in got["topk_hit"]] == transcribed[b] and int(got["q_cells"]) == 0, (b, got, transcribed[b])
        for k in ("policy_ce", "value_ce"):
            assert close(float(got[k]), w[k]), (b, k, float(got[k]), w[k])
    compare_total(total, want, "NaN rows")


def test_chaining_and_determinism(agx_lib):
    """the same 70 samples as one call, as 7 calls of 10 accumulated into one total, on a stream confined to 8 compute units, and without
    per-sample records: the 72 bytes of the total are identical"""
    from alphagomoku_amd import check, lib, selfplay
    from alphagomoku_amd.networks import score_clear
    batch = make_batch(15, 15, 70, True, seed=77)
    _, want = ref.batch_score(batch["policy"], batch["value"], batch["policy_target"], batch["value_target"], batch["q"], batch["q_target"])
    totals = {}
    whole = Staged(batch, 70)
    whole.score(15, 15)
    records, totals["one call"] = whole.results()
    whole.free()
    parts = Staged(batch, 70)
    for first in range(0, 70, 10):
        parts.score(15, 15, first, 10)
    part_records, totals["7 x 10"] = parts.results()
    parts.free()
    assert np.array_equal(records.view(np.uint8), part_records.view(np.uint8))
    masked = Staged(batch, 70)
    stream = selfplay.cu_mask_stream(0, 8)
    check(lib.agx_device_synchronize())
    masked.score(15, 15, stream=stream)
    check(lib.agx_stream_synchronize(stream))
    _, totals["8 compute units"] = masked.results()
    masked.free()
    fused = Staged(batch, 70, records=False)
    fused.total.upload(np.full(2 * GUARD + 72, SENTINEL, np.uint8))
    score_clear(fused.total.ptr.value + GUARD)       # agx_net_score_clear: 72 bytes, the guard zones stay
    fused.score(15, 15, 0, 33)
    fused.score(15, 15, 33, 37)
    _, totals["no records, 33 + 37"] = fused.results()
    fused.free()
    compare_total(totals["one call"], want, "one call")
    for k, t in totals.items():
        assert np.array_equal(t, totals["one call"]), k


@pytest.fixture(scope="module")
def olib():
    return ol.load()


def fragment(olib, tmp_path, n, seed):
    games = [tb.oracle_game(olib, 0, n, seed, sims=32), tb.crafted_game(olib, n)]
    path = tmp_path / ("freestyle_%d.bin" % n)
    tb.write_fragment(path, "FREESTYLE", n, games)
    parsed = [tb.parse_game(g) for g in games]
    samples = np.array([(0, g, k, a) for g, game in enumerate(parsed) for k in range(len(game["samples"])) for a in range(8)], np.int32)
    step = (len(samples) // 100) | 1     # odd: keeps all 8 symmetries in the selection
    return path, samples[::step]


def network(n, blocks, action_values):
    from alphagomoku_amd import synthetic
    from alphagomoku_amd.networks import AGNetwork
    desc = synthetic.net_desc(rows=n, cols=n, blocks=blocks, filters=64, action_values=action_values)
    blob, _ = synthetic.make_weights(desc, seed=5 + blocks)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    return net, blob


@pytest.mark.parametrize("n,blocks,action_values", [(15, 2, 0), (15, 1, 1), (9, 2, 0)], ids=["15x15_pv", "15x15_pvq", "9x9_pv"])
def test_score_dataset_end_to_end(agx_lib, olib, tmp_path, n, blocks, action_values):
    """TrainingDataset.score == load_batch_host, AGNetwork.forward and the numpy reference, one after the other"""
    from alphagomoku_amd.dataset import TrainingDataset
    path, samples = fragment(olib, tmp_path, n, seed=31 + n)
    assert 60 <= len(samples) <= 200 and len(set(int(a) for a in samples[:, 3])) == 8
    net, _ = network(n, blocks, action_values)
    ds = TrainingDataset(0, n, n)
    ds.add_fragment(path, index=0)
    got = ds.score(net, samples, chunk=16)
    again = ds.score(net, samples)           # chunk 0: 1024 at a time, here one launch of each kind
    assert got == again                      # (floats compared with ==: the same bits)
    host = ds.load_batch_host(samples)
    out = net.forward(host["features"])
    q = out[2] if action_values else None
    _, want = ref.batch_score(out[0], out[1], host["policy_target"].reshape(len(samples), -1), host["value_target"], q,
                              host["action_values_target"].reshape(len(samples), -1, 3) if action_values else None)
    assert got["samples"] == len(samples) == want["samples"] and got["q_cells"] == want["q_cells"] and got["topk_hit"] == want["topk_hit"]
    assert (want["q_cells"] > 0) == bool(action_values)
    for k in ("policy_ce", "value_ce", "q_ce"):
        print("%dx%d %s: device %.17g reference %.17g" % (n, n, k, got[k], want[k]))
        assert close(got[k], want[k]), (k, got[k], want[k])
    assert got["policy_loss"] == got["policy_ce"] / len(samples) and got["accuracy"] == [h / len(samples) for h in got["topk_hit"]]
    ds.close()
    net.close()


def test_refusals(agx_lib, olib, tmp_path):
    from alphagomoku_amd import AgxError, _lib, build
    from alphagomoku_amd.dataset import TrainingDataset
    path, samples = fragment(olib, tmp_path, 15, seed=46)
    ds = TrainingDataset(0, 15, 15)
    ds.add_fragment(path, index=0)
    small, _ = network(9, 1, 0)
    with pytest.raises(AgxError, match="agx error 1: .*15x15.*9x9"):      # AGX_ERR_INVALID: the dataset's board is not the network's
        ds.score(small, samples)
    small.close()
    # datasets are square (agx_dataset_create), the networks' boards are not: each dimension is compared on its own
    from alphagomoku_amd import synthetic
    from alphagomoku_amd.networks import AGNetwork
    square = TrainingDataset(0, 12, 12)
    for r, c in ((7, 12), (12, 7)):
        desc = synthetic.net_desc(rows=r, cols=c, blocks=1, filters=64, action_values=0)
        wide = AGNetwork(desc)
        wide.loadWeights(synthetic.make_weights(desc, seed=3)[0])
        with pytest.raises(AgxError, match="agx error 1: .*12x12.*%dx%d" % (r, c)):
            square.score(wide, samples[:4])
        wide.close()
    square.close()
    net, blob = network(15, 2, 0)
    with pytest.raises(AgxError, match="agx error 1"):                   # n == 0
        ds.score(net, np.zeros((0, 4), np.int32))
    with pytest.raises(AgxError, match="agx error 1"):
        ds.score(net, samples, chunk=-1)
    with pytest.raises(AgxError, match="agx error 1: .*fragment 3"):      # the dataset's own refusal passes through
        ds.score(net, np.array([[3, 0, 0, 0]], np.int32))
    total = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first
    assert agx_lib.agx_net_score_outputs(15, 15, 0, total, total, None, total, total, None, None, total, None) == 1      # n == 0
    assert agx_lib.agx_net_score_outputs(15, 15, 4, total, total, total, total, total, None, None, total, None) == 1    # q without its target
    assert agx_lib.agx_net_score_outputs(15, 15, 4, total, total, None, total, total, None, None, None, None) == 1      # no total
    assert agx_lib.agx_net_score_outputs(21, 15, 4, total, total, None, total, total, None, None, total, None) == 1     # no such board
    assert agx_lib.agx_net_score_clear(None, None) == 1
    out = _lib.AgxNetScore()
    assert agx_lib.agx_net_score_dataset(None, ds._h, 1, samples.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(out), None) == 1
    # top_k = 5 through the compiled ag::getAccuracy (tests/cpp/net_score_main.cpp); its counts are TrainingDataset.score's
    want = ds.score(net, samples)
    listing, weights = tmp_path / "samples.txt", tmp_path / "weights.bin"
    listing.write_text("".join("%d %d %d\n" % (g, k, a) for _, g, k, a in samples))
    blob.astype(np.float32).tofile(weights)
    run = subprocess.run([build.SCORE_TEST, str(path), str(listing), str(weights), "15", "2", "64"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == "accuracy %d %d %d %d %d" % tuple([len(samples)] + want["topk_hit"])
    assert lines[1] == "top2 %d %d %d" % tuple([len(samples)] + want["topk_hit"][:2])
    assert lines[2].startswith("refused: ") and "top_k" in lines[2]
    # the same through agx::TrainingDataset::score and agx::NetScore (include/agx.hpp): sums and means, the same bits as the Python dict's
    facade, means = lines[3].split(), lines[4].split()
    assert facade[0] == "facade" and [int(x) for x in [facade[1]] + facade[5:]] == [want["samples"], want["q_cells"]] + want["topk_hit"]
    assert [float(x) for x in facade[2:5]] == [want["policy_ce"], want["value_ce"], want["q_ce"]] and want["policy_ce"] > 0
    assert means[0] == "means" and [float(x) for x in means[1:]] == [want["policy_loss"], want["value_loss"], want["q_loss"]] + want["accuracy"]
    assert lines[5].startswith("refused: ") and "accuracy" in lines[5] and lines[-1] == "ok" and len(lines) == 7
    ds.close()
    net.close()
