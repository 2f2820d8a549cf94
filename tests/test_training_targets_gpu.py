"""The reference's default training targets on the device (csrc/training_batch.hip: AGX_BATCH_POLICY_VALUES and action_values_weight)
against their CPU restatement (tests/training_targets_ref.py).  Every output lies between two guard zones filled with a sentinel that must
survive the launch.

What is compared how, and why the policy of "values" has a bar where everything else is array_equal on the raw bits: its formula goes through
logf and expf, which the device and a host libm each give to within 1 ulp, not to the same bits.  The logits 50 * Q + log(eps + P) reach 150
in magnitude (Q = 1 + 2 / (1 + distance) <= 3), where one float32 step is 1.5e-5.  A 1-ulp difference in logf can move a logit by one such
step and the maximum of the logits by another, the subtraction logit - maximum rounds once more: up to about 5e-5 absolute in the argument
of expf, which is 5e-5 RELATIVE in every exponential and, because all terms are positive, at most as much in their sum (the float32 additions
themselves run in the same order on both sides).  The quotient exponential / sum doubles that, expf's own ulp and the division add a few
1e-7: about 1.2e-4, the bar is |got - want| <= 2e-4 * want.  tests/test_training_targets_cpu.py holds the float32 restatement to the same
bar against float64.  Cells that are exactly 0.0f (the occupied ones) are compared as a set."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import training_batch_ref as ref
import training_targets_ref as tref

pytestmark = pytest.mark.gpu

CONFIGS = [("FREESTYLE", 15), ("RENJU", 15), ("CARO5", 20), ("FREESTYLE", 9)]   # 9x9: n < N on the 15-wide instantiation
GUARD = 333
SENTINEL = 0x5A
OUTPUTS = ["input", "features", "policy_target", "value_target", "moves_left_target", "action_values_target", "action_values_weight"]
NP_KIND = {"input": np.float32, "features": np.int32}
BAR = 2e-4


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@pytest.fixture(scope="module")
def device(agx_lib):
    return agx_lib


@pytest.fixture(scope="module")
def cases(olib, tmp_path_factory):
    """per configuration: two oracle self-play games and the two crafted games, saved as a fragment file"""
    out, root = {}, tmp_path_factory.mktemp("targets")
    for i, (rules, n) in enumerate(CONFIGS):
        games = [ref.oracle_game(olib, ol.RULES[rules], n, 23 + 5 * i + k, sims=32) for k in range(2)] + tref.crafted_games(olib, n)
        path = root / ("%s_%d.bin" % (rules, n))
        ref.write_fragment(path, rules, n, games)
        out[(rules, n)] = dict(path=path, games=[ref.parse_game(g) for g in games])
    return out


@pytest.fixture(scope="module")
def expected(olib, cases):
    """the restatement of every sample under every symmetry, once per configuration and policy mode, shared by the tests"""
    memo = {}

    def get(rules, n, policy):
        if (rules, n, policy) not in memo:
            games = cases[(rules, n)]["games"]
            memo[(rules, n, policy)] = tref.reference_batch(olib, ol.RULES[rules], n, {0: games}, all_samples(games), policy=policy)
        return memo[(rules, n, policy)]
    return get


def all_samples(games, fragment=0):
    return np.array([(fragment, g, k, a) for g, game in enumerate(games) for k in range(len(game["samples"])) for a in range(8)], np.int32)


def guarded(shapes, names):
    from alphagomoku_amd.networks import DeviceBuffer
    whole, pointers = {}, {}
    for k in names:
        t = np.dtype(NP_KIND.get(k, np.float32))
        count = int(np.prod(shapes[k]))
        buf = DeviceBuffer((count + 2 * GUARD) * t.itemsize)
        buf.upload(np.full((count + 2 * GUARD) * t.itemsize, SENTINEL, np.uint8))
        whole[k] = (buf, t, count)
        pointers[k] = buf.ptr.value + GUARD * t.itemsize
    return whole, pointers


def collect(lib, whole, shapes, what):
    """the outputs, after checking the guard zones"""
    from alphagomoku_amd import check
    check(lib.agx_device_synchronize())
    got = {}
    for k, (buf, t, count) in whole.items():
        flat = buf.download((count + 2 * GUARD,), t)
        buf.free()
        raw = flat.view(np.uint8)
        assert (raw[:GUARD * t.itemsize] == SENTINEL).all() and (raw[-GUARD * t.itemsize:] == SENTINEL).all(), "%s: guard zone of %s overwritten" % (what, k)
        got[k] = flat[GUARD:GUARD + count].reshape(shapes[k]).copy()
    return got


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def load(lib, ds, samples, policy, q_weights, what):
    shapes = ds.tensor_shapes(len(samples), q_weights)
    whole, pointers = guarded(shapes, [k for k in OUTPUTS if k in shapes])
    ds.load_batch_pointers(samples, pointers, policy=policy, q_weights=q_weights)
    return collect(lib, whole, shapes, what)


def test_chosen_inputs_are_not_vacuous(expected):
    """(helper only) over the compared set: a proven win without visits, a proven loss, a proven draw, a visited unknown cell, an empty cell
    without an entry, a sample with a proven minimax score and sum_visits == 0, one with sum_P > 1, one with unvisited_actions_count == 0,
    a cell where the -20 clamp is active and one where it is not, a sample whose weight sum is 0"""
    from alphagomoku_amd import _lib
    assert _lib.BATCH_POLICY_FLAGS["values"] == 4      # the mode the set is compared in
    seen = dict(wins_without_visits=0, losses=0, draws=0, visited_unknown=0, empty_without_entry=0, proven_root_without_visits=0, sum_P_above_1=0, no_unvisited=0,
                clamped=0, unclamped=0, weight_sum_0=0)
    for rules, n in CONFIGS:
        for st in expected(rules, n, "values")["stats"]:
            for key in ("wins_without_visits", "losses", "draws", "visited_unknown", "empty_without_entry", "clamped", "unclamped"):
                seen[key] += st[key]
            seen["proven_root_without_visits"] += st["sum_visits"] == 0 and st["minimax_proven"]
            seen["sum_P_above_1"] += st["sum_P"] > 1.0
            seen["no_unvisited"] += st["unvisited"] == 0
            seen["weight_sum_0"] += st["weight_sum"] == 0
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("rules,n", CONFIGS)
def test_values_targets_of_every_sample_under_every_symmetry(device, cases, expected, rules, n):
    from alphagomoku_amd.dataset import TrainingDataset
    case = cases[(rules, n)]
    ds = TrainingDataset(ol.RULES[rules], n, n)
    ds.add_fragment(case["path"], index=0)
    samples = all_samples(case["games"])
    want = expected(rules, n, "values")
    worst = 0.0
    for at in range(0, len(samples), 1024):      # a launch per 1024 rows
        part, what = samples[at:at + 1024], "%s %d rows %d.." % (rules, n, at)
        got = load(device, ds, part, "values", True, what)
        for k in ("features", "input", "value_target", "moves_left_target", "action_values_target", "action_values_weight"):
            expect = want[k][at:at + 1024]
            assert same_bits(got[k], expect.view(np.int32) if k == "features" else expect), "%s: %s differs" % (what, k)
        p, e = got["policy_target"].astype(np.float64), want["policy_target"][at:at + 1024].astype(np.float64)
        assert np.array_equal(got["policy_target"].view(np.uint32) == 0, want["policy_target"][at:at + 1024].view(np.uint32) == 0), "%s: the zero cells differ" % what
        deviation = np.abs(p - e) / np.where(e > 0, e, 1.0)
        worst = max(worst, float(deviation.max()))
        print("%s: values policy, largest relative deviation %.3g (bar %.3g)" % (what, float(deviation.max()), BAR))
        assert (np.abs(p - e) <= BAR * e).all(), what
        # the policy sums to 1 as far as float32 lets it: the divisor is a sequential float32 sum of up to n * n positive terms (each addition
        # rounds, relative 2^-24 at the most), every quotient rounds once more
        assert np.abs(p.reshape(len(part), -1).sum(axis=1) - 1.0).max() <= (n * n + 1) * 2.0 ** -24
        without = load(device, ds, part, "values", False, what + " without weights")   # the weight pointer may be NULL: the other outputs do not change
        assert all(same_bits(without[k], got[k]) for k in without) and "action_values_weight" not in without
    ds.close()


@pytest.mark.parametrize("rules,n", CONFIGS)
@pytest.mark.parametrize("policy", ["torch_api", "visits"])
def test_weights_of_the_visit_count_modes_and_the_old_call(device, cases, expected, rules, n, policy):
    """action_values_weight in the two existing modes against the restatement, and everything else the extended call writes there against the
    old call: bit-identical"""
    from alphagomoku_amd import check
    from alphagomoku_amd.dataset import TrainingDataset
    case = cases[(rules, n)]
    ds = TrainingDataset(ol.RULES[rules], n, n)
    ds.add_fragment(case["path"], index=0)
    samples = all_samples(case["games"])
    want = expected(rules, n, "values")["action_values_weight"]   # one rule in every mode
    flags = 2 if policy == "visits" else 0
    for at in range(0, len(samples), 1024):
        part, what = samples[at:at + 1024], "%s %d %s rows %d.." % (rules, n, policy, at)
        got = load(device, ds, part, policy, True, what)
        assert same_bits(got["action_values_weight"], want[at:at + 1024]), what
        shapes = ds.tensor_shapes(len(part))
        whole, pointers = guarded(shapes, OUTPUTS[:6])
        rec = np.ascontiguousarray(part)
        ptr = lambda k: ctypes.c_void_p(pointers[k])  # noqa: E731
        check(device.agx_dataset_load_batch(ds._h, len(part), rec.ctypes.data_as(ctypes.c_void_p), ptr("input"), ptr("features"), ptr("policy_target"), ptr("value_target"),
                                            ptr("moves_left_target"), ptr("action_values_target"), flags, None))
        old = collect(device, whole, shapes, what + " old call")
        for k in OUTPUTS[:6]:
            assert same_bits(old[k], got[k]), "%s: %s of the extended call differs from the old call's" % (what, k)
    ds.close()


def test_host_pointer_form_and_a_batch_larger_than_a_launch(device, cases, expected):
    """agx_dataset_load_batch_host_ex; 2500 rows (more samples than one launch has waves), repeated samples"""
    from alphagomoku_amd.dataset import TrainingDataset
    case = cases[("FREESTYLE", 15)]
    ds = TrainingDataset(0, 15, 15)
    ds.add_fragment(case["path"], index=0)
    samples = all_samples(case["games"])
    pick = np.random.default_rng(4).integers(0, len(samples), 2500)
    want = expected("FREESTYLE", 15, "values")
    got = ds.load_batch_host(samples[pick], policy="values", q_weights=True)
    for k in ("value_target", "moves_left_target", "action_values_target", "action_values_weight"):
        assert same_bits(got[k], want[k][pick]), k
    assert same_bits(got["features"].view(np.uint32), want["features"][pick])
    p, e = got["policy_target"].astype(np.float64), want["policy_target"][pick].astype(np.float64)
    assert (np.abs(p - e) <= BAR * e).all() and np.array_equal(p == 0, e == 0)
    plain = ds.load_batch_host(samples[pick][:70], policy="visits")
    assert "action_values_weight" not in plain
    ds.close()


def test_the_facade_from_a_compiled_program(device, cases, tmp_path):
    """tests/cpp/training_targets_main.cpp: agx::TrainingDataset::loadBatch(AgxBatchTensors), the weighted agx::head_loss_grad and the
    extended agx::TrainingDataset::score print and write what the Python calls give: the same bits, the same totals"""
    from alphagomoku_amd import build, check, synthetic, _lib
    from alphagomoku_amd.dataset import TrainingDataset
    from alphagomoku_amd.networks import AGNetwork, DeviceBuffer
    case = cases[("FREESTYLE", 15)]
    samples = all_samples(case["games"])[::7][:150]
    n, hw = len(samples), 225
    desc = synthetic.net_desc(blocks=1, filters=64, action_values=1)
    blob, _ = synthetic.make_weights(desc)
    listing, weights, result = tmp_path / "samples.txt", tmp_path / "weights.bin", tmp_path / "out.bin"
    listing.write_text("".join("%d %d %d\n" % (g, k, a) for _, g, k, a in samples))
    np.ascontiguousarray(blob, dtype=np.float32).tofile(weights)
    run = subprocess.run([build.TARGETS_TEST, str(case["path"]), str(listing), str(weights), "0", "15", "1", "64", str(result)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == "batch %d %d" % (n, hw) and lines[-1] == "ok"

    ds = TrainingDataset(0, 15, 15)
    ds.add_fragment(case["path"], index=0)
    mine = ds.load_batch_host(samples, policy="values", q_weights=True)
    expect = np.concatenate([mine[k].reshape(-1) for k in ("policy_target", "action_values_target", "action_values_weight")])
    got = np.fromfile(result, dtype=np.float32)
    assert got.size == expect.size and np.array_equal(got.view(np.uint32), expect.view(np.uint32))

    bufs = {k: DeviceBuffer(mine[k].nbytes) for k in ("policy_target", "value_target", "action_values_target", "action_values_weight")}
    for k, b in bufs.items():
        b.upload(mine[k])
    zeros = {k: DeviceBuffer(4 * c) for k, c in (("policy", n * hw), ("value", n * 3), ("q", n * hw * 3))}
    for k, c in (("policy", n * hw), ("value", n * 3), ("q", n * hw * 3)):
        zeros[k].upload(np.zeros(c, np.float32))
    records, total = DeviceBuffer(48 * n), DeviceBuffer(72)
    check(device.agx_net_score_clear(total.ptr, None))
    check(device.agx_head_loss_grad_weighted(15, 15, n, zeros["policy"].ptr, zeros["value"].ptr, zeros["q"].ptr, bufs["policy_target"].ptr, bufs["value_target"].ptr,
                                             bufs["action_values_target"].ptr, bufs["action_values_weight"].ptr, 1.0, 1.0, 0.05, None, None, None, records.ptr, total.ptr,
                                             None))
    check(device.agx_device_synchronize())
    out = _lib.AgxNetScore()
    check(device.agx_memcpy_d2h(ctypes.byref(out), total.ptr, 72))
    assert lines[1] == "loss %d %.17g %.17g %.17g %d" % (out.samples, out.policy_ce, out.value_ce, out.q_ce, out.q_cells)
    assert out.samples == n and out.q_cells == int((mine["action_values_weight"] > 0).sum()) and out.q_ce > 0
    for b in list(bufs.values()) + list(zeros.values()) + [records, total]:
        b.free()

    net = AGNetwork(desc)
    net.loadWeights(blob)
    score = ds.score(net, samples, policy="values", q_weights=True)
    assert lines[2] == "score %d %.17g %.17g %.17g %d %d %d %d %d" % ((score["samples"], score["policy_ce"], score["value_ce"], score["q_ce"], score["q_cells"])
                                                                      + tuple(score["topk_hit"]))
    for chunk in (1, 64, 149):                       # the total does not depend on chunk
        assert ds.score(net, samples, chunk=chunk, policy="values", q_weights=True) == score
    plain = ds.score(net, samples)
    assert plain == ds.score(net, samples, policy="torch_api", q_weights=False) and plain["q_ce"] != score["q_ce"]
    net.close()
    ds.close()


def test_trainer_on_the_reference_targets(agx_lib, cases, tmp_path):
    """Trainer(policy="values", q_weights=True) on a ResnetPVQ module, head_loss against head_loss_reference with weights: in a process of its
    own, torch's HIP runtime has to be shared with the library before either touches the GPU"""
    case = cases[("FREESTYLE", 15)]
    samples = tmp_path / "samples.npy"
    np.save(samples, all_samples(case["games"])[::11][:96])
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "training_targets_torch_main.py")
    run = subprocess.run([sys.executable, script, str(case["path"]), str(samples)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1].startswith("ok"), run.stdout[-3000:] + run.stderr[-3000:]
