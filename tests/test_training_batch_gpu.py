"""Training batches on the device (csrc/training_batch.hip, alphagomoku_amd/dataset.py) against the CPU restatement of the reference's
load_batch (tests/training_batch_ref.py).  Every comparison is array_equal on the raw bits; every output tensor lies between two
guard zones filled with a sentinel that must survive the launch."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import training_batch_ref as ref

pytestmark = pytest.mark.gpu

CONFIGS = [("FREESTYLE", 15), ("STANDARD", 15), ("RENJU", 15), ("CARO5", 15), ("CARO6", 15), ("FREESTYLE", 20), ("CARO5", 20)]
GUARD = 333          # elements before and after every output (odd on purpose: the outputs are then only element-aligned)
SENTINEL = 0x5A
OUTPUTS = ["input", "features", "policy_target", "value_target", "moves_left_target", "action_values_target"]


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@pytest.fixture(scope="module")
def device(agx_lib):
    """the tests below stage their outputs in device memory of the library's own runtime (agx_malloc); torch tensors as the destination are
    covered by test_torch_tensors_on_a_torch_stream, in a process of its own"""
    return agx_lib


@pytest.fixture(scope="module")
def cases(olib, tmp_path_factory):
    """per configuration: two oracle self-play games and the crafted game, saved as a fragment file (every other one compressed)"""
    import zlib
    out, root = {}, tmp_path_factory.mktemp("fragments")
    for i, (rules, n) in enumerate(CONFIGS):
        games = [ref.oracle_game(olib, ol.RULES[rules], n, 11 + 7 * i + k, sims=32) for k in range(2)]
        games.append(ref.crafted_game(olib, n, with_filler=(n == 20)))
        path = root / ("%s_%d.bin" % (rules, n))
        ref.write_fragment(path, rules, n, games)
        if i % 2:
            path.write_bytes(zlib.compress(path.read_bytes()))
        out[(rules, n)] = dict(path=path, games=[ref.parse_game(g) for g in games], raw=games)
    return out


NP_KIND = {"input": np.float32, "features": np.int32}


def guarded(shapes, half=False):
    """the six outputs inside larger device allocations filled with the sentinel"""
    from alphagomoku_amd.networks import DeviceBuffer
    whole, pointers = {}, {}
    for k in OUTPUTS:
        t = np.dtype(np.float16 if (k == "input" and half) else NP_KIND.get(k, np.float32))
        count = int(np.prod(shapes[k]))
        buf = DeviceBuffer((count + 2 * GUARD) * t.itemsize)
        buf.upload(np.full((count + 2 * GUARD) * t.itemsize, SENTINEL, np.uint8))
        whole[k] = (buf, t, count)
        pointers[k] = buf.ptr.value + GUARD * t.itemsize
    return whole, pointers


def check_against(lib, whole, shapes, want, what=""):
    from alphagomoku_amd import check
    check(lib.agx_device_synchronize())
    for k in OUTPUTS:
        buf, t, count = whole[k]
        flat = buf.download((count + 2 * GUARD,), t)
        buf.free()
        raw = flat.view(np.uint8)
        item = t.itemsize
        assert (raw[:GUARD * item] == SENTINEL).all() and (raw[-GUARD * item:] == SENTINEL).all(), "%s: guard zone of %s overwritten" % (what, k)
        got = flat[GUARD:GUARD + count].reshape(shapes[k])
        expect = want[k]
        assert got.shape == expect.shape, (what, k, got.shape, expect.shape)
        a, b = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(expect).view(np.uint8)
        assert np.array_equal(a, b), "%s: %s differs in %d bytes (first at flat element %d)" % (what, k, int((a != b).sum()), int(np.flatnonzero(a != b)[0]) // item)


def run_and_check(lib, ds, olib, rules, n, fragments, samples, half=False, policy="torch_api", what="", stream=None):
    shapes = ds.tensor_shapes(len(samples))
    whole, pointers = guarded(shapes, half)
    ds.load_batch_pointers(samples, pointers, half=half, policy=policy, stream=stream)
    want = ref.reference_batch(olib, ol.RULES[rules], n, fragments, samples, policy=policy, dtype=np.float16 if half else np.float32)
    want["features"] = want["features"].view(np.int32)
    check_against(lib, whole, shapes, want, what)
    return want


def all_samples(games, fragment=0):
    return np.array([(fragment, g, k, a) for g, game in enumerate(games) for k in range(len(game["samples"])) for a in range(8)], np.int32)


def test_chosen_inputs_are_not_vacuous(olib, cases):
    """(helper only) over the compared set: proven win / loss / draw edges, a proven draw without visits, a renju foul bit, a 20x20
    sample with a 255-gap filler entry, a sample with sum_visits == 0"""
    seen = dict(wins=0, losses=0, draws=0, draws_without_visits=0, no_visits=0, filler20=0, fouls=0)
    for (rules, n), case in cases.items():
        for game in case["games"]:
            for k in range(len(game["samples"])):
                st = ref.sample_stats(olib, game, k, n)
                for key in ("wins", "losses", "draws", "draws_without_visits"):
                    seen[key] += st[key]
                seen["no_visits"] += st["sum_visits"] == 0
                seen["filler20"] += (n == 20 and st["filler"])
                if rules == "RENJU":
                    seen["fouls"] += int(((ref.reference_sample(olib, 2, n, game, k, 0)["features"] >> 6) & 1).sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("rules,n", CONFIGS)
def test_every_sample_under_every_symmetry(device, olib, cases, rules, n):
    from alphagomoku_amd.dataset import TrainingDataset
    case = cases[(rules, n)]
    ds = TrainingDataset(ol.RULES[rules], n, n)
    ds.add_fragment(case["path"], index=0)
    fouls = 0
    samples = all_samples(case["games"])          # every sample of every game under all 8 symmetries
    assert len(samples) == 8 * sum(len(g["samples"]) for g in case["games"]) >= 8 * 20
    fragments = {0: case["games"]}
    for at in range(0, len(samples), 1024):      # a launch per 1024 rows
        part = samples[at:at + 1024]
        want = run_and_check(device, ds, olib, rules, n, fragments, part, what="%s %d float32 rows %d.." % (rules, n, at))
        run_and_check(device, ds, olib, rules, n, fragments, part, half=True, policy="visits", what="%s %d float16 visits rows %d.." % (rules, n, at))
        sums = want["policy_target"].reshape(len(part), -1).sum(axis=1, dtype=np.float64)
        assert np.abs(sums - 1.0).max() < 1e-5
        fouls = fouls + int(((want["features"].view(np.uint32) >> 6) & 1).sum())
    assert rules != "RENJU" or fouls > 0
    ds.close()


def test_batch_shapes_repeats_and_mixed_fragments(device, olib, cases):
    """batches of 1, 63, 64, 65, 1024 and 2500 (more samples than one launch has waves), drawn by the sampler from TWO fragments, with
    repeated samples; sample b's action values at index b"""
    from alphagomoku_amd.dataset import TrainingDataset
    case = cases[("FREESTYLE", 15)]
    ds = TrainingDataset(0, 15, 15)
    ds.add_fragment(case["path"], index=3)
    second = [case["raw"][2], case["raw"][0]]
    path = case["path"].parent / "second.bin"
    ref.write_fragment(path, "FREESTYLE", 15, second)
    ds.add_fragment(path, index=9)
    fragments = {3: case["games"], 9: [ref.parse_game(g) for g in second]}
    rng = np.random.default_rng(5)
    for size in (1, 63, 64, 65, 1024, 2500):
        samples = ds.sample(size, rng)
        if size >= 63:
            samples[5] = samples[1]
            samples[-1] = samples[1]
            assert len({int(f) for f in samples[:, 0]}) == 2
        want = run_and_check(device, ds, olib, "FREESTYLE", 15, fragments, samples, what="batch of %d" % size)
        if size >= 63:   # what the reference's pointer slip would break: different samples have different action values
            av = want["action_values_target"].reshape(size, -1)
            assert any(not np.array_equal(av[0], av[b]) for b in range(1, size))
    ds.close()


def test_two_batches_back_to_back_on_one_stream(device, olib, cases):
    """two batches enqueued on one non-default stream with no host wait between them; one stream synchronise, then both are right"""
    import ctypes
    from alphagomoku_amd import check
    from alphagomoku_amd.dataset import TrainingDataset
    case = cases[("RENJU", 15)]
    ds = TrainingDataset(2, 15, 15)
    ds.add_fragment(case["path"], index=0)
    samples = all_samples(case["games"])
    parts = [samples[:300], samples[300:700]]
    stream = ctypes.c_void_p()
    check(device.agx_stream_create(ctypes.byref(stream)))
    staged = [guarded(ds.tensor_shapes(len(p))) for p in parts]
    check(device.agx_device_synchronize())
    for part, (whole, pointers) in zip(parts, staged):
        ds.load_batch_pointers(part, pointers, stream=stream)      # no host wait between the two
    check(device.agx_stream_synchronize(stream))
    for part, (whole, pointers) in zip(parts, staged):
        want = ref.reference_batch(olib, 2, 15, {0: case["games"]}, part)
        want["features"] = want["features"].view(np.int32)
        check_against(device, whole, ds.tensor_shapes(len(part)), want, "back to back")
    ds.close()
    check(device.agx_stream_destroy(stream))


def test_feature_words_feed_the_network(device, olib, cases):
    """the uint32 words the loader writes, fed to agx_nn_forward where they lie, give the bits the helper's words give"""
    from alphagomoku_amd import check, synthetic
    from alphagomoku_amd.dataset import TrainingDataset
    from alphagomoku_amd.networks import AGNetwork, DeviceBuffer
    case = cases[("STANDARD", 15)]
    ds = TrainingDataset(1, 15, 15)
    ds.add_fragment(case["path"], index=0)
    samples = all_samples(case["games"])[:64]
    shapes = ds.tensor_shapes(64)
    bufs = {k: DeviceBuffer(int(np.prod(shapes[k])) * 4) for k in OUTPUTS}
    ds.load_batch_pointers(samples, {k: b.ptr.value for k, b in bufs.items()})
    want = ref.reference_batch(olib, 1, 15, {0: case["games"]}, samples)
    desc = synthetic.net_desc(blocks=2, filters=64)
    blob, _ = synthetic.make_weights(desc)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    policy, value = DeviceBuffer(64 * 225 * 4), DeviceBuffer(64 * 3 * 4)
    net.forwardDevice(bufs["features"].ptr, 64, policy.ptr, value.ptr, None)   # (the default stream, like the loader's launch)
    check(device.agx_device_synchronize())
    p_ref, v_ref = net.forward(want["features"])
    assert np.array_equal(policy.download((64, 225), np.uint32), p_ref.view(np.uint32)) and np.array_equal(value.download((64, 3), np.uint32), v_ref.view(np.uint32))
    for b in list(bufs.values()) + [policy, value]:
        b.free()
    net.close()
    ds.close()


def test_games_of_a_device_pool_from_the_live_buffer(device, olib):
    """self-play games of a small device pool, collected with agx_game_buffer_collect and loaded straight from the buffer handle"""
    from alphagomoku_amd import selfplay, synthetic
    from alphagomoku_amd.dataset import TrainingDataset
    from alphagomoku_amd.networks import AGNetwork
    desc = synthetic.net_desc(blocks=2, filters=64)
    blob, _ = synthetic.make_weights(desc)
    net = AGNetwork(desc)
    net.loadWeights(blob)
    pool = selfplay.GeneratorPool(selfplay.default_config(n_games=16, max_batch_size=8, max_simulations=32, tss_table_entries=1 << 14, record_format=2))
    pool.begin(selfplay.pack_openings(synthetic.make_openings(15, 64, seed0=3)))
    buffer = selfplay.GameBuffer(0, 15, 15)
    for _ in range(40):
        for _ in range(100):
            pool.step(net)
        buffer.collect(pool)
        if buffer.stats()["games"] >= 3:
            break
    assert pool.stats()["first_error"] == 0 and buffer.stats()["games"] >= 3
    ds = TrainingDataset(0, 15, 15)
    ds.add_fragment(buffer, index=0)
    games = [ref.parse_game(buffer.game(i)) for i in range(buffer.stats()["games"])]
    sizes = ds.games()
    assert [int(x) for x in sizes[:, 2]] == [len(g["samples"]) for g in games] and ds.stats() == buffer.stats()
    samples = all_samples(games)[::3][:1500]
    run_and_check(device, ds, olib, "FREESTYLE", 15, {0: games}, samples, what="device pool")
    ds.close()
    buffer.close()
    pool.close()
    net.close()


def test_reference_named_entry_points_from_a_compiled_program(device, olib, cases, tmp_path):
    """ag::load_dataset_fragment / get_dataset_size / get_tensor_shapes / load_batch (host pointers) from tests/cpp/training_batch_main.cpp"""
    from alphagomoku_amd import build
    case = cases[("CARO5", 15)]   # (a compressed fragment)
    samples = all_samples(case["games"])[::5][:200]
    listing, result = tmp_path / "samples.txt", tmp_path / "out.bin"
    listing.write_text("".join("%d %d %d\n" % (g, k, a) for _, g, k, a in samples))
    run = subprocess.run([build.TRAINING_TEST, str(case["path"]), str(listing), str(result)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[0] == "games %d" % len(case["games"]) and lines[-1] == "ok"
    assert [ln.split()[1:] for ln in lines[1:1 + len(case["games"])]] == [["7", str(g), str(len(game["samples"])), "8"] for g, game in enumerate(case["games"])]
    assert lines[1 + len(case["games"])] == "shapes 4 %d 15 15 32 | 4 1 3 3" % len(samples)
    want = ref.reference_batch(olib, 3, 15, {0: case["games"]}, samples)
    got = np.fromfile(result, dtype=np.float32)
    expect = np.concatenate([want[k].reshape(-1) for k in ("input", "policy_target", "value_target", "moves_left_target", "action_values_target")])
    assert got.size == expect.size and np.array_equal(got.view(np.uint32), expect.view(np.uint32))
    assert os.path.getsize(result) == 4 * expect.size


def test_torch_tensors_on_a_torch_stream(agx_lib, tmp_path):
    """TrainingDataset.load_batch: torch allocates on the current ROCm device, the kernel writes through data_ptr() on torch's current stream.
    In a process of its own: torch's HIP runtime has to be shared with the library before either touches the GPU."""
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "training_batch_torch_main.py")
    run = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1].startswith("ok"), run.stdout[-3000:] + run.stderr[-3000:]
