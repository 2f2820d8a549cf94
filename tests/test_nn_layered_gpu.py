"""The layered residual towers (csrc/nn_layered.hip: 192 .. 512 filters, activations in global memory, a launch per layer) on the GPU.

  * exact parity with nn_exact.reference (criterion: test_nn_exact_gpu.assert_exact, imported) on the networks of nn_layered_cases.py, which
    test_nn_layered_cpu.py proves exact: 5x5, 7x9, 15x15, 20x20 x 192 / 256 / 512 filters x 0, 1, 2 blocks x pv / raw / pvq x random and
    transparent heads, random and directed boards;
  * batch shapes: 1, 3 and more boards than the grid has waves' items, a permuted slot list, a device count below max_batch and of 0, launch
    widths 1, 7 and all, a launch longer than the activation planes (run slice by slice): bit-identical rows;
  * AGX_NN_LAYERED=1 at 64 / 128 filters against the default kernels (a child process: the variable is read when weights are loaded);
  * He-init networks against the storage-rounding restatement within a bound derived on the CPU;
  * through the layers: whole games with the network in the loop, a pool stepped on the device, evaluate_positions, the dataset score, the
    trainer and export (a child process with torch), a reload that fails, ag::AGNetwork from a compiled program;
  * what stays refused.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import nn_exact as nx
import nn_layered_cases as lc
import oracle_lib as ol
from alphagomoku_amd import synthetic
from test_nn_exact_gpu import assert_exact, load

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = np.uint32(0x7FC0DEAD)                                 # a NaN payload no kernel produces


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@functools.lru_cache(maxsize=None)
def reference_of(case, batch):
    desc, blob = lc.weights(*case)
    return nx.reference_in_chunks(desc, blob, lc.feature_batch(case[0], case[1], batch))


# ------------------------------------------------------------------------------------------------------------------------ exact parity

@pytest.mark.parametrize("rows,cols,filters,kind,blocks,heads", lc.network_cases())
def test_layered_tower_is_exact(agx_lib, rows, cols, filters, kind, blocks, heads):
    case = (rows, cols, filters, kind, blocks, heads)
    desc, blob = lc.weights(*case)
    net = load(desc, blob)
    try:
        for batch in lc.BATCHES:
            out = net.forward(lc.feature_batch(rows, cols, batch))
            assert_exact(out, desc, blob, reference_of(case, batch), "%s %s, %s boards" % (nx.describe(desc), heads, batch))
        if kind == "raw":                                         # the upper 24 bits of every word set: a raw network reads the low byte only
            f = lc.feature_batch(rows, cols, "random")
            assert all(np.array_equal(a, b) for a, b in zip(net.forward(f), net.forward(f | np.uint32(0xFFFFFF00))))
    finally:
        net.close()


# -------------------------------------------------------------------------------------------------------------------- launch shapes

def net_cdesc(d):
    from alphagomoku_amd._lib import AgxNetDesc
    return AgxNetDesc(d["rows"], d["cols"], d["blocks"], d["filters"], d["in_channels"], d["value_hidden"], d.get("action_values", 0))


def device_buffers(hw, slots, with_q):
    from alphagomoku_amd.networks import DeviceBuffer
    sizes = [slots * hw, slots * 3] + ([slots * hw * 2] if with_q else [])
    bufs = [DeviceBuffer(n * 4) for n in sizes]
    for b, n in zip(bufs, sizes):
        b.upload(np.full(n, SENTINEL, np.uint32))
    return bufs, [(slots, hw), (slots, 3), (slots, hw, 2)][:len(sizes)]


@pytest.mark.parametrize("rows,cols,filters,kind", lc.SHAPE_NETWORKS)
def test_batch_shapes_slot_lists_and_launch_width(agx_lib, rows, cols, filters, kind):
    """600 boards (more wave items than the widest grid has waves, more boards than it has head workgroups) are exact; batches of 1 and 3, a
    scattered selection, launches 1 and 7 compute units wide, and the indirect entry points with a permuted slot list and device counts of
    0, 1, 37, max_batch and above give the same bits for the same board, and leave every other slot alone"""
    from alphagomoku_amd import check
    from alphagomoku_amd.networks import DeviceBuffer
    case = (rows, cols, filters, kind) + lc.POOL_NETWORK
    desc, blob = lc.weights(*case)
    pool = lc.feature_batch(rows, cols, "pool")
    hw, with_q = rows * cols, kind == "pvq"
    net = load(desc, blob)
    try:
        full = net.forward(pool)
        assert_exact(full, desc, blob, reference_of(case, "pool"), "%s, %d boards" % (nx.describe(desc), len(pool)))
        for n in (1, 3, 257):
            idx = (np.arange(n) * 7 + n) % len(pool)
            assert all(np.array_equal(a, b[idx]) for a, b in zip(net.forward(pool[idx]), full)), n
        for width in (1, 7, 0):
            check(agx_lib.agx_net_set_launch_width(net._net, width))
            assert all(np.array_equal(a, b[:40]) for a, b in zip(net.forward(pool[:40]), full)), width
            slots, max_batch = 64, 48
            boards = pool[:slots]
            d_f, d_list, d_count = DeviceBuffer(boards.nbytes), DeviceBuffer(slots * 4), DeviceBuffer(4)
            d_f.upload(boards)
            for count in (0, 1, 37, max_batch, max_batch + 5):
                order = np.random.default_rng(count + rows).permutation(slots).astype(np.int32)
                d_list.upload(order)
                d_count.upload(np.array([count], np.int32))
                bufs, shapes = device_buffers(hw, slots, with_q)
                if with_q:
                    check(agx_lib.agx_nn_forward_indirect_pvq(net._net, d_f.ptr, d_list.ptr, d_count.ptr, max_batch, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None))
                else:
                    check(agx_lib.agx_nn_forward_indirect(net._net, d_f.ptr, d_list.ptr, d_count.ptr, max_batch, bufs[0].ptr, bufs[1].ptr, None))
                check(agx_lib.agx_device_synchronize())
                listed = order[:min(count, max_batch)]
                others = np.setdiff1d(np.arange(slots), listed)
                for b, s, want in zip(bufs, shapes, full):
                    got = b.download(s, np.uint32)
                    assert np.array_equal(got[listed], want.view(np.uint32)[listed]), (width, count)
                    assert (got[others] == SENTINEL).all(), (width, count)
                    b.free()
            for b in (d_f, d_list, d_count):
                b.free()
    finally:
        net.close()


def test_a_launch_longer_than_the_activation_planes(agx_lib):
    """the planes of a stream hold a bounded number of boards (3799 at 192 filters on 5x5) and a longer launch runs slice by slice: 4100
    boards give, board for board, the bits of launches that fit, and are exact where they are looked at"""
    desc, blob = lc.weights(*lc.SLICE_CASE)
    pool, seam = lc.slice_pool(), lc.SLICE_SEAM
    assert agx_lib.agx_net_blob_floats(ctypes.byref(net_cdesc(desc))) == len(blob) and seam.start < 3799 < seam.stop < len(pool)
    net = load(desc, blob)
    try:
        parts = [net.forward(pool[a:b]) for a, b in ((0, 1000), (3700, 3900), (4000, 4100))]
        full = net.forward(pool)
        for (a, b), part in zip(((0, 1000), (3700, 3900), (4000, 4100)), parts):
            assert all(np.array_equal(x, y[a:b]) for x, y in zip(part, full)), (a, b)
        again = net.forward(pool[seam])
        assert all(np.array_equal(x, y[seam]) for x, y in zip(again, full))
        assert_exact(again, desc, blob, reference_of(lc.SLICE_CASE, "slice seam"), "%s, across the slice seam" % nx.describe(desc))
    finally:
        net.close()


def test_pvq_network_without_the_q_buffer_and_a_q_buffer_without_the_head(agx_lib):
    from alphagomoku_amd import AgxError
    from alphagomoku_amd.networks import DeviceBuffer
    rows, cols = 7, 9
    desc, blob = lc.weights(rows, cols, 192, "pvq", 1, "random")
    plain = dict(desc, action_values=0)
    f = lc.feature_batch(rows, cols, "random")
    hw = rows * cols
    net = load(desc, blob)
    net0 = load(plain, blob[:int(sum(np.prod(s) for s in nx.part_shapes(plain)))])
    bufs = [DeviceBuffer(f.nbytes), DeviceBuffer(len(f) * hw * 4), DeviceBuffer(len(f) * 3 * 4), DeviceBuffer(len(f) * hw * 2 * 4)]
    try:
        full, pv = net.forward(f), net0.forward(f)
        bufs[0].upload(f)
        net.forwardDevice(bufs[0].ptr, len(f), bufs[1].ptr, bufs[2].ptr)       # agx_nn_forward on the pvq network: the head is skipped
        agx_lib.agx_device_synchronize()
        skipped = (bufs[1].download((len(f), hw), np.float32), bufs[2].download((len(f), 3), np.float32))
        for a, b, c in zip(full, pv, skipped):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        with pytest.raises(AgxError):                                          # the network has no action-values head: an error, no launch
            net0.forwardDevice(bufs[0].ptr, len(f), bufs[1].ptr, bufs[2].ptr, None, bufs[3].ptr)
    finally:
        for b in bufs:
            b.free()
        net.close()
        net0.close()


def test_one_network_on_two_streams(agx_lib):
    """activations live in a global scratch: one network launched on two streams at the same time keeps a scratch per stream"""
    from alphagomoku_amd import lib, check
    from alphagomoku_amd.networks import AGNetwork, DeviceBuffer
    rows, cols, boards = 9, 9, 300
    hw = rows * cols
    d = synthetic.net_desc(rows=rows, cols=cols, blocks=2, filters=192)
    blob, _ = synthetic.make_weights(d)
    net = AGNetwork(d)
    net.loadWeights(blob)
    batches = [synthetic.random_features(boards, rows, cols, seed=s) for s in (11, 12)]
    expected = [net.forward(b) for b in batches]
    streams, feats, pols, vals = [], [], [], []
    for b in batches:
        s = ctypes.c_void_p()
        check(lib.agx_stream_create(ctypes.byref(s)))
        streams.append(s)
        df = DeviceBuffer(b.nbytes)
        df.upload(b)
        feats.append(df)
        pols.append(DeviceBuffer(boards * hw * 4))
        vals.append(DeviceBuffer(boards * 3 * 4))
    for _ in range(4):
        for k in range(2):
            net.forwardDevice(feats[k].ptr, boards, pols[k].ptr, vals[k].ptr, stream=streams[k])
    for s in streams:
        check(lib.agx_stream_synchronize(s))
    for k in range(2):
        assert np.array_equal(pols[k].download((boards, hw), np.float32), expected[k][0])
        assert np.array_equal(vals[k].download((boards, 3), np.float32), expected[k][1])
    for s in streams:
        check(lib.agx_stream_destroy(s))
    for b in feats + pols + vals:
        b.free()
    net.close()


# ----------------------------------------------------------------------------------------------------- against the existing kernels

SWITCH_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import nn_layered_cases as lc
from test_nn_exact_gpu import load
outputs = {}
for r, c, f, k in lc.SWITCH_CASES:
    desc, blob = lc.weights(r, c, f, k, *lc.POOL_NETWORK)
    net = load(desc, blob)
    for batch in lc.BATCHES:
        for name, a in zip("pvq", net.forward(lc.feature_batch(r, c, batch))):
            outputs["%%d %%d %%d %%s %%s %%s" %% (r, c, f, k, batch, name)] = a
    net.close()
np.savez(sys.argv[1], **outputs)
print("ok")
"""


def test_the_switch_sends_narrow_networks_through_the_layered_tower(agx_lib, tmp_path):
    """AGX_NN_LAYERED=1 (read when weights are loaded: a child process per setting) at 64 and 128 filters on 15x15, 20x20 and 7x9: exact
    networks, so the layered tower's logits equal the default kernels' — both are exact against the float64 reference, and the outputs agree
    to the softmax's last bits; unset and 0 are the default kernels, bit for bit"""
    script = tmp_path / "switch_child.py"
    script.write_text(SWITCH_CHILD % (HERE, os.path.dirname(HERE)))
    results = {}
    for setting in (None, "0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "AGX_NN_LAYERED"}
        if setting is not None:
            env["AGX_NN_LAYERED"] = setting
        out = tmp_path / ("switch_%s.npz" % setting)
        run = subprocess.run([sys.executable, str(script), str(out)], capture_output=True, text=True, timeout=240, env=env)
        assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-3000:]
        results[setting] = dict(np.load(out))
    assert all(results[None][k].tobytes() == results["0"][k].tobytes() for k in results[None])
    differs = 0
    for r, c, f, k in lc.SWITCH_CASES:
        case = (r, c, f, k) + lc.POOL_NETWORK
        desc, blob = lc.weights(*case)
        for batch in lc.BATCHES:
            key = "%d %d %d %s %s " % (r, c, f, k, batch)
            on = [results["1"][key + name] for name in "pvq" if key + name in results["1"]]
            off = [results[None][key + name] for name in "pvq" if key + name in results[None]]
            assert_exact(on, desc, blob, reference_of(case, batch), "AGX_NN_LAYERED=1 %s, %s boards" % (nx.describe(desc), batch))
            assert_exact(off, desc, blob, reference_of(case, batch), "default %s, %s boards" % (nx.describe(desc), batch))
            assert all(np.abs(a - b).max() < 1e-5 for a, b in zip(on, off))
            differs += sum(a.tobytes() != b.tobytes() for a, b in zip(on, off))
    print("outputs whose last bits differ between the two towers: %d" % differs)


# ------------------------------------------------------------------------------------------------------------------ He-init networks

@pytest.mark.parametrize("rows,cols,blocks,filters,kind", lc.HE_INIT_CASES)
def test_he_init_network_within_the_derived_tolerance(agx_lib, rows, cols, blocks, filters, kind):
    """synthetic.make_weights against oracle.nn_ref.forward(storage="fp16") and its restatement with reversible sums.  The bound per output
    is nn_layered_cases.tolerance: 1e-3, or 4 x the restatement's forwards / backwards gap where that is larger — computed on the CPU before
    the device's outputs are looked at.  The measured table is in DESIGN 3.16."""
    from oracle import nn_ref
    desc, blob, f = lc.he_init_case(rows, cols, blocks, filters, kind)
    forwards = lc.restatement(desc, blob, f)
    bounds, gaps = lc.tolerance(desc, blob, f, forwards)
    oracle = nn_ref.forward(desc, blob, f, storage="fp16")
    net = load(desc, blob)
    try:
        out = net.forward(f)
    finally:
        net.close()
    assert len(out) == len(forwards) == len(oracle)
    for name, o, w, r, bound, gap in zip(("policy", "value", "q"), out, oracle, forwards, bounds, gaps):
        dev, dev_r = float(np.abs(o - w).max()), float(np.abs(o - r).max())
        print("tolerance %dx%d %dx%d %s %s: device deviation %.3e from the oracle, %.3e from the restatement; bound %.3e (CPU gap %.3e)"
              % (rows, cols, blocks, filters, kind, name, dev, dev_r, bound, gap))
        assert np.isfinite(o).all() and dev <= bound and dev_r <= bound, (name, dev, dev_r, bound)
    assert (out[0].argmax(1) == oracle[0].argmax(1)).all()


# ----------------------------------------------------------------------------------------------------------------- through the layers

def wide_network(n, blocks, filters, action_values=0, seed=1234):
    d = synthetic.net_desc(rows=n, cols=n, blocks=blocks, filters=filters, action_values=action_values)
    blob, _ = synthetic.make_weights(d, seed=seed)
    return d, blob, load(d, blob)


def test_games_bit_exact_with_the_wide_network_in_the_loop(agx_lib, olib):
    """test_engine_gpu's whole-game comparison (the procedure of test_games_bit_exact_with_the_hip_network_in_the_loop) with a 1 x 192
    network as the evaluator of both sides: 4 games on 15x15, every root compared bit for bit"""
    from test_engine_gpu import _play_and_compare
    _, _, net = wide_network(15, 1, 192)

    def evaluator(feats):
        p, v = net.forward(np.ascontiguousarray(feats, dtype=np.uint32))
        return p, np.ascontiguousarray(v[:, :2])
    try:
        compared, stats = _play_and_compare(olib, 0, games=4, batch=4, sims=100, max_steps=250, evaluator=evaluator, n=15)
        assert compared > 300 and stats["moves_played"] > 0
    finally:
        net.close()


def test_pool_steps_with_the_wide_network_on_the_device(agx_lib):
    """GeneratorPool.step(net) (the pool's network stage on the device: slot list and count read there) == the network's outputs written by
    hand into the slot buffers, with a 1 x 192 ResnetPVQ network"""
    from alphagomoku_amd import selfplay
    _, _, net = wide_network(15, 1, 192, action_values=1)
    openings = synthetic.make_openings(15, 4, seed0=3)
    pools = []
    for _ in range(2):
        pool = selfplay.GeneratorPool(selfplay.default_config(n_games=4, max_batch_size=4, max_simulations=40, tss_table_entries=1 << 14,
                                                              node_capacity=2048, edge_capacity=32768, action_values=1))
        pool.begin(selfplay.pack_openings(openings))
        pools.append(pool)
    try:
        for step in range(12):
            pools[0].step(net)
            pools[1].select_solve()
            slots, feats = pools[1].scheduled()
            if len(slots):
                p, v, q = net.forward(feats)
                pools[1].provide(slots, p, v, q)
            pools[1].expand_backup()
            for g in range(4):
                a, b = pools[0].game_info(g), pools[1].game_info(g)
                assert a["n_moves"] == b["n_moves"] and a["root_visits"] == b["root_visits"], (step, g)
                assert [(e["move"], e["visits"], e["win"], e["draw"], e["prior"]) for e in a["edges"]] == \
                       [(e["move"], e["visits"], e["win"], e["draw"], e["prior"]) for e in b["edges"]], (step, g)
        assert any(e["win"] != 0.0 for e in pools[0].game_info(0)["edges"])   # the q outputs really seed the edges
    finally:
        for pool in pools:
            pool.close()
        net.close()


def test_evaluate_positions_with_a_wide_network(agx_lib):
    """evaluate_positions == tests/position_eval_ref.py applied to what forward returns on the encoded features, bit for bit"""
    import position_eval_ref as ref
    from test_position_eval_gpu import Evaluator, combine_positions, check_against_restatement, tower_rows
    n = 15
    _, _, net = wide_network(n, 1, 192, action_values=1, seed=8)
    positions = combine_positions(n)
    boards, signs = [b for b, _ in positions], [s for _, s in positions]
    pe = Evaluator(agx_lib, ol.RULES["RENJU"], n, len(positions))
    try:
        for mask in (0x01, 0xFF):
            features, status = pe.encode(boards, signs, mask)
            rows = tower_rows(net, features)
            assert not status.any() and rows[2] is not None
            for flags, top_k in ((0, 0), (ref.RENORMALISE, 8)):
                out = pe.evaluate(net, boards, signs, mask, flags, top_k, True)
                assert not out["status"].any()
                check_against_restatement(out, n, positions, mask, flags, top_k, rows, features)
        out = net.evaluate_positions(np.stack(boards), np.array(signs, np.uint8), ol.RULES["RENJU"], top_k=4)
        assert out["policy"].shape == (len(boards), n, n) and out["action_values"].shape == (len(boards), n, n, 2) and np.isfinite(out["value"]).all()
    finally:
        pe.close()
        net.close()


def test_position_searcher_with_a_wide_network(agx_lib):
    """PositionSearcher takes a 1 x 192 network like any other: two 15x15 positions are searched, and searched again with the same
    rows (the result is a function of the position and the network alone)"""
    from test_position_search_gpu import make_searcher
    _, _, net = wide_network(15, 1, 192, seed=8)
    searcher = make_searcher(0, 15, 2)
    try:
        boards = np.zeros((2, 15, 15), np.uint8)
        boards[1, 7, 7] = 1
        signs = np.array([1, 2], np.uint8)
        out = searcher.search(boards, signs, net, max_pv=4)
        again = searcher.search(boards, signs, net, max_pv=4)
        assert not out["status"].any() and (out["root"][:, 0] > 0).all() and (out["visits"].sum(1) > 0).all()
        assert all(np.array_equal(out[k], again[k]) for k in ("status", "root", "best_move", "visits", "prior", "pv"))
    finally:
        searcher.close()
        net.close()


def test_dataset_score_trainer_steps_and_export(agx_lib, olib, tmp_path):
    """in a process of its own (tests/nn_layered_torch_main.py): a 1 x 192 TowerModule -> load_module -> tower against module.eval() within
    the derived tolerance; TrainingDataset.score runs; three Trainer.steps lower the loss; Trainer.export_to reproduces the trained module"""
    import training_batch_ref as tb
    n = 9
    games = [tb.oracle_game(olib, 0, n, 40, sims=32), tb.crafted_game(olib, n)]
    path = tmp_path / "freestyle_9.bin"
    tb.write_fragment(path, "FREESTYLE", n, games)
    parsed = [tb.parse_game(g) for g in games]
    samples = np.array([(0, g, k, a) for g, game in enumerate(parsed) for k in range(len(game["samples"])) for a in range(8)], np.int32)
    samples = samples[::(len(samples) // 64) | 1]
    listing = tmp_path / "samples.npy"
    np.save(listing, samples)
    run = subprocess.run([sys.executable, os.path.join(HERE, "nn_layered_torch_main.py"), str(path), str(listing)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-4000:])
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout[-3000:] + run.stderr[-3000:]


def test_a_failed_reload_keeps_the_old_weights(agx_lib):
    """agx_net_load_weights on a wide network in use: a blob of the wrong size is refused and the loaded weights keep giving their bits; a
    second blob then replaces them and gives a fresh network's bits"""
    from alphagomoku_amd import AgxError
    from alphagomoku_amd.networks import AGNetwork
    d = synthetic.net_desc(rows=7, cols=9, blocks=1, filters=192, action_values=1)
    blob_a, blob_b = synthetic.make_weights(d, seed=1234)[0], synthetic.make_weights(d, seed=4321)[0]
    small, large = synthetic.random_features(3, 7, 9, seed=21), synthetic.random_features(40, 7, 9, seed=22)
    fresh = AGNetwork(d)
    fresh.loadWeights(blob_b)
    want_b = fresh.forward(large)
    fresh.close()
    net = AGNetwork(d)
    try:
        net.loadWeights(blob_a)
        first = net.forward(small)
        assert agx_lib.agx_net_load_weights(net._net, blob_a.ctypes.data_as(ctypes.c_void_p), len(blob_a) - 1) == 1     # AGX_ERR_INVALID
        assert b"expected" in agx_lib.agx_last_error()
        with pytest.raises((AgxError, ValueError, AssertionError)):
            net.loadWeights(blob_a[:-7])
        assert all(np.array_equal(a, b) for a, b in zip(net.forward(small), first))
        net.loadWeights(blob_b)                                                # (a larger batch behind the reload: the scratch is the new tower's)
        assert all(np.array_equal(a, b) for a, b in zip(net.forward(large), want_b))
        net.loadWeights(blob_a)
        assert all(np.array_equal(a, b) for a, b in zip(net.forward(small), first))
    finally:
        net.close()


def test_reference_named_classes_from_a_compiled_program(agx_lib, tmp_path):
    """tests/cpp/layered_main.cpp (built by build.py; the classes themselves needed no change): ag::AGNetwork(config, "ResnetPVQ", 1, 256), a
    weight container read back, one batch forwarded; the program prints its outputs, which must be the Python wrapper's"""
    from alphagomoku_amd import build
    d = synthetic.net_desc(15, 15, 1, 256, action_values=1)
    blob, _ = synthetic.make_weights(d, seed=6)
    path = tmp_path / "wide.agxw"
    synthetic.save_weights(path, d, blob)
    f = synthetic.random_features(3, 15, 15, seed=2)
    fpath = tmp_path / "features.bin"
    f.tofile(fpath)
    run = subprocess.run([build.LAYERED_TEST, str(path), str(fpath), "3"], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().splitlines()[-1] == "ok"
    lines = dict(line.split(" ", 1) for line in run.stdout.strip().splitlines() if " " in line)
    assert lines["name"] == "ResnetPVQ" and lines["outputs"] == "pvq"
    net = load(d, blob)
    try:
        p, v, q = net.forward(f)
    finally:
        net.close()
    want = ["%.9g" % float(np.float32(x)) for x in (p[2].max(), v[2, 0], q[2, 7, 0])]
    assert lines["values"].split() == want


# -------------------------------------------------------------------------------------------------------------------------- refusals

@pytest.mark.parametrize("overrides", [dict(filters=96), dict(filters=200), dict(filters=576), dict(filters=256, in_channels=8, action_values=1),
                                       dict(filters=256, rows=21), dict(filters=256, cols=4)])
def test_unsupported_networks_are_refused(agx_lib, overrides):
    from alphagomoku_amd import AgxError
    from alphagomoku_amd.networks import AGNetwork
    with pytest.raises(AgxError):
        AGNetwork(synthetic.net_desc(**dict(dict(rows=12, cols=12, blocks=1), **overrides)))


def test_wide_bottleneck_and_convnext_networks_are_refused(agx_lib):
    from alphagomoku_amd import AgxError
    from alphagomoku_amd.networks import AGNetwork
    with pytest.raises(AgxError, match="supported: 5..20 rows and cols"):
        AGNetwork(synthetic.bottleneck_desc(15, 15, 2, 256))
    with pytest.raises(AgxError, match="ConvNeXt"):
        AGNetwork(synthetic.convnext_desc(15, 15, 2, 256))
