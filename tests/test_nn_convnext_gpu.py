"""The ConvNeXt towers (csrc/nn_convnext.hip: ConvNextPVQraw / ConvNextPVQMraw) on the GPU.

  * exact parity with the float64 reference of nn_convnext_ref.py on networks that round nowhere before the softmax
    (test_nn_convnext_cpu.py proves it for every case here): live squeeze-and-excitation gates on boards whose cell count is a power of
    two, all four heads; constant gates on 5x5, 6x20, 15x15, 20x20 and 7x19, policy and q.  Logit differences are recovered from the softmax
    outputs (nn_exact.logit_deviation) and must stay within a quarter of the finest head grid in use: a wrong or missing term moves a logit
    by at least one grid step, the softmax's own error is one __expf and one division.
  * the entry points: slot list, narrowed launch, batch sizes, NULL heads, refusals, and a Resnet network through the dispatching calls.
  * He-init networks against the storage-rounding restatement, bound derived on the CPU (nn_convnext_ref.tolerance).
  * the network in a pool, under a position evaluator, and from / under the trainer.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import nn_convnext_ref as cr
import nn_exact as nx
from alphagomoku_amd import synthetic

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7FC0DEAD)                                 # a NaN payload no kernel produces


@pytest.fixture(scope="module")
def olib():
    import oracle_lib as ol
    return ol.load()


def load(desc, blob):
    from alphagomoku_amd.networks import AGNetwork
    net = AGNetwork(desc)
    net.loadWeights(blob)
    return net


def grid_of(desc, blob, name):
    """the spacing of a head's logits: the product of the grids of its layers behind the last integer activation"""
    w = cr.split(desc, blob)
    if name in ("policy", "q"):
        return min(cr.lowest_bit(w[name + ".w2"]), cr.lowest_bit(w[name + ".b2"]))
    hw = desc["rows"] * desc["cols"]                             # pooled heads: integers / HW, then two dense layers on a grid of 1 / 8
    return 2.0 ** -desc["blocks"] / hw / 8.0 / 8.0


def assert_exact(outputs, desc, blob, ref, heads, label):
    report = []
    for name, out, logits in zip(("policy", "value", "q", "m"), outputs, (ref.policy, ref.value, ref.q, ref.m)):
        assert np.isfinite(out).all() and (out >= 0).all(), (label, name)
        if name not in heads:
            continue
        g = grid_of(desc, blob, name)
        dev = nx.logit_deviation(out, logits)
        report.append("%s %.2e (g/%.0f)" % (name, dev.max(), g / max(dev.max(), 1e-30)))
        assert (dev <= g / 4).all(), "%s %s: logit deviation %.3e on board %d, grid %.3e" % (label, name, dev.max(), int(dev.argmax()), g)
    assert np.abs(outputs[0].sum(1) - 1.0).max() < 1e-5 and np.abs(outputs[1].sum(1) - 1.0).max() < 1e-5, label
    if len(outputs) > 3:
        assert np.abs(outputs[3].sum(1) - 1.0).max() < 1e-5, label
    print("exact %s: %s" % (label, ", ".join(report)))


@pytest.mark.parametrize("rows,cols,filters,blocks,moves_left", cr.live_cases())
def test_live_gates_are_exact(agx_lib, rows, cols, filters, blocks, moves_left):
    """policy, q, value and m logits EQUAL the float64 reference at every cell and class"""
    desc, blob = cr.cached_weights(rows, cols, filters, blocks, moves_left, "live")
    net = load(desc, blob)
    try:
        out = net.forward(cr.feature_batch(rows, cols, "mixed"))
        assert len(out) == 3 + moves_left
        assert_exact(out, desc, blob, cr.cached_reference(rows, cols, filters, blocks, moves_left, "live"),
                     ("policy", "value", "q", "m")[:3 + moves_left], cr.describe(desc) + " live gates")
    finally:
        net.close()


@pytest.mark.parametrize("rows,cols,filters,blocks,moves_left", cr.constant_cases())
def test_constant_gates_are_exact(agx_lib, rows, cols, filters, blocks, moves_left):
    """every board shape class: smaller than the 7x7 window, one side at the maximum, the two common sizes, odd x odd; a stone in every
    corner and on every border column among the inputs.  Policy and q logits equal the reference at every cell."""
    desc, blob = cr.cached_weights(rows, cols, filters, blocks, moves_left, "constant")
    net = load(desc, blob)
    try:
        out = net.forward(cr.feature_batch(rows, cols, "mixed"))
        assert_exact(out, desc, blob, cr.cached_reference(rows, cols, filters, blocks, moves_left, "constant"), ("policy", "q"),
                     cr.describe(desc) + " constant gates")
    finally:
        net.close()


# ------------------------------------------------------------------------------------------------------------------------ entry points

def device_buffers(hw, slots, with_m):
    from alphagomoku_amd.networks import DeviceBuffer
    sizes = [slots * hw, slots * 3, slots * hw * 2] + ([slots * hw] if with_m else [])
    bufs = [DeviceBuffer(n * 4) for n in sizes]
    for b, n in zip(bufs, sizes):
        b.upload(np.full(n, SENTINEL, np.uint32))
    return bufs, [(slots, hw), (slots, 3), (slots, hw, 2), (slots, hw)][:len(sizes)]


@pytest.mark.parametrize("filters,moves_left", [(64, 1), (128, 0), (128, 1)])
def test_slot_list_launch_width_and_batch_sizes(agx_lib, filters, moves_left):
    """the indirect (slot-list) call equals the direct call bit for bit, listed slots only; a launch narrowed to 3 workgroups equals the
    full-width launch bit for bit; batches of 1, 2 and 3 x 2 + 1 boards; a board's bits do not depend on where it sits"""
    from alphagomoku_amd import check
    from alphagomoku_amd.networks import DeviceBuffer
    rows, cols = 8, 16
    desc, blob = cr.cached_weights(rows, cols, filters, 1, moves_left, "live")
    hw = rows * cols
    f = np.concatenate([cr.feature_batch(rows, cols, "mixed"), synthetic.random_features(8, rows, cols, seed=9)])
    net = load(desc, blob)
    try:
        base = net.forward(f)
        assert_exact(base, desc, blob, cr.reference(desc, blob, f), ("policy", "value", "q", "m")[:3 + moves_left], "entry points")
        check(agx_lib.agx_net_set_launch_width(net._net, 3))
        for n in (1, 2, 7, len(f)):
            out = net.forward(f[:n])
            assert all(np.array_equal(a, b[:n]) for a, b in zip(out, base)), n
        idx = (np.arange(7) * 5 + 3) % len(f)
        assert all(np.array_equal(a, b[idx]) for a, b in zip(net.forward(f[idx]), base))
        for width in (3, 0):
            check(agx_lib.agx_net_set_launch_width(net._net, width))
            slots, max_batch = len(f) + 5, len(f)
            order = np.random.default_rng(3).permutation(slots)[:max_batch].astype(np.int32)
            slot_features = np.zeros((slots, hw), np.uint32)
            slot_features[order] = f
            d_f, d_list, d_count = DeviceBuffer(slot_features.nbytes), DeviceBuffer(order.nbytes), DeviceBuffer(4)
            d_f.upload(slot_features)
            d_list.upload(order)
            for count in (1, 7, max_batch, max_batch + 9):           # (a count above max_batch is capped)
                d_count.upload(np.array([count], np.int32))
                bufs, shapes = device_buffers(hw, slots, moves_left)
                if moves_left:
                    check(agx_lib.agx_nn_forward_indirect_pvqm(net._net, d_f.ptr, d_list.ptr, d_count.ptr, max_batch, *[b.ptr for b in bufs], None))
                else:
                    check(agx_lib.agx_nn_forward_indirect_pvq(net._net, d_f.ptr, d_list.ptr, d_count.ptr, max_batch, *[b.ptr for b in bufs], None))
                check(agx_lib.agx_device_synchronize())
                used = order[:min(count, max_batch)]
                for b, shape, want in zip(bufs, shapes, base):
                    got = b.download(shape, np.float32)
                    assert np.array_equal(got[used], want[:len(used)]), (width, count)
                    untouched = np.setdiff1d(np.arange(slots), used)
                    assert (got[untouched].view(np.uint32) == SENTINEL).all(), (width, count)
                    b.free()
            for b in (d_f, d_list, d_count):
                b.free()
    finally:
        net.close()


def test_null_heads_and_refusals(agx_lib):
    from alphagomoku_amd import check
    from alphagomoku_amd.networks import DeviceBuffer
    rows, cols = 8, 8
    hw = rows * cols
    f = cr.feature_batch(rows, cols, "random")
    d_f = DeviceBuffer(f.nbytes)
    d_f.upload(f)
    for moves_left in (1, 0):
        desc, blob = cr.cached_weights(rows, cols, 64, 1, moves_left, "live")
        net = load(desc, blob)
        arch, ml = ctypes.c_int(-1), ctypes.c_int(-1)
        check(agx_lib.agx_net_architecture(net._net, ctypes.byref(arch), ctypes.byref(ml)))
        assert (arch.value, ml.value) == (1, moves_left)
        full = net.forward(f)
        bufs, shapes = device_buffers(hw, len(f), True)
        if moves_left:
            # d_moves_left = NULL, then d_action_values = NULL as well: the other outputs keep their bits, the skipped buffers stay untouched
            check(agx_lib.agx_nn_forward_pvqm(net._net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, None))
            check(agx_lib.agx_device_synchronize())
            assert all(np.array_equal(bufs[i].download(shapes[i], np.float32), full[i]) for i in range(3))
            assert (bufs[3].download(shapes[3], np.uint32) == SENTINEL).all()
            bufs[2].upload(np.full(len(f) * hw * 2, SENTINEL, np.uint32))
            check(agx_lib.agx_nn_forward(net._net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, None))
            check(agx_lib.agx_device_synchronize())
            assert all(np.array_equal(bufs[i].download(shapes[i], np.float32), full[i]) for i in range(2))
            assert (bufs[2].download(shapes[2], np.uint32) == SENTINEL).all()
        else:
            # a moves-left buffer on a network without the head is refused and nothing is launched
            assert agx_lib.agx_nn_forward_pvqm(net._net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, None) == 1    # AGX_ERR_INVALID
            assert b"moves-left" in agx_lib.agx_last_error()
            check(agx_lib.agx_device_synchronize())
            assert all((b.download(s, np.uint32) == SENTINEL).all() for b, s in zip(bufs, shapes))
            check(agx_lib.agx_nn_forward_pvqm(net._net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, None))      # NULL is fine
            check(agx_lib.agx_device_synchronize())
            assert all(np.array_equal(bufs[i].download(shapes[i], np.float32), full[i]) for i in range(3))
        for b in bufs:
            b.free()
        net.close()
    d_f.free()


def test_resnet_network_keeps_its_bits_through_the_dispatching_calls(agx_lib):
    """a Resnet AgxNet made by agx_net_create_ex(..., AGX_ARCH_RESNET, 0) through agx_nn_forward_pvq / _pvqm(NULL) gives the bits of
    agx_net_create + agx_nn_forward (policy, value) and agx_nn_forward_pvq (q) as used before"""
    from alphagomoku_amd import check
    from alphagomoku_amd._lib import AgxNetDesc
    from alphagomoku_amd.networks import DeviceBuffer
    d = synthetic.net_desc(rows=15, cols=15, blocks=2, filters=64, action_values=1)
    blob, _ = synthetic.make_weights(d, seed=5)
    f = synthetic.random_features(9, 15, 15, seed=4)
    hw = 225
    cdesc = AgxNetDesc(d["rows"], d["cols"], d["blocks"], d["filters"], d["in_channels"], d["value_hidden"], 1)
    old, new = ctypes.c_void_p(), ctypes.c_void_p()
    check(agx_lib.agx_net_create(ctypes.byref(cdesc), ctypes.byref(old)))
    check(agx_lib.agx_net_create_ex(ctypes.byref(cdesc), 0, 0, ctypes.byref(new)))
    d_f = DeviceBuffer(f.nbytes)
    d_f.upload(f)
    results = []
    for net, call in ((old, "old"), (new, "pvq"), (new, "pvqm")):
        check(agx_lib.agx_net_load_weights(net, blob.ctypes.data_as(ctypes.c_void_p), blob.size))
        bufs, shapes = device_buffers(hw, len(f), True)
        if call == "old":
            check(agx_lib.agx_nn_forward_pvq(net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None))
            pv, _ = device_buffers(hw, len(f), False)
            check(agx_lib.agx_nn_forward(net, d_f.ptr, len(f), pv[0].ptr, pv[1].ptr, None))
            check(agx_lib.agx_device_synchronize())
            assert all(np.array_equal(pv[i].download(shapes[i], np.uint32), bufs[i].download(shapes[i], np.uint32)) for i in range(2))
            for b in pv:
                b.free()
        elif call == "pvq":
            check(agx_lib.agx_nn_forward_pvq(net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None))
        else:
            check(agx_lib.agx_nn_forward_pvqm(net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, None))
            assert agx_lib.agx_nn_forward_pvqm(net, d_f.ptr, len(f), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, None) == 1
        check(agx_lib.agx_device_synchronize())
        results.append([b.download(s, np.uint32) for b, s in zip(bufs[:3], shapes[:3])])
        for b in bufs:
            b.free()
    assert all(np.array_equal(a, b) for a, b in zip(results[0], results[1])) and all(np.array_equal(a, b) for a, b in zip(results[0], results[2]))
    assert not (results[0][0] == SENTINEL).any()
    arch, ml = ctypes.c_int(-1), ctypes.c_int(-1)
    check(agx_lib.agx_net_architecture(new, ctypes.byref(arch), ctypes.byref(ml)))
    assert (arch.value, ml.value) == (0, 0)
    d_f.free()
    agx_lib.agx_net_destroy(old)
    agx_lib.agx_net_destroy(new)


# --------------------------------------------------------------------------------------------------------------------------- tolerance

@pytest.mark.parametrize("rows,cols,blocks,filters", [(15, 15, 6, 128), (20, 20, 6, 128), (9, 9, 2, 64)])
def test_he_init_network_within_the_derived_tolerance(agx_lib, rows, cols, blocks, filters):
    """ConvNextPVQMraw with make_convnext_weights against the storage-rounding restatement (fp16 where the kernel stores, fp32 sums).  The
    bound per output is nn_convnext_ref.tolerance: 1e-3, or 4 x the restatement's forwards / backwards gap where that is larger - measured
    on the CPU before the device's outputs are looked at.
    Measured on MI355X (gap -> bound, device deviation) are recorded in DESIGN 3.13."""
    desc = synthetic.convnext_desc(rows, cols, blocks, filters, 1)
    blob, _ = synthetic.make_convnext_weights(desc)
    f = synthetic.random_features(4, rows, cols, seed=7)
    forwards = cr.restatement(desc, blob, f)
    bounds, gaps = cr.tolerance(desc, blob, f, forwards)
    net = load(desc, blob)
    try:
        out = net.forward(f)
    finally:
        net.close()
    deviations = [float(np.abs(o - w).max()) for o, w in zip(out, forwards)]
    for name, dev, bound, gap in zip(("policy", "value", "q", "m"), deviations, bounds, gaps):
        print("tolerance %dx%d %dx%d %s: device deviation %.3e, bound %.3e (CPU gap %.3e)" % (rows, cols, blocks, filters, name, dev, bound, gap))
    for name, o, dev, bound in zip(("policy", "value", "q", "m"), out, deviations, bounds):
        assert np.isfinite(o).all() and dev <= bound, (name, dev, bound)
    assert (out[0].argmax(1) == forwards[0].argmax(1)).all()


# --------------------------------------------------------------------------------------------------------------------- above the tower

def test_games_bit_exact_with_the_convnext_network_in_the_loop(agx_lib, olib):
    """the pattern of test_engine_gpu.test_games_bit_exact_with_the_raw_network_in_the_loop with a 2 x 64 ConvNextPVQraw network: freestyle
    15x15, 4 games; the oracle tree is fed the device network's outputs (policy, value, q), root edges are compared bit for bit after every
    step"""
    from test_engine_gpu import _play_and_compare
    d = synthetic.convnext_desc(15, 15, 2, 64, 0)
    blob, _ = synthetic.make_convnext_weights(d)
    net = load(d, blob)

    def evaluator(feats):
        p, v, q = net.forward(np.ascontiguousarray(feats, dtype=np.uint32))
        return p, np.ascontiguousarray(v[:, :2]), q
    try:
        compared, stats = _play_and_compare(olib, 0, games=4, batch=4, sims=100, max_steps=250, evaluator=evaluator, action_values=1,
                                            speculative_solver=1, speculative_waves=48)
        assert compared > 300 and stats["moves_played"] > 0
    finally:
        net.close()


def test_pool_steps_with_the_network_on_the_device(agx_lib):
    """GeneratorPool.step(net) (the pool's network stage on the device) == the network's outputs written by hand into the slot buffers"""
    from alphagomoku_amd import selfplay
    d = synthetic.convnext_desc(15, 15, 2, 64, 1)
    blob, _ = synthetic.make_convnext_weights(d)
    net = load(d, blob)
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
                p, v, q, _ = net.forward(feats)
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


def test_evaluate_positions_with_a_convnext_network(agx_lib):
    """evaluate_positions == tests/position_eval_ref.py applied to the tower's own outputs, bit for bit"""
    import oracle_lib as ol
    import position_eval_ref as ref
    from test_position_eval_gpu import Evaluator, combine_positions, check_against_restatement, tower_rows
    n = 15
    d = synthetic.convnext_desc(n, n, 1, 64, 1)
    blob, _ = synthetic.make_convnext_weights(d, seed=8)
    net = load(d, blob)
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


def test_module_export_and_trainer_steps(agx_lib, olib, tmp_path):
    """in a process of its own (tests/nn_convnext_torch_main.py): ConvNextModule -> load_module -> tower against module.eval() within the
    derived tolerance; three Trainer.steps with the moves-left loss"""
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
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nn_convnext_torch_main.py")
    run = subprocess.run([sys.executable, script, str(path), str(listing)], capture_output=True, text=True, timeout=300)
    print(run.stdout[-4000:])
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout[-3000:] + run.stderr[-3000:]


def test_reference_named_classes_from_a_compiled_program(agx_lib, tmp_path):
    """tests/cpp/convnext_main.cpp: ag::AGNetwork(..., "ConvNextPVQMraw"), a ConvNeXt weight container read back, one batch forwarded; the
    program prints its outputs' checksums, which must be the Python wrapper's"""
    from alphagomoku_amd import build
    d = synthetic.convnext_desc(15, 15, 1, 64, 1)
    blob, _ = synthetic.make_convnext_weights(d, seed=6)
    path = tmp_path / "convnext.agxw"
    synthetic.save_weights(path, d, blob)
    f = synthetic.random_features(3, 15, 15, seed=2)
    fpath = tmp_path / "features.bin"
    f.tofile(fpath)
    run = subprocess.run([build.CONVNEXT_TEST, str(path), str(fpath), "3"], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().splitlines()[-1] == "ok"
    lines = dict(line.split(" ", 1) for line in run.stdout.strip().splitlines() if " " in line)
    assert lines["name"] == "ConvNextPVQMraw" and lines["outputs"] == "pvqm"
    net = load(d, blob)
    try:
        p, v, q, m = net.forward(f)
    finally:
        net.close()
    from alphagomoku_amd.networks import moves_left_mean
    want = ["%.9g" % float(np.float32(x)) for x in (p[2].max(), v[2, 0], q[2, 7, 0], moves_left_mean(m[2]))]
    assert lines["values"].split() == want
