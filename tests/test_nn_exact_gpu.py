"""Exact-arithmetic parity of the HIP network kernels (nn_tower_kernel, value_head_kernel) against the float64 reference of nn_exact.py.

The networks evaluated here round nowhere before the softmax (nn_exact.py says why; test_nn_exact_cpu.py proves it for every case of
this file), so the device's logits must EQUAL the reference's at every cell of every board.  The comparison recovers logit differences
from the softmax outputs (nn_exact.logit_deviation) and allows a quarter of the head's grid spacing g: a wrong or missing term moves a
logit by at least g, the softmax's own error is one __expf on an argument in [-16, 0] and one division.  g / 4 is derived, not measured
(g = 2^-6 for random heads; 2^-7 policy / 2^-8 value for transparent heads).

Measured on MI355X, largest deviation over the 253 cases of this file: 3.9e-5 g policy, 1.1e-4 g value, 2.6e-5 g q (1.6e-7, 4.2e-7
and 3.9e-7 absolute: the softmax's own error, as expected; g / 4 is 2 400 times the worst of them, g / 64 still 150 times).  No case
had to be left out and no kernel bug turned up.  Wall time of the file on the GPU machine: 17 s.
"""
import ctypes
import functools

import numpy as np
import pytest

import nn_exact as nx

pytestmark = pytest.mark.gpu

WORST = {"policy": 0.0, "value": 0.0, "q": 0.0}               # in units of the head's grid spacing, over the whole module


@functools.lru_cache(maxsize=None)
def reference_of(rows, filters, kind, blocks, heads, seed, batch):
    desc, blob = nx.cached_weights(rows, filters, kind, blocks, heads, seed)
    return nx.reference(desc, blob, nx.feature_batch(rows, batch, seed), stats=False)


def assert_exact(outputs, desc, blob, ref, label=""):
    """device outputs (policy, value[, q]) against reference logits: every board within g / 4 in logit differences, arg-max equal
    wherever the reference's top two logits differ"""
    g = nx.head_grids(desc, blob)
    report = []
    for name, out, logits in zip(("policy", "value", "q"), outputs, (ref.policy, ref.value, ref.q)):
        assert np.isfinite(out).all() and (out >= 0).all(), (label, name)
        dev = nx.logit_deviation(out, logits)
        report.append("%s %.2e (g/%.0f)" % (name, dev.max(), g[name] / max(dev.max(), 1e-30)))
        WORST[name] = max(WORST[name], float(dev.max()) / g[name])
        assert (dev <= g[name] / 4).all(), "%s %s: logit deviation %.3e on board %d, grid %.3e" % (label, name, dev.max(), int(dev.argmax()), g[name])
        if name != "q":
            top2 = np.sort(logits, axis=1)[:, -2:]
            decided = top2[:, 1] > top2[:, 0]
            assert (out.argmax(1) == logits.argmax(1))[decided].all(), (label, name)
    assert np.abs(outputs[0].sum(1) - 1.0).max() < 1e-5 and np.abs(outputs[1].sum(1) - 1.0).max() < 1e-5, label
    print("exact %s: %s" % (label, ", ".join(report)))


def load(desc, blob):
    from alphagomoku_amd.networks import AGNetwork
    net = AGNetwork(desc)
    net.loadWeights(blob)
    return net


def test_parametrisation_covers_the_dispatch_table(agx_lib):
    cases = {(filters, rows, rows == 20 or single == "1", kind == "pvq", kind == "raw") for rows, single, filters, kind, _, _, _ in nx.network_cases()}
    assert cases == set(nx.dispatch_table()) and len(cases) == 18
    for inst in cases:
        assert {b for r, s, f, k, b, _, _ in nx.network_cases() if (f, r, r == 20 or s == "1", k == "pvq", k == "raw") == inst} == {0, 1, 10}


@pytest.mark.parametrize("rows,single,filters,kind,blocks,heads,seed", nx.network_cases())
def test_tower_instantiation_is_exact(agx_lib, monkeypatch, rows, single, filters, kind, blocks, heads, seed):
    """all 18 instantiations of nn_tower_kernel (and so the two value_head_kernels), at 0 blocks (input conv and heads alone), 1 block
    (first = last) and 10 blocks, random and transparent heads, random and directed boards"""
    monkeypatch.setenv("AGX_NN_SINGLE_PLANE", single)
    desc, blob = nx.cached_weights(rows, filters, kind, blocks, heads, seed)
    net = load(desc, blob)
    try:
        first = None
        for batch in nx.batches_of(kind, seed):
            out = net.forward(nx.feature_batch(rows, batch, seed))
            assert_exact(out, desc, blob, reference_of(rows, filters, kind, blocks, heads, seed, batch),
                         "%s single=%s %s seed %d, %s boards" % (nx.describe(desc), single, heads, seed, batch))
            if batch == "random":
                first = out
            if batch == "high bits":                             # the same boards with the upper 24 bits of every word set
                assert all(np.array_equal(a, b) for a, b in zip(first, out))
    finally:
        net.close()


SHAPE_NETWORKS = [(15, "0", 128, "pv"), (15, "1", 64, "pvq"), (20, "0", 128, "pvq"), (20, "0", 64, "raw")]


def pool_case(rows, filters, kind):
    desc, blob = nx.cached_weights(rows, filters, kind, *nx.POOL_NETWORK)
    return desc, blob, nx.feature_batch(rows, "pool", nx.POOL_NETWORK[2])


@pytest.mark.parametrize("rows,single,filters,kind", SHAPE_NETWORKS)
def test_batch_shapes_around_the_persistent_grid(agx_lib, monkeypatch, rows, single, filters, kind):
    """1, c - 1, c, c + 1, 2 c + 1 boards (c compute units = the persistent grid), and 5 boards between a 700-board and a 900-board launch
    on the same network (the value head's scratch grows and is zeroed again): a board's outputs are bit-identical wherever it sits, and exact"""
    monkeypatch.setenv("AGX_NN_SINGLE_PLANE", single)
    desc, blob, pool = pool_case(rows, filters, kind)
    count = ctypes.c_int()
    assert agx_lib.agx_device_cu_count(ctypes.byref(count)) == 0 and count.value > 1
    c = count.value
    net = load(desc, blob)
    try:
        ref = nx.reference_in_chunks(desc, blob, pool)
        a700 = net.forward(pool[:700])
        a5 = net.forward(pool[700:705])
        full = net.forward(pool)
        assert_exact(full, desc, blob, ref, "%s single=%s, 900 boards" % (nx.describe(desc), single))
        assert all(np.array_equal(a, b[:700]) for a, b in zip(a700, full))
        assert all(np.array_equal(a, b[700:705]) for a, b in zip(a5, full))
        for n in (1, c - 1, c, c + 1, 2 * c + 1):
            idx = (np.arange(n) * 7 + n) % len(pool)
            out = net.forward(pool[idx])
            assert all(np.array_equal(a, b[idx]) for a, b in zip(out, full)), n
    finally:
        net.close()


@pytest.mark.parametrize("rows,single,filters,kind", SHAPE_NETWORKS)
def test_launch_width_does_not_change_results(agx_lib, monkeypatch, rows, single, filters, kind):
    monkeypatch.setenv("AGX_NN_SINGLE_PLANE", single)
    desc, blob, pool = pool_case(rows, filters, kind)
    from alphagomoku_amd import check
    net = load(desc, blob)
    try:
        f = pool[:300]
        base = net.forward(f)
        assert_exact(base, desc, blob, nx.reference_in_chunks(desc, blob, f), "%s single=%s, full width" % (nx.describe(desc), single))
        for width in (1, 3, 64, 0):
            check(agx_lib.agx_net_set_launch_width(net._net, width))
            out = net.forward(f)
            assert all(np.array_equal(a, b) for a, b in zip(out, base)), width
    finally:
        net.close()


SENTINEL = np.uint32(0x7FC0DEAD)                                 # a NaN payload no kernel produces
SLOTS, MAX_BATCH = 64, 48


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("kind", ["pv", "pvq"])
@pytest.mark.parametrize("filters", nx.FILTERS)
@pytest.mark.parametrize("rows,single", nx.GEOMETRIES)
def test_indirect_entry_points(agx_lib, monkeypatch, rows, single, filters, kind, own_stream):
    """agx_nn_forward_indirect / _indirect_pvq (slot list and batch size read on the device: the path of every pool step): listed slots
    hold bit for bit what the direct entry point gives for the same boards, which is exact; every other slot keeps the sentinel the
    buffers were filled with; a device count above max_batch is clamped; count 0 writes nothing"""
    from alphagomoku_amd import check
    from alphagomoku_amd.networks import DeviceBuffer
    monkeypatch.setenv("AGX_NN_SINGLE_PLANE", single)
    desc, blob = nx.cached_weights(rows, filters, kind, *nx.POOL_NETWORK)
    boards = nx.feature_batch(rows, "pool", nx.POOL_NETWORK[2])[:SLOTS]
    hw, with_q = rows * rows, kind == "pvq"
    net = load(desc, blob)
    stream = ctypes.c_void_p()
    if own_stream:
        check(agx_lib.agx_stream_create(ctypes.byref(stream)))
    shapes = [(SLOTS, hw), (SLOTS, 3)] + ([(SLOTS, hw, 2)] if with_q else [])
    bufs = [DeviceBuffer(int(np.prod(s)) * 4) for s in shapes]
    d_f, d_list, d_count = DeviceBuffer(boards.nbytes), DeviceBuffer(SLOTS * 4), DeviceBuffer(4)
    try:
        d_f.upload(boards)
        direct = net.forward(boards)
        assert_exact(direct, desc, blob, nx.reference(desc, blob, boards, stats=False), "%s single=%s, direct entry point" % (nx.describe(desc), single))
        for count in (0, 1, 37, MAX_BATCH, MAX_BATCH + 5):
            slots = np.random.default_rng(count + rows).permutation(SLOTS).astype(np.int32)   # every entry a valid slot, also beyond the count
            d_list.upload(slots)
            d_count.upload(np.array([count], np.int32))
            for b, s in zip(bufs, shapes):
                b.upload(np.full(s, SENTINEL, np.uint32))
            if with_q:
                check(agx_lib.agx_nn_forward_indirect_pvq(net._net, d_f.ptr, d_list.ptr, d_count.ptr, MAX_BATCH, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, stream))
            else:
                check(agx_lib.agx_nn_forward_indirect(net._net, d_f.ptr, d_list.ptr, d_count.ptr, MAX_BATCH, bufs[0].ptr, bufs[1].ptr, stream))
            check(agx_lib.agx_stream_synchronize(stream) if own_stream else agx_lib.agx_device_synchronize())
            listed = slots[:min(count, MAX_BATCH)]
            others = np.setdiff1d(np.arange(SLOTS), listed)
            for b, s, want in zip(bufs, shapes, direct):
                got = b.download(s, np.uint32)
                assert np.array_equal(got[listed], want.view(np.uint32)[listed]), count
                assert (got[others] == SENTINEL).all(), count
    finally:
        for b in bufs + [d_f, d_list, d_count]:
            b.free()
        net.close()
        if own_stream:
            check(agx_lib.agx_stream_destroy(stream))


@pytest.mark.parametrize("rows,single", nx.GEOMETRIES)
def test_pvq_network_without_the_q_buffer_is_the_pv_network(agx_lib, monkeypatch, rows, single):
    from alphagomoku_amd import AgxError
    from alphagomoku_amd.networks import DeviceBuffer
    monkeypatch.setenv("AGX_NN_SINGLE_PLANE", single)
    desc, blob = nx.cached_weights(rows, 64, "pvq", *nx.POOL_NETWORK)
    f = nx.feature_batch(rows, "random", 1)
    hw = rows * rows
    net = load(desc, blob)
    net0 = load(dict(desc, action_values=0), blob[:int(sum(np.prod(s) for s in nx.part_shapes(dict(desc, action_values=0))))])
    bufs = [DeviceBuffer(f.nbytes), DeviceBuffer(len(f) * hw * 4), DeviceBuffer(len(f) * 3 * 4), DeviceBuffer(len(f) * hw * 2 * 4)]
    try:
        full = net.forward(f)
        pv = net0.forward(f)
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


def test_zz_report_the_largest_deviation():
    """last in the file: the largest logit deviation seen by assert_exact in this run, in units of the head's grid spacing"""
    print("largest logit deviation / grid spacing: policy %.3e, value %.3e, q %.3e" % (WORST["policy"], WORST["value"], WORST["q"]))
    assert all(w <= 0.25 for w in WORST.values())
