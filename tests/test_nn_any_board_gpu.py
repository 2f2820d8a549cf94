"""The run-time-shaped network kernel (csrc/nn_any_board.hip) on the GPU: every board from 5x5 to 20x20, rows and cols independent.

  * exact parity with nn_exact.reference (criterion: test_nn_exact_gpu.assert_exact, imported) on the networks of nn_any_board.py, which
    test_nn_any_board_cpu.py proves exact; the same on 15x15 / 20x20 with AGX_NN_ANY_BOARD=1, where the specialised kernels already agree
    with the reference;
  * He-init networks against the fp16-storage oracle, tolerances of test_nn_gpu.py;
  * launch shapes, launch width, the indirect entry points, two streams;
  * the network in the loop of whole games on 12x12 and 19x19, and a pool stepped with the network on the device;
  * what is still refused; a tripwire under the rate relative to the specialised 20x20 kernel.
"""
import ctypes
import functools

import numpy as np
import pytest

import nn_any_board as ab
import nn_exact as nx
import oracle_lib as ol
from alphagomoku_amd import synthetic
from test_nn_exact_gpu import assert_exact, load
from test_nn_gpu import FP16_ORACLE_TOL, relative_logit_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def olib():
    return ol.load()


@functools.lru_cache(maxsize=None)
def reference_of(rows, cols, filters, kind, blocks, heads, batch):
    desc, blob = ab.weights(rows, cols, filters, kind, blocks, heads)
    return nx.reference(desc, blob, ab.feature_batch(rows, cols, batch), stats=False)


# ------------------------------------------------------------------------------------------------------------------------ exact parity

@pytest.mark.parametrize("rows,cols,filters,kind,blocks,heads", ab.gpu_network_cases())
def test_any_board_kernel_is_exact(agx_lib, monkeypatch, rows, cols, filters, kind, blocks, heads):
    """the full cross of filters x kinds x blocks x heads on 12x12, 19x19, 13x17 and 5x20; one network per kind and filter count on every
    other square size 5 .. 19 and on 10x20, 20x10, 17x15; random and directed boards"""
    monkeypatch.delenv("AGX_NN_ANY_BOARD", raising=False)
    desc, blob = ab.weights(rows, cols, filters, kind, blocks, heads)
    net = load(desc, blob)
    try:
        for batch in ab.BATCHES:
            out = net.forward(ab.feature_batch(rows, cols, batch))
            assert_exact(out, desc, blob, reference_of(rows, cols, filters, kind, blocks, heads, batch), "%s %s, %s boards" % (nx.describe(desc), heads, batch))
        if kind == "raw":                                         # the upper 24 bits of every word set: a raw network reads the low byte only
            f = ab.feature_batch(rows, cols, "random")
            assert all(np.array_equal(a, b) for a, b in zip(net.forward(f), net.forward(f | np.uint32(0xFFFFFF00))))
    finally:
        net.close()


@functools.lru_cache(maxsize=None)
def square_reference_of(rows, filters, kind, blocks, heads, batch):
    desc, blob = nx.cached_weights(rows, filters, kind, blocks, heads, ab.SEED)
    return nx.reference(desc, blob, nx.feature_batch(rows, batch, ab.SEED), stats=False)


@pytest.mark.parametrize("rows,cols,filters,kind,blocks,heads", ab.cross(ab.SPECIALISED))
def test_any_board_kernel_is_exact_where_a_second_kernel_is(agx_lib, monkeypatch, rows, cols, filters, kind, blocks, heads):
    """AGX_NN_ANY_BOARD=1: the networks and boards of test_nn_exact_gpu.py (seed 1) on 15x15 and 20x20 through the new kernel"""
    monkeypatch.setenv("AGX_NN_ANY_BOARD", "1")
    desc, blob = nx.cached_weights(rows, filters, kind, blocks, heads, ab.SEED)
    net = load(desc, blob)
    try:
        for batch in ("random", "directed"):
            out = net.forward(nx.feature_batch(rows, batch, ab.SEED))
            assert_exact(out, desc, blob, square_reference_of(rows, filters, kind, blocks, heads, batch), "%s any-board %s, %s boards" % (nx.describe(desc), heads, batch))
    finally:
        net.close()


@pytest.mark.parametrize("rows", [15, 20])
@pytest.mark.parametrize("kind", ["pv", "pvq"])
def test_switch_off_is_the_variable_unset(agx_lib, monkeypatch, rows, kind):
    """AGX_NN_ANY_BOARD=0 and the variable unset give byte-equal outputs on 15x15 and 20x20 (their own kernels); =1 gives the same logits
    through another kernel (exact networks: equal up to the softmax's last bits)"""
    desc, blob = nx.cached_weights(rows, 128, kind, 1, "random", ab.SEED)
    f = nx.feature_batch(rows, "random", ab.SEED)
    outs = {}
    for setting in (None, "0", "1"):
        if setting is None:
            monkeypatch.delenv("AGX_NN_ANY_BOARD", raising=False)
        else:
            monkeypatch.setenv("AGX_NN_ANY_BOARD", setting)
        net = load(desc, blob)
        try:
            outs[setting] = net.forward(f)
        finally:
            net.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs[None], outs["0"]))
    assert all(np.abs(a - b).max() < 1e-5 for a, b in zip(outs[None], outs["1"]))


# ------------------------------------------------------------------------------------------------------------------ He-init networks

@pytest.mark.parametrize("rows,cols,blocks,filters,gain,kind,seed", ab.ORACLE_CASES)
def test_forward_matches_the_fp16_storage_oracle(agx_lib, rows, cols, blocks, filters, gain, kind, seed):
    """dense He-init weights against nn_ref.forward(storage="fp16"): softmax outputs within FP16_ORACLE_TOL, logits within 5e-3 of their
    range, arg-max equal (test_nn_gpu.test_forward_matches_the_fp16_storage_oracle); the action values within the 1e-2 of
    test_action_values_head_matches_oracle.  The boards are those of nn_any_board.ORACLE_CASES: the reference decides their arg-max."""
    from alphagomoku_amd.networks import AGNetwork
    from oracle import nn_ref
    d = ab.make_desc(rows, cols, filters, kind, blocks)
    blob, _ = synthetic.make_weights(d, residual_gain=gain)
    net = AGNetwork(d)
    net.loadWeights(blob)
    try:
        f = synthetic.random_features(8, rows, cols, seed=seed)
        out = net.forward(f)
        ref = nn_ref.forward(d, blob, f, storage="fp16")
        p, v, pr, vr = out[0], out[1], ref[0], ref[1]
        err_p, err_v, err_l = float(np.abs(p - pr).max()), float(np.abs(v - vr).max()), relative_logit_error(p, pr)
        print("fp16-storage oracle %dx%d %dx%d %s gain %.1f: policy %.2e value %.2e logits %.2e" % (rows, cols, blocks, filters, kind, gain, err_p, err_v, err_l))
        assert err_p <= FP16_ORACLE_TOL and err_v <= FP16_ORACLE_TOL
        assert err_l <= 5.0e-3
        assert (p.argmax(1) == pr.argmax(1)).all()
        if kind == "pvq":
            print("action values: %.2e" % float(np.abs(out[2] - ref[2]).max()))
            assert np.abs(out[2] - ref[2]).max() <= 1e-2
            assert (out[2] >= 0).all() and (out[2].sum(2) <= 1.0 + 1e-5).all()
    finally:
        net.close()


# -------------------------------------------------------------------------------------------------------------------- launch shapes

SHAPE_NETWORKS = [(19, 19, 128, "pvq"), (13, 17, 64, "raw"), (13, 17, 128, "pv"), (19, 19, 64, "pv")]
POOL_NETWORK = (1, "random")


def pool_case(rows, cols, filters, kind):
    desc, blob = ab.weights(rows, cols, filters, kind, *POOL_NETWORK)
    return desc, blob, ab.feature_batch(rows, cols, "pool")


@pytest.mark.parametrize("rows,cols,filters,kind", SHAPE_NETWORKS)
def test_batch_shapes_and_launch_width(agx_lib, rows, cols, filters, kind):
    """1, c - 1, c, c + 1, 2 c + 1 boards (c compute units = the persistent grid) and launches narrowed to 1, 3, 64 workgroups: a board's
    outputs are bit-identical wherever it sits and however wide the launch is, and exact"""
    from alphagomoku_amd import check
    desc, blob, pool = pool_case(rows, cols, filters, kind)
    count = ctypes.c_int()
    assert agx_lib.agx_device_cu_count(ctypes.byref(count)) == 0 and count.value > 1
    c = count.value
    assert 2 * c + 1 <= len(pool)
    net = load(desc, blob)
    try:
        full = net.forward(pool)
        assert_exact(full, desc, blob, nx.reference_in_chunks(desc, blob, pool), "%s, %d boards" % (nx.describe(desc), len(pool)))
        for n in (1, c - 1, c, c + 1, 2 * c + 1):
            idx = (np.arange(n) * 7 + n) % len(pool)
            out = net.forward(pool[idx])
            assert all(np.array_equal(a, b[idx]) for a, b in zip(out, full)), n
        for width in (1, 3, 64, 0):
            check(agx_lib.agx_net_set_launch_width(net._net, width))
            out = net.forward(pool[:150])
            assert all(np.array_equal(a, b[:150]) for a, b in zip(out, full)), width
    finally:
        net.close()


SENTINEL = np.uint32(0x7FC0DEAD)                                 # a NaN payload no kernel produces
SLOTS, MAX_BATCH = 64, 48


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("rows,cols,filters,kind", [(19, 19, 128, "pv"), (19, 19, 64, "pvq"), (13, 17, 64, "pv"), (13, 17, 128, "pvq")])
def test_indirect_entry_points(agx_lib, rows, cols, filters, kind, own_stream):
    """agx_nn_forward_indirect / _indirect_pvq with a shuffled slot list and a device-side count below, at and above max_batch: listed slots
    hold bit for bit what the direct entry point gives, every other slot keeps its sentinel"""
    from alphagomoku_amd import check
    from alphagomoku_amd.networks import DeviceBuffer
    desc, blob = ab.weights(rows, cols, filters, kind, *POOL_NETWORK)
    boards = ab.feature_batch(rows, cols, "pool")[:SLOTS]
    hw, with_q = rows * cols, kind == "pvq"
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
        assert_exact(direct, desc, blob, nx.reference(desc, blob, boards, stats=False), "%s, direct entry point" % nx.describe(desc))
        for count in (0, 1, 37, MAX_BATCH, MAX_BATCH + 5):
            slots = np.random.default_rng(count + rows).permutation(SLOTS).astype(np.int32)
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


def test_one_network_on_two_streams(agx_lib):
    """the kernel parks residual inputs in a global scratch: one network launched on two streams at the same time keeps a scratch per stream"""
    from alphagomoku_amd import lib, check
    from alphagomoku_amd.networks import AGNetwork, DeviceBuffer
    rows, cols, boards = 19, 19, 768
    hw = rows * cols
    d = synthetic.net_desc(rows=rows, cols=cols, blocks=4, filters=128)
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
    for _ in range(6):
        for k in range(2):
            net.forwardDevice(feats[k].ptr, boards, pols[k].ptr, vals[k].ptr, stream=streams[k])
    for s in streams:
        check(lib.agx_stream_synchronize(s))
    for k in range(2):
        p = pols[k].download((boards, hw), np.float32)
        v = vals[k].download((boards, 3), np.float32)
        assert np.array_equal(p, expected[k][0]) and np.array_equal(v, expected[k][1])
    for s in streams:
        check(lib.agx_stream_destroy(s))
    for b in feats + pols + vals:
        b.free()
    net.close()


# ----------------------------------------------------------------------------------------------------------------------- in the loop

@pytest.mark.parametrize("rules,n,max_steps,floor", [(0, 12, 250, 300), (1, 19, 250, 300)])
def test_games_bit_exact_with_the_hip_network_in_the_loop(agx_lib, olib, rules, n, max_steps, floor):
    """test_engine_gpu's whole-game comparison with a 2-block / 64-filter network of the board's size as the evaluator of both sides: 4 games
    x 250 steps as there, the same floor of compared roots"""
    from alphagomoku_amd.networks import AGNetwork
    from test_engine_gpu import _play_and_compare
    d = synthetic.net_desc(rows=n, cols=n, blocks=2, filters=64)
    blob, _ = synthetic.make_weights(d)
    net = AGNetwork(d)
    net.loadWeights(blob)

    def evaluator(feats):
        p, v = net.forward(np.ascontiguousarray(feats, dtype=np.uint32))
        return p, np.ascontiguousarray(v[:, :2])
    try:
        compared, stats = _play_and_compare(olib, rules, games=4, batch=4, sims=100, max_steps=max_steps, evaluator=evaluator, n=n)
        assert compared > floor and stats["moves_played"] > 0
    finally:
        net.close()


def test_pool_stepped_with_the_network_on_the_device(agx_lib, olib):
    """GeneratorPool.step on 19x19 — search kernels, network and expansion on the device with no host in between, the path that did not
    exist for this board: every game finishes, and its records (moves, root visits, root edge visits) are those of an oracle tree played
    from the same opening and fed the same network's outputs"""
    from alphagomoku_amd import selfplay
    from alphagomoku_amd.networks import AGNetwork
    n, rules, games, batch, sims = 19, 0, 4, 4, 40
    hw = n * n
    d = synthetic.net_desc(rows=n, cols=n, blocks=2, filters=64)
    blob, _ = synthetic.make_weights(d)
    net = AGNetwork(d)
    net.loadWeights(blob)
    cfg = selfplay.default_config(rules=rules, board_size=n, draw_after=hw, n_games=games, max_batch_size=batch, max_simulations=sims, tss_table_entries=1 << 16,
                                  node_capacity=4096, edge_capacity=131072, record_edge_capacity=games * hw * hw)
    pool = selfplay.GeneratorPool(cfg)
    ocfg = ol.default_search_config(max_batch_size=batch, max_simulations=sims, table_entries=1 << 16)
    openings = []
    for g in range(games):
        op = np.zeros(64, np.uint16)
        k = olib.ago_prepare_opening(rules, n, n, 500 + g, ol.ptr(op))
        openings.append([int(x) for x in op[:k]])
    try:
        pool.begin(selfplay.pack_openings(openings))
        for step in range(40000):
            pool.step(net)
            if step % 50 == 49 and pool.stats()["active_games"] == 0:
                break
        st = pool.stats()
        assert st["first_error"] == 0 and st["games_finished"] == games, st
        recs, edges = pool.records()
        for g in range(games):
            h = olib.ago_game_create(rules, n, n, ctypes.byref(ocfg))
            op = np.array(openings[g] + [0] * (64 - len(openings[g])), np.uint16)
            olib.ago_game_begin(h, ol.ptr(op), len(openings[g]))
            f = np.zeros((batch, hw), np.uint32)
            while olib.ago_game_outcome(h) == 0:
                c = olib.ago_game_step_select(h, ol.ptr(f), batch)
                if c:
                    p, v = net.forward(np.ascontiguousarray(f[:c]))
                else:
                    p, v = np.zeros((0, hw), np.float32), np.zeros((0, 3), np.float32)
                olib.ago_game_step_expand(h, ol.ptr(np.ascontiguousarray(p)), ol.ptr(np.ascontiguousarray(v[:, :2])))
            mine = sorted((r.move_number, r) for r in recs if r.game_serial == g)
            assert len(mine) == olib.ago_game_num_records(h) and len(mine) > 0, g
            for i, (_, r) in enumerate(mine):
                mv, rv, rs = ctypes.c_uint16(), ctypes.c_int(), ctypes.c_uint16()
                rval = (ctypes.c_float * 2)()
                em, ev_ = np.zeros(512, np.uint16), np.zeros(512, np.int32)
                ep, evl, es = np.zeros(512, np.float32), np.zeros(1024, np.float32), np.zeros(512, np.uint16)
                ne = olib.ago_game_record(h, i, ctypes.byref(mv), ctypes.byref(rv), rval, ctypes.byref(rs), ol.ptr(em), ol.ptr(ev_), ol.ptr(ep), ol.ptr(evl), ol.ptr(es), 512)
                assert (r.move, r.root_visits, r.n_edges) == (mv.value, rv.value, ne), (g, i)
                assert [e.visits for e in edges[r.edge_offset:r.edge_offset + r.n_edges]] == [int(x) for x in ev_[:ne]], (g, i)
            olib.ago_game_destroy(h)
    finally:
        pool.close()
        net.close()


# -------------------------------------------------------------------------------------------------------------------------- refusals

@pytest.mark.parametrize("overrides", [dict(rows=4, cols=15), dict(rows=21, cols=15), dict(rows=15, cols=21), dict(rows=12, cols=12, filters=96),
                                       dict(rows=12, cols=12, in_channels=8, action_values=1)])
def test_unsupported_networks_are_refused(agx_lib, overrides):
    from alphagomoku_amd import AgxError
    from alphagomoku_amd.networks import AGNetwork
    with pytest.raises(AgxError):
        AGNetwork(synthetic.net_desc(**dict(dict(blocks=1, filters=64), **overrides)))


# ------------------------------------------------------------------------------------------------------------------------------ rate

def measure_tflops(rows, cols, blocks, filters, boards=4096):
    """the method of test_nn_gpu.test_network_rate_floor: 4096 boards, 3 warm-up and 5 timed launches, FLOPs by its formula with hw = rows * cols"""
    from alphagomoku_amd import lib, check
    from alphagomoku_amd.networks import AGNetwork, DeviceBuffer
    d = synthetic.net_desc(rows=rows, cols=cols, blocks=blocks, filters=filters)
    blob, _ = synthetic.make_weights(d)
    net = AGNetwork(d)
    net.loadWeights(blob)
    hw = rows * cols
    fb = synthetic.random_features(boards, rows, cols, seed=5)
    df = DeviceBuffer(fb.nbytes)
    df.upload(fb)
    dp, dv = DeviceBuffer(boards * hw * 4), DeviceBuffer(boards * 3 * 4)
    t = ctypes.c_void_p()
    check(lib.agx_timer_create(ctypes.byref(t)))
    for _ in range(3):
        net.forwardDevice(df.ptr, boards, dp.ptr, dv.ptr)
    check(lib.agx_device_synchronize())
    check(lib.agx_timer_start(t, None))
    launches = 5
    for _ in range(launches):
        net.forwardDevice(df.ptr, boards, dp.ptr, dv.ptr)
    check(lib.agx_timer_stop(t, None))
    ms = ctypes.c_float()
    check(lib.agx_timer_elapsed_ms(t, ctypes.byref(ms)))
    check(lib.agx_timer_destroy(t))
    for b in (df, dp, dv):
        b.free()
    net.close()
    f, dense = filters, d["value_hidden"]
    flops = 2 * hw * (25 * 32 * f + blocks * 2 * 9 * f * f + 9 * f * f + f + 4 * f) + 2 * 4 * hw * dense + 6 * dense
    return boards * flops / (ms.value / launches * 1e-3) / 1e12


def test_rate_tripwire_against_the_specialised_kernel(agx_lib, monkeypatch):
    """Not a target, a tripwire (a mapping accident costs far more than a factor of two): on 20x20 10x128 the general kernel reaches at
    least half the TFLOP/s of the specialised kernel, measured in the same process.  Measured on MI355X: see profiles/any_board_rate.txt."""
    monkeypatch.setenv("AGX_NN_ANY_BOARD", "0")
    special = measure_tflops(20, 20, 10, 128)
    monkeypatch.setenv("AGX_NN_ANY_BOARD", "1")
    general = measure_tflops(20, 20, 10, 128)
    print("20x20 10x128: specialised %.0f TFLOP/s, any-board %.0f TFLOP/s, ratio %.3f" % (special, general, general / special))
    assert general >= 0.5 * special, "any-board kernel %.0f TFLOP/s against %.0f" % (general, special)
