"""CPU side of the ConvNeXt network tests: the blob layout and the refusals of the C ABI, the float64 reference against the torch module,
the export / import bridge, moves_left_mean, and the proof that every network test_nn_convnext_gpu.py compares exactly is exact."""
import ctypes

import numpy as np
import pytest

import nn_convnext_ref as cr
from alphagomoku_amd import synthetic
from alphagomoku_amd._lib import AgxNetDesc, ARCH_CONVNEXT, ARCH_RESNET


def cdesc(d):
    return AgxNetDesc(d["rows"], d["cols"], d["blocks"], d["filters"], d["in_channels"], d["value_hidden"], d.get("action_values", 0))


@pytest.mark.parametrize("rows,cols", [(5, 5), (15, 15), (7, 19)])
@pytest.mark.parametrize("filters", [64, 128])
@pytest.mark.parametrize("blocks", [0, 1, 6])
@pytest.mark.parametrize("moves_left", [0, 1])
def test_blob_floats_is_the_layouts_count(agx_lib, rows, cols, filters, blocks, moves_left):
    d = synthetic.convnext_desc(rows, cols, blocks, filters, moves_left)
    F, HW = filters, rows * cols
    by_hand = 200 * F + F + blocks * (49 * F + F + 4 * (F * F + F)) + (F * F + F + F + 1) + (F * F + F + F * 256 + 256 + 256 * 3 + 3) + (F * F + F + F * 3 + 3)
    by_hand += moves_left * (F * 32 + 32 + 32 * 128 + 128 + 128 * HW + HW)
    assert agx_lib.agx_net_blob_floats_ex(ctypes.byref(cdesc(d)), ARCH_CONVNEXT, moves_left) == by_hand == cr.blob_floats(d)
    assert len(synthetic.make_convnext_weights(d)[0]) == by_hand


def test_resnet_through_the_extended_entry_points(agx_lib):
    d = synthetic.net_desc(blocks=2, filters=64, action_values=1)
    assert agx_lib.agx_net_blob_floats_ex(ctypes.byref(cdesc(d)), ARCH_RESNET, 0) == agx_lib.agx_net_blob_floats(ctypes.byref(cdesc(d)))
    assert agx_lib.agx_net_blob_floats_ex(ctypes.byref(cdesc(d)), ARCH_RESNET, 1) == 0      # no residual network has the head


@pytest.mark.parametrize("change", [dict(in_channels=32), dict(action_values=0), dict(filters=96), dict(value_hidden=128), dict(rows=4), dict(cols=21)])
def test_refusals(agx_lib, change):
    d = dict(synthetic.convnext_desc(15, 15, 2, 64, 1), **change)
    net = ctypes.c_void_p()
    assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(d)), ARCH_CONVNEXT, 1, ctypes.byref(net)) == 3      # AGX_ERR_UNSUPPORTED
    assert b"ConvNeXt" in agx_lib.agx_last_error() and not net
    assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(synthetic.net_desc())), ARCH_RESNET, 1, ctypes.byref(net)) == 3
    assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(d)), 7, 0, ctypes.byref(net)) == 3


@pytest.mark.parametrize("rows,cols,filters,blocks,moves_left", [(5, 6, 64, 2, 1), (9, 7, 64, 1, 0)])
def test_reference_agrees_with_the_torch_module(agx_lib, rows, cols, filters, blocks, moves_left):
    """float64 on both sides; only the order of summation differs"""
    import torch
    from alphagomoku_amd.training import ConvNextModule, import_blob
    d = synthetic.convnext_desc(rows, cols, blocks, filters, moves_left)
    blob, _ = synthetic.make_convnext_weights(d, seed=5)
    module = import_blob(ConvNextModule(d).double(), blob).eval()    # (float64 parameters BEFORE the import: the blob's values are kept as they are)
    features = synthetic.random_features(5, rows, cols, seed=2)
    planes = ((features[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.float64).reshape(5, rows, cols, 32)
    with torch.no_grad():
        got = module(torch.from_numpy(planes))
    ref = cr.reference(d, blob, features)
    for name, mine, theirs in zip(("policy", "value", "q", "m"), (ref.policy, ref.value, ref.q.reshape(5, rows, cols, 3), ref.m), got):
        if mine is None:
            assert theirs is None and not moves_left
            continue
        assert np.abs(mine - theirs.numpy()).max() < 1e-9, name


@pytest.mark.parametrize("moves_left", [0, 1])
def test_export_of_an_imported_blob_is_the_blob(agx_lib, moves_left):
    from alphagomoku_amd.training import ConvNextModule, import_blob, export_blob
    d = synthetic.convnext_desc(6, 5, 2, 64, moves_left)
    blob, _ = synthetic.make_convnext_weights(d, seed=9)
    back = export_blob(import_blob(ConvNextModule(d), blob))
    assert back.shape == blob.shape
    assert (np.abs(back - blob) <= np.spacing(np.abs(blob))).all()          # one fp32 rounding


def test_moves_left_mean_is_the_references_loop():
    from alphagomoku_amd.networks import moves_left_mean
    rng = np.random.default_rng(4)
    m = cr.softmax(rng.standard_normal((3, 225))).astype(np.float32)
    want = []
    for row in m:                                               # NetworkDataPack.cpp:231-233: float result = 0; result += tmp[i] * i
        result = np.float32(0.0)
        for i in range(len(row)):
            result = np.float32(result + np.float32(row[i] * np.float32(i)))
        want.append(result)
    assert np.array_equal(moves_left_mean(m), np.array(want, np.float32))
    one_hot = np.zeros(225, np.float32)
    one_hot[17] = 1.0
    assert moves_left_mean(one_hot) == 17.0


@pytest.mark.parametrize("rows,cols,filters,blocks,moves_left", cr.live_cases())
def test_live_gate_networks_are_exact(rows, cols, filters, blocks, moves_left):
    desc, blob = cr.cached_weights(rows, cols, filters, blocks, moves_left, "live")
    cr.check_exact(desc, blob, cr.feature_batch(rows, cols, "mixed"), "live")


@pytest.mark.parametrize("rows,cols,filters,blocks,moves_left", cr.constant_cases())
def test_constant_gate_networks_are_exact(rows, cols, filters, blocks, moves_left):
    """policy and q; the value and moves-left heads pool over a cell count that is no power of two and are left to the tolerance test"""
    desc, blob = cr.cached_weights(rows, cols, filters, blocks, moves_left, "constant")
    cr.check_exact(desc, blob, cr.feature_batch(rows, cols, "mixed"), "constant", pooled_heads=False)


def test_directed_boards_reach_every_corner_and_border_column():
    for rows, cols in cr.CONSTANT_BOARDS:
        f = cr.directed_boards(rows, cols).reshape(-1, rows, cols)
        stone = (f & 6) != 0
        assert all(stone[:, r, c].any() for r in (0, rows - 1) for c in (0, cols - 1))
        assert all((stone[:, 0, c] | stone[:, rows - 1, c]).any() for c in range(cols))
        assert all((stone[:, r, 0] | stone[:, r, cols - 1]).any() for r in (0, rows - 1))
