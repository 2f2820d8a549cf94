"""CPU side of the bottleneck network tests: the blob layout and the refusals of the C ABI, the float64 reference against the torch module and
against nn_exact.reference, the export / import bridge, and the proof that every network test_nn_bottleneck_gpu.py compares exactly is exact."""
import ctypes

import numpy as np
import pytest

import nn_bottleneck_ref as br
import nn_exact as nx
from alphagomoku_amd import synthetic
from alphagomoku_amd._lib import AgxNetDesc

ARCH_BOTTLENECK = 2                                             # AgxNetArchitecture, include/agx.h


def cdesc(d):
    return AgxNetDesc(d["rows"], d["cols"], d["blocks"], d["filters"], d["in_channels"], d["value_hidden"], d.get("action_values", 0))


@pytest.mark.parametrize("rows,cols", [(5, 5), (15, 15), (7, 19)])
@pytest.mark.parametrize("filters", [64, 128])
@pytest.mark.parametrize("blocks", [0, 1, 6])
@pytest.mark.parametrize("kind", br.KINDS)
def test_blob_floats_is_the_layouts_count(agx_lib, rows, cols, filters, blocks, kind):
    d = br.make_desc(rows, cols, filters, kind, blocks)
    F, H, C, HW, D = filters, filters // 2, d["in_channels"], rows * cols, min(256, 2 * filters)
    by_hand = 25 * C * F + F + blocks * (F * H + H + 9 * H * H + H + 9 * H * F + F) + (9 * F * F + F + F + 1) + (F * 4 + 4 + HW * 4 * D + D + D * 3 + 3)
    if kind == "pvq":
        by_hand += 9 * F * F + F + F * 3 + 3
    assert agx_lib.agx_net_blob_floats_ex(ctypes.byref(cdesc(d)), ARCH_BOTTLENECK, 0) == by_hand == br.blob_floats(d)
    assert agx_lib.agx_net_blob_floats_ex(ctypes.byref(cdesc(d)), ARCH_BOTTLENECK, 1) == 0      # no bottleneck network has the moves-left head
    assert len(synthetic.make_bottleneck_weights(d)[0]) == by_hand
    assert len(br.exact_weights(d, 1)) == by_hand


def test_python_names_the_architecture():
    from alphagomoku_amd import _lib
    assert _lib.ARCH_BOTTLENECK == ARCH_BOTTLENECK and _lib.ARCHITECTURES["bottleneck"] == ARCH_BOTTLENECK
    d = synthetic.bottleneck_desc(9, 7, 2, 64, in_channels=8)
    assert d["architecture"] == "bottleneck" and d["value_hidden"] == 128 and d["moves_left"] == 0 and d["in_channels"] == 8


@pytest.mark.parametrize("change,moves_left", [(dict(filters=96, value_hidden=192), 0), (dict(in_channels=8, action_values=1), 0), (dict(rows=21), 0),
                                               (dict(), 1), (dict(cols=4), 0), (dict(value_hidden=64), 0)])
def test_refusals(agx_lib, change, moves_left):
    d = dict(synthetic.bottleneck_desc(15, 15, 2, 64), **change)
    net = ctypes.c_void_p()
    assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(d)), ARCH_BOTTLENECK, moves_left, ctypes.byref(net)) == 3      # AGX_ERR_UNSUPPORTED
    message = agx_lib.agx_last_error()
    assert b"bottleneck" in message and b"supported: 5..20 rows and cols" in message and not net
    assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(synthetic.bottleneck_desc())), 7, 0, ctypes.byref(net)) == 3     # architecture 7 is still refused
    assert not net


@pytest.mark.parametrize("rows,cols,filters,blocks,kind", [(5, 6, 64, 2, "pvq"), (9, 7, 64, 1, "raw"), (6, 5, 128, 1, "pv")])
def test_reference_agrees_with_the_torch_module(agx_lib, rows, cols, filters, blocks, kind):
    """float64 on both sides: TowerModule(desc).double().eval() with non-trivial batch-norm statistics and shifts against the reference on the
    module's fold kept in float64 (export_blob(module, float64=True)); only the order of summation differs"""
    import torch
    from alphagomoku_amd.training import TowerModule, export_blob
    d = br.make_desc(rows, cols, filters, kind, blocks)
    torch.manual_seed(11)
    module = TowerModule(d).double()
    assert len(module.blocks) == blocks and all(len(b) == 3 for b in module.blocks)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(0.3 * torch.randn_like(m.running_mean))
                m.running_var.copy_(0.5 + torch.rand_like(m.running_var))
        for name, p in module.named_parameters():
            if name.endswith("shift"):
                p.copy_(0.1 * torch.randn_like(p))
    module.eval()
    blob = export_blob(module, float64=True)
    assert blob.dtype == np.float64 and blob.size == br.blob_floats(d)
    assert np.array_equal(blob.astype(np.float32), export_blob(module))
    features = synthetic.random_features(5, rows, cols, seed=2)
    planes = ((features[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.float64).reshape(5, rows, cols, 32)
    with torch.no_grad():
        got = module(torch.from_numpy(planes))
    ref = br.reference(d, blob, features, stats=False)
    for name, mine, theirs in zip(("policy", "value", "q"), (ref.policy, ref.value, None if ref.q is None else ref.q.reshape(5, rows, cols, 3)), got):
        if mine is None:
            assert theirs is None and kind != "pvq"
            continue
        assert np.abs(mine - theirs.numpy()).max() < 1e-9, name


@pytest.mark.parametrize("kind", br.KINDS)
def test_export_of_an_imported_blob_is_the_blob(agx_lib, kind):
    from alphagomoku_amd.training import TowerModule, import_blob, export_blob
    d = br.make_desc(6, 5, 64, kind, 2)
    blob, _ = synthetic.make_bottleneck_weights(d, seed=9)
    first = export_blob(import_blob(TowerModule(d), blob))
    assert first.shape == blob.shape
    assert (np.abs(first - blob) <= np.spacing(np.abs(blob))).all()          # one fp32 rounding
    again = export_blob(import_blob(TowerModule(d).double(), first))
    assert np.array_equal(again, first)                                     # export -> import -> export is the identity


@pytest.mark.parametrize("rows,cols,filters,kind,heads", [(7, 9, 64, "pvq", "random"), (15, 15, 128, "raw", "random"), (6, 20, 64, "pv", "transparent")])
def test_without_blocks_the_reference_is_nn_exacts(rows, cols, filters, kind, heads):
    """blocks = 0: the layout coincides with the residual one and the two references agree bit for bit, on an exact network and on a He-init
    one — the new reference's input block and heads are the ones the residual kernels are already held to"""
    d = br.make_desc(rows, cols, filters, kind, 0)
    plain = br.resnet_desc(d)
    assert br.part_shapes(d) == nx.part_shapes(plain) and br.part_names(d) == nx.part_names(plain)
    features = br.features_of(rows, cols)
    assert np.array_equal(synthetic.make_weights(plain, seed=3)[0], synthetic.make_bottleneck_weights(d, seed=3)[0])
    for blob in (br.exact_weights(d, 1, heads), synthetic.make_bottleneck_weights(d, seed=3)[0]):
        mine, theirs = br.reference(d, blob, features), nx.reference(plain, blob, features)
        assert np.array_equal(mine.policy, theirs.policy) and np.array_equal(mine.value, theirs.value)
        assert (mine.q is None and theirs.q is None) or np.array_equal(mine.q, theirs.q)
        assert [tuple(s) for s in mine.stats] == [tuple(s) for s in theirs.stats]
    assert np.array_equal(br.exact_weights(d, 1, heads), nx.exact_weights(plain, 1, heads))


@pytest.mark.parametrize("rows,cols,filters,kind,blocks,heads,seed", br.network_cases() + br.ENTRY_POINT_CASES)
def test_gpu_networks_are_exact(rows, cols, filters, kind, blocks, heads, seed):
    """check_exact for every network and input batch test_nn_bottleneck_gpu.py compares exactly"""
    br.cached_reference(rows, cols, filters, kind, blocks, heads, seed)


def test_cases_cover_what_the_kernel_can_get_wrong():
    cases = br.network_cases()
    assert 28 <= len(cases) <= 36
    for shape in br.SHAPES:
        for f in (64, 128):
            assert any(c[:3] == shape + (f,) and c[4] >= 1 for c in cases), (shape, f)
    assert {c[4] for c in cases} == {0, 1, 3} and {c[3] for c in cases} == set(br.KINDS) and {c[5] for c in cases} == {"random", "transparent"}
    assert any(c[5] == "transparent" and c[4] >= 1 for c in cases) and {c[6] for c in cases if c[5] == "random"} == {1, 2}
    for rows, cols in br.SHAPES:                                 # a stone in every corner and on every border column among the inputs
        f = br.features_of(rows, cols).reshape(-1, rows, cols)
        stone = (f & 6) != 0
        assert all(stone[:, r, c].any() for r in (0, rows - 1) for c in (0, cols - 1))
        assert all((stone[:, 0, c] | stone[:, rows - 1, c]).any() for c in range(cols))


def test_restatement_rounds_where_the_kernel_stores():
    """on an exact network nothing rounds: the restatement, forwards and backwards, gives the float64 reference's outputs"""
    rows, cols, filters, kind, blocks, heads, seed = 8, 8, 64, "pvq", 1, "random", 1
    desc, blob = br.cached_weights(rows, cols, filters, kind, blocks, heads, seed)
    f = br.features_of(rows, cols)[:6]
    want = nx.reference_outputs(br.reference(desc, blob, f, stats=False))
    for backwards in (False, True):
        got = br.restatement(desc, blob, f, backwards)
        assert all(np.abs(a - b).max() < 1e-6 for a, b in zip(got, want))   # (tanh(8) is 1 - 2.3e-7 in float64 and 1 in fp16)
    bounds, gaps = br.tolerance(desc, blob, f)
    assert all(g < 1e-12 for g in gaps) and bounds == [br.BASE_TOLERANCE] * 3
