"""CPU side of the layered-tower tests (residual networks with 192 .. 512 filters): blob sizes and creation through the C ABI, what stays
refused, the float64 reference against the torch module at F = 192, the export / import bridge, and the proof that every (network, inputs)
pair test_nn_layered_gpu.py compares exactly is exact."""
import ctypes

import numpy as np
import pytest

import nn_exact as nx
import nn_layered_cases as lc
from alphagomoku_amd import synthetic
from alphagomoku_amd._lib import AgxNetDesc
from oracle import nn_ref

ARCH_RESNET, ARCH_CONVNEXT, ARCH_BOTTLENECK = 0, 1, 2           # AgxNetArchitecture, include/agx.h
UNSUPPORTED = 3                                                 # AGX_ERR_UNSUPPORTED


def cdesc(d):
    return AgxNetDesc(d["rows"], d["cols"], d["blocks"], d["filters"], d["in_channels"], d["value_hidden"], d.get("action_values", 0))


@pytest.mark.parametrize("kind", lc.KINDS)
@pytest.mark.parametrize("filters", lc.WIDE)
def test_wide_networks_are_created_and_sized_by_the_layout(agx_lib, filters, kind):
    """agx_net_blob_floats_ex is the count of include/agx.h's layout and agx_net_create_ex takes the network (no GPU needed for either)"""
    for rows, cols, blocks in ((15, 15, 10), (7, 9, 0), (20, 20, 20)):
        d = lc.make_desc(rows, cols, filters, kind, blocks)
        F, C, HW, D = filters, d["in_channels"], rows * cols, 256
        assert d["value_hidden"] == D
        by_hand = 25 * C * F + F + blocks * 2 * (9 * F * F + F) + (9 * F * F + F + F + 1) + (F * 4 + 4 + HW * 4 * D + D + D * 3 + 3)
        if kind == "pvq":
            by_hand += 9 * F * F + F + F * 3 + 3
        assert agx_lib.agx_net_blob_floats_ex(ctypes.byref(cdesc(d)), ARCH_RESNET, 0) == by_hand == sum(int(np.prod(s)) for s in nx.part_shapes(d))
        assert agx_lib.agx_net_blob_floats(ctypes.byref(cdesc(d))) == by_hand
        net = ctypes.c_void_p()
        assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(d)), ARCH_RESNET, 0, ctypes.byref(net)) == 0, agx_lib.agx_last_error()
        assert net
        back = AgxNetDesc()
        assert agx_lib.agx_net_description(net, ctypes.byref(back)) == 0 and (back.filters, back.rows, back.cols, back.blocks) == (filters, rows, cols, blocks)
        assert agx_lib.agx_net_destroy(net) == 0
    assert len(synthetic.make_weights(lc.make_desc(5, 5, filters, kind, 1))[0]) == sum(int(np.prod(s)) for s in nx.part_shapes(lc.make_desc(5, 5, filters, kind, 1)))


REFUSED = [
    (ARCH_RESNET, dict(filters=96, value_hidden=192)),
    (ARCH_RESNET, dict(filters=96, value_hidden=256)),
    (ARCH_RESNET, dict(filters=200, value_hidden=256)),        # no multiple of 64
    (ARCH_RESNET, dict(filters=160, value_hidden=256)),
    (ARCH_RESNET, dict(filters=576, value_hidden=256)),        # above 512
    (ARCH_RESNET, dict(filters=1024, value_hidden=256)),
    (ARCH_RESNET, dict(filters=32, value_hidden=64)),
    (ARCH_RESNET, dict(filters=0, value_hidden=0)),
    (ARCH_RESNET, dict(filters=256, value_hidden=512)),        # hidden is min(256, 2F)
    (ARCH_RESNET, dict(filters=256, value_hidden=256, in_channels=8, action_values=1)),
    (ARCH_RESNET, dict(filters=256, value_hidden=256, rows=21)),
    (ARCH_RESNET, dict(filters=256, value_hidden=256, cols=4)),
    (ARCH_RESNET, dict(filters=256, value_hidden=256, blocks=-1)),
    (ARCH_BOTTLENECK, dict(filters=256, value_hidden=256)),    # wide bottleneck networks
    (ARCH_BOTTLENECK, dict(filters=96, value_hidden=192)),
    (ARCH_CONVNEXT, dict(filters=256, value_hidden=256, in_channels=8, action_values=1)),   # wide ConvNeXt networks
    (ARCH_CONVNEXT, dict(filters=96, value_hidden=256, in_channels=8, action_values=1)),
    (3, dict(filters=256, value_hidden=256)),                   # architecture ids other than 0..2
    (-1, dict(filters=256, value_hidden=256)),
]


@pytest.mark.parametrize("architecture,change", REFUSED)
def test_what_stays_refused(agx_lib, architecture, change):
    d = dict(synthetic.net_desc(15, 15, 2, 64), **change)
    net = ctypes.c_void_p()
    assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(d)), architecture, 0, ctypes.byref(net)) == UNSUPPORTED
    message = agx_lib.agx_last_error()
    assert message and not net
    if architecture == ARCH_BOTTLENECK:
        assert b"bottleneck" in message and b"supported: 5..20 rows and cols" in message
    if architecture == ARCH_RESNET:
        assert b"multiple of 64 from 64 to 512" in message      # the message names the new range


def test_the_moves_left_head_stays_refused_for_wide_residual_networks(agx_lib):
    d = lc.make_desc(15, 15, 256, "pvq", 2)
    net = ctypes.c_void_p()
    assert agx_lib.agx_net_create_ex(ctypes.byref(cdesc(d)), ARCH_RESNET, 1, ctypes.byref(net)) == UNSUPPORTED and not net
    assert agx_lib.agx_net_blob_floats_ex(ctypes.byref(cdesc(d)), ARCH_RESNET, 1) == 0


@pytest.mark.parametrize("case,batch", lc.exact_pairs(), ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else v)
def test_every_compared_pair_is_exact(case, batch):
    """nn_exact.check_exact for every (network, inputs) pair of the GPU file: nothing rounds before the softmax, whatever the order of the
    sums — the device's logits must equal the float64 reference's"""
    rows, cols = case[:2]
    desc, blob = lc.weights(*case)
    nx.check_exact(desc, blob, lc.feature_batch(rows, cols, batch)[:100])


def test_the_cases_are_what_the_kernel_can_get_wrong():
    cases = lc.network_cases()
    assert len(cases) == len(set(cases)) <= 64
    for filters, shapes in lc.SHAPES.items():
        for shape in shapes:
            mine = [c for c in cases if c[:3] == shape + (filters,)]
            assert {c[4] for c in mine} == ({0, 1} if shape == (20, 20) else {0, 1, 2}) and {c[5] for c in mine} == set(lc.HEADS)
        assert {(c[3], c[5]) for c in cases if c[2] == filters} == {(k, h) for k in lc.KINDS for h in lc.HEADS}, filters
    assert set(lc.SHAPES) == {192, 256, 512} and set(lc.SHAPES[512]) == {(5, 5), (7, 9)}
    for rows, cols in lc.SHAPES[192]:                           # a stone in every corner among the inputs, and on both sides of every tile seam
        f = lc.feature_batch(rows, cols, "directed").reshape(-1, rows, cols)
        stone = (f & 6) != 0
        assert all(stone[:, r, c].any() for r in (0, rows - 1) for c in (0, cols - 1))
        for seam in range(16, rows * (cols + 1), 16):
            for p in (seam - 1, seam):
                r, c = divmod(p, cols + 1)
                assert c == cols or stone[:, r, c].any(), (rows, cols, p)


def test_reference_agrees_with_the_torch_module_at_192_filters():
    """float64 on both sides: TowerModule(desc).double().eval() with non-trivial batch-norm statistics and shifts against nn_exact.reference on
    the module's fold kept in float64; only the order of summation differs"""
    import torch
    from alphagomoku_amd.training import TowerModule, export_blob
    rows, cols = 6, 5
    d = lc.make_desc(rows, cols, 192, "pvq", 2)
    torch.manual_seed(11)
    module = TowerModule(d).double()
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
    assert blob.dtype == np.float64 and blob.size == sum(int(np.prod(s)) for s in nx.part_shapes(d))
    features = synthetic.random_features(5, rows, cols, seed=2)
    planes = ((features[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.float64).reshape(5, rows, cols, 32)
    with torch.no_grad():
        got = module(torch.from_numpy(planes))
    ref = nx.reference(d, blob, features, stats=False)
    for name, mine, theirs in zip(("policy", "value", "q"), (ref.policy, ref.value, ref.q.reshape(5, rows, cols, 3)), got):
        assert np.abs(mine.reshape(theirs.shape) - theirs.numpy()).max() < 1e-9, name


@pytest.mark.parametrize("kind", lc.KINDS)
def test_export_of_an_imported_blob_is_the_blob_at_192_filters(kind):
    from alphagomoku_amd.training import TowerModule, import_blob, export_blob
    d = lc.make_desc(6, 5, 192, kind, 2)
    blob, _ = synthetic.make_weights(d, seed=9)
    first = export_blob(import_blob(TowerModule(d), blob))
    assert first.shape == blob.shape
    assert (np.abs(first - blob) <= np.spacing(np.abs(blob))).all()          # one fp32 rounding
    again = export_blob(import_blob(TowerModule(d).double(), first))
    assert np.array_equal(again, first)                                     # export -> import -> export is the identity


def test_restatement_is_the_numpy_oracles_and_rounds_where_the_kernel_stores():
    """the restatement whose summation order can be turned round is oracle.nn_ref.forward(storage="fp16") up to that order (another order
    moves a sum by fp32 roundings, which now and then turns the fp16 rounding of a stored activation: the two agree within the bound the
    device is held to, not to the last bit); on an exact network nothing rounds and both directions give the float64 reference's outputs"""
    desc, blob, f = lc.he_init_case(7, 9, 1, 192, "pvq")
    for mine, theirs in zip(lc.restatement(desc, blob, f), nn_ref.forward(desc, blob, f, storage="fp16")):
        assert np.abs(mine - theirs).max() < lc.BASE_TOLERANCE
    desc, blob = lc.weights(7, 9, 192, "pvq", 1, "random")
    f = lc.feature_batch(7, 9, "random")
    want = nx.reference_outputs(nx.reference(desc, blob, f, stats=False))
    for backwards in (False, True):
        assert all(np.abs(a - b).max() < 1e-6 for a, b in zip(lc.restatement(desc, blob, f, backwards), want))
    bounds, gaps = lc.tolerance(desc, blob, f)
    assert all(g < 1e-12 for g in gaps) and bounds == [lc.BASE_TOLERANCE] * 3
