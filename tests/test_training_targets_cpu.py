"""The restatement of the reference's default training targets (tests/training_targets_ref.py) checked without a device: against numbers worked
out by hand, against a float64 evaluation of the same formulas, plus the refusals of the loader that need no device and the weighted
head_loss_reference against a hand-written loop."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import training_batch_ref as ref
import training_targets_ref as tref

F32 = np.float32
BAR = 2e-4   # the device test's bar on the values policy (derived in tests/test_training_targets_gpu.py)

# score_info tuples (proven, proven value, distance, win, draw) made by hand
WIN3, LOSS2, DRAW5 = (True, 3, 3, F32(1.0), F32(0.0)), (True, 0, 2, F32(0.0), F32(0.0)), (True, 1, 5, F32(0.0), F32(1.0))
NOTHING = (False, 2, 0, F32(0.5), F32(0.0))


@pytest.fixture(scope="module")
def olib():
    return ol.load()


def test_a_sample_worked_out_by_hand():
    """Eight cells: 0 occupied; 1 a proven win in 3 without visits, prior 0.4; 2 a proven loss in 2, 5 visits, prior 0.1; 3 a proven draw in 5
    without visits, prior 0.05; 4 unknown with 37 visits, value (0.5, 0.25), prior 0.25; 5, 6, 7 empty without an entry.  Minimax value
    (0.5, 0.2) under an unproven minimax score: V = 0.6.
      first loop   q = 1, 0, 0.5, 0.625;  sum_PxQ = 0.4 + 0 + 0.025 + 0.15625 = 0.58125;  sum_P = 0.8;  three unvisited cells
      base Q       0.8 * 0.58125 + 0.2 * 0.6 = 0.585;   default P = 0.2 / 3
      logits       win 50 * 1.5 + ln 0.4 = 74.083710;  loss -50 / 3 + ln 0.1 = -18.969251;  draw 25 + ln 0.05 = 22.004270;
                   unknown 31.25 + ln 0.25 = 29.863706;  unvisited 29.25 + ln(0.2 / 3) = 26.541952
      every cell but the win lies more than 20 below it: six times exp(-20) = 2.0611536e-9, sum 1.0000000123669
      policy       win 0.999999987633, the six others 2.0611536e-9, the occupied cell 0
      action values  (1, 0, 0), (0, 0, 1), (0, 1, 0), (0.5, 0.25, 0.25) on cells 1..4, (0, 0, 1) elsewhere
      weights      counts 0, 1, 5, 1, 37, 0, 0, 0 (the proven cells have at least one visit): sum 44"""
    board = np.array([1, 0, 0, 0, 0, 0, 0, 0], np.uint8)
    visits = np.array([0, 0, 5, 0, 37, 0, 0, 0], np.int32)
    prior = np.array([0, 0.4, 0.1, 0.05, 0.25, 0, 0, 0], np.float32)
    win = np.array([0, 0.9, 0.1, 0.3, 0.5, 0, 0, 0], np.float32)      # the stored values of the proven cells are never used
    draw = np.array([0, 0.05, 0.2, 0.6, 0.25, 0, 0, 0], np.float32)
    infos = [NOTHING, WIN3, LOSS2, DRAW5, NOTHING, NOTHING, NOTHING, NOTHING]
    for T, tol in ((np.float32, 1e-6), (np.float64, 1e-9)):
        policy, av, stats = tref.values_targets(T, board, visits, prior, win, draw, infos, np.array([0.5, 0.2], np.float32), NOTHING)
        assert policy.dtype == T and policy[0] == 0.0
        assert abs(policy[1] - 0.999999987633078) <= tol
        assert np.allclose(policy[2:], 2.061153596948432e-09, rtol=1e-5 if T is np.float32 else 1e-7, atol=0.0)
        assert np.allclose(av, [[0, 0, 1], [1, 0, 0], [0, 0, 1], [0, 1, 0], [0.5, 0.25, 0.25], [0, 0, 1], [0, 0, 1], [0, 0, 1]], rtol=0, atol=1e-7)
        assert stats["unvisited"] == 3 and abs(stats["sum_P"] - 0.8) < 1e-6 and stats["clamped"] == 6 and stats["unclamped"] == 1
        assert (stats["wins_without_visits"], stats["losses"], stats["draws"], stats["visited_unknown"], stats["empty_without_entry"]) == (1, 1, 1, 1, 3)
    counts = tref.fixed_up_counts(board, visits, [i[0] for i in infos])
    assert counts.tolist() == [0, 1, 5, 1, 37, 0, 0, 0]
    weights = tref.weights_of(counts)
    assert weights.dtype == np.float32 and np.array_equal(weights, np.array([F32(c) * (F32(1.0) / F32(44.0)) for c in counts], np.float32))
    assert np.array_equal(tref.weights_of(np.zeros(5, np.int64)), np.zeros(5, np.float32))


def test_a_sample_without_the_clamp_worked_out_by_hand():
    """Two empty cells: one visited, value (0.5, 0.25), prior 0.5; one without an entry; V = 0.6.
      sum_PxQ = 0.3125, sum_P = 0.5, base Q = 0.5 * 0.3125 + 0.5 * 0.6 = 0.45625, default P = 0.5 / 1
      logits 31.25 + ln 0.5 = 30.556853 and 22.8125 + ln 0.5 = 22.119353: 8.4375 apart, exp(-8.4375) = 2.1659095e-4
      policy 1 / 1.00021659095 = 0.99978345595 and 2.1654404990e-4"""
    board, visits = np.zeros(2, np.uint8), np.array([3, 0], np.int32)
    args = (board, visits, np.array([0.5, 0], np.float32), np.array([0.5, 0], np.float32), np.array([0.25, 0], np.float32), [NOTHING, NOTHING],
            np.array([0.5, 0.2], np.float32), NOTHING)
    policy, _, stats = tref.values_targets(np.float64, *args)
    assert np.allclose(policy, [0.9997834559501049, 0.00021654404989510323], rtol=1e-7, atol=0) and stats["clamped"] == 0
    policy32, _, _ = tref.values_targets(np.float32, *args)
    assert (np.abs(policy32 - policy) <= BAR * policy).all()


def test_proven_minimax_score_replaces_the_minimax_value():
    """get_value(minimax_value, minimax_score): one unvisited cell and one visited one; under a proven draw V is 0.5 whatever was stored"""
    args = (np.zeros(2, np.uint8), np.array([3, 0], np.int32), np.array([0.5, 0], np.float32), np.array([0.5, 0], np.float32), np.array([0.25, 0], np.float32),
            [NOTHING, NOTHING])
    a, _, _ = tref.values_targets(np.float64, *args, np.array([0.9, 0.0], np.float32), DRAW5)
    b, _, _ = tref.values_targets(np.float64, *args, np.array([0.5, 0.0], np.float32), NOTHING)
    assert np.array_equal(a, b)


def test_float32_restatement_lies_within_the_bar_of_float64(olib):
    """every sample of the crafted games and of one self-play game, under two symmetries: the float32 restatement against the same formulas in
    float64 on the same dequantised numbers: the same cells are exactly 0, every other cell within 2e-4 relative"""
    n = 15
    games = [ref.parse_game(g) for g in tref.crafted_games(olib, n)] + [ref.parse_game(ref.oracle_game(olib, 0, n, 5, sims=32))]
    checked, worst = 0, 0.0
    for game in games:
        for k in range(len(game["samples"])):
            for a in (0, 5):
                base = ref.reference_sample(olib, 0, n, game, k, a)
                visits, prior, win, draw, score, header, mm = tref.dequantised(olib, n, game, k, a)
                infos = [tref.score_info(olib, x) for x in score]
                root = tref.score_info(olib, int(header[0]) & 0xFFFF)
                p32, av32, _ = tref.values_targets(np.float32, base["board"], visits, prior, win, draw, infos, mm, root)
                p64, av64, _ = tref.values_targets(np.float64, base["board"], visits, prior, win, draw, infos, mm, root)
                assert np.array_equal(p32 == 0, p64 == 0) and np.array_equal(p32 == 0, base["board"] != 0)
                assert (np.abs(p32 - p64) <= BAR * p64).all(), (k, a)
                assert abs(float(p64.sum()) - 1.0) < 1e-12 and np.allclose(av32, av64, rtol=0, atol=1e-6)
                worst = max(worst, float(np.max(np.abs(p32 - p64) / np.where(p64 > 0, p64, 1.0))))
                checked += 1
    print("samples %d, worst relative difference %.3g" % (checked, worst))
    assert checked >= 40


def test_crafted_games_hold_what_they_promise(olib):
    n = 15
    games = [ref.parse_game(g) for g in tref.crafted_games(olib, n)]
    stats = [tref.reference_sample(olib, 0, n, games[0], k, 0)["stats"] for k in range(4)] + [tref.reference_sample(olib, 0, n, games[1], 0, 0)["stats"]]
    assert stats[0]["wins_without_visits"] == 1 and stats[0]["losses"] == 1 and stats[0]["draws"] == 1 and stats[0]["visited_unknown"] == 2
    assert stats[0]["clamped"] > 0 and stats[0]["unclamped"] > 0 and stats[0]["empty_without_entry"] == n * n - 8 - 5
    assert stats[1]["sum_visits"] == 0 and stats[1]["minimax_proven"] and stats[1]["weight_sum"] == 2
    assert stats[2]["sum_P"] > 1.0
    assert stats[3]["weight_sum"] == 0 and stats[3]["unvisited"] == n * n - 6
    assert stats[4]["unvisited"] == 0 and stats[4]["weight_sum"] == 14


def _dataset(agx_lib, tmp_path, olib, n=15):
    from alphagomoku_amd.dataset import TrainingDataset
    path = tmp_path / "crafted.bin"
    ref.write_fragment(path, "FREESTYLE", n, tref.crafted_games(olib, n))
    ds = TrainingDataset(0, n, n)
    ds.add_fragment(path, index=0)
    return ds


def test_flag_refusals_need_no_device(agx_lib, olib, tmp_path):
    """both policy flags together and unknown flags are AGX_ERR_INVALID before anything is resolved, uploaded or launched — through the old
    call, the extended one and the host-pointer forms"""
    from alphagomoku_amd import _lib
    from alphagomoku_amd._lib import AgxError, AgxBatchTensors
    ds = _dataset(agx_lib, tmp_path, olib)
    rec = np.array([[0, 0, 0, 0]], np.int32)
    room = np.zeros(15 * 15 * 3, np.float32)       # never written: the calls are refused
    p = room.ctypes.data
    tensors = AgxBatchTensors(None, None, p, p, p, p, None)
    both = _lib.BATCH_POLICY_VISITS | _lib.BATCH_POLICY_VALUES
    for flags, word in ((both, "two different policy targets"), (8, "unknown flags"), (both | 64, "unknown flags")):
        for call in (lambda f: agx_lib.agx_dataset_load_batch_ex(ds._h, 1, rec.ctypes.data, ctypes.byref(tensors), f, None),
                     lambda f: agx_lib.agx_dataset_load_batch(ds._h, 1, rec.ctypes.data, None, None, p, p, p, p, f, None),
                     lambda f: agx_lib.agx_dataset_load_batch_host_ex(ds._h, 1, rec.ctypes.data, ctypes.byref(tensors), f),
                     lambda f: agx_lib.agx_dataset_load_batch_host(ds._h, 1, rec.ctypes.data, None, None, p, p, p, p, f)):
            with pytest.raises(AgxError, match=word):
                _lib.check(call(flags))
    assert not room.any()
    with pytest.raises(ValueError, match="policy must be"):
        ds.load_batch_pointers(rec, dict(policy_target=p, value_target=p, moves_left_target=p, action_values_target=p), policy="value")
    with pytest.raises(ValueError, match="policy must be"):
        ds.load_batch_host(rec, policy="both")
    ds.close()


def test_weight_key_needs_q_weights(agx_lib, olib, tmp_path, monkeypatch):
    """out= (and the pointers of load_batch_pointers) may name action_values_weight exactly when q_weights is set; refused on the host"""
    import torch
    from alphagomoku_amd import _lib
    ds = _dataset(agx_lib, tmp_path, olib)
    assert "action_values_weight" not in ds.tensor_shapes(3)
    assert ds.tensor_shapes(3, q_weights=True)["action_values_weight"] == (3, 15, 15)
    assert {k: v for k, v in ds.tensor_shapes(3, q_weights=True).items() if k != "action_values_weight"} == ds.tensor_shapes(3)
    rec = np.array([[0, 0, 0, 0]], np.int32)
    monkeypatch.setattr(_lib, "torch_shares_hip_runtime", lambda: True)
    shapes = ds.tensor_shapes(1, q_weights=True)
    out = {k: torch.zeros(shapes[k]) for k in shapes if k not in ("input", "features")}     # host tensors: a valid call would be refused later
    with pytest.raises(ValueError, match="only then"):
        ds.load_batch(rec, out=out)
    del out["action_values_weight"]
    with pytest.raises(ValueError, match="missing \\['action_values_weight'\\]"):
        ds.load_batch(rec, out=out, q_weights=True)
    pointers = dict(policy_target=1, value_target=1, moves_left_target=1, action_values_target=1)
    with pytest.raises(ValueError, match="only then"):
        ds.load_batch_pointers(rec, dict(pointers, action_values_weight=1))
    with pytest.raises(ValueError, match="only then"):
        ds.load_batch_pointers(rec, pointers, q_weights=True)
    ds.close()


def test_weighted_head_loss_reference_against_a_loop():
    """head_loss_reference with action_values_weight: w * ce per cell over the cells with w > 0, whatever the policy target says; NaN in the
    targets and the weights of the cells that do not count reaches neither the loss nor a gradient"""
    import torch
    from alphagomoku_amd.training import head_loss_reference
    rng = np.random.default_rng(3)
    n, rows, cols = 3, 5, 6
    hw = rows * cols
    policy, value, q = (torch.tensor(rng.normal(size=s), dtype=torch.float64, requires_grad=True) for s in ((n, hw), (n, 3), (n, rows, cols, 3)))
    pt = rng.random((n, hw)) * (rng.random((n, hw)) < 0.5)
    pt /= pt.sum(axis=1, keepdims=True)
    vt = np.eye(3)[rng.integers(0, 3, n)]
    qt = rng.dirichlet(np.ones(3), size=(n, hw))
    w = rng.random((n, hw)) * (rng.random((n, hw)) < 0.4)
    w[1] = 0.0                                       # a sample without any weight
    w[0] /= w[0].sum()
    w[2] /= w[2].sum()
    dead = w <= 0
    qt[dead & (rng.random((n, hw)) < 0.5)] = np.nan
    w[2, np.flatnonzero(dead[2])[:2]] = np.nan       # NaN weights do not count either
    w[0, np.flatnonzero(dead[0])[0]] = -0.25
    targets = dict(policy_target=torch.tensor(pt.reshape(n, rows, cols)), value_target=torch.tensor(vt), action_values_target=torch.tensor(qt.reshape(n, rows, cols, 3)),
                   action_values_weight=torch.tensor(w.reshape(n, rows, cols)))
    loss, components = head_loss_reference(policy, value, q, targets, weights=(1.0, 1.0, 0.05))
    loss.backward()
    z = q.detach().numpy().reshape(n, hw, 3)
    want, grad = 0.0, np.zeros((n, hw, 3))
    for b in range(n):
        for i in range(hw):
            if not w[b, i] > 0:
                continue
            lse = np.log(np.exp(z[b, i]).sum())
            want += w[b, i] * sum(qt[b, i, c] * (lse - z[b, i, c]) for c in range(3))
            grad[b, i] = 0.05 / n * w[b, i] * (np.exp(z[b, i] - lse) * qt[b, i].sum() - qt[b, i])
    assert abs(float(components[2].detach()) - want / n) < 1e-12
    assert np.isfinite(float(loss.detach())) and np.allclose(q.grad.numpy().reshape(n, hw, 3), grad, rtol=0, atol=1e-14)
    assert (q.grad.numpy().reshape(n, hw, 3)[~(w > 0)] == 0).all()
    # without the key the mask is the policy target's, as before
    del targets["action_values_weight"]
    targets["action_values_target"] = torch.tensor(np.nan_to_num(qt).reshape(n, rows, cols, 3))
    _, plain = head_loss_reference(policy, value, q, targets)
    edge = pt > 0
    lse = np.log(np.exp(z).sum(axis=2, keepdims=True))
    assert abs(float(plain[2].detach()) - float((np.nan_to_num(qt) * (lse - z))[edge].sum()) / n) < 1e-12
