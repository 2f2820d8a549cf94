"""CPU side of the any-board network tests: every (network, feature batch) test_nn_any_board_gpu.py compares exactly is proved exact
(nn_exact.check_exact: nothing rounds before the softmax, and the comparison is not vacuous), the directed boards hit the seams they are
named after, and nn_exact.reference agrees with the numpy oracle on the new shapes."""
import numpy as np
import pytest

import nn_any_board as ab
import nn_exact as nx
from alphagomoku_amd import synthetic
from oracle import nn_ref


def case_id(case):
    return "%dx%d-%d-%s-%d-%s" % case


ALL_CASES = sorted(set(ab.gpu_network_cases()) | set(ab.cross(ab.CPU_CROSS)))


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_every_compared_network_is_exact(case):
    """the 360 combinations of the CPU cross and every network of the GPU file, on the random and the directed boards"""
    rows, cols = case[:2]
    desc, blob = ab.weights(*case)
    for batch in ab.BATCHES:
        nx.check_exact(desc, blob, ab.feature_batch(rows, cols, batch))


def test_the_gpu_cases_are_what_the_issue_asks_for():
    cases = ab.gpu_network_cases()
    assert len(cases) == len(set(cases))
    for shape in ab.FULL_CROSS:                                   # the full cross on four shapes
        assert {c[2:] for c in cases if c[:2] == shape} == {(f, k, b, h) for f in ab.FILTERS for k in ab.KINDS for b in ab.BLOCKS for h in ab.HEADS}
    squares = {(n, n) for n in range(5, 21)} - {(15, 15), (20, 20)}
    for shape in squares | {(10, 20), (20, 10), (17, 15)}:        # one network per kind and filter count on every other shape
        assert {(f, k) for r, c, f, k, b, h in cases if (r, c) == shape and b == 1 and h == "random"} == {(f, k) for f in ab.FILTERS for k in ab.KINDS}, shape
    assert all(5 <= r <= 20 and 5 <= c <= 20 and (r, c) not in ab.SPECIALISED for r, c, *_ in cases)


@pytest.mark.parametrize("rows,cols", ab.CPU_CROSS + [(6, 6), (20, 5), (18, 18)])
def test_directed_boards_reach_every_tile_seam(rows, cols):
    boards, names = ab.directed_boards(rows, cols)
    assert boards.shape[1] == rows * cols and len(names) == len(boards) == len(set(names))
    stride = cols + 1
    touched = set()
    empty = boards[names.index("empty")]
    for b, name in zip(boards, names):
        if name.startswith(("stone", "seam")):
            for cell in np.nonzero(b != empty)[0]:
                touched.add((cell // cols) * stride + cell % cols)
    for seam in range(16, rows * stride, 16):
        for p in (seam - 1, seam, seam + 1):
            if p // stride < rows and p % stride < cols:
                assert p in touched, (seam, p)
    for corner in (0, cols - 1, (rows - 1) * stride, (rows - 1) * stride + cols - 1):
        assert corner in touched
    frame = boards[names.index("border frame")].reshape(rows, cols)
    assert (frame[0] != empty[0]).all() and (frame[:, -1] != empty[0]).all() and (frame[1:-1, 1:-1] == empty[0]).all()


@pytest.mark.parametrize("rows,cols,blocks,filters,kind", [(13, 17, 2, 64, "pvq"), (19, 19, 1, 128, "raw")])
def test_reference_matches_the_numpy_oracle(rows, cols, blocks, filters, kind):
    """dense He-init weights: softmax of the float64 logits against the fp32 oracle, bounds of test_nn_exact_cpu.py"""
    d = ab.make_desc(rows, cols, filters, kind, blocks)
    blob, _ = synthetic.make_weights(d, seed=7)
    f = synthetic.random_features(3, rows, cols, seed=11)
    out = nn_ref.forward(d, blob, f)
    p, v, q = nx.reference_outputs(nx.reference(d, blob, f))
    assert np.abs(p - out[0]).max() < 1e-6
    assert np.abs(v - out[1]).max() < 1e-5
    if kind == "pvq":
        assert np.abs(q - out[2]).max() < 1e-5


@pytest.mark.parametrize("rows,cols,blocks,filters,gain,kind,seed", ab.ORACLE_CASES)
def test_oracle_cases_have_a_decided_arg_max(rows, cols, blocks, filters, gain, kind, seed):
    """the feature seed of every He-init case of the GPU file is the first from 3 * blocks + rows on whose boards all have an arg-max the
    reference decides within its own error"""
    d = ab.make_desc(rows, cols, filters, kind, blocks)
    blob, _ = synthetic.make_weights(d, residual_gain=gain)
    first = 3 * blocks + rows
    assert first <= seed < first + 4
    for s in range(first, seed + 1):
        assert ab.arg_max_is_decided(d, blob, synthetic.random_features(8, rows, cols, seed=s)) == (s == seed), s
