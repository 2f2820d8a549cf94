"""numpy restatement of the output stage of the position searcher (csrc/engine.hip: k_harvest_positions; agx.h: AgxPositionSearchOutputs):
the root's edges, in root order, scattered over the board's cells; edge_index; the pick of the final selector.  A root edge is a dict
(move, visits, prior, win, draw, score) as tests/test_engine_gpu.py reads them from the oracle."""
import numpy as np

from test_engine_gpu import _best_edge

F32 = np.float32


def move_cell(move, n):
    """Move::toShort = sign | row << 2 | col << 9 -> row * n + col"""
    return ((move >> 2) & 127) * n + ((move >> 9) & 127)


def board_of(moves, n):
    board = np.zeros(n * n, np.uint8)
    for m in moves:
        board[move_cell(m, n)] = m & 3
    return board


def dense_rows(n, edges):
    """visits [cells] int32, prior [cells] f32, q [cells][2] f32, score [cells] uint16, edge_index [cells] int16: the edge of every cell,
    0 / 0.0f / -1 where the root has none"""
    cells = n * n
    out = dict(visits=np.zeros(cells, np.int32), prior=np.zeros(cells, F32), q=np.zeros((cells, 2), F32), score=np.zeros(cells, np.uint16),
               edge_index=np.full(cells, -1, np.int16))
    for i, e in enumerate(edges):
        c = move_cell(e["move"], n)
        assert out["edge_index"][c] == -1, "two root edges on one cell"
        out["visits"][c], out["prior"][c], out["score"][c], out["edge_index"][c] = e["visits"], e["prior"], e["score"], i
        out["q"][c] = (e["win"], e["draw"])
    return out


def final_pick(selector, root_visits, edges):
    """index of the edge cfg.final_selector picks (EdgeSelector.cpp:476-536: 0 best, 1 max visits, 2 min visits, 3 max value, 4 max
    policy), first maximum wins; -1 without edges.  The LCB selector (5) is not restated: its pick is held against the oracle's move."""
    if not edges:
        return -1
    if selector == 0:
        return _best_edge(root_visits, edges)
    best, best_value = -1, F32(-3.0e38)
    for i, e in enumerate(edges):
        pv, distance = (e["score"] >> 13) & 3, F32((e["score"] & 8191) - 4000)
        if selector == 1:
            value = F32(e["visits"])
        elif selector == 2:
            value = F32(-e["visits"])
        elif selector == 3:
            expectation = F32(e["win"]) + F32(0.5) * F32(e["draw"])
            value = {0: F32(-1000.0) + distance, 1: F32(0.5), 3: F32(1000.0) + distance}.get(pv, expectation)
        elif selector == 4:
            value = F32(e["prior"])
        else:
            raise ValueError("selector %d is not restated" % selector)
        if value > best_value:
            best, best_value = i, value
    return best


def edges_from_rows(n, rows):
    """the root's edges back out of the dense rows of one position, in root order (through edge_index)"""
    order = sorted((int(i), c) for c, i in enumerate(rows["edge_index"]) if i >= 0)
    assert [i for i, _ in order] == list(range(len(order))), "edge_index is no permutation of the root's edges"
    return [dict(cell=c, visits=int(rows["visits"][c]), prior=F32(rows["prior"][c]), win=F32(rows["q"][c][0]), draw=F32(rows["q"][c][1]),
                 score=int(rows["score"][c])) for _, c in order]
