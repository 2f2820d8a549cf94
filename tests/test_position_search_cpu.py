"""The output stage of the position searcher as restated in tests/position_search_ref.py (which tests/test_position_search_gpu.py holds the
device against) on cases computed by hand, the interface in step (agx.h, exported symbols, ctypes prototypes, the Python wrapper), and the
refusals of agx_position_searcher_* that are decided before a device is touched.  No GPU needed."""
import ctypes
import os
import re

import numpy as np

import position_search_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
N = 5
UNKNOWN = (2 << 13) | 4000

NAMES = ["create", "destroy", "info", "engine", "begin", "select_solve", "buffers", "evaluate", "expand", "harvest", "slots", "finished", "search"]


def move(sign, row, col):
    return sign | (row << 2) | (col << 9)


def edge(m, visits, prior, win, draw, score=UNKNOWN):
    return dict(move=m, visits=visits, prior=F32(prior), win=F32(win), draw=F32(draw), score=score)


EDGES = [edge(move(1, 2, 3), 7, 0.25, 0.5, 0.125), edge(move(1, 0, 0), 9, 0.5, 0.25, 0.25), edge(move(1, 4, 4), 0, 0.125, 0.0, 0.0, (3 << 13) | 3997)]


def test_dense_rows_scatter_the_edges_in_root_order():
    rows = pref.dense_rows(N, EDGES)
    assert rows["edge_index"].tolist().count(-1) == N * N - 3
    assert rows["edge_index"][2 * N + 3] == 0 and rows["edge_index"][0] == 1 and rows["edge_index"][4 * N + 4] == 2
    assert rows["visits"][0] == 9 and rows["prior"][2 * N + 3] == F32(0.25) and rows["q"][0].tolist() == [0.25, 0.25]
    assert rows["score"][4 * N + 4] == (3 << 13) | 3997 and rows["score"][1] == 0 and rows["visits"].sum() == 16
    back = pref.edges_from_rows(N, rows)
    assert [e["cell"] for e in back] == [13, 0, 24] and [e["visits"] for e in back] == [7, 9, 0]
    empty = pref.dense_rows(N, [])
    assert (empty["edge_index"] == -1).all() and not empty["visits"].any() and not empty["q"].any()


def test_final_selectors_pick_the_first_maximum():
    assert pref.final_pick(0, 16, EDGES) == 2            # a proven win beats every rating
    assert pref.final_pick(0, 16, EDGES[:2]) == 0        # 7 + 0.5625 * 16 + ... = 16.0003 against 9 + 0.375 * 16 + ... = 15.0005
    assert pref.final_pick(1, 16, EDGES) == 1 and pref.final_pick(2, 16, EDGES) == 2 and pref.final_pick(4, 16, EDGES) == 1
    assert pref.final_pick(3, 16, EDGES) == 2 and pref.final_pick(3, 16, EDGES[:2]) == 0
    tie = [edge(move(1, 0, 1), 4, 0.1, 0.5, 0.0), edge(move(1, 0, 2), 4, 0.1, 0.5, 0.0)]
    assert pref.final_pick(1, 8, tie) == 0 and pref.final_pick(0, 8, tie) == 0
    assert pref.final_pick(0, 0, []) == -1
    assert pref.board_of([move(1, 0, 1), move(2, 4, 4)], N).tolist() == [0, 1] + [0] * 22 + [2]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "agx.h")).read(), flags=re.S)


def test_interface_is_declared_exported_and_bound(agx_lib):
    from alphagomoku_amd import _lib
    header = _header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("agx_position_searcher_" + n for n in NAMES):
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(cdll, name), name
        assert getattr(agx_lib, name).argtypes is not None, name
    fields = re.search(r"typedef struct AgxPositionSearchOutputs\s*\{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [n for n, _ in _lib.AgxPositionSearchOutputs._fields_]
    assert ctypes.sizeof(_lib.AgxPositionSearchOutputs) == 12 * ctypes.sizeof(ctypes.c_void_p)
    for word, value in (("BAD_INPUT", 1), ("ENGINE_ERROR", 2), ("STEP_LIMIT", 3)):
        assert re.search(r"AGX_POSSEARCH_STATUS_%s = %d\b" % (word, value), header) and getattr(_lib, "POSSEARCH_STATUS_" + word) == value
    from alphagomoku_amd import search
    assert set(search._OUTPUTS) == {n for n, _ in _lib.AgxPositionSearchOutputs._fields_}
    for method in ("search", "begin", "select_solve", "scheduled", "provide", "evaluate", "expand", "harvest", "slot_positions", "finished", "results"):
        assert callable(getattr(search.PositionSearcher, method)), method
    hpp = open(os.path.join(ROOT, "include", "agx.hpp")).read()
    assert "class PositionSearcher" in hpp and all("agx_position_searcher_" + n in hpp for n in NAMES)


def test_refusals_that_need_no_device(agx_lib):
    """argument checks come before the first HIP call: they give their code on a machine without a GPU, and *out stays NULL"""
    from alphagomoku_amd import _lib, selfplay
    INVALID, UNSUPPORTED = 1, 3
    lib, handle = agx_lib, ctypes.c_void_p()
    cfg = selfplay.default_config(n_games=4)
    assert lib.agx_position_searcher_create(None, ctypes.byref(handle)) == INVALID and b"null" in lib.agx_last_error()
    assert lib.agx_position_searcher_create(ctypes.byref(cfg), None) == INVALID
    for mode in (dict(match_mode=1), dict(search_threads=2, n_games=2), dict(search_buffers=2, n_games=2), dict(search_threads=2, search_buffers=2)):
        bad = selfplay.default_config(**dict(dict(n_games=4), **mode))
        assert lib.agx_position_searcher_create(ctypes.byref(bad), ctypes.byref(handle)) == UNSUPPORTED and not handle.value, mode
    out = _lib.AgxPositionSearchOutputs()
    assert lib.agx_position_searcher_begin(None, 1, None, None, None, ctypes.byref(out), 8, 0, None) == INVALID
    assert lib.agx_position_searcher_search(None, None, 1, None, None, None, ctypes.byref(out), 8, 0, None) == INVALID
    for name in ("select_solve", "expand", "harvest"):
        assert getattr(lib, "agx_position_searcher_" + name)(None, None) == INVALID, name
    assert lib.agx_position_searcher_evaluate(None, None, None) == INVALID
    assert lib.agx_position_searcher_buffers(None, None) == INVALID and lib.agx_position_searcher_engine(None, None) == INVALID
    assert lib.agx_position_searcher_slots(None, None, None) == INVALID
    assert lib.agx_position_searcher_finished(None, None, None) == INVALID
    assert lib.agx_position_searcher_info(None, None, None) == INVALID
    assert lib.agx_position_searcher_destroy(None) == 0
