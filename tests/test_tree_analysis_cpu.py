"""CPU-side checks of the tree-analysis entry points: declared in include/agx.h, exported by libagx.so, bound in Python, and
GeneratorPool.set_board keeps its positional form."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["agx_engine_set_board_ex", "agx_engine_node_info", "agx_engine_principal_variation"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "agx.h")).read(), flags=re.S)


def test_header_declares_the_tree_analysis_calls():
    text = _header()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"\}\s*AgxNodeView\s*;", text)


def test_library_exports_and_binds_them(agx_lib):
    from alphagomoku_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(cdll, name), name
        assert getattr(agx_lib, name).argtypes is not None, name
    # AgxNodeView: eleven 4-byte fields, the C layout
    assert ctypes.sizeof(_lib.AgxNodeView) == 44
    assert [f for f, _ in _lib.AgxNodeView._fields_] == ["found", "visits", "win", "draw", "moves_left", "score", "flags", "sign_to_move", "depth",
                                                         "virtual_loss", "n_edges"]


def test_set_board_keeps_its_positional_form():
    from alphagomoku_amd import selfplay
    params = inspect.signature(selfplay.GeneratorPool.set_board).parameters
    assert list(params)[:5] == ["self", "game", "board", "sign_to_move", "stream"]
    assert params["stream"].default is None
    assert params["force_remove_root"].kind is inspect.Parameter.KEYWORD_ONLY and params["force_remove_root"].default is False
    for name in ["node_info", "principal_variation"]:
        assert callable(getattr(selfplay.GeneratorPool, name))


def test_node_view_layout_compiles_as_c(tmp_path):
    import subprocess
    src = tmp_path / "view.c"
    src.write_text('#include "agx.h"\n_Static_assert(sizeof(AgxNodeView) == 44, "AgxNodeView layout");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
