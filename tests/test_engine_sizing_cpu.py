"""agx_engine_estimate_device_bytes (csrc/engine_host.cpp: engine_create's sizing pass over its one allocator) against byte counts recorded
from the library of the commit before the engine's host layer left engine.hip: the order and the sizes of the allocations did not change.
Four pools that between them take every branch of the allocation list, each for a device of 256 compute units.  No device is needed
and none is touched: the pass runs in a process of its own that sees no GPU even where the box has one, so the speculative wave count (asked of
the runtime per instantiation of k_search_spec, 12 per compute unit where it will not say) is the same everywhere."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bench.py's C2 (its defaults: freestyle 15x15, 1024 games, batch 8, 400 playouts, 4 Mi table entries, yield 0.5, arena reserve 3, format-201
# samples, speculative solver)
C2 = dict(rules=0, board_size=15, n_games=1024, max_batch_size=8, max_simulations=400, tss_table_entries=4 * 1024 * 1024, solver_yield_fraction=0.5,
          action_values=0, node_capacity=max(4096, 8 * 400), edge_capacity=max(65536, 192 * 400), arena_reserve=3.0, record_format=2,
          speculative_solver=1, speculative_waves=0)
POOLS = {
    "C2": C2,
    "C2 serial solver": dict(C2, speculative_solver=0),
    "renju, yielding (parking areas)": dict(C2, rules=2),
    "match pool with action values": dict(C2, match_mode=1, action_values=1),
}
# recorded with the library built from commit 78026c3 (source hash 9f335d799f7730c9), on a box without a GPU
PARENT_BYTES = {
    "C2": 90563739832,
    "C2 serial solver": 89559909224,
    "renju, yielding (parking areas)": 90596246184,
    "match pool with action values": 90578485416,
}

WORKER = textwrap.dedent('''
    import ctypes, json, sys
    sys.path.insert(0, sys.argv[1])
    from alphagomoku_amd import build
    build.build(verbose=False)
    from alphagomoku_amd import lib, check, selfplay, _lib
    _lib.require_current_build()
    out = {}
    for name, fields in json.loads(sys.argv[2]).items():
        cfg = selfplay.default_config(**fields)
        need = ctypes.c_ulonglong()
        check(lib.agx_engine_estimate_device_bytes(ctypes.byref(cfg), 256, ctypes.byref(need)))
        out[name] = need.value
    print(json.dumps(out))
''')


def test_sizing_pass_adds_up_what_the_parent_allocated():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")   # no device for this process, whatever the box has
    p = subprocess.run([sys.executable, "-c", WORKER, ROOT, json.dumps(POOLS)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    print(got)
    assert got == PARENT_BYTES
