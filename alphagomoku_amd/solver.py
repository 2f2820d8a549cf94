"""The threat solver on boards (agx.h: agx_position_solver_*): a batch of positions -> proven scores and the solver's action lists.
All arithmetic happens in libagx.so (HIP); this class only owns the handle and stages buffers."""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check
from .networks import DeviceBuffer, _address

# name -> (shape behind [n] with `cells` = board_size ** 2, numpy dtype)
_OUTPUTS = dict(score=((), np.uint16), flags=((), np.uint32), n_actions=((), np.int32), moves=(("cells",), np.uint16), move_scores=(("cells",), np.uint16),
                nodes=((), np.uint32), value=((3,), np.float32), status=((), np.int32))


class PositionSolver:
    """Every position is solved as a fresh AlphaBetaSearch with an empty table of `table_entries` entries and node limit `max_positions`
    would solve it.  `capacity` positions per call; a wave of the launch owns its own table and spill areas (`waves`, `bytes_per_wave`,
    `device_bytes`)."""

    def __init__(self, rules, board_size, capacity, max_positions=100, table_entries=1 << 16, zobrist_seed=0x9E3779B97F4A7C15):
        self.rules, self.board_size, self.capacity = rules, board_size, capacity
        self._solver = None   # (__del__ after a refused create)
        handle = ctypes.c_void_p()
        check(lib.agx_position_solver_create(rules, board_size, capacity, max_positions, table_entries, zobrist_seed, ctypes.byref(handle)))
        self._solver = handle
        waves, per_wave, total = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib.agx_position_solver_info(self._solver, ctypes.byref(waves), ctypes.byref(per_wave), ctypes.byref(total)))
        self.waves, self.bytes_per_wave, self.device_bytes = waves.value, per_wave.value, total.value

    @property
    def handle(self):
        return self._solver

    def _shapes(self):
        cells = self.board_size * self.board_size
        return {k: (tuple(cells if d == "cells" else d for d in shape), dtype) for k, (shape, dtype) in _OUTPUTS.items()}

    def solve(self, boards, signs, stream=None, out=None):
        """boards [n, size, size] (or [n, size * size]) uint8 with 0 empty / 1 cross / 2 circle and signs [n] uint8 (1 cross / 2 circle to
        move) -> score [n] uint16, flags [n] uint32, n_actions [n] int32, moves and move_scores [n, cells] uint16 (the solver's list in the
        solver's order, zeros behind it), nodes [n] uint32, value [n, 3], status [n] int32.
        numpy arrays make a host round trip and come back as a dict of arrays.  Contiguous device torch tensors stay on the device: the
        launch goes on torch.cuda.current_stream() unless `stream` names one (the library must share torch's HIP runtime, as for
        AGNetwork.evaluate_positions), the outputs named in the dict `out` are written where they lie (without `out` torch allocates all
        of them; torch has no unsigned 16 / 32-bit arithmetic, so score, moves and move_scores are int16 tensors and flags and nodes int32
        tensors holding the same bits), nothing is waited for, and the dict is returned."""
        n, size = int(boards.shape[0]), self.board_size
        if tuple(boards.shape[1:]) not in ((size, size), (size * size,)) or tuple(signs.shape) != (n,):
            raise ValueError("solve: boards [n, %d, %d] and signs [n] expected" % (size, size))
        shapes = self._shapes()
        c_out = _lib.AgxSolvedPositions()
        if hasattr(boards, "data_ptr"):
            import torch
            if not _lib.torch_shares_hip_runtime():
                raise _lib.AgxError("this torch carries a HIP runtime of its own: call alphagomoku_amd._lib.share_torch_hip_runtime() before the "
                                    "library is first used in this process")
            if boards.dtype != torch.uint8 or signs.dtype != torch.uint8:
                raise ValueError("solve: boards and signs are uint8 tensors")
            kinds = {np.uint16: torch.int16, np.uint32: torch.int32, np.int32: torch.int32, np.float32: torch.float32}
            if stream is None:
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if out is None:
                out = {k: torch.empty((n,) + shape, dtype=kinds[dtype], device=boards.device) for k, (shape, dtype) in shapes.items()}
            for k, t in out.items():
                if k not in shapes or tuple(t.shape) != (n,) + shapes[k][0] or t.dtype != kinds[shapes[k][1]]:
                    raise ValueError("solve: output '%s' has no place in this call, or another shape or dtype than the call writes" % k)
                setattr(c_out, k, _address(t))
            check(lib.agx_position_solver_solve(self._solver, n, _address(boards), _address(signs), ctypes.byref(c_out), stream))
            return out
        b = np.ascontiguousarray(boards, dtype=np.uint8)
        s = np.ascontiguousarray(signs, dtype=np.uint8)
        bufs = {k: DeviceBuffer(n * int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize) for k, (shape, dtype) in shapes.items()}
        d_boards, d_signs = DeviceBuffer(b.nbytes), DeviceBuffer(s.nbytes)
        try:
            d_boards.upload(b)
            d_signs.upload(s)
            for k, buf in bufs.items():
                setattr(c_out, k, buf.ptr)
            check(lib.agx_position_solver_solve(self._solver, n, d_boards.ptr, d_signs.ptr, ctypes.byref(c_out), stream))
            check(lib.agx_stream_synchronize(stream))
            return {k: buf.download((n,) + shapes[k][0], shapes[k][1]) for k, buf in bufs.items()}
        finally:
            for buf in list(bufs.values()) + [d_boards, d_signs]:
                buf.free()

    def close(self):
        """frees the tables and spill areas of every wave (device_bytes); waits for the solver's last launch"""
        if self._solver:
            lib.agx_position_solver_destroy(self._solver)
            self._solver = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone already
            pass
