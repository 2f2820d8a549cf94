"""The whole search on boards (agx.h: agx_position_searcher_*): a batch of positions -> the root of a full search of each (PUCT, threat
solver and network together).  All arithmetic happens in libagx.so (HIP); this class only owns the handle and stages buffers."""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check
from .networks import DeviceBuffer, _address
from .selfplay import GeneratorPool, default_config

# name -> (shape behind [n] with `cells` = board_size ** 2 and `pv` = max_pv, numpy dtype)
_OUTPUTS = dict(status=((), np.int32), root=((4,), np.int32), root_value=((2,), np.float32), best_move=((), np.uint16), visits=(("cells",), np.int32),
                prior=(("cells",), np.float32), q=(("cells", 2), np.float32), score=(("cells",), np.uint16), edge_index=(("cells",), np.int16),
                pv=(("pv",), np.uint16), pv_length=((), np.int32), info=((4,), np.int32))


class _EngineView(GeneratorPool):
    """the searcher's own engine through GeneratorPool's read-only calls (stats, game_info, principal_variation, scheduled / provide) and
    set_max_simulations / set_batch_size; everything that steps or restarts the engine belongs to the searcher"""

    def __init__(self, cfg, handle, buffers):   # noqa: super().__init__ would create an engine
        self.cfg, self._h, self.buffers = cfg, handle, buffers
        self.cells, self.slots = buffers.cells, buffers.slots

    def close(self):
        self._h = ctypes.c_void_p()   # the searcher destroys it


class PositionSearcher:
    """cfg.n_games slots search positions taken off a device-side list: each as a fresh self-play GameGenerator would search for its first
    move after an opening that produced the board (empty tree and solver table, `serials` as the noise / symmetry serial), until the
    engine's move rule fires.  The result is a function of the position, its serial and the configuration alone."""

    def __init__(self, cfg=None, **overrides):
        if cfg is None:
            cfg = default_config(**overrides)
        else:
            for k, v in overrides.items():
                if not hasattr(cfg, k):
                    raise KeyError(k)
                setattr(cfg, k, v)
        self.cfg = cfg
        self._searcher = None   # (__del__ after a refused create)
        handle = ctypes.c_void_p()
        check(lib.agx_position_searcher_create(ctypes.byref(cfg), ctypes.byref(handle)))
        self._searcher = handle
        slots, total = ctypes.c_int(), ctypes.c_uint64()
        check(lib.agx_position_searcher_info(self._searcher, ctypes.byref(slots), ctypes.byref(total)))
        self.slots, self.device_bytes = slots.value, total.value
        self.board_size = cfg.board_size
        self.buffers = _lib.AgxEngineBuffers()
        check(lib.agx_position_searcher_buffers(self._searcher, ctypes.byref(self.buffers)))
        engine = ctypes.c_void_p()
        check(lib.agx_position_searcher_engine(self._searcher, ctypes.byref(engine)))
        self.engine = _EngineView(cfg, engine, self.buffers)
        self._staged = None   # device buffers of a job begun from numpy arrays

    @property
    def handle(self):
        return self._searcher

    def _shapes(self, max_pv):
        cells = self.board_size * self.board_size
        sizes = dict(cells=cells, pv=max_pv)
        return {k: (tuple(sizes.get(d, d) for d in shape), dtype) for k, (shape, dtype) in _OUTPUTS.items()}

    def _check_inputs(self, boards, signs, serials):
        n, size = int(boards.shape[0]), self.board_size
        if tuple(boards.shape[1:]) not in ((size, size), (size * size,)) or tuple(signs.shape) != (n,):
            raise ValueError("boards [n, %d, %d] and signs [n] expected" % (size, size))
        if serials is not None and tuple(serials.shape) != (n,):
            raise ValueError("serials [n] expected")
        return n

    def _sample_shapes(self):
        """the sample sink's two arrays behind [n]: sample [stride] uint8 (the format-201 bytes), sample_bytes int32 (how many of them)"""
        return dict(sample=((_lib.sample_stride(self.board_size * self.board_size),), np.uint8), sample_bytes=((), np.int32))

    def _sink(self, sample, sample_bytes):
        return _lib.AgxPositionSampleSink(sample, _lib.sample_stride(self.board_size * self.board_size), sample_bytes)

    def _torch_job(self, boards, signs, serials, max_pv, stream, out, samples=False):
        import torch
        if not _lib.torch_shares_hip_runtime():
            raise _lib.AgxError("this torch carries a HIP runtime of its own: call alphagomoku_amd._lib.share_torch_hip_runtime() before the "
                                "library is first used in this process")
        if boards.dtype != torch.uint8 or signs.dtype != torch.uint8 or (serials is not None and serials.dtype != torch.int32):
            raise ValueError("boards and signs are uint8 tensors, serials an int32 tensor")
        n = int(boards.shape[0])
        shapes = self._shapes(max_pv)
        kinds = {np.uint16: torch.int16, np.int16: torch.int16, np.int32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8}
        given = out is not None
        if samples:
            shapes.update(self._sample_shapes())
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if out is None:
            out = {k: torch.empty((n,) + shape, dtype=kinds[dtype], device=boards.device) for k, (shape, dtype) in shapes.items()}
        c_out = _lib.AgxPositionSearchOutputs()
        for k, t in out.items():
            if k not in shapes or tuple(t.shape) != (n,) + shapes[k][0] or t.dtype != kinds[shapes[k][1]]:
                raise ValueError("output '%s' has no place in this call, or another shape or dtype than the call writes" % k)
            if k not in ("sample", "sample_bytes"):
                setattr(c_out, k, _address(t))
        sink = None
        if samples:
            if given and ("sample" not in out or "sample_bytes" not in out):
                raise ValueError("with samples=True the dict `out` must hold 'sample' and 'sample_bytes'")
            sink = self._sink(_address(out["sample"]), _address(out["sample_bytes"]))
        return c_out, out, stream, sink

    def _free_staged(self):
        if self._staged is not None:
            for buf in self._staged["bufs"]:
                buf.free()
            self._staged = None

    def _numpy_job(self, boards, signs, serials, max_pv, samples=False):
        n = int(boards.shape[0])
        shapes = self._shapes(max_pv)
        if samples:
            shapes.update(self._sample_shapes())
        self._free_staged()
        b = np.ascontiguousarray(boards, dtype=np.uint8)
        s = np.ascontiguousarray(signs, dtype=np.uint8)
        outs = {k: DeviceBuffer(n * int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize) for k, (shape, dtype) in shapes.items()}
        d_boards, d_signs = DeviceBuffer(b.nbytes), DeviceBuffer(s.nbytes)
        bufs = list(outs.values()) + [d_boards, d_signs]
        d_serials = None
        if serials is not None:
            r = np.ascontiguousarray(serials, dtype=np.int32)
            d_serials = DeviceBuffer(r.nbytes)
            bufs.append(d_serials)
        self._staged = dict(bufs=bufs, outs=outs, shapes=shapes, n=n)
        d_boards.upload(b)
        d_signs.upload(s)
        if d_serials is not None:
            d_serials.upload(r)
        c_out = _lib.AgxPositionSearchOutputs()
        for k, buf in outs.items():
            if k not in ("sample", "sample_bytes"):
                setattr(c_out, k, buf.ptr)
        sink = self._sink(outs["sample"].ptr, outs["sample_bytes"].ptr) if samples else None
        return c_out, d_boards.ptr, d_signs.ptr, (d_serials.ptr if d_serials is not None else None), sink

    def search(self, boards, signs, net, serials=None, max_pv=8, max_steps=None, stream=None, out=None, samples=False):
        """boards [n, size, size] (or [n, size * size]) uint8 with 0 empty / 1 cross / 2 circle, signs [n] uint8 (1 cross / 2 circle to move),
        serials [n] int32 or None (all 0), net an AGNetwork -> dict of status [n] int32 (0 searched, 1 bad input, 2 engine error, 3 step
        limit), root [n, 4] int32 (visits, score bits, flags, edges), root_value [n, 2], best_move [n] uint16, the dense per-cell rows visits
        [n, cells] int32, prior [n, cells], q [n, cells, 2], score [n, cells] uint16, edge_index [n, cells] int16 (-1: no edge), pv [n, max_pv]
        uint16, pv_length [n] int32, info [n, 4] int32 (nodes, edges, steps, engine error).  max_steps None: the library's default.
        numpy arrays make a host round trip and come back as a dict of arrays.  Contiguous device torch tensors stay on the device: the
        launches go on torch.cuda.current_stream() unless `stream` names one (the library must share torch's HIP runtime, as for
        PositionSolver.solve), the outputs named in the dict `out` are written where they lie (without `out` torch allocates all of them;
        torch has no unsigned 16-bit arithmetic, so best_move, score and pv are int16 tensors holding the same bits).  Either way the call
        returns with the stream drained.  samples=True adds sample [n, stride] uint8 and sample_bytes [n] int32: the root of every position
        as the reference's format-201 sample (the bytes a self-play game started from the position would record for its first move),
        sample[i][:sample_bytes[i]]; 0 bytes where there is no root (status 1, 2, or 3 before the first expansion)."""
        n = self._check_inputs(boards, signs, serials)
        steps = 0 if max_steps is None else int(max_steps)
        if hasattr(boards, "data_ptr"):
            c_out, out, stream, sink = self._torch_job(boards, signs, serials, max_pv, stream, out, samples)
            check(lib.agx_position_searcher_search_ex(self._searcher, net._net, n, _address(boards), _address(signs), _address(serials), ctypes.byref(c_out),
                                                      sink, int(max_pv), steps, stream))
            return out
        c_out, d_boards, d_signs, d_serials, sink = self._numpy_job(boards, signs, serials, max_pv, samples)
        try:
            check(lib.agx_position_searcher_search_ex(self._searcher, net._net, n, d_boards, d_signs, d_serials, ctypes.byref(c_out), sink, int(max_pv), steps,
                                                      stream))
            return self.results(stream)
        finally:
            self._free_staged()

    # ---- staged stepping: a caller with an evaluator of its own (and the tests) ----
    def begin(self, boards, signs, serials=None, max_pv=8, max_steps=None, stream=None, out=None, samples=False):
        """records the job and loads the first positions.  Torch device tensors: returns the dict of output tensors (as search); numpy
        arrays: the job is staged in device buffers the searcher keeps, results() downloads the outputs once finished() == n.
        samples=True: the format-201 samples too, as in search."""
        n = self._check_inputs(boards, signs, serials)
        steps = 0 if max_steps is None else int(max_steps)
        if hasattr(boards, "data_ptr"):
            c_out, out, stream, sink = self._torch_job(boards, signs, serials, max_pv, stream, out, samples)
            check(lib.agx_position_searcher_begin_ex(self._searcher, n, _address(boards), _address(signs), _address(serials), ctypes.byref(c_out), sink,
                                                     int(max_pv), steps, stream))
            return out
        c_out, d_boards, d_signs, d_serials, sink = self._numpy_job(boards, signs, serials, max_pv, samples)
        check(lib.agx_position_searcher_begin_ex(self._searcher, n, d_boards, d_signs, d_serials, ctypes.byref(c_out), sink, int(max_pv), steps, stream))
        return None

    def results(self, stream=None):
        """the outputs of the job staged from numpy arrays, as a dict of arrays (waits for `stream`)"""
        if self._staged is None:
            raise _lib.AgxError("results: no job staged from numpy arrays")
        check(lib.agx_stream_synchronize(stream))
        st = self._staged
        return {k: buf.download((st["n"],) + st["shapes"][k][0], st["shapes"][k][1]) for k, buf in st["outs"].items()}

    def select_solve(self, stream=None):
        check(lib.agx_position_searcher_select_solve(self._searcher, stream))

    def scheduled(self):
        """(slot list, features uint32 [n][cells]) of the positions awaiting evaluation (GeneratorPool.scheduled)"""
        return self.engine.scheduled()

    def provide(self, slots, policy, value3, action_values=None):
        """policy [n][cells], value (win, draw, loss) [n][3] and, with action_values configured, q [n][cells][2] of the given slots
        (GeneratorPool.provide)"""
        self.engine.provide(slots, policy, value3, action_values)

    def evaluate(self, net, stream=None):
        check(lib.agx_position_searcher_evaluate(self._searcher, net._net, stream))

    def expand(self, stream=None):
        check(lib.agx_position_searcher_expand(self._searcher, stream))

    def harvest(self, stream=None):
        check(lib.agx_position_searcher_harvest(self._searcher, stream))

    def slot_positions(self, stream=None):
        """int32 [slots]: the position every slot works on, -1 for a free slot (waits for `stream` only)"""
        out = np.zeros(self.slots, np.int32)
        check(lib.agx_position_searcher_slots(self._searcher, stream, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def finished(self, stream=None):
        """positions of the job whose outputs are written (waits for `stream` only)"""
        count = ctypes.c_int()
        check(lib.agx_position_searcher_finished(self._searcher, stream, ctypes.byref(count)))
        return count.value

    def stats(self):
        return self.engine.stats()

    def close(self):
        """waits for the searcher's last launch, frees the pool"""
        if self._searcher:
            lib.agx_position_searcher_destroy(self._searcher)
            self._searcher = ctypes.c_void_p()
            self.engine.close()
            self._free_staged()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone already
            pass
