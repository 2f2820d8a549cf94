"""Host-side mirror of the reference's AGNetwork interface for the ResnetPV path (include/alphagomoku/networks/
AGNetwork.hpp:60-98): the subset the self-play path uses — construct from a config, load weights, forward a batch.
All arithmetic happens in libagx.so (HIP); this class only owns handles and device buffers."""
import ctypes
import numpy as np

from ._lib import lib, check, AgxNetDesc, ARCHITECTURES


class DeviceBuffer:
    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        self.nbytes = nbytes
        check(lib.agx_malloc(ctypes.byref(self.ptr), max(nbytes, 16)))

    def upload(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes <= self.nbytes
        check(lib.agx_memcpy_h2d(self.ptr, a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib.agx_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib.agx_free(self.ptr)
            self.ptr = ctypes.c_void_p()


class AGNetwork:
    """A network on the device.  `desc` is a dict as made by synthetic.net_desc() (ResnetPV / PVraw / PVQ) or synthetic.convnext_desc()
    (ConvNextPVQraw / PVQMraw: desc["architecture"] == "convnext", desc["moves_left"] 0 or 1) or synthetic.bottleneck_desc() (BottleneckPV /
    PVraw / PVQ: desc["architecture"] == "bottleneck")."""

    def __init__(self, desc):
        self.desc = dict(desc)
        self._cdesc = AgxNetDesc(desc["rows"], desc["cols"], desc["blocks"], desc["filters"],
                                 desc["in_channels"], desc["value_hidden"], desc.get("action_values", 0))
        self._net = ctypes.c_void_p()
        self._evaluators = {}          # rules -> (AgxPositionEvaluator, capacity), made by evaluate_positions
        self._retired_evaluators = []  # replaced by larger ones; destroyed in close() (destroying one waits for its last launch)
        name = desc.get("architecture", "resnet")
        if name not in ARCHITECTURES:
            raise ValueError("AGNetwork: unknown architecture %r (known: %s)" % (name, ", ".join(sorted(ARCHITECTURES))))
        self._architecture, self._moves_left = ARCHITECTURES[name], int(desc.get("moves_left", 0))
        check(lib.agx_net_create_ex(ctypes.byref(self._cdesc), self._architecture, self._moves_left, ctypes.byref(self._net)))

    def blobFloats(self):
        return int(lib.agx_net_blob_floats_ex(ctypes.byref(self._cdesc), self._architecture, self._moves_left))

    def loadWeights(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        check(lib.agx_net_load_weights(self._net, blob.ctypes.data_as(ctypes.c_void_p), blob.size))

    def load_module(self, module):
        """loadWeights(training.export_blob(module)): a training.TowerModule or ConvNextModule of this network's description, its batch norms
        folded with their running statistics"""
        from .training import export_blob
        keys = set(self.desc) | set(module.desc)
        defaults = dict(architecture="resnet")
        if {k: module.desc.get(k, defaults.get(k, 0)) for k in keys} != {k: self.desc.get(k, defaults.get(k, 0)) for k in keys}:
            raise ValueError("load_module: the module's description %s is not the network's %s" % (module.desc, self.desc))
        self.loadWeights(export_blob(module))

    def forwardDevice(self, d_features, batch, d_policy, d_value, stream=None, d_action_values=None, d_moves_left=None):
        if d_moves_left is not None:
            check(lib.agx_nn_forward_pvqm(self._net, d_features, batch, d_policy, d_value, d_action_values, d_moves_left, stream))
        elif d_action_values is None:
            check(lib.agx_nn_forward(self._net, d_features, batch, d_policy, d_value, stream))
        else:
            check(lib.agx_nn_forward_pvq(self._net, d_features, batch, d_policy, d_value, d_action_values, stream))

    def forward(self, features):
        """Convenience host round trip (tests): features uint32 [B, HW] -> (policy [B, HW], value [B, 3]) and, for a network
        with the action-values head, additionally q [B, HW, 2] = (win, draw) per cell; for one with the moves-left head, moves_left [B, HW]
        (the softmax of the 'm' output: moves_left_mean) is appended."""
        features = np.ascontiguousarray(features, dtype=np.uint32)
        batch, hw = features.shape
        with_q = bool(self.desc.get("action_values", 0))
        f = DeviceBuffer(features.nbytes)
        p = DeviceBuffer(batch * hw * 4)
        v = DeviceBuffer(batch * 3 * 4)
        q = DeviceBuffer(batch * hw * 2 * 4) if with_q else None
        m = DeviceBuffer(batch * hw * 4) if self._moves_left else None
        try:
            f.upload(features)
            self.forwardDevice(f.ptr, batch, p.ptr, v.ptr, None, q.ptr if with_q else None, m.ptr if m is not None else None)
            check(lib.agx_device_synchronize())
            out = (p.download((batch, hw), np.float32), v.download((batch, 3), np.float32))
            if with_q:
                out = out + (q.download((batch, hw, 2), np.float32),)
            if m is not None:
                out = out + (m.download((batch, hw), np.float32),)
            return out
        finally:
            f.free(); p.free(); v.free()
            if q is not None:
                q.free()
            if m is not None:
                m.free()

    def _position_evaluator(self, rules, n):
        """the network's AgxPositionEvaluator for `rules`, with room for n positions.  A larger batch than any before gets a new one (device
        allocations, which the runtime may serialise with the device's work); the old one is kept until close(), so no call waits for it"""
        cache = self._evaluators
        have = cache.get(rules)
        if have is None or have[1] < n:
            if have is not None:
                self._retired_evaluators.append(have[0])
                del cache[rules]
            handle = ctypes.c_void_p()
            capacity = max(n, 64, 2 * have[1] if have is not None else 0)
            check(lib.agx_position_evaluator_create(rules, self.desc["rows"], capacity, ctypes.byref(handle)))
            cache[rules] = (handle, capacity)
        return cache[rules][0]

    def evaluate_positions(self, boards, signs, rules, symmetries=0x01, flags=0, top_k=0, stream=None, out=None, solver=None):
        """agx_position_evaluator_evaluate: boards [n, rows, cols] (or [n, rows * cols]) uint8 with 0 empty / 1 cross / 2 circle and signs [n]
        uint8 (1 cross / 2 circle to move) -> policy [n, rows, cols], value [n, 3], action_values [n, rows, cols, 2] ('pvq' networks),
        top_cells [n, top_k] int32 (row * cols + col, -1 once no legal cell is left), top_probs [n, top_k], status [n] int32.  The rows of
        the symmetries in the mask `symmetries` are averaged; flags: _lib.POSEVAL_MASK_FORBIDDEN | _lib.POSEVAL_RENORMALISE (agx.h).
        numpy arrays make a host round trip and come back as a dict of arrays.  Contiguous device torch tensors stay on the device: the
        launches go on torch.cuda.current_stream() unless `stream` names one (the library must share torch's HIP runtime, as for
        score_outputs), the outputs named in the dict `out` are written where they lie (without `out` torch allocates all of them), nothing
        is waited for, and the dict is returned.
        solver: a solver.PositionSolver of the same rules and board selects agx_position_evaluator_evaluate_solved — the solver's action
        list is the move set (policy 0.0 outside it), a proven position gets its score's value and 1 / k on its k best actions; the dict
        then has one more entry, 'solved': the dict PositionSolver.solve returns (with tensors, `out['solved']` names the ones to write)."""
        from . import _lib
        rows, cols = self.desc["rows"], self.desc["cols"]
        hw, with_q = rows * cols, bool(self.desc.get("action_values", 0))
        shapes = dict(policy=(rows, cols), value=(3,), action_values=(rows, cols, 2), top_cells=(top_k,), top_probs=(top_k,), status=())
        kinds = dict(top_cells=np.int32, status=np.int32)
        names = [k for k in shapes if (with_q or k != "action_values") and (top_k > 0 or not k.startswith("top_"))]
        on_device = hasattr(boards, "data_ptr")
        n = int(boards.shape[0])
        if tuple(boards.shape[1:]) not in ((rows, cols), (hw,)) or tuple(signs.shape) != (n,):
            raise ValueError("evaluate_positions: boards [n, %d, %d] and signs [n] expected" % (rows, cols))
        pe = self._position_evaluator(rules, n)
        c_out = _lib.AgxPositionOutputs()
        c_solved = _lib.AgxSolvedPositions()

        def launch(d_boards, d_signs, on_stream):
            if solver is None:
                check(lib.agx_position_evaluator_evaluate(pe, self._net, n, d_boards, d_signs, symmetries, flags, top_k, ctypes.byref(c_out), on_stream))
            else:
                check(lib.agx_position_evaluator_evaluate_solved(pe, solver.handle, self._net, n, d_boards, d_signs, symmetries, flags, top_k, ctypes.byref(c_out),
                                                                 ctypes.byref(c_solved), on_stream))
        solved_shapes = solver._shapes() if solver is not None else {}
        if on_device:
            import torch
            if not _lib.torch_shares_hip_runtime():
                raise _lib.AgxError("this torch carries a HIP runtime of its own: call alphagomoku_amd._lib.share_torch_hip_runtime() before the "
                                    "library is first used in this process")
            if boards.dtype != torch.uint8 or signs.dtype != torch.uint8:
                raise ValueError("evaluate_positions: boards and signs are uint8 tensors")
            if stream is None:
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            torch_kinds = {np.uint16: torch.int16, np.uint32: torch.int32, np.int32: torch.int32, np.float32: torch.float32}   # (the same bits: PositionSolver.solve)
            if out is None:
                out = {k: torch.empty((n,) + shapes[k], dtype=torch.int32 if k in kinds else torch.float32, device=boards.device) for k in names}
                if solver is not None:
                    out["solved"] = {k: torch.empty((n,) + shape, dtype=torch_kinds[dtype], device=boards.device) for k, (shape, dtype) in solved_shapes.items()}
            for k, t in out.items():
                if k == "solved" and solver is not None:
                    continue
                if k not in names or tuple(t.shape) != (n,) + shapes[k] or t.dtype != (torch.int32 if k in kinds else torch.float32):
                    raise ValueError("evaluate_positions: output '%s' has no place in this call, or another shape or dtype than the call writes" % k)
                setattr(c_out, k, _address(t))
            for k, t in (out.get("solved", {}) if solver is not None else {}).items():
                if k not in solved_shapes or tuple(t.shape) != (n,) + solved_shapes[k][0] or t.dtype != torch_kinds[solved_shapes[k][1]]:
                    raise ValueError("evaluate_positions: output 'solved.%s' has no place in this call, or another shape or dtype than the call writes" % k)
                setattr(c_solved, k, _address(t))
            launch(_address(boards), _address(signs), stream)
            return out
        b = np.ascontiguousarray(boards, dtype=np.uint8)
        s = np.ascontiguousarray(signs, dtype=np.uint8)
        bufs = {k: DeviceBuffer(n * int(np.prod(shapes[k], dtype=np.int64)) * 4) for k in names}
        solved_bufs = {k: DeviceBuffer(n * int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize) for k, (shape, dtype) in solved_shapes.items()}
        d_boards, d_signs = DeviceBuffer(b.nbytes), DeviceBuffer(s.nbytes)
        try:
            d_boards.upload(b)
            d_signs.upload(s)
            for k, buf in bufs.items():
                setattr(c_out, k, buf.ptr)
            for k, buf in solved_bufs.items():
                setattr(c_solved, k, buf.ptr)
            launch(d_boards.ptr, d_signs.ptr, stream)
            check(lib.agx_stream_synchronize(stream))
            result = {k: buf.download((n,) + shapes[k], kinds.get(k, np.float32)) for k, buf in bufs.items()}
            if solver is not None:
                result["solved"] = {k: buf.download((n,) + solved_shapes[k][0], solved_shapes[k][1]) for k, buf in solved_bufs.items()}
            return result
        finally:
            for buf in list(bufs.values()) + list(solved_bufs.values()) + [d_boards, d_signs]:
                buf.free()

    def close(self):
        for handle in [h for h, _ in self._evaluators.values()] + self._retired_evaluators:
            lib.agx_position_evaluator_destroy(handle)
        self._evaluators, self._retired_evaluators = {}, []
        if self._net:
            lib.agx_net_destroy(self._net)
            self._net = ctypes.c_void_p()


def moves_left_mean(m):
    """the expected number of moves left from the 'm' output [..., HW] (NetworkDataPack::unpackMovesLeft, NetworkDataPack.cpp:224-235):
    sum_i i * p_i, added in index order in fp32 like the reference's loop"""
    m = np.asarray(m, dtype=np.float32)
    out = np.zeros(m.shape[:-1], dtype=np.float32)
    for i in range(m.shape[-1]):
        out = out + np.float32(i) * m[..., i]
    return out


def score_dict(score):
    """an AgxNetScore as a dict: the sums, and the means a learning curve plots (policy / value loss per sample, q loss per cell that had
    an edge, accuracy[k - 1] = fraction of the samples whose best target move is among the network's k best)"""
    n, cells = int(score.samples), int(score.q_cells)
    hits = [int(h) for h in score.topk_hit]
    return dict(samples=n, policy_ce=score.policy_ce, value_ce=score.value_ce, q_ce=score.q_ce, q_cells=cells, topk_hit=hits,
                policy_loss=score.policy_ce / n if n else 0.0, value_loss=score.value_ce / n if n else 0.0,
                q_loss=score.q_ce / cells if cells else 0.0, accuracy=[h / n if n else 0.0 for h in hits])


def _address(x):
    if x is None:
        return None
    if hasattr(x, "data_ptr"):   # a torch tensor
        if not (x.is_cuda and x.is_contiguous()):
            raise ValueError("a torch tensor passed as a device buffer must be a contiguous device tensor")
        return ctypes.c_void_p(x.data_ptr())
    return x.ptr if isinstance(x, DeviceBuffer) else ctypes.c_void_p(int(x))


def score_outputs(rows, cols, n, policy, value, policy_target, value_target, action_values=None, action_values_target=None, *,
                  sample_scores=None, total=None, stream=None, action_values_weight=None):
    """agx_net_score_outputs: losses and top-4 hits of n samples from a network's outputs (the layout agx_nn_forward[_pvq] writes: policy
    [n, rows * cols], value [n, 3], action_values [n, rows * cols, 2]) and the targets (the layout load_batch writes: [n, rows, cols],
    [n, 3], [n, rows, cols, 3]), all float32 on the device: torch tensors, DeviceBuffers or raw addresses.  With torch tensors the
    launches go on torch.cuda.current_stream() unless `stream` names one (the library must share torch's HIP runtime, as for
    TrainingDataset.load_batch).  sample_scores: room for n AgxSampleScore records (48 bytes each) or None.
    total: a 72-byte device AgxNetScore the samples are ADDED to (clear it with score_clear; read it with score_total) — the call
    then only enqueues and returns None.  Without it the call scores into a total of its own, waits and returns score_dict().
    action_values_weight: [n, rows, cols] (load_batch's q_weights=True) — the action-value cells that count are then those with a weight
    > 0, each term multiplied by its weight (agx_net_score_outputs_weighted)."""
    from . import _lib
    tensors = [policy, value, policy_target, value_target, action_values, action_values_target, sample_scores, total, action_values_weight]
    if any(hasattr(t, "data_ptr") for t in tensors):
        if not _lib.torch_shares_hip_runtime():
            raise _lib.AgxError("this torch carries a HIP runtime of its own: call alphagomoku_amd._lib.share_torch_hip_runtime() before the "
                                "library is first used in this process")
        if stream is None:
            import torch
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    own = DeviceBuffer(ctypes.sizeof(_lib.AgxNetScore)) if total is None else None
    try:
        if own is not None:
            check(lib.agx_net_score_clear(own.ptr, stream))
        check(lib.agx_net_score_outputs_weighted(rows, cols, n, _address(policy), _address(value), _address(action_values), _address(policy_target),
                                                 _address(value_target), _address(action_values_target), _address(action_values_weight),
                                                 _address(sample_scores), own.ptr if own is not None else _address(total), stream))
        if own is None:
            return None
        check(lib.agx_stream_synchronize(stream))
        return score_total(own)
    finally:
        if own is not None:
            own.free()


def score_clear(total, stream=None):
    """agx_net_score_clear: zeroes a device AgxNetScore (a torch tensor, a DeviceBuffer or a raw address) on `stream`"""
    check(lib.agx_net_score_clear(_address(total), stream))


def score_total(total):
    """reads a device AgxNetScore (a DeviceBuffer or a raw address) back with a blocking copy: score_dict()"""
    from . import _lib
    out = _lib.AgxNetScore()
    check(lib.agx_memcpy_d2h(ctypes.byref(out), _address(total), ctypes.sizeof(out)))
    return score_dict(out)
