"""Training batches from self-play games: format-201 fragments -> torch tensors on the ROCm device.

TrainingDataset binds the agx_dataset_* calls of include/agx.h (csrc/training_batch.hip: one wavefront per sample, a batch per launch).
It is what the reference's dataset reader for PyTorch (include/alphagomoku/dataset/torch_api.h, src/dataset/torch_api.cpp) does on one
host thread: load_dataset_fragment / get_dataset_size / load_batch, plus BaseSampler::pick_sample's sampling scheme.  torch only
allocates the tensors and names the stream; the kernel writes through data_ptr().  A PyTorch-ROCm wheel that bundles its own HIP runtime
has to share it with the library first: see _lib.share_torch_hip_runtime().
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, check, AgxError, AgxBatchTensors, AgxDatasetSample, AgxGameBufferStats, AgxTensorShape, BATCH_INPUT_FP16, batch_policy_flag

SYMMETRIES = 8   # number_of_available_symmetries of a square board


class TrainingDataset:
    """Numbered fragments of self-play games of one game configuration (Dataset, src/dataset/Dataset.cpp).  Loading and indexing are
    host work; a fragment's bytes go to the device at the first load_batch that uses it."""

    def __init__(self, rules, rows, cols):
        self.rules, self.rows, self.cols = rules, rows, cols
        self._h = ctypes.c_void_p()
        check(lib.agx_dataset_create(rules, rows, cols, ctypes.byref(self._h)))
        self._next_fragment = 0
        self._order, self._cursor = None, 0   # the sampler's shuffled list of games

    def add_fragment(self, source, index=None):
        """source: the path of a file written by GameBuffer.save (compressed or not), or a live GameBuffer (its finished games are
        copied).  Returns the fragment's number."""
        index = self._next_fragment if index is None else index
        if hasattr(source, "_h"):
            check(lib.agx_dataset_add_fragment_buffer(self._h, index, source._h))
        else:
            check(lib.agx_dataset_add_fragment_file(self._h, index, str(source).encode()))
        self._next_fragment = max(self._next_fragment, index + 1)
        self._order = None
        return index

    def unload_fragment(self, index):
        check(lib.agx_dataset_unload_fragment(self._h, index))
        self._order = None

    def number_of_games(self):
        n = ctypes.c_int()
        check(lib.agx_dataset_games(self._h, ctypes.byref(n)))
        return n.value

    def games(self):
        """get_dataset_size: int32 [games, 4] = (fragment, game, samples, symmetries)"""
        out = np.zeros((self.number_of_games(), 4), np.int32)
        if out.size:
            check(lib.agx_dataset_sizes(self._h, out.ctypes.data_as(ctypes.c_void_p), out.shape[0]))
        return out

    def stats(self):
        s = AgxGameBufferStats()
        check(lib.agx_dataset_stats(self._h, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def tensor_shapes(self, batch_size, q_weights=False):
        """get_tensor_shapes, plus the packed feature words and, with q_weights, action_values_weight [n, rows, cols]"""
        shapes = [AgxTensorShape() for _ in range(6)]
        check(lib.agx_dataset_tensor_shapes(self._h, batch_size, *[ctypes.byref(s) for s in shapes]))
        names = ["input", "features", "policy_target", "value_target", "moves_left_target", "action_values_target"]
        out = {k: tuple(s.dim[:s.rank]) for k, s in zip(names, shapes)}
        if q_weights:
            out["action_values_weight"] = out["policy_target"]
        return out

    @staticmethod
    def _tensors(address):
        """AgxBatchTensors from a function name -> address or None"""
        names = ["input", "features", "policy_target", "value_target", "moves_left_target", "action_values_target", "action_values_weight"]
        return AgxBatchTensors(*[address(k) for k in names])

    @staticmethod
    def _records(samples):
        a = np.ascontiguousarray(np.asarray(samples, dtype=np.int32).reshape(-1, 4))
        assert ctypes.sizeof(AgxDatasetSample) == 16
        return a

    def load_batch(self, samples, *, dtype=None, out=None, features=True, policy="torch_api", q_weights=False):
        """samples: [n, 4] (fragment, game, sample, augmentation).  Returns a dict of torch tensors on the current ROCm device:
        input [n, rows, cols, 32] (dtype torch.float32 or torch.float16), features [n, rows * cols] (the uint32 feature words agx_nn_forward
        takes, as int32), policy_target [n, rows, cols], value_target [n, 3], moves_left_target [n, 1], action_values_target
        [n, rows, cols, 3].  The launch is enqueued on torch.cuda.current_stream(); nothing is synchronised.  features=False leaves the
        feature words out.  out: a dict of tensors to write into, e.g. from an earlier call of the same batch size: it must hold the four
        targets, and exactly what it holds of "input" and "features" is written (dtype and features are then taken from it).
        policy: "torch_api" (proven draw: max(1, visits)), "visits" (SamplerVisits) or "values" (SamplerValues, the reference's default
        sampler: a softmax over 50 * Q + log(eps + P) on the empty cells; action values only on the visited or proven cells).
        q_weights=True adds action_values_weight [n, rows, cols]: visits / sum of visits per cell, the weight training.head_loss gives the
        cell's action-value loss (out= must then hold it, and may hold it only then).  policy="values" with q_weights=True is what the
        reference's default configuration trains on.  The dataset lives on the device of its first batch; a call with another device
        current is refused."""
        if not _lib.torch_shares_hip_runtime():
            raise AgxError("this torch carries a HIP runtime of its own: call alphagomoku_amd._lib.share_torch_hip_runtime() before the library is first "
                           "used in this process, or use load_batch_pointers / load_batch_host")
        import torch
        rec = self._records(samples)
        n = rec.shape[0]
        if out is not None and "input" in out:
            if dtype is not None and dtype != out["input"].dtype:
                raise ValueError("dtype %s does not match out['input'] (%s)" % (dtype, out["input"].dtype))
            dtype = out["input"].dtype
        dtype = dtype or torch.float32
        if dtype not in (torch.float32, torch.float16):
            raise ValueError("input dtype must be torch.float32 or torch.float16")
        policy_flag = batch_policy_flag(policy)
        shapes = self.tensor_shapes(n, q_weights)
        if out is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            out = {k: torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in shapes if k not in ("input", "features")}
            out["input"] = torch.empty(shapes["input"], dtype=dtype, device=dev)
            if features:
                out["features"] = torch.empty(shapes["features"], dtype=torch.int32, device=dev)
        else:
            required = ("policy_target", "value_target", "moves_left_target", "action_values_target") + (("action_values_weight",) if q_weights else ())
            missing = [k for k in required if k not in out]
            if missing or any(k not in shapes for k in out):
                raise ValueError("out must hold the four targets (with q_weights also 'action_values_weight', and only then) and at most 'input' and "
                                 "'features' besides (missing %s)" % missing)
            for k, t in out.items():
                want = dtype if k == "input" else (torch.int32 if k == "features" else torch.float32)
                if tuple(t.shape) != shapes[k] or t.dtype != want or not t.is_contiguous() or not t.is_cuda:
                    raise ValueError("out[%r] must be a contiguous %s device tensor of shape %s" % (k, want, shapes[k]))
        flags = (BATCH_INPUT_FP16 if dtype == torch.float16 else 0) | policy_flag
        tensors = self._tensors(lambda k: out[k].data_ptr() if k in out else None)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib.agx_dataset_load_batch_ex(self._h, n, rec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(tensors), flags, stream))
        return out

    def load_batch_pointers(self, samples, pointers, *, half=False, policy="torch_api", q_weights=False, stream=None):
        """agx_dataset_load_batch_ex on raw device addresses: pointers maps the output names of tensor_shapes() to integers ("input" and
        "features" may be missing; "action_values_weight" is needed, and allowed, exactly with q_weights), stream is a hipStream_t as an
        integer / c_void_p or None"""
        rec = self._records(samples)
        flags = (BATCH_INPUT_FP16 if half else 0) | batch_policy_flag(policy)
        if bool(pointers.get("action_values_weight")) != bool(q_weights):
            raise ValueError("pointers must name 'action_values_weight' with q_weights, and only then")
        tensors = self._tensors(lambda k: pointers.get(k) or None)
        check(lib.agx_dataset_load_batch_ex(self._h, rec.shape[0], rec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(tensors), flags, stream))

    def load_batch_host(self, samples, *, half=False, features=True, policy="torch_api", q_weights=False):
        """the same through the C ABI's host-pointer form (what ag::load_batch forwards to): numpy arrays, no torch"""
        rec = self._records(samples)
        n = rec.shape[0]
        shapes = self.tensor_shapes(n, q_weights)
        out = {k: np.zeros(shapes[k], np.float32) for k in shapes if k not in ("input", "features")}
        out["input"] = np.zeros(shapes["input"], np.float16 if half else np.float32)
        if features:
            out["features"] = np.zeros(shapes["features"], np.uint32)
        flags = (BATCH_INPUT_FP16 if half else 0) | batch_policy_flag(policy)
        tensors = self._tensors(lambda k: out[k].ctypes.data if k in out else None)
        check(lib.agx_dataset_load_batch_host_ex(self._h, n, rec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(tensors), flags))
        return out

    def score(self, net, samples, chunk=0, stream=None, policy="torch_api", q_weights=False):
        """How well `net` (networks.AGNetwork) fits these samples ([n, 4] as for load_batch): batch, network and reductions run on the
        device, `chunk` samples at a time (0 = 1024), on `stream`; the call waits for the 72-byte result.  Returns networks.score_dict():
        the sums (policy_ce, value_ce, q_ce, q_cells, topk_hit[4], samples) and their means (policy_loss, value_loss, q_loss,
        accuracy[4]).  The total does not depend on chunk.  policy: the targets to score against, as for load_batch.  q_weights=True
        weights every cell's action-value term by visits / sum of visits: q_ce / samples is then the weighted mean per sample (q_loss stays
        q_ce / q_cells, q_cells counting the cells with a weight)."""
        from .networks import score_dict
        rec = self._records(samples)
        out = _lib.AgxNetScore()
        check(lib.agx_net_score_dataset_ex(net._net, self._h, rec.shape[0], rec.ctypes.data_as(ctypes.c_void_p), chunk, batch_policy_flag(policy),
                                           1 if q_weights else 0, ctypes.byref(out), stream))
        return score_dict(out)

    def positions(self, samples, *, torch_tensors=None, stream=None):
        """The positions of `samples` ([n, 4] or [n, 3]: fragment, game, sample; an augmentation is ignored) as PositionSearcher takes them:
        (boards [n, rows * cols] uint8 with 0 empty / 1 cross / 2 circle, signs [n] uint8: 1 cross / 2 circle to move), scattered on the
        device from the fragment's resident bytes.  When torch shares the library's HIP runtime (torch_tensors=None: decided by that) the
        two are device torch tensors and the launch goes on torch.cuda.current_stream(), nothing synchronised; otherwise numpy arrays
        after a round trip on `stream`."""
        rec = np.asarray(samples, dtype=np.int32)
        if rec.ndim == 2 and rec.shape[1] == 3:
            rec = np.concatenate([rec, np.zeros((rec.shape[0], 1), np.int32)], axis=1)
        rec = self._records(rec)
        n, cells = rec.shape[0], self.rows * self.cols
        if torch_tensors is None:
            torch_tensors = _lib.torch_shares_hip_runtime()
        if torch_tensors:
            if not _lib.torch_shares_hip_runtime():
                raise AgxError("this torch carries a HIP runtime of its own: call alphagomoku_amd._lib.share_torch_hip_runtime() before the library is "
                               "first used in this process, or ask for numpy arrays (torch_tensors=False)")
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            boards, signs = torch.empty((n, cells), dtype=torch.uint8, device=dev), torch.empty((n,), dtype=torch.uint8, device=dev)
            if stream is None:
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            check(lib.agx_dataset_positions(self._h, n, rec.ctypes.data_as(ctypes.c_void_p), boards.data_ptr(), signs.data_ptr(), stream))
            return boards, signs
        from .networks import DeviceBuffer
        d_boards, d_signs = DeviceBuffer(max(n * cells, 1)), DeviceBuffer(max(n, 1))
        try:
            check(lib.agx_dataset_positions(self._h, n, rec.ctypes.data_as(ctypes.c_void_p), d_boards.ptr, d_signs.ptr, stream))
            check(lib.agx_stream_synchronize(stream))
            if n == 0:
                return np.zeros((0, cells), np.uint8), np.zeros((0,), np.uint8)
            return d_boards.download((n, cells), np.uint8), d_signs.download((n,), np.uint8)
        finally:
            d_boards.free()
            d_signs.free()

    def reanalyse(self, searcher, net, fragment=0, out=None, chunk=0, serial_base=0, max_steps=None, stream=None):
        """The samples of `fragment` searched again with `net` by `searcher` (search.PositionSearcher of the same rules and board): returns
        (GameBuffer, stats) — the same games, moves and outcomes, every sample whose search ended by the move rule (status 0) replaced by
        the fresh root's format-201 bytes, the others kept as they were.  `chunk` positions per searcher job (0 = 16384); position j of
        the pass, in (game, sample) order, is searched with serial serial_base + j.  The result depends neither on chunk nor on the
        searcher's slot count.  out: a GameBuffer to append to (default: a new one).  stats: games, samples, replaced, kept, status
        (samples per status word 0..3), steps."""
        from .selfplay import GameBuffer
        if out is None:
            out = GameBuffer(self.rules, self.rows, self.cols)
        options = _lib.AgxReanalyseOptions(int(chunk), int(serial_base), 0 if max_steps is None else int(max_steps))
        stats = _lib.AgxReanalyseStats()
        check(lib.agx_dataset_reanalyse(self._h, int(fragment), searcher.handle, net._net, out._h, ctypes.byref(options), ctypes.byref(stats), stream))
        return out, dict(games=stats.games, samples=stats.samples, replaced=stats.replaced, kept=stats.kept, status=list(stats.status), steps=stats.steps)

    def sample(self, batch_size, generator):
        """BaseSampler::pick_sample (torch_api.cpp:46-77) batch_size times: the games in a shuffled order, of every game one random
        sample under one random symmetry; when every game has been visited the order is shuffled again.  generator: a
        numpy.random.Generator — the same seed gives the same sequence.  The reference draws from std::random_shuffle and its own
        randInt, whose sequences are not reproduced: only the scheme is.  Returns int32 [batch_size, 4]."""
        games = self.games()
        games = games[games[:, 2] > 0]   # (a fragment with a game without samples is refused when it is loaded)
        if games.shape[0] == 0:
            raise ValueError("the dataset holds no games")
        out = np.zeros((batch_size, 4), np.int32)
        for b in range(batch_size):
            if self._order is None or self._order.shape[0] != games.shape[0]:
                self._order, self._cursor = generator.permutation(games.shape[0]), 0
            fragment, game, samples, symmetries = games[self._order[self._cursor]]
            out[b] = (fragment, game, generator.integers(0, samples), generator.integers(0, symmetries))
            self._cursor += 1
            if self._cursor >= games.shape[0]:
                self._order, self._cursor = generator.permutation(games.shape[0]), 0
        return out

    def close(self):
        if self._h:
            lib.agx_dataset_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone already
            pass
