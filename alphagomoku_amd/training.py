"""Training a network on the device batches and handing it to the tower.

The last link of the loop self-play -> GameBuffer -> TrainingDataset.load_batch -> train -> AGNetwork -> self-play.  PyTorch-ROCm runs the
convolutions forward and backward and the optimiser; the project adds
  head_loss        the loss of the three heads and dL/dlogits in one hand-written launch (csrc/head_loss.hip, agx.h: agx_head_loss_grad), the
                   same cross-entropies TrainingDataset.score reports,
  TowerModule      ResnetPV / ResnetPVraw / ResnetPVQ as the reference builds them (src/networks/blocks.cpp:32-55,99-127,
                   src/networks/networks.cpp:71-168): no bias and a batch norm WITHOUT a learnable scale but with a shift behind every conv
                   and the hidden dense layer, a bias on the last 1x1 convs and the last dense layer,
  ConvNextModule   ConvNextPVQraw / ConvNextPVQMraw (networks.cpp:1090-1140 / 1154-1219): depthwise 7x7 blocks with squeeze-and-excitation,
                   1x1 heads over global average pooling, the moves-left output 'm' with the loss weight 0.25 (networks.cpp:1214),
  export_blob / import_blob   the exact bridge between such a module and the BN-folded weight blob of agx.h,
  Trainer          RAdam (networks.cpp:89: graph.setOptimizer(ml::RAdam())) over the module on batches of a TrainingDataset.
The architecture, the optimiser and the weight 0.05 of the action-values output (networks.cpp:161) follow reference text; the loss formulas
are the project's own (MinML's are not in the reference tree).  The module runs in fp32; an fp16 `input` tensor is widened.
"""
import ctypes
import math

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

from . import _lib
from ._lib import lib, check, AgxError, AgxNetDesc

LOSS_WEIGHTS = (1.0, 1.0, 0.05)   # policy, value, action values (networks.cpp:161: graph.addOutput(q, ml::CrossEntropyLoss(), 0.05f))
MOVES_LEFT_WEIGHT = 0.25          # networks.cpp:1214: graph.addOutput(mlh, ml::CrossEntropyLoss(), 0.25f)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the loss
# ----------------------------------------------------------------------------------------------------------------------------------------
def _targets(targets, n):
    """policy [n, hw], value [n, 3], action values [n, hw, 3] from a load_batch dict"""
    pt = targets["policy_target"].reshape(n, -1)
    return pt, targets["value_target"].reshape(n, 3), targets["action_values_target"].reshape(n, pt.shape[1], 3)


def head_loss_reference(policy_logits, value_logits, q_logits, targets, weights=LOSS_WEIGHTS):
    """The loss of head_loss as a plain torch composite, in the dtype of the logits: the CPU path and the yardstick of the tests.
    Per sample and head: sum over the entries with target t > 0 of t * (logsumexp(z) - z); the action values per cell over its 3 classes, on
    the cells whose POLICY target is > 0 only.  Targets that do not count are replaced by 0 BEFORE anything is multiplied, so a NaN among the
    filler reaches neither the loss nor, through autograd, a gradient.  When targets holds "action_values_weight" (load_batch's q_weights=True)
    the action-value cells that count are those with a weight > 0, and a cell's cross-entropy enters q_ce multiplied by its weight (w * ce).
    Returns (loss, components): loss = (w_p * policy_ce + w_v * value_ce + w_q * q_ce) / n, components = the three sums / n."""
    n = policy_logits.shape[0]
    dtype = policy_logits.dtype
    pt, vt, qt = _targets(targets, n)
    edge = pt > 0
    zero = torch.zeros((), dtype=dtype, device=policy_logits.device)
    pt = torch.where(edge, pt.to(dtype), zero)
    vt = torch.where(vt > 0, vt.to(dtype), zero)
    policy_ce = -(pt * F.log_softmax(policy_logits.reshape(n, -1), dim=1)).sum()
    value_ce = -(vt * F.log_softmax(value_logits, dim=1)).sum()
    if q_logits is not None and "action_values_weight" in targets:
        w = targets["action_values_weight"].reshape(n, -1)
        counts = w > 0
        w = torch.where(counts, w.to(dtype), zero)
        qt = torch.where(counts.unsqueeze(2) & (qt > 0), qt.to(dtype), zero)
        q_ce = -(w * (qt * F.log_softmax(q_logits.reshape(n, -1, 3), dim=2)).sum(dim=2)).sum()
    elif q_logits is not None:
        qt = torch.where(edge.unsqueeze(2) & (qt > 0), qt.to(dtype), zero)
        q_ce = -(qt * F.log_softmax(q_logits.reshape(n, -1, 3), dim=2)).sum()
    else:
        q_ce = zero
    components = torch.stack([policy_ce, value_ce, q_ce]) / n
    loss = weights[0] * components[0] + weights[1] * components[1] + weights[2] * components[2]
    return loss, components


class _HeadLoss(torch.autograd.Function):
    """forward runs csrc/head_loss.hip once and keeps dL/dlogits; backward multiplies them by grad_output"""

    @staticmethod
    def forward(ctx, policy_logits, value_logits, q_logits, policy_target, value_target, q_target, weights, q_weight=None):
        n, hw = policy_logits.shape
        rows, cols = policy_target.shape[1:3]
        with_q = q_logits is not None
        dev = policy_logits.device
        tensors = [policy_logits, value_logits, q_logits if with_q else None, policy_target, value_target, q_target if with_q else None,
                   q_weight if with_q else None]
        for t in tensors:
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.device == dev):
                raise ValueError("head_loss takes float32 tensors of one ROCm device")
        shapes = [(n, rows * cols), (n, 3), (n, rows * cols, 3), (n, rows, cols), (n, 3), (n, rows, cols, 3), (n, rows, cols)]
        for t, shape in zip(tensors, shapes):   # the kernel trusts the shapes
            if t is not None and tuple(t.shape) != shape:
                raise ValueError("head_loss: a tensor of shape %s where %s is expected" % (tuple(t.shape), shape))
        tensors = [None if t is None else t.detach().contiguous() for t in tensors]
        need = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], with_q and ctx.needs_input_grad[2]]
        grads = [torch.empty_like(t) if t is not None and any(need) else None for t in tensors[:3]]
        records = torch.empty((n, 6), dtype=torch.float64, device=dev)      # n AgxSampleScore, 48 bytes each
        total = torch.zeros(9, dtype=torch.float64, device=dev)             # one AgxNetScore, 72 bytes: [1..3] are the three sums
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            check(lib.agx_head_loss_grad_weighted(rows, cols, n, *[ptr(t) for t in tensors], weights[0] / n, weights[1] / n, weights[2] / n,
                                                  *[ptr(g) for g in grads], ptr(records), ptr(total), stream))
        ctx.grads = grads
        components = total[1:4] / n
        loss = (weights[0] * components[0] + weights[1] * components[1] + weights[2] * components[2]).to(torch.float32)
        ctx.mark_non_differentiable(components, total)
        return loss, components, total

    @staticmethod
    def backward(ctx, grad_loss, _grad_components, _grad_total):
        return tuple(None if (g is None or not need) else g * grad_loss for g, need in zip(ctx.grads, ctx.needs_input_grad[:3])) + (None,) * 5


def _head_loss_total(policy_logits, value_logits, q_logits, targets, weights):
    if not _lib.torch_shares_hip_runtime():
        raise AgxError("this torch carries a HIP runtime of its own: call alphagomoku_amd._lib.share_torch_hip_runtime() before the library is first "
                       "used in this process")
    n = policy_logits.shape[0]
    return _HeadLoss.apply(policy_logits.reshape(n, -1), value_logits, None if q_logits is None else q_logits.reshape(n, -1, 3),
                           targets["policy_target"], targets["value_target"], targets["action_values_target"], tuple(float(w) for w in weights),
                           targets.get("action_values_weight"))


def head_loss(policy_logits, value_logits, q_logits, targets, weights=LOSS_WEIGHTS):
    """The training loss on the device: policy_logits [n, rows * cols], value_logits [n, 3], q_logits [n, rows, cols, 3] or None (float32,
    pre-softmax), targets a load_batch dict (policy_target, value_target, action_values_target, and action_values_weight when the batch was
    loaded with q_weights=True: the action-value loss is then the weighted form of agx_head_loss_grad_weighted).  One call on torch's
    current stream computes the losses AND the gradients of the logits (scales weight / n); autograd's backward only multiplies them by
    grad_output.  Returns (loss, components): loss a float32 device scalar (w_p * policy_ce + w_v * value_ce + w_q * q_ce) / n, components a
    float64 device tensor of the three sums / n (not differentiable).  Nothing is synchronised with the host."""
    loss, components, _ = _head_loss_total(policy_logits, value_logits, q_logits, targets, weights)
    return loss, components


# ----------------------------------------------------------------------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------------------------------------------------------------------
class _Normed(nn.Module):
    """a conv or dense layer without bias + BatchNormalization(...).useGamma(false): normalisation without a learnable scale, with a shift"""

    def __init__(self, layer, channels, spatial):
        super().__init__()
        self.layer = layer
        self.norm = (nn.BatchNorm2d if spatial else nn.BatchNorm1d)(channels, affine=False)
        self.shift = nn.Parameter(torch.zeros(channels))
        self._shape = (1, channels, 1, 1) if spatial else (1, channels)

    def forward(self, x):
        return self.norm(self.layer(x)) + self.shift.view(self._shape)


class _NormedGamma(nn.Module):
    """a conv or dense layer without bias + BatchNormalization(...): normalisation WITH a learnable scale (gamma) and a shift"""

    def __init__(self, layer, channels, spatial):
        super().__init__()
        self.layer = layer
        self.norm = (nn.BatchNorm2d if spatial else nn.BatchNorm1d)(channels, affine=True)

    def forward(self, x):
        return self.norm(self.layer(x))


def _conv(cin, cout, k, bias=False):
    return nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias)


class TowerModule(nn.Module):
    """ResnetPV (desc in_channels 32), ResnetPVraw (in_channels 8) or ResnetPVQ (action_values 1); desc as synthetic.net_desc() makes it.
    With desc["architecture"] == "bottleneck" (synthetic.bottleneck_desc()) BottleneckPV / BottleneckPVraw / BottleneckPVQ: the same input block
    and heads around blocks of three normed convolutions, 1x1 F -> F/2, 3x3 F/2 -> F/2, 3x3 F/2 -> F (createBottleneckBlock_v3, blocks.cpp:84-97).
    forward(input): load_batch's `input` [n, rows, cols, 32] (float32, or float16 which is widened); in_channels == 8 takes planes 0..7 (bit c of
    the feature word = channel c, AGNetwork.cpp:249-258).  Returns the LOGITS: policy [n, rows * cols], value [n, 3], q [n, rows, cols, 3]
    contiguous (None without the head); the softmaxes belong to the loss and to the device tower."""

    def __init__(self, desc):
        super().__init__()
        self.desc = dict(desc)
        f, c, hw, d = desc["filters"], desc["in_channels"], desc["rows"] * desc["cols"], desc["value_hidden"]
        if c not in (8, 32):
            raise ValueError("in_channels must be 32 or 8")
        self.conv_in = _Normed(_conv(c, f, 5), f, True)
        self.bottleneck = desc.get("architecture", "resnet") == "bottleneck"
        if self.bottleneck:
            h = f // 2
            self.blocks = nn.ModuleList(nn.ModuleList([_Normed(_conv(f, h, 1), h, True), _Normed(_conv(h, h, 3), h, True), _Normed(_conv(h, f, 3), f, True)])
                                        for _ in range(desc["blocks"]))
        else:
            self.blocks = nn.ModuleList(nn.ModuleList([_Normed(_conv(f, f, 3), f, True), _Normed(_conv(f, f, 3), f, True)]) for _ in range(desc["blocks"]))
        self.policy1 = _Normed(_conv(f, f, 3), f, True)
        self.policy2 = _conv(f, 1, 1, bias=True)
        self.value1 = _Normed(_conv(f, 4, 1), 4, True)
        self.value2 = _Normed(nn.Linear(hw * 4, d, bias=False), d, False)
        self.value3 = nn.Linear(d, 3)
        if desc.get("action_values", 0):
            self.q1 = _Normed(_conv(f, f, 3), f, True)
            self.q2 = _conv(f, 3, 1, bias=True)
        else:
            self.q1 = self.q2 = None

    def forward(self, x):
        n = x.shape[0]
        x = x[..., :self.desc["in_channels"]].to(self.policy2.weight.dtype).permute(0, 3, 1, 2)   # NHWC planes -> NCHW
        x = F.relu(self.conv_in(x))
        for block in self.blocks:
            y = x
            for layer in block[:-1]:
                y = F.relu(layer(y))
            x = F.relu(x + block[-1](y))
        policy = self.policy2(F.relu(self.policy1(x))).reshape(n, -1)
        v = F.relu(self.value1(x)).permute(0, 2, 3, 1).reshape(n, -1)                           # the value head flattens in NHWC order
        value = self.value3(F.relu(self.value2(v)))
        q = None
        if self.q1 is not None:
            q = self.q2(torch.tanh(self.q1(x))).permute(0, 2, 3, 1).contiguous()
        return policy, value, q

    def _layers(self):
        """(normed layers, biased layers) in blob order: ('normed', m) | ('biased', m)"""
        out = [("normed", self.conv_in)]
        for block in self.blocks:
            out += [("normed", layer) for layer in block]
        out += [("normed", self.policy1), ("biased", self.policy2), ("normed", self.value1), ("normed", self.value2), ("biased", self.value3)]
        if self.q1 is not None:
            out += [("normed", self.q1), ("biased", self.q2)]
        return out


class _ConvNextBlock(nn.Module):
    """networks.cpp:1102-1111: depthwise 7x7 + batch norm, 1x1 + ReLU, 1x1 + residual (no activation), squeeze-and-excitation"""

    def __init__(self, f):
        super().__init__()
        self.depthwise = _NormedGamma(nn.Conv2d(f, f, 7, padding=3, groups=f, bias=False), f, True)
        self.conv1 = _conv(f, f, 1, bias=True)
        self.conv2 = _conv(f, f, 1, bias=True)
        self.se1 = nn.Linear(f, f)
        self.se2 = nn.Linear(f, f)

    def forward(self, x):
        x = self.conv2(F.relu(self.conv1(self.depthwise(x)))) + x
        gate = torch.sigmoid(self.se2(F.relu(self.se1(x.mean(dim=(2, 3))))))
        return x * gate[:, :, None, None]

    def _layers(self):
        return [("gamma", self.depthwise), ("biased", self.conv1), ("biased", self.conv2), ("biased", self.se1), ("biased", self.se2)]


class ConvNextModule(nn.Module):
    """ConvNextPVQraw (desc moves_left 0) or ConvNextPVQMraw (moves_left 1); desc as synthetic.convnext_desc() makes it.
    forward(input): load_batch's `input` [n, rows, cols, 32] (planes 0..7 are read: bit c of the feature word = channel c).  Returns the
    LOGITS: policy [n, rows * cols], value [n, 3], q [n, rows, cols, 3] contiguous, m [n, rows * cols] (None without the head)."""

    def __init__(self, desc):
        super().__init__()
        self.desc = dict(desc)
        f, hw = desc["filters"], desc["rows"] * desc["cols"]
        if desc.get("architecture") != "convnext" or desc["in_channels"] != 8 or desc["value_hidden"] != 256 or not desc.get("action_values", 0):
            raise ValueError("ConvNextModule takes a synthetic.convnext_desc()")
        self.conv_in = _NormedGamma(_conv(8, f, 5), f, True)
        self.blocks = nn.ModuleList(_ConvNextBlock(f) for _ in range(desc["blocks"]))
        self.policy1 = _Normed(_conv(f, f, 1), f, True)
        self.policy2 = _conv(f, 1, 1, bias=True)
        self.value1 = _conv(f, f, 1, bias=True)
        self.value2 = _NormedGamma(nn.Linear(f, 256, bias=False), 256, False)
        self.value3 = nn.Linear(256, 3)
        self.q1 = _Normed(_conv(f, f, 1), f, True)
        self.q2 = _conv(f, 3, 1, bias=True)
        if desc.get("moves_left", 0):
            self.m1 = _conv(f, 32, 1, bias=True)
            self.m2 = _NormedGamma(nn.Linear(32, 128, bias=False), 128, False)
            self.m3 = nn.Linear(128, hw)
        else:
            self.m1 = self.m2 = self.m3 = None

    def forward(self, x):
        n = x.shape[0]
        x = x[..., :8].to(self.policy2.weight.dtype).permute(0, 3, 1, 2)   # NHWC planes -> NCHW
        x = F.relu(self.conv_in(x))
        for block in self.blocks:
            x = block(x)
        policy = self.policy2(F.relu(self.policy1(x))).reshape(n, -1)
        value = self.value3(F.relu(self.value2(F.relu(self.value1(x)).mean(dim=(2, 3)))))
        q = self.q2(F.relu(self.q1(x))).permute(0, 2, 3, 1).contiguous()
        m = None
        if self.m1 is not None:
            m = self.m3(F.relu(self.m2(F.relu(self.m1(x)).mean(dim=(2, 3)))))
        return policy, value, q, m

    def _layers(self):
        out = [("gamma", self.conv_in)]
        for block in self.blocks:
            out += block._layers()
        out += [("normed", self.policy1), ("biased", self.policy2), ("biased", self.value1), ("gamma", self.value2), ("biased", self.value3),
                ("normed", self.q1), ("biased", self.q2)]
        if self.m1 is not None:
            out += [("biased", self.m1), ("gamma", self.m2), ("biased", self.m3)]
        return out


def blob_floats(desc):
    cdesc = AgxNetDesc(desc["rows"], desc["cols"], desc["blocks"], desc["filters"], desc["in_channels"], desc["value_hidden"], desc.get("action_values", 0))
    return int(lib.agx_net_blob_floats_ex(ctypes.byref(cdesc), _lib.ARCHITECTURES[desc.get("architecture", "resnet")], desc.get("moves_left", 0)))


def _to_blob_order(w):
    """torch's [cout, cin, kh, kw] -> [kh][kw][cin][cout]; torch's dense [out, in] -> [in][out]"""
    return w.permute(2, 3, 1, 0) if w.dim() == 4 else w.t()


def _from_blob_order(w, like):
    return w.permute(3, 2, 0, 1) if like.dim() == 4 else w.t()


def export_blob(module, float64=False):
    """The module as the canonical weight blob of agx.h (what AGNetwork.loadWeights takes): every batch norm is folded into its layer with
    its RUNNING statistics — w * s, shift - mean * s, s = 1 / sqrt(var + eps), with a learnable scale ('gamma' layers) s = gamma / sqrt(var +
    eps) and shift = beta — in float64, rounded once to float32 (float64=True: not rounded, for comparisons in float64; the device takes float32),
    transposed to the blob's order.  Returns a numpy float32 array of agx_net_blob_floats(desc) values (the call waits for the copy from the device)."""
    parts = []
    with torch.no_grad():
        for kind, m in module._layers():
            if kind == "normed":
                w = m.layer.weight.double()
                s = 1.0 / torch.sqrt(m.norm.running_var.double() + m.norm.eps)
                parts += [_to_blob_order(w * s.view([-1] + [1] * (w.dim() - 1))), m.shift.double() - m.norm.running_mean.double() * s]
            elif kind == "gamma":
                w = m.layer.weight.double()
                s = m.norm.weight.double() / torch.sqrt(m.norm.running_var.double() + m.norm.eps)
                parts += [_to_blob_order(w * s.view([-1] + [1] * (w.dim() - 1))), m.norm.bias.double() - m.norm.running_mean.double() * s]
            else:
                parts += [_to_blob_order(m.weight.double()), m.bias.double()]
        blob = torch.cat([p.reshape(-1) for p in parts]).to(torch.float64 if float64 else torch.float32).cpu().numpy()
    want = blob_floats(module.desc)
    if blob.size != want:
        raise AgxError("export_blob: the module holds %d values, the blob of its description %d" % (blob.size, want))
    return blob


def import_blob(module, blob):
    """The inverse of export_blob, so that training can start from any existing network (a synthetic one included): the batch norms' running
    statistics become mean 0 and variance 1, their shifts the blob's biases, and the weights are multiplied by sqrt(1 + eps), which the fold
    of export_blob divides out again.  Returns the module."""
    blob = np.ascontiguousarray(blob, dtype=np.float32).reshape(-1)
    if blob.size != blob_floats(module.desc):
        raise AgxError("import_blob: %d values, the blob of the module's description has %d" % (blob.size, blob_floats(module.desc)))
    pos = 0

    def take(shape):
        nonlocal pos
        count = int(np.prod(shape))
        out = torch.from_numpy(blob[pos:pos + count].astype(np.float64)).reshape(tuple(shape))
        pos += count
        return out

    with torch.no_grad():
        for kind, m in module._layers():
            layer = m if kind == "biased" else m.layer
            w = _from_blob_order(take(_to_blob_order(layer.weight).shape), layer.weight)
            if kind == "normed":
                layer.weight.copy_(w * math.sqrt(1.0 + m.norm.eps))
                m.shift.copy_(take(m.shift.shape))
                m.norm.running_mean.zero_()
                m.norm.running_var.fill_(1.0)
            elif kind == "gamma":   # (the learnable scale becomes 1)
                layer.weight.copy_(w * math.sqrt(1.0 + m.norm.eps))
                m.norm.weight.fill_(1.0)
                m.norm.bias.copy_(take(m.norm.bias.shape))
                m.norm.running_mean.zero_()
                m.norm.running_var.fill_(1.0)
            else:
                layer.weight.copy_(w)
                layer.bias.copy_(take(layer.bias.shape))
    assert pos == blob.size
    return module


# ----------------------------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------------------------
class Trainer:
    """RAdam over the trainable parameters of `module` on batches of `dataset`: a TrainingDataset, or anything with its load_batch(samples, out=,
    features=) and sample(batch_size, generator).  A module on a ROCm device trains through head_loss (the HIP kernel), a module on the CPU
    through head_loss_reference.  policy and q_weights choose the targets, as TrainingDataset.load_batch names them (they are passed to
    load_batch only when they differ from its defaults); reference_targets() is the pair the reference's default configuration trains on."""

    def __init__(self, module, dataset, lr=1e-3, weights=LOSS_WEIGHTS, policy="torch_api", q_weights=False):
        self.module, self.dataset, self.weights = module, dataset, tuple(float(w) for w in weights)
        self.target_options = {}
        if policy != "torch_api":
            self.target_options["policy"] = policy
        if q_weights:
            self.target_options["q_weights"] = True
        self.optimizer = torch.optim.RAdam([p for p in module.parameters() if p.requires_grad], lr=lr)
        self._buffers = {}   # batch size -> the tensors load_batch writes into, reused

    @staticmethod
    def reference_targets():
        """Trainer(module, dataset, **Trainer.reference_targets()): what the reference's default configuration trains on — the policy target of
        SamplerValues (TrainingConfig::sampler_type = "values") and the action-value loss weighted per cell by visits / sum of visits
        (fill_action_values_mask), for which its loss weight 0.05 was chosen"""
        return dict(policy="values", q_weights=True)

    def _on_device(self):
        return next(self.module.parameters()).is_cuda

    def _forward(self, samples, reuse):
        n = len(samples)
        batch = self.dataset.load_batch(samples, out=self._buffers.get(n) if reuse else None, features=False, **self.target_options)
        if reuse:
            self._buffers[n] = batch
        return batch, self.module(batch["input"])

    def step(self, samples):
        """one training step on samples [n, 4] (fragment, game, sample, augmentation): load_batch into reused buffers -> module -> loss ->
        backward -> optimiser.  Returns the three loss components (sums / n) as a device tensor — four for a module with the moves-left output
        (ConvNextModule with moves_left: the mean cross-entropy of 'm' last) —; on a ROCm device nothing waits for the host."""
        self.module.train()
        batch, outputs = self._forward(samples, True)
        policy, value, q = outputs[:3]
        loss, components = (head_loss if self._on_device() else head_loss_reference)(policy, value, q, batch, self.weights)
        if len(outputs) > 3 and outputs[3] is not None:
            # the moves-left output 'm' (ConvNextPVQMraw): cross-entropy against the class clamp(int(moves left), 0, HW - 1), weight 0.25, with
            # torch ops; its mean per sample is appended to the components
            m = outputs[3]
            target = batch["moves_left_target"].reshape(-1).to(torch.int64).clamp(0, m.shape[1] - 1)
            m_ce = F.cross_entropy(m, target)
            loss = loss + MOVES_LEFT_WEIGHT * m_ce
            components = torch.cat([components, m_ce.detach().to(components.dtype).reshape(1)])
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        return components.detach()

    def train(self, steps, batch_size, generator):
        """`steps` steps on batches drawn by dataset.sample(batch_size, generator) (a numpy.random.Generator); returns the components of every
        step as a [steps, 3] tensor"""
        return torch.stack([self.step(self.dataset.sample(batch_size, generator)) for _ in range(steps)])

    def evaluate(self, samples, chunk=256):
        """the eval-mode losses (running batch-norm statistics: what export_blob folds) over samples [n, 4], as TrainingDataset.score names them:
        policy_loss and value_loss per sample, q_loss per cell that had an edge, plus the sums.  With q_weights every cell's term carries its
        weight (they sum to 1 per sample): q_loss is then q_ce / samples, the weighted mean per sample, and q_cells counts the cells with a
        weight.  Waits for the result."""
        samples = np.asarray(samples, dtype=np.int32).reshape(-1, 4)
        was_training = self.module.training
        self.module.eval()
        sums, cells = torch.zeros(3, dtype=torch.float64), 0
        try:
            with torch.no_grad():
                for first in range(0, len(samples), chunk):
                    part = samples[first:first + chunk]
                    batch, outputs = self._forward(part, False)
                    policy, value, q = outputs[:3]
                    _, components = (head_loss if self._on_device() else head_loss_reference)(policy, value, q, batch, self.weights)
                    sums += components.double().cpu() * len(part)
                    if q is not None:
                        cells += int((batch["action_values_weight" if "action_values_weight" in batch else "policy_target"] > 0).sum())
        finally:
            self.module.train(was_training)
        n = len(samples)
        policy_ce, value_ce, q_ce = (float(s) for s in sums)
        q_loss = (q_ce / n if n else 0.0) if self.target_options.get("q_weights") else (q_ce / cells if cells else 0.0)
        return dict(samples=n, policy_ce=policy_ce, value_ce=value_ce, q_ce=q_ce, q_cells=cells, policy_loss=policy_ce / n if n else 0.0,
                    value_loss=value_ce / n if n else 0.0, q_loss=q_loss)

    def export_to(self, net):
        """loads the module, batch norms folded, into an AGNetwork"""
        net.load_module(self.module)
        return net
