"""The SwAV ResNet-50 feature extractor of the GAN metrics (drop-in for maua/GAN/metrics/extractors/swav.py).

``ResNetFeatures`` runs the bottleneck backbone of the reference's ``ResNet(Bottleneck, layers)`` on the library's strided
implicit-GEMM convolution (csrc/resnet_conv.hip, csrc/resnet.hip): 7x7 stem, max-pool, four layers, global average pool ->
float32 [B, 32 * width].  BatchNorm never reaches the device code: every ``bnX`` is folded into its convolution here, in float64,
and rounded once to float32.  Forward only; the projection head and the prototypes are not built.

``SwAV(checkpoint)`` is the reference's ``SwAV()`` with the weights read from a local ``swav_800ep_pretrain.pth.tar``-style file.
The weights are not bundled and nothing is downloaded; without a file only ``checkpoint="random"`` with ``allow_random_init=True``
works (the reference's own initialisation).  There is no CPU path.
"""
import ctypes as C

import torch

from . import _lib as L

BN_EPS = 1e-5
IGNORED_PREFIXES = ("projection_head.", "prototypes.")      # the reference loads with strict=False and never builds them (output_dim=0)


def conv_names(layers):
    """The convolutions in the state dict's order, each with its BatchNorm: [(conv key prefix, bn key prefix)]."""
    names = [("conv1", "bn1")]
    for l, blocks in enumerate(layers, start=1):
        for b in range(blocks):
            p = f"layer{l}.{b}."
            names += [(p + "conv1", p + "bn1"), (p + "conv2", p + "bn2"), (p + "conv3", p + "bn3")]
            if b == 0:
                names.append((p + "downsample.0", p + "downsample.1"))
    return names


def fold_bn(weight, gamma, beta, mean, var, eps=BN_EPS):
    """conv followed by BatchNorm (running statistics) as one convolution with bias, in float64:
    s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s; rounded once to float32."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    w = weight.double() * s.reshape(-1, 1, 1, 1)
    b = beta.double() - mean.double() * s
    return w.float().contiguous(), b.float().contiguous()


def clean_state_dict(sd):
    """``module.`` stripped (swav.py:352); head, prototypes and num_batches_tracked dropped."""
    out = {}
    for k, v in sd.items():
        k = k[len("module."):] if k.startswith("module.") else k
        if k.startswith(IGNORED_PREFIXES) or k.endswith("num_batches_tracked"):
            continue
        out[k] = v
    return out


def random_state_dict(layers=(3, 4, 6, 3), width=64, generator=None):
    """The reference's own initialisation (swav.py:225-230): kaiming_normal_(mode="fan_out", nonlinearity="relu") for every
    convolution, BatchNorm weight 1, bias 0, running statistics 0 / 1."""
    sd = {}
    lib_shapes = conv_shapes(layers, width)
    for (conv, bn), (ci, co, k, _) in zip(conv_names(layers), lib_shapes):
        std = (2.0 / (co * k * k)) ** 0.5
        sd[conv + ".weight"] = torch.randn((co, ci, k, k), generator=generator) * std
        sd[bn + ".weight"], sd[bn + ".bias"] = torch.ones(co), torch.zeros(co)
        sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.zeros(co), torch.ones(co)
    return sd


def conv_shapes(layers, width=64, dtype=torch.float32):
    """[(Ci, Co, k, stride)] of every convolution as the library builds the network - no device needed."""
    lib = L.lib()
    net = C.c_void_p()
    L.check(lib.maua_resnet_create(None, L.dtype_id(dtype), (C.c_int * 4)(*layers), int(width), C.byref(net)))
    try:
        out = []
        ci, co, k, st = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        for i in range(lib.maua_resnet_conv_count(net)):
            L.check(lib.maua_resnet_conv_shape(net, i, C.byref(ci), C.byref(co), C.byref(k), C.byref(st)))
            out.append((ci.value, co.value, k.value, st.value))
        return out
    finally:
        lib.maua_resnet_destroy(net)


class ResNetFeatures:
    """``ResNet(Bottleneck, layers).forward_backbone`` (+ the identity ``forward_head``) on the device.

    ``state_dict``: the reference's keys (``conv1.weight``, ``bn1.{weight,bias,running_mean,running_var}``, ``layerN.M.convK.weight``,
    ``layerN.M.downsample.{0,1}.*``; ``module.`` prefixes, head / prototype keys and ``num_batches_tracked`` are ignored);
    None: the reference's initialisation drawn from ``generator``.  ``dtype``: torch.float32 (exact products) or torch.bfloat16."""

    def __init__(self, layers=(3, 4, 6, 3), width=64, dtype=torch.float32, state_dict=None, generator=None):
        L.require_device()
        if dtype not in (torch.float32, torch.bfloat16):
            raise L.MauaHipError(f"ResNetFeatures: dtype must be float32 or bfloat16, got {dtype}")
        self.layers, self.width, self.dtype = tuple(int(n) for n in layers), int(width), dtype
        if len(self.layers) != 4:
            raise ValueError("ResNetFeatures: layers must name four block counts")
        self.out_dim = 32 * self.width
        self._lib = L.lib()
        self._net = C.c_void_p()
        L.check(self._lib.maua_resnet_create(L.ctx(), L.dtype_id(dtype), (C.c_int * 4)(*self.layers), self.width, C.byref(self._net)))
        self.load_state_dict(random_state_dict(self.layers, self.width, generator) if state_dict is None else state_dict)

    def __del__(self):
        net, self._net = getattr(self, "_net", None), None
        if net:
            self._lib.maua_resnet_destroy(net)

    def load_state_dict(self, sd):
        sd = clean_state_dict(sd)
        names = conv_names(self.layers)
        n = self._lib.maua_resnet_conv_count(self._net)
        assert n == len(names), (n, len(names))
        wanted = {c + ".weight" for c, _ in names} | {f"{b}.{p}" for _, b in names for p in ("weight", "bias", "running_mean", "running_var")}
        missing, unexpected = sorted(wanted - set(sd)), sorted(set(sd) - wanted)
        if missing or unexpected:
            raise KeyError(f"ResNetFeatures{self.layers}: missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                           f"unexpected keys {unexpected[:4]}{'...' if len(unexpected) > 4 else ''}")
        ci, co, k, st = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        for i, (conv, bn) in enumerate(names):
            L.check(self._lib.maua_resnet_conv_shape(self._net, i, C.byref(ci), C.byref(co), C.byref(k), C.byref(st)))
            w = torch.as_tensor(sd[conv + ".weight"]).detach().cpu()
            if tuple(w.shape) != (co.value, ci.value, k.value, k.value):
                raise ValueError(f"{conv}.weight: shape {tuple(w.shape)}, the network has {(co.value, ci.value, k.value, k.value)}")
            wf, bf = fold_bn(w, *(torch.as_tensor(sd[f"{bn}.{p}"]).detach().cpu() for p in ("weight", "bias", "running_mean", "running_var")))
            L.check(self._lib.maua_resnet_load(self._net, i, 0, L.ptr(wf), wf.numel()))
            L.check(self._lib.maua_resnet_load(self._net, i, 1, L.ptr(bf), bf.numel()))

    def _backbone(self, x):
        x = L.dev_tensor(x, torch.float32)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"ResNetFeatures: images must be [B, 3, H, W], got {tuple(x.shape)}")
        B, _, H, W = map(int, x.shape)
        out = torch.empty((B, self.out_dim), dtype=torch.float32, device=x.device)
        L.ctx(x.device)      # (binds the context to torch's current stream)
        L.check(self._lib.maua_resnet_forward(self._net, L.ptr(x), B, H, W, L.ptr(out)))
        self._B, self._device = B, x.device
        return out

    @torch.no_grad()
    def forward(self, inputs):
        """A [B, 3, H, W] tensor, or a list of them grouped by consecutive equal width (swav.py:314-332) -> float32 [B, 32 * width]."""
        if not isinstance(inputs, (list, tuple)):
            return self._backbone(inputs)
        widths = [int(t.shape[-1]) for t in inputs]
        outs, start = [], 0
        for end in range(1, len(inputs) + 1):
            if end == len(inputs) or widths[end] != widths[start]:
                outs.append(self._backbone(torch.cat([L.dev_tensor(t, torch.float32) for t in inputs[start:end]])))
                start = end
        return torch.cat(outs)

    __call__ = forward

    def tap(self, stage):
        """Stage ``stage`` of the last backbone run (0 stem, 1 max-pool, 2 .. 5 layer1 .. layer4) -> float32 [B, C, h, w]."""
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        L.check(self._lib.maua_resnet_tap_shape(self._net, int(stage), C.byref(c), C.byref(h), C.byref(w)))
        out = torch.empty((self._B, c.value, h.value, w.value), dtype=torch.float32, device=self._device)
        L.check(self._lib.maua_resnet_tap(self._net, int(stage), L.ptr(out)))
        return out


class SwAV(ResNetFeatures):
    """swav.py:349-354 ``SwAV()``: ResNet-50 with the SwAV weights, read from ``checkpoint`` (a local file; nothing is fetched)."""

    def __init__(self, checkpoint, dtype=torch.float32, allow_random_init=False, generator=None):
        if str(checkpoint) == "random":
            if not allow_random_init:
                raise FileNotFoundError("SwAV: no checkpoint given; the weights (swav_800ep_pretrain.pth.tar) are not bundled and are never "
                                        "downloaded - pass a local file, or allow_random_init=True for the reference's initialisation")
            sd = None
        else:
            from .load import load_state_dict_file
            sd = load_state_dict_file(checkpoint)
        super().__init__((3, 4, 6, 3), 64, dtype, sd, generator)
