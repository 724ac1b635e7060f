"""A float64 CPU restatement of the SwAV ResNet bottleneck backbone (maua/GAN/metrics/extractors/swav.py ResNet.forward_backbone),
written from the architecture with torch.nn.functional: test infrastructure only.

  stem     ConstantPad2d(1, 0) + Conv2d(3, width, 7, stride 2, padding 2), BatchNorm (running statistics, eps 1e-5), ReLU
  pool     MaxPool2d(3, stride 2, padding 1)
  layerN   bottleneck blocks: 1x1 -> BN -> ReLU -> 3x3 (the layer's stride in its first block) -> BN -> ReLU -> 1x1 -> BN,
           plus the input (through a strided 1x1 + BN in a layer's first block), then ReLU
  features the mean over the pixels of layer4

``forward(sd, x, layers)`` takes the reference's state dict and returns the six taps (stem, pool, layer1 .. layer4) and the features.
``bf16=True`` instead evaluates what the library's bfloat16 path computes up to summation order: BatchNorm folded into weight and bias in
float64 and rounded to float32, the folded weight rounded to bfloat16, the image and every stored activation rounded to bfloat16, the sums
in float64 (so the only roundings are the ones the path is bound to make).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


def conv_names(layers):
    """[(conv prefix, bn prefix, Ci, Co, k)] in the state dict's order (width 64)."""
    out = [("conv1", "bn1", 3, 64, 7)]
    inplanes = 64
    for l, blocks in enumerate(layers):
        planes = 64 << l
        for b in range(blocks):
            p = f"layer{l + 1}.{b}."
            out += [(p + "conv1", p + "bn1", inplanes, planes, 1), (p + "conv2", p + "bn2", planes, planes, 3),
                    (p + "conv3", p + "bn3", planes, planes * 4, 1)]
            if b == 0:
                out.append((p + "downsample.0", p + "downsample.1", inplanes, planes * 4, 1))
            inplanes = planes * 4
    return out


def make_state_dict(seed, layers):
    """Kaiming-scaled (fan_out) weights and non-trivial BatchNorm statistics from np.random.RandomState(seed): gamma and the running
    variance uniform in [0.75, 1.25], beta and the running mean 0.1 N(0, 1).  float32 tensors under the reference's key names."""
    rs = np.random.RandomState(seed)
    sd = {}
    for conv, bn, ci, co, k in conv_names(layers):
        sd[conv + ".weight"] = torch.from_numpy((rs.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (co * k * k))).astype(np.float32))
        sd[bn + ".weight"] = torch.from_numpy(rs.uniform(0.75, 1.25, co).astype(np.float32))
        sd[bn + ".bias"] = torch.from_numpy((0.1 * rs.standard_normal(co)).astype(np.float32))
        sd[bn + ".running_mean"] = torch.from_numpy((0.1 * rs.standard_normal(co)).astype(np.float32))
        sd[bn + ".running_var"] = torch.from_numpy(rs.uniform(0.75, 1.25, co).astype(np.float32))
    return sd


def checksums(sd):
    """float64 sum of every tensor times a fixed ramp (position-sensitive) -> {key: float}.  math.fsum: the correctly rounded sum,
    whatever the order or the number of threads."""
    out = {}
    for k in sorted(sd):
        v = sd[k].double().reshape(-1).numpy()
        out[k] = math.fsum(v * (1.0 + np.arange(v.size, dtype=np.float64) / max(v.size, 1)))
    return out


def make_input(seed, shape):
    return torch.from_numpy(np.random.RandomState(seed).uniform(0.0, 1.0, shape).astype(np.float32))


def r16(t):
    """round to bfloat16 (nearest even), back in float64"""
    return t.float().bfloat16().double()


def forward(sd, x, layers, bf16=False, dtype=torch.float64):
    """-> ([stem, pool, layer1, layer2, layer3, layer4] [B, C, h, w], features [B, 2048]) in ``dtype`` (float32: the same operations in
    single precision - the reference network's own arithmetic; not with bf16)"""
    rnd = r16 if bf16 else (lambda t: t)
    assert dtype == torch.float64 or not bf16

    def conv_bn(t, conv, bn, stride, padding):
        w = sd[conv + ".weight"].to(dtype)
        g, b, m, v = (sd[f"{bn}.{p}"].to(dtype) for p in ("weight", "bias", "running_mean", "running_var"))
        if not bf16:
            return F.batch_norm(F.conv2d(t, w, None, stride, padding), m, v, g, b, False, 0.0, EPS)
        s = g / torch.sqrt(v + EPS)
        wf, bias = (w * s.reshape(-1, 1, 1, 1)).float(), (b - m * s).float()     # the fold, rounded once to float32
        return F.conv2d(t, r16(wf), bias.double(), stride, padding)

    t = F.pad(rnd(x.to(dtype)), (1, 1, 1, 1))
    stem = rnd(F.relu(conv_bn(t, "conv1", "bn1", 2, 2)))
    pool = F.max_pool2d(stem, 3, 2, 1)
    taps, t = [stem, pool], pool
    for l, blocks in enumerate(layers):
        for b in range(blocks):
            p = f"layer{l + 1}.{b}."
            stride = 2 if (l > 0 and b == 0) else 1
            o = rnd(F.relu(conv_bn(t, p + "conv1", p + "bn1", 1, 0)))
            o = rnd(F.relu(conv_bn(o, p + "conv2", p + "bn2", stride, 1)))
            o = conv_bn(o, p + "conv3", p + "bn3", 1, 0)
            idt = rnd(conv_bn(t, p + "downsample.0", p + "downsample.1", stride, 0)) if b == 0 else t
            t = rnd(F.relu(o + idt))
        taps.append(t)
    return taps, t.mean(dim=(2, 3))
