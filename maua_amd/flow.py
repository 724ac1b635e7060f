"""What the video pipeline uses of maua/flow/ (flow/__init__.py:9-64, flow/lib.py:18-80, flow/consistency.py:78-127) and the per-frame
operators of maua/diffusion/video.py:153-162, 221-277, each a library call (csrc/flow.hip).

Same names and arguments as the reference where it has them.  What differs, on purpose:
  * ``get_flow_model``: "farneback" only - and that estimator runs on the device, restated from the published algorithm (the
    reference calls ``cv2.calcOpticalFlowFarneback`` on the host; parity with OpenCV itself is unpinned).  The neural
    models (unflow, pwc, spynet, liteflownet, the mmflow names, deepflow2) need checkpoints and packages that are not part of this
    build and raise by name;
  * ``flow_warp_map`` does not divide its argument in place (not observable through the pipeline);
  * ``get_consistency_map``: the "full" mode (and the trivial "magnitude" / all-ones ones); "numpy" raises.
"""
import ctypes as C
import struct

import numpy as np
import torch

from . import _lib as L

SUPPORTED_FLOW_MODELS = ("farneback",)
INF = float("inf")


def _flow(t, name):
    t = L.dev_tensor(t, torch.float32)
    if t.dim() != 4 or t.shape[-1] != 2:
        raise ValueError(f"{name}: expected a [B, H, W, 2] flow, got {tuple(t.shape)}")
    return t


def _planar(x, name, channels=None):
    x = L.dev_tensor(x, torch.float32)
    if x.dim() != 4 or (channels is not None and x.shape[1] != channels):
        raise ValueError(f"{name}: expected a [B, {channels or 'C'}, H, W] image, got {tuple(x.shape)}")
    return x


# ------------------------------------------------------------------------------------------------------------------ mflo (host, numpy)
def encode_mflo(flow):
    """Optical flow encoding which can be saved as JPEG (flow/lib.py:18-34)."""
    absmax = np.max(np.abs(flow))  # find maximal flow magnitude
    one, two, three, four = struct.pack("!f", absmax)  # encode float32 value as 4 bytes

    # encode each byte into a quadrant of the image
    h, w, _ = flow.shape
    absmax_channel = np.zeros((h, w, 1), dtype=np.uint8)
    absmax_channel[: h // 2, : w // 2] = one
    absmax_channel[: h // 2, w // 2:] = two
    absmax_channel[h // 2:, : w // 2] = three
    absmax_channel[h // 2:, w // 2:] = four

    # normalize flow u,v components to range [0, 255]
    mflo = np.round((flow / absmax + 1) * 127.5).astype(np.uint8)
    mflo = np.concatenate((mflo, absmax_channel), axis=2)  # insert encoded magnitude to last channel
    return mflo


def decode_mflo(mflo):
    """flow/lib.py:37-48."""
    h, w, _ = mflo.shape
    absmax_channel = mflo[..., 2]
    one = np.mean(absmax_channel[: h // 2, : w // 2].astype(np.float32)).round().astype(np.uint8)
    two = np.mean(absmax_channel[: h // 2, w // 2:].astype(np.float32)).round().astype(np.uint8)
    three = np.mean(absmax_channel[h // 2:, : w // 2].astype(np.float32)).round().astype(np.uint8)
    four = np.mean(absmax_channel[h // 2:, w // 2:].astype(np.float32)).round().astype(np.uint8)
    (absmax,) = struct.unpack("!f", bytearray([one, two, three, four]))

    flow = mflo[..., :2]
    flow = (flow.astype(np.float32) / 127.5 - 1) * absmax
    return flow


# ------------------------------------------------------------------------------------------------------------------ warp
def flow_warp_map(flow: torch.Tensor) -> torch.Tensor:
    """flow/lib.py:51-63: the sampling grid [B, H, W, 2] of a flow, for callers that want it (``warp_flow`` and the composition do not
    materialise it).  Plain torch arithmetic on the flow's device."""
    b, h, w, two = flow.shape
    neutral = torch.stack(torch.meshgrid(torch.linspace(-1, 1, w), torch.linspace(-1, 1, h), indexing="xy"), axis=2).unsqueeze(0).to(flow)
    return neutral + torch.stack((flow[..., 0] / w, flow[..., 1] / h), dim=-1)


def warp_flow(x, flow, flow_exaggeration=1.0, out=None):
    """``warp(x, flow_warp_map(flow * flow_exaggeration))`` (diffusion/video.py:225-230, :260-263) in one launch."""
    x, f = _planar(x, "warp_flow"), _flow(flow, "warp_flow")
    B, Cn, H, W = x.shape
    if tuple(f.shape) != (B, H, W, 2):
        raise ValueError(f"warp_flow: flow {tuple(f.shape)} does not match the image {tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    L.check(L.lib().maua_flow_warp(L.ctx(x.device), L.ptr(x), L.ptr(f), flow_exaggeration, B, Cn, H, W, L.ptr(out)))
    return out


def warp(x, f):
    """diffusion/video.py:161-162 for a grid that came from ``flow_warp_map``: the flow is recovered from the grid (grid - neutral, times
    W and H) and the library's warp runs.  The pipeline itself calls ``warp_flow``."""
    b, h, w, _ = f.shape
    neutral = torch.stack(torch.meshgrid(torch.linspace(-1, 1, w), torch.linspace(-1, 1, h), indexing="xy"), axis=2).unsqueeze(0).to(f)
    d = f - neutral
    return warp_flow(x, torch.stack((d[..., 0] * w, d[..., 1] * h), dim=-1))


# ------------------------------------------------------------------------------------------------------------------ consistency
def check_consistency(flow_forward, flow_backward, clamp=INF, out=None):
    """flow/consistency.py:85-127 -> [B, H, W] (the reference: one pair, [1, H, W]).  ``clamp``: the flows are read clamped to +-clamp
    (diffusion/video.py:148-149).  Two launches: classify, blur and clip."""
    ff, fb = _flow(flow_forward, "check_consistency"), _flow(flow_backward, "check_consistency")
    if ff.shape != fb.shape:
        raise ValueError("check_consistency: the two flows differ in shape")
    B, H, W, _ = ff.shape
    buf = torch.empty((2, B, H, W), dtype=torch.float32, device=ff.device) if out is None else None
    classes, res = (buf[0], buf[1]) if out is None else out
    L.check(L.lib().maua_flow_consistency(L.ctx(ff.device), L.ptr(ff), L.ptr(fb), B, H, W, clamp, L.ptr(classes), L.ptr(res)))
    return res


def get_consistency_map(forward_flow, backward_flow, consistency="full"):
    """flow/lib.py:66-80."""
    if consistency == "magnitude":
        reliable_flow = torch.sqrt(forward_flow[..., 0] ** 2 + forward_flow[..., 1] ** 2)
    elif consistency == "full":
        reliable_flow = check_consistency(forward_flow, backward_flow)
    elif consistency == "numpy":
        raise NotImplementedError('get_consistency_map(consistency="numpy"): the host restatement (check_consistency_np) is not built; use "full"')
    else:
        reliable_flow = torch.ones((forward_flow.shape[0], forward_flow.shape[1]))
    return reliable_flow


def resize_bilinear(x, size, multiplier=1.0, clamp=INF, out=None):
    """``interpolate(clamp(x, +-clamp), size, mode="bilinear") * multiplier`` of a channels-last tensor [B, H, W, C] (flows) or [B, H, W]
    (consistency maps) -> [B, size[0], size[1], C] / [B, size[0], size[1]] (diffusion/video.py:149-157)."""
    x = L.dev_tensor(x, torch.float32)
    squeeze = x.dim() == 3
    if squeeze:
        x = x.unsqueeze(-1)
    if x.dim() != 4:
        raise ValueError(f"resize_bilinear: expected [B, H, W, C] or [B, H, W], got {tuple(x.shape)}")
    B, H, W, Cn = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((B, Ho, Wo, Cn), dtype=torch.float32, device=x.device)
    L.check(L.lib().maua_flow_resize_bilinear(L.ctx(x.device), L.ptr(x), B, H, W, Cn, L.ptr(out), Ho, Wo, multiplier, clamp))
    return out.squeeze(-1) if squeeze else out


# ------------------------------------------------------------------------------------------------------------------ composition
def draw_noise_key():
    """The Philox key of one frame's injected noise: one ``torch.randint`` draw from torch's host generator, so ``seed_everything`` /
    ``torch.manual_seed`` repeats it (the match_histogram precedent)."""
    return int(torch.randint(0, 2 ** 62, ()))


def compose(frame, prev=None, flow=None, consistency=None, cached=None, flow_exaggeration=1.0, consistency_trust=0.75, blend=2.0, fade=1.0,
            noise_injection=0.0, seed=0, out=None):
    """diffusion/video.py:248-277 in one launch: ``(frame + mask * warp(prev)) / (1 + mask)`` with ``mask = (consistency * trust + 1 -
    trust) * blend`` (``consistency=None``: ``blend``), then ``fade * init + (1 - fade) * cached`` when ``cached`` is given, then
    ``+ noise_injection * N(0, 1)`` from stream 0 of Philox key ``seed`` (element i of the image = element i of the stream; the
    reference's ``randn_like`` values are not reproduced).  ``prev=None``: no blend (the noise step alone, with ``cached=None``)."""
    x = _planar(frame, "compose", 3)
    B, _, H, W = x.shape
    same = lambda t, name: None if t is None else _planar(t, name, 3)
    prev, cached = same(prev, "compose prev"), same(cached, "compose cached")
    for t in (prev, cached):
        if t is not None and t.shape != x.shape:
            raise ValueError("compose: prev / cached must have the frame's shape")
    if prev is not None:
        flow = _flow(flow, "compose")
        if tuple(flow.shape) != (B, H, W, 2):
            raise ValueError(f"compose: flow {tuple(flow.shape)} does not match the frame {tuple(x.shape)}")
        if consistency is not None:
            consistency = L.dev_tensor(consistency, torch.float32)
            if consistency.numel() != B * H * W:
                raise ValueError("compose: consistency must hold one value per pixel")
    else:
        flow = consistency = None
    if out is None:
        out = torch.empty_like(x)
    L.check(L.lib().maua_flow_compose(L.ctx(x.device), L.ptr(x), L.ptr(prev), L.ptr(flow), L.ptr(consistency), L.ptr(cached), B, H, W,
                                      flow_exaggeration, consistency_trust, blend, fade,
                                      noise_injection, int(seed), L.ptr(out)))
    return out


def turbo_step(prev, nxt, flow, flow_exaggeration, warp_next, blend_t, out=None):
    """One skipped frame of diffusion/video.py:224-237 in one launch -> (warped prev or None, next - warped when ``warp_next`` -, img).
    ``out``: (prev_out, next_out, img) tensors of the caller's to write (the first two as far as they are produced)."""
    nxt, f = _planar(nxt, "turbo_step", 3), _flow(flow, "turbo_step")
    B, _, H, W = nxt.shape
    prev = None if prev is None else _planar(prev, "turbo_step", 3)
    new = lambda i: torch.empty_like(nxt) if out is None else out[i]
    prev_out = new(0) if prev is not None else None
    next_out = new(1) if warp_next else None
    img = new(2)
    L.check(L.lib().maua_flow_turbo(L.ctx(nxt.device), L.ptr(prev), L.ptr(nxt), L.ptr(f), B, H, W, flow_exaggeration, int(bool(warp_next)),
                                    blend_t, L.ptr(prev_out), L.ptr(next_out), L.ptr(img)))
    return prev_out, (next_out if warp_next else nxt), img


# ------------------------------------------------------------------------------------------------------------------ Farneback
class Farneback:
    """A handle on the estimator's workspace, planned for images up to ``max_height`` x ``max_width`` (csrc/flow.hip)."""

    def __init__(self, max_height, max_width, device=None):
        L.require_device()
        self.device = torch.device("cuda" if device is None else device)
        self.max_height, self.max_width = int(max_height), int(max_width)
        self._h = C.c_void_p()
        L.check(L.lib().maua_farneback_create(L.ctx(self.device), self.max_height, self.max_width, C.byref(self._h)))

    def pair(self, im_a, im_b):
        """im_a / im_b [3, H, W] or [1, 3, H, W] in [0, 1] -> (flow(a -> b), flow(b -> a)), [1, H, W, 2] each: both directions batched."""
        a, b = (L.dev_tensor(t, torch.float32).reshape(3, *t.shape[-2:]) for t in (im_a, im_b))
        if a.shape != b.shape:
            raise ValueError("Farneback.pair: the two images differ in shape")
        H, W = int(a.shape[1]), int(a.shape[2])
        out = torch.empty((2, 1, H, W, 2), dtype=torch.float32, device=a.device)
        L.check(L.lib().maua_farneback_pair(self._h, L.ctx(a.device), L.ptr(a), L.ptr(b), H, W, L.ptr(out[0]), L.ptr(out[1])))
        return out[0], out[1]

    def pair_ex(self, im_a, im_b, height, width, flow_ab, flow_ba, level_hi=-1, level_lo=-1, iterations=0, init_ab=None, init_ba=None,
                **dumps):
        """maua_farneback_pair_ex for the parity tests: every argument a device address (an integer; 0 or None: absent) of a buffer
        of the caller's, ``dumps`` any of gray / blur / level / coef / flow_in / mat (include/maua_hip.h: maua_farneback_desc)."""
        d = farneback_desc(im_a, im_b, height, width, flow_ab, flow_ba, level_hi, level_lo, iterations, init_ab, init_ba, **dumps)
        L.check(L.lib().maua_farneback_pair_ex(self._h, L.ctx(self.device), C.byref(d)))

    def __call__(self, im1, im2):
        return self.pair(im1, im2)[0]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            L.lib().maua_farneback_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def farneback_desc(im_a, im_b, height, width, flow_ab, flow_ba, level_hi=-1, level_lo=-1, iterations=0, init_ab=None, init_ba=None, **dumps):
    """A maua_farneback_desc from device addresses (integers; 0 or None: absent)."""
    d = L.FbDesc(im_a=im_a or None, im_b=im_b or None, H=int(height), W=int(width), flow_ab=flow_ab or None, flow_ba=flow_ba or None,
                 level_hi=int(level_hi), level_lo=int(level_lo), iterations=int(iterations), init_ab=init_ab or None, init_ba=init_ba or None)
    for k, v in dumps.items():
        if k not in ("gray", "blur", "level", "coef", "flow_in", "mat"):
            raise ValueError(f"farneback_desc: no dump named {k}")
        setattr(d, k, v or None)
    return d


def farneback_check(desc, handle=None):
    """maua_farneback_check (host only): None, or the launcher's own refusal.  Without a handle the descriptor alone is checked."""
    if L.lib().maua_farneback_check(None if handle is None else handle._h, C.byref(desc)) != 0:
        return L.lib().maua_last_error().decode()
    return None


def farneback_level_size(height, width, level):
    """(rows, cols) of pyramid level ``level`` of a height x width pair (host arithmetic of the library)."""
    h, w = C.c_int(), C.c_int()
    L.check(L.lib().maua_farneback_level_size(int(height), int(width), int(level), C.byref(h), C.byref(w)))
    return h.value, w.value


def farneback_levels(height, width):
    """The number of pyramid levels an image pair of this size is processed at (host arithmetic of the library)."""
    return int(L.lib().maua_farneback_levels(int(height), int(width)))


class FlowModel:
    """What ``get_flow_model`` returns: ``model(im1, im2)`` -> [1, H, W, 2] (flow/__init__.py:64), and ``model.pair(im1, im2)`` for both
    directions in one batched pass.  The workspace grows to the largest image seen."""

    def __init__(self):
        self._fb = None

    def _handle(self, H, W, device):
        if self._fb is None or H * W > self._fb.max_height * self._fb.max_width or self._fb.device != torch.device(device):
            if self._fb is not None:
                self._fb.close()
            self._fb = Farneback(H, W, device)
        return self._fb

    def pair(self, im1, im2):
        im1 = L.dev_tensor(im1, torch.float32)
        return self._handle(im1.shape[-2], im1.shape[-1], im1.device).pair(im1, im2)

    def __call__(self, im1, im2):
        return self.pair(im1, im2)[0]


def get_flow_model(which=["farneback"]):
    """flow/__init__.py:9-64 for the reference's default list."""
    which = [which] if isinstance(which, str) else list(which)
    for w in which:
        if w not in SUPPORTED_FLOW_MODELS:
            raise NotImplementedError(f'flow model "{w}" is not built (its checkpoint and package are not part of this build); the models are: '
                                      f'{list(SUPPORTED_FLOW_MODELS)}')
    if not which:
        raise ValueError("get_flow_model: no model named")
    return FlowModel()
