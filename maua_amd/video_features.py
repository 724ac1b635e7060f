"""Per-frame visual features on the device (drop-in for maua/audiovisual/audioreactive/selfsupervised/features/video.py:12-75).

``VideoAnalyzer`` takes the frames batch by batch, as the render loop holds them (packed uint8 HWC), and keeps the features of the
stream on the device: one C-ABI call per batch (maua_vfeat_push, csrc/video_features.hip), nothing goes through the host.  The
reference's function names take a whole ``video`` tensor [T, 3, H, W] in [0, 1] and run it through the same analyser.

Not built (each raises ``NotImplementedError`` by name): the features that go through ``cv2.linearPolar`` (fft, video_spectrogram, the
``*_freq_rms`` family, video_spectral_onsets) and the ones on Farneback flow at winsize 25 / poly_n 25 (optical_flow_cpu, directogram,
video_flow_onsets; the library's estimator, flow.Farneback, is built for 15 / 7).  HSV follows kornia.color.rgb_to_hsv's published form;
parity with a kornia install is unpinned.
"""
import ctypes as C

import torch

from . import _lib as L

CHANNELS = ("r", "g", "b", "h", "s", "v")


def layout_of(frames, H, W):
    """The C ABI's layout id of a batch of frames [b, ...] for an H x W analyser: uint8 HWC, uint8 planar CHW or float32 planar CHW."""
    shape = tuple(frames.shape[1:])
    if frames.dtype == torch.uint8 and shape == (H, W, 3):
        return L.VFEAT_LAYOUTS["u8_hwc"]
    if frames.dtype == torch.uint8 and shape == (3, H, W):
        return L.VFEAT_LAYOUTS["u8_chw"]
    if frames.dtype == torch.float32 and shape == (3, H, W):
        return L.VFEAT_LAYOUTS["f32_chw"]
    raise ValueError(f"VideoAnalyzer: frames of dtype {frames.dtype} and shape {tuple(frames.shape)} are neither uint8 [b, {H}, {W}, 3], "
                     f"uint8 [b, 3, {H}, {W}] nor float32 [b, 3, {H}, {W}]")


def check_push(H, W, bins, max_batch, layout, B):
    """maua_vfeat_push's refusals for such a plan and batch, without a device (maua_vfeat_check): raises MauaHipError with the launcher's own
    message.  Pointers are only checked for NULL, so any non-NULL value stands for them."""
    one = 256
    L.check(L.lib().maua_vfeat_check(None, int(H), int(W), int(bins), int(max_batch), one, int(layout), int(B), one, None, one, one))


def assemble_absdiff(diff):
    """video.py:66-75 from the per-frame differences of a stream: diff[t] = sum |frame[t] - frame[t - 1]| (diff[0] = 0) ->
    absdiff [T, 1] = the T - 1 differences with the last one repeated."""
    if diff.shape[0] < 2:
        raise ValueError("absdiff needs at least two frames")   # (the reference fails on y[-1] of an empty list)
    return torch.cat((diff[1:], diff[-1:])).unsqueeze(-1)


class VideoAnalyzer:
    """The features of a stream of H x W frames.  ``push(frames)`` any number of times (uint8 [b, H, W, 3], uint8 [b, 3, H, W] or float32
    [b, 3, H, W] in [0, 1]; one layout per stream), ``features()`` for what has been pushed since the last ``reset()``."""

    def __init__(self, H, W, bins=32, max_batch=64, device=None):
        L.require_device()
        self.device = torch.device("cuda" if device is None else device)
        self.H, self.W, self.bins, self.max_batch = int(H), int(W), int(bins), int(max_batch)
        self._h = C.c_void_p()
        L.check(L.lib().maua_vfeat_create(L.ctx(self.device), self.H, self.W, self.bins, self.max_batch, C.byref(self._h)))
        self._out = []

    def push_raw(self, frames, hist, counts, variance, diff, layout=None):
        """One maua_vfeat_push into caller-owned outputs (hist [b, 6, bins] f32, counts [b, 6, bins] i32 or None, variance [b], diff [b])."""
        layout = layout_of(frames, self.H, self.W) if layout is None else layout
        L.check(L.lib().maua_vfeat_push(self._h, L.ctx(frames.device), L.ptr(frames), layout, int(frames.shape[0]), self.H, self.W,
                                        L.ptr(hist), L.ptr(counts), L.ptr(variance), L.ptr(diff)))

    def push(self, frames):
        frames = L.dev_tensor(frames)
        layout = layout_of(frames, self.H, self.W)
        for i in range(0, frames.shape[0], self.max_batch):
            part = frames[i:i + self.max_batch]
            b = part.shape[0]
            hist = torch.empty((b, 6, self.bins), dtype=torch.float32, device=part.device)
            vd = torch.empty((2, b), dtype=torch.float32, device=part.device)
            self.push_raw(part, hist, None, vd[0], vd[1], layout)
            self._out.append((hist, vd))
        return self

    def reset(self):
        """Forget the stream: the features collected so far and the carried frame."""
        L.check(L.lib().maua_vfeat_reset(self._h))
        self._out = []

    def __len__(self):
        return sum(h.shape[0] for h, _ in self._out)

    def features(self):
        if not self._out:
            raise ValueError("VideoAnalyzer.features: nothing has been pushed")
        hist = torch.cat([h for h, _ in self._out])
        vd = torch.cat([v for _, v in self._out], dim=1)
        T = hist.shape[0]
        return {"rgb_hist": hist[:, :3].reshape(T, 3 * self.bins), "hsv_hist": hist[:, 3:].reshape(T, 3 * self.bins),
                "visual_variance": vd[0].unsqueeze(-1), "absdiff": assemble_absdiff(vd[1])}

    def close(self):
        if getattr(self, "_h", None):
            L.lib().maua_vfeat_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _analyse(video, bins, max_batch=64):
    if video.dim() != 4 or video.shape[1] != 3:
        raise ValueError(f"video must be [T, 3, H, W], got {tuple(video.shape)}")
    an = VideoAnalyzer(video.shape[2], video.shape[3], bins=bins, max_batch=max_batch)
    try:
        return an.push(video if video.dtype == torch.uint8 else video.float())
    except Exception:
        an.close()
        raise


def _hist(video, bins, channels):
    an = _analyse(video, bins)
    hist = torch.cat([h for h, _ in an._out])
    an.close()
    return hist[:, channels].reshape(hist.shape[0], -1)


def redogram(video, bins: int = 32):
    return _hist(video, bins, [0])


def greenogram(video, bins: int = 32):
    return _hist(video, bins, [1])


def blueogram(video, bins: int = 32):
    return _hist(video, bins, [2])


def rgb_hist(video, bins: int = 96):
    return _hist(video, bins // 3, [0, 1, 2])


def huestogram(video, bins: int = 32):
    return _hist(video, bins, [3])


def saturogram(video, bins: int = 32):
    return _hist(video, bins, [4])


def valueogram(video, bins: int = 32):
    return _hist(video, bins, [5])


def hsv_hist(video, bins: int = 96):
    return _hist(video, bins // 3, [3, 4, 5])


def visual_variance(video):
    an = _analyse(video, 1)
    out = torch.cat([v for _, v in an._out], dim=1)[0].unsqueeze(-1)
    an.close()
    return out


def absdiff(video, stride: int = 64):
    """``stride`` is the reference's chunk length (video.py:66-75): it changes nothing in the result and is ignored."""
    an = _analyse(video, 1)
    out = assemble_absdiff(torch.cat([v for _, v in an._out], dim=1)[1])
    an.close()
    return out


def _unbuilt(name, why):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"{name} is not built: {why}")
    fn.__name__ = name
    fn.__doc__ = f"Not built: {why}"
    return fn


_CV2 = ("it goes through cv2.linearPolar (features/video.py:89-98), which has no definition in this tree; the features that are built are "
        "rgb_hist, hsv_hist and their six channels, visual_variance and absdiff")
_FFT = ("it only feeds video_spectrogram (features/video.py:79-98), which goes through cv2.linearPolar and is not built; torch.fft.rfft2 is "
        "the whole of it")
_FLOW = ("it uses cv2.calcOpticalFlowFarneback at winsize=25, poly_n=25 (features/video.py:125-143); the library's estimator "
         "(maua_amd.flow.Farneback) is built for winsize=15, poly_n=7")
UNBUILT = {"fft": _FFT, "video_spectrogram": _CV2, "low_freq_rms": _CV2, "mid_freq_rms": _CV2, "high_freq_rms": _CV2, "adaptive_freq_rms": _CV2,
           "video_spectral_onsets": _CV2, "optical_flow_cpu": _FLOW, "directogram": _FLOW, "video_flow_onsets": _FLOW}
fft = _unbuilt("fft", _FFT)
video_spectrogram = _unbuilt("video_spectrogram", _CV2)
low_freq_rms = _unbuilt("low_freq_rms", _CV2)
mid_freq_rms = _unbuilt("mid_freq_rms", _CV2)
high_freq_rms = _unbuilt("high_freq_rms", _CV2)
adaptive_freq_rms = _unbuilt("adaptive_freq_rms", _CV2)
video_spectral_onsets = _unbuilt("video_spectral_onsets", _CV2)
optical_flow_cpu = _unbuilt("optical_flow_cpu", _FLOW)
directogram = _unbuilt("directogram", _FLOW)
video_flow_onsets = _unbuilt("video_flow_onsets", _FLOW)
