"""Generate the golden fixtures under tests/golden/ by IMPORTING the reference.

Runs only in the authoring container (needs /root/reference; the GPU box only
consumes the committed .npz files).  This script contains no reference code: it
imports ``maua`` from /root/reference, calls its functions on seeded inputs and
stores inputs + outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

Third-party modules the reference imports at module scope but that are absent
here (librosa, torchaudio, torchcubicspline, ...) are replaced by MagicMock
stubs; none of the functions captured below calls into them.  The reference's
only native file (efficient_quantile.cpp) is compiled from where it lies into
oracle/_ref/ (see oracle/build_ref.py) and registered under its import name.
"""
import importlib.abc
import importlib.machinery
import os
import sys
from math import sqrt
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
REF = "/root/reference"
sys.path.insert(0, str(REPO))

ABSENT = {"librosa", "madmom", "torchaudio", "openunmix", "torchcubicspline", "torchtyping", "torch_geometric",
          "kornia", "cv2", "resampy", "soundfile", "ffmpeg", "decord", "npy_append_array", "fire", "numba",
          "matplotlib", "sklearn", "joblib", "resize_right", "medpy", "torchvision", "PIL", "glumpy", "pycuda", "clip", "lpips",
          "gdown"}


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.startswith("maua.GAN.nv") or name.startswith("maua.submodules"):  # un-vendored git submodules (empty directories in the reference tree)
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        if name.split(".")[0] in ABSENT:
            try:  # prefer the real module when the image has it
                for f in sys.meta_path:
                    if f is self:
                        continue
                    s = f.find_spec(name, path, target) if hasattr(f, "find_spec") else None
                    if s is not None:
                        return s
            except Exception:
                pass
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = MagicMock(name=spec.name)
        m.__path__ = []
        m.__name__ = spec.name
        m.__spec__ = spec
        return m

    def exec_module(self, module):
        pass


def import_reference():
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, REF)
    from oracle.build_ref import load_reference_quantile
    ext = load_reference_quantile()
    sys.modules[
        "maua.audiovisual.audioreactive.selfsupervised.features.efficient_quantile.efficient_quantile"] = ext


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = HERE / f"{name}.npz"
    np.savez_compressed(path, **out)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB  {len(out)} arrays")


T = torch.tensor


# --------------------------------------------------------------------------------------- ops
def golden_ops():
    from maua.GAN.wrappers.inference import ops as R

    g = torch.Generator().manual_seed(100)
    f = R.setup_filter([1, 3, 3, 1])
    save("g01_setup_filter", f=f)

    # G2 bias_act
    x = torch.randn(2, 8, 16, 16, generator=g) * 3
    b = torch.randn(8, generator=g)
    out = {"x": x, "b": b}
    for act in ["linear", "lrelu"]:
        for gi, gain in enumerate([1.0, sqrt(2)]):
            for ci, clamp in enumerate([None, 2.5]):
                y = R.bias_act(x, b, act=act, gain=T(gain), clamp=None if clamp is None else T(clamp))
                out[f"y_{act}_g{gi}_c{ci}"] = y
    out["y_relu_default"] = R.bias_act(x, b, act="relu")
    out["y_sigmoid_nobias"] = R.bias_act(x, None, act="sigmoid")
    out["y_tanh"] = R.bias_act(x, b, act="tanh")
    out["y_swish"] = R.bias_act(x, b, act="swish")
    out["y_lrelu_clamp256"] = R.bias_act(x * 100, b, act="lrelu", gain=T(sqrt(2)), clamp=T(256.0))
    save("g02_bias_act", **out)

    # G3 upfirdn2d
    x = torch.randn(2, 3, 8, 8, generator=g)
    y_up = R.upfirdn2d(x, f, up=T(2), padding=T([2, 1, 2, 1]), gain=T(4))
    x17 = torch.randn(2, 4, 17, 17, generator=g)
    y_fir = R.upfirdn2d(x17, f, padding=T([1, 1, 1, 1]), gain=T(4))
    y_down = R.upfirdn2d(x, f, down=T(2), padding=T([1, 1, 1, 1]))
    y_crop = R.upfirdn2d(x, f, padding=T([2, -1, -1, 3]))
    xr = torch.randn(1, 2, 5, 9, generator=g)
    y_rect = R.upfirdn2d(xr, f, up=T(2), padding=T([2, 1, 2, 1]), gain=T(4))
    save("g03_upfirdn2d", f=f, x=x, y_up=y_up, x17=x17, y_fir=y_fir, y_down=y_down, y_crop=y_crop, xr=xr,
         y_rect=y_rect)

    # G4 upsample2d
    x = torch.randn(2, 3, 8, 8, generator=g)
    save("g04_upsample2d", f=f, x=x, y=R.upsample2d(x, f))

    # G5 modulated_conv2d up=1
    x = torch.randn(2, 8, 12, 12, generator=g)
    w3 = torch.randn(6, 8, 3, 3, generator=g)
    s = torch.randn(2, 8, generator=g) + 1
    nz = torch.randn(2, 1, 12, 12, generator=g)
    y_demod = R.modulated_conv2d(x, w3, s, noise=nz, up=T(1), padding=T(1))
    y_demod_nonoise = R.modulated_conv2d(x, w3, s, up=T(1), padding=T(1))
    w1 = torch.randn(3, 8, 1, 1, generator=g)
    y_1x1 = R.modulated_conv2d(x, w1, s, demodulate=False)
    save("g05_modconv_up1", x=x, w3=w3, s=s, noise=nz, y_demod=y_demod, y_demod_nonoise=y_demod_nonoise, w1=w1,
         y_1x1=y_1x1)

    # G6 up=2 composition (Q1): the in-tree branch ops.py:211-225 cannot execute (torch.max(t, 0) namedtuple),
    # so compose the same calls by hand: weight regroup (:215-217), conv_transpose2d stride 2 pad 0 (:224),
    # reference upfirdn2d with padding (1,1,1,1) and gain 4 (:225).
    B, ci, co, h = 2, 8, 4, 8
    x = torch.randn(B, ci, h, h, generator=g)
    w3 = torch.randn(co, ci, 3, 3, generator=g)
    s = torch.randn(B, ci, generator=g) + 1
    nz = torch.randn(B, 1, 2 * h, 2 * h, generator=g)
    w = w3.unsqueeze(0) * s[:, None, :, None, None]
    w = w / ((w * w).sum((2, 3, 4)) + 1e-8).sqrt()[..., None, None, None]
    wg = w.reshape(B * co, ci, 3, 3).reshape(B, co, ci, 3, 3).permute(0, 2, 1, 3, 4).reshape(B * ci, co, 3, 3)
    t = torch.nn.functional.conv_transpose2d(x.reshape(1, B * ci, h, h), wg, stride=2, padding=0, groups=B)
    y = R.upfirdn2d(t, f, padding=T([1, 1, 1, 1]), gain=T(4)).reshape(B, co, 2 * h, 2 * h) + nz
    save("g06_modconv_up2", x=x, w3=w3, s=s, noise=nz, f=f, y=y)

    # G7 normalize_2nd_moment
    z = torch.randn(4, 16, generator=g)
    save("g07_norm2nd", z=z, y=R.normalize_2nd_moment(z))


# --------------------------------------------------------------------------------------- modules
def golden_modules():
    from maua.GAN.wrappers.inference import stylegan2 as S

    # FullyConnectedLayer linear + MappingNetwork (small) incl. truncation
    torch.manual_seed(7)
    fc = S.FullyConnectedLayer(16, 24, bias_init=1)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 16, generator=g)
    save("g07_fc_linear", x=x, weight=fc.weight, bias=fc.bias, y=fc(x))

    torch.manual_seed(9)
    m = S.MappingNetwork(16, 0, 16, 6, num_layers=2)
    m.w_avg.copy_(torch.randn(16, generator=g))
    z = torch.randn(5, 16, generator=g)
    sd = {k: v for k, v in m.state_dict().items()}
    save("g07_mapping", z=z, y_psi1=m(z, None), y_psi07=m(z, None, truncation_psi=0.7),
         y_cut2=m(z, None, truncation_psi=0.5, truncation_cutoff=2), **{k.replace(".", "__"): v for k, v in sd.items()})

    # full-size mapping init parity: seed -> state dict checksum + a forward
    torch.manual_seed(11)
    m = S.MappingNetwork(512, 0, 512, 18)
    z = torch.randn(2, 512, generator=g)
    w = m(z, None)
    save("g07_mapping512", z=z, w=w[:, 0], w0_sum=np.float64(m.fcs[0].weight.double().sum().item()),
         w7_sum=np.float64(m.fcs[7].weight.double().sum().item()))

    # G8 SynthesisLayer up=1 + ToRGBLayer with exported params
    torch.manual_seed(12)
    lay = S.SynthesisLayer(8, 6, w_dim=16, resolution=12, conv_clamp=256.0)
    lay.padding = T(1)
    lay.up = T(1)
    lay.bias.data.copy_(torch.randn(6, generator=g))
    x = torch.randn(2, 8, 12, 12, generator=g)
    w = torch.randn(2, 16, generator=g)
    y = lay(x, w)
    save("g08_synth_layer", x=x, w=w, y=y, **{k.replace(".", "__"): v for k, v in lay.state_dict().items()})

    torch.manual_seed(13)
    rgb = S.ToRGBLayer(8, 3, w_dim=16, conv_clamp=256.0)
    rgb.bias.data.copy_(torch.randn(3, generator=g))
    y = rgb(x, w)
    save("g08_torgb", x=x, w=w, y=y, **{k.replace(".", "__"): v for k, v in rgb.state_dict().items()})

    # constructor draw order: reference SynthesisNetwork(16, 32, 3, channel_base=256, channel_max=16) under a seed
    torch.manual_seed(21)
    net = S.SynthesisNetwork(w_dim=16, img_resolution=32, img_channels=3, channel_base=256, channel_max=16)
    sd = net.state_dict()
    save("g08_synth_init", **{k.replace(".", "__"): v for k, v in sd.items()})
    torch.manual_seed(22)
    net = S.SynthesisNetwork(w_dim=512, img_resolution=1024, img_channels=3)
    sums = {k.replace(".", "__"): np.float64(v.double().sum().item()) for k, v in net.state_dict().items()}
    sums["num_ws"] = np.int64(net.num_ws)
    save("g08_synth_init1024_sums", **sums)


# --------------------------------------------------------------------------------------- audio
def synth_audio(n, sr, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / sr
    u = torch.rand(n, generator=g, dtype=torch.float64)
    nz = torch.randn(n, generator=g, dtype=torch.float64)
    click = ((2 * t) % 1 < 0.05).double()
    a = 0.3 * torch.sin(2 * np.pi * 220 * t) + 0.2 * (u - 0.5) * click + 0.01 * nz
    return a.float()


def golden_audio():
    from maua.audiovisual.audioreactive.selfsupervised.features import audio as FA
    from maua.audiovisual.audioreactive.selfsupervised.features import processing as FP
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import beat, convert, spectral
    from maua.audiovisual.audioreactive.selfsupervised.features.efficient_quantile import quantile

    sr = 30720
    a = synth_audio(4 * sr, sr, 1234)  # 4 s -> 120 frames
    D = spectral.stft(a)
    S1 = spectral.spectrogram(a, power=1)
    basis = spectral.mel(sr, 2048, fmax=11025.0)
    M = spectral.melspectrogram(a, sr, fmax=11025.0)
    db = convert.power_to_db(M)
    env = beat.onset_strength(a, sr)
    # keep fixtures small: store audio as f32 (480 KB) once, spectra as column samples
    cols = np.array([0, 1, 2, 17, 59, 118, 119, 120])
    save("g09_audio_clip", audio=a, sr=np.int64(sr))
    save("g09_stft", cols=cols, D_re=D.real[:, cols], D_im=D.imag[:, cols], n_cols=np.int64(D.shape[1]),
         S1_cols=S1[:, cols[:-1]], S1_shape=np.array(S1.shape))
    save("g09_mel", basis_rowsum=basis.sum(1), basis_colsum=basis.sum(0), basis_rows=basis[[0, 1, 63, 127]],
         M_cols=M[:, cols[:-1]], db_cols=db[:, cols[:-1]], db_max=db.max(), env=env,
         mel_f=spectral.mel_frequencies(130, fmin=0.0, fmax=11025.0))

    # G10 hpss + istft, 1 s clip
    a1 = a[:sr].contiguous()
    D1 = spectral.stft(a1)
    Hh, Hp = spectral.hpss(D1, margin=8.0)
    H1, P1 = spectral.hpss(D1, margin=1.0)
    perc = FA.percussive(a1)
    harm = FA.harmonic(a1)
    mag = D1.abs()
    med_t = FP.median_filter2d(mag[None, None], k=(1, 31), p=(15, 15, 0, 0)).squeeze()
    med_f = FP.median_filter2d(mag[None, None], k=(31, 1), p=(0, 0, 15, 15)).squeeze()
    save("g10_hpss", n=np.int64(sr), med_t=med_t.half(), med_f=med_f.half(), med_t_f32_cols=med_t[:, [0, 7, 30]],
         med_f_f32_cols=med_f[:, [0, 7, 30]], Hp_re=Hp.real[:, [0, 7, 30]], Hp_im=Hp.imag[:, [0, 7, 30]],
         Hh_re=Hh.real[:, [0, 7, 30]], Hh_im=Hh.imag[:, [0, 7, 30]], P1_re=P1.real[:, [0, 7, 30]],
         H1_re=H1.real[:, [0, 7, 30]], perc=perc, harm=harm)
    ons = FA.onsets(a, sr)
    rms = FA.rms(a, sr)
    save("g10_onsets_rms", onsets=ons, rms=rms)

    # G11 envelope post-processing
    g = torch.Generator().manual_seed(5)
    e = torch.rand(200, generator=g)
    e2 = torch.rand(200, 3, generator=g)
    e4 = torch.rand(40, 2, 3, 4, generator=g)
    short = torch.rand(6, 2, generator=g)
    out = {"e": e, "e2": e2, "e4": e4, "short": short}
    for sg in [1, 2, 5]:
        out[f"p_circ_s{sg}"] = FP.gaussian_filter(e, sg)
        out[f"p_refl_s{sg}"] = FP.gaussian_filter(e, sg, mode="reflect")
    out["p_2d_s2"] = FP.gaussian_filter(e2, 2)
    out["p_4d_s1"] = FP.gaussian_filter(e4, 1)
    import io, contextlib
    with contextlib.redirect_stdout(io.StringIO()):
        out["p_short_s2"] = FP.gaussian_filter(short, 2)  # radius 8 > n_frames 6 -> fallback branch
    out["p_normalize"] = FP.normalize(e2)
    out["p_standardize"] = FP.standardize(e)
    qs = [0.025, 0.25, 0.5, 0.75, 0.975]
    big = torch.randn(100001, generator=g)
    out["q_small"] = np.array([quantile(e, q).item() for q in qs], dtype=np.float32)
    out["q_big"] = np.array([quantile(big, q).item() for q in qs], dtype=np.float32)
    out["big_seed_check"] = big[:4]
    withnan = e.clone()
    withnan[::7] = float("nan")
    out["q_nan"] = np.array([quantile(withnan, q).item() for q in qs], dtype=np.float32)
    save("g11_processing", **out)

    sig = sys.modules["maua.audiovisual.audioreactive.signal"]
    out = {"e": e, "e2": e2}
    out["s_circ_s2"] = sig.gaussian_filter(e, 2)
    out["s_causal0_s2"] = sig.gaussian_filter(e, 2, causal=0)
    out["s_causal05_s2"] = sig.gaussian_filter(e, 2, causal=0.5)
    out["s_refl_s5"] = sig.gaussian_filter(e2, 5, mode="reflect")
    out["s_percentile_clip95"] = sig.percentile_clip(e.clone(), 95)
    out["s_percentile_clip80_2d"] = sig.percentile_clip(e2.clone(), 80)
    out["s_percentile_50"] = np.float32(sig.percentile(e, 50))
    out["s_percentile_95"] = np.float32(sig.percentile(e, 95))
    out["s_resample_1d"] = sig.resample(e, 333)
    out["s_resample_2d"] = sig.resample(e2, 77)
    out["s_normalize"] = sig.normalize(e2)
    save("g11_signal", **out)

    # salience_weighted (selfsupervised/mir.py:13-21) needs librosa at import -> stubbed module import works
    from maua.audiovisual.audioreactive.selfsupervised import mir as SM
    env800 = torch.rand(800, 1, generator=g) ** 3  # long enough for the sigma=80 reflect padding (radius 320)
    feat = SM.normalize(SM.salience_weighted(SM.gaussian_filter(env800, sigma=2)))
    save("g11_salience", env=env800, feat=feat)


# --------------------------------------------------------------------------------------- latents / noise / io
def golden_latents():
    lat = sys.modules.get("maua.audiovisual.audioreactive.latent")
    if lat is None:
        import maua.audiovisual.audioreactive  # noqa
        lat = sys.modules["maua.audiovisual.audioreactive.latent"]
    g = torch.Generator().manual_seed(31)
    y = torch.randn(5, 3, 8, generator=g)
    env = torch.rand(64, generator=g)
    envs = torch.rand(64, 7, generator=g) + 0.1
    out = {"y": y, "env": env, "envs": envs}
    out["slerp_loops"] = lat.slerp_loops(y, 64, 2)
    out["single_weighted"] = lat.single_weighted(y[0], y[1], env)
    out["multi_weighted"] = lat.multi_weighted(y, envs.clone())
    # select_modulo: also capture the int64 index vector (the "onset-bin assignment")
    sig = sys.modules["maua.audiovisual.audioreactive.signal"]
    low, high = torch.quantile(env, 0.25), torch.quantile(env, 0.75)
    idx = (sig.normalize(env.clamp(low, high)) * (len(y) - 1)).round().long()
    out["select_modulo_idx"] = idx
    out["select_modulo"] = lat.select_modulo(y, env)
    save("g12_latents", **out)

    # natural cubic spline loops: torchcubicspline is un-vendored (setup.py:104, unpinned git dep); the natural
    # cubic spline through given knots is unique, so the fixture is produced with scipy's CubicSpline("natural")
    # on the knot/eval grids of latent.py:83-92 and selfsupervised/latent.py:7-13.
    from scipy.interpolate import CubicSpline
    yn = y.double().numpy()
    Y = np.concatenate([yn] * 3 + [yn[:1]])
    cs = CubicSpline(np.linspace(0, 1, len(Y)), Y, axis=0, bc_type="natural")
    out_classic = cs(np.linspace(0, 1, 50))
    Y2 = np.concatenate([yn, yn[:1]])
    cs2 = CubicSpline(np.linspace(0, 1, len(Y2)), Y2, axis=0, bc_type="natural")
    t_out = (torch.linspace(0, 2.5, 50) % 1).double().numpy()
    out_self = cs2(t_out)
    save("g12_spline", y=y, classic_size50_loops3=out_classic, selfsup_size50_loops2p5=out_self)

    # seeds (wrappers/stylegan.py:58-69) — numpy MT19937 is available everywhere, store two rows as a cross-check
    z = np.concatenate([np.random.RandomState(s).randn(1, 512) for s in [0, 1, 2, 7]])
    save("g12_seeds", seeds=np.array([0, 1, 2, 7]), z=z[:, :8])


def golden_noise():
    from maua.audiovisual.audioreactive.selfsupervised import noise as N
    rng = torch.Generator("cpu").manual_seed(42)
    loop = N.Loop(rng, length=48, size=(8, 12), n_loops=2, sigma=5)
    out = {"loop_noise": loop.noise, "loop_idx": loop.idx, "loop_y_0_16": loop.forward(0, 16),
           "loop_y_40_8": loop.forward(40, 8)}
    mod = torch.rand(48, 3, generator=rng)
    bl = N.Blend(rng, 48, (8, 12), mod)
    mu = N.Multiply(rng, 48, (8, 12), mod)
    out.update(mod=mod, blend_noise=bl.noise, blend_y=bl.forward(8, 4), mul_noise=mu.noise, mul_y=mu.forward(8, 4))
    avg = N.Average(loop, mu)
    md = N.Modulate(loop, mu, mod)
    sb = N.ScaleBias(md, 0.7, 0.1)
    out.update(avg_y=avg.forward(8, 4), modulate_y=md.forward(8, 4), scalebias_y=sb.forward(8, 4))
    save("g13_noise", **out)


def golden_io():
    from maua.ops import io as RIO
    # edge values incl. exact .5 ties after *255
    vals = torch.tensor([-0.2, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.5, 127.5 / 255, 128.5 / 255, 1.0, 1.3,
                         254.5 / 255, 0.999], dtype=torch.float32)
    g = torch.Generator().manual_seed(3)
    img = torch.rand(1, 3, 4, 8, generator=g) * 1.2 - 0.1
    img.view(-1)[: len(vals)] = vals
    b = np.frombuffer(RIO.tensor2bytes(img), dtype=np.uint8).reshape(4, 8, 3)
    save("g14_tensor2bytes", img=img, bytes=b)
    # other value ranges and a 1-channel image (ops/video.py passes the writer's value_range through)
    out = {}
    for k, (mn, mx, c) in enumerate([(-1, 1, 3), (0, 255, 3), (-0.5, 2.5, 1), (0.1, 0.7, 4)]):
        x = torch.rand(1, c, 5, 7, generator=g) * (mx - mn) * 1.2 + mn - 0.1 * (mx - mn)
        ties = mn + (mx - mn) * (torch.tensor([0.5, 1.5, 2.5, 126.5, 127.5, 253.5, 254.5]) / 255)
        x.view(-1)[: len(ties)] = ties
        out[f"img{k}"], out[f"range{k}"] = x, torch.tensor([mn, mx], dtype=torch.float64)
        out[f"bytes{k}"] = np.frombuffer(RIO.tensor2bytes(x, (mn, mx)), dtype=np.uint8).reshape(5, 7, c)
    save("g26_tensor2bytes_ranges", **out)


def golden_features():
    """SURVEY 8(f) N3 first batch: features/audio.py mfcc, spectral_flatness, spectral_contrast, drop_strength,
    tonnetz (on a synthetic chromagram: chroma_cens needs the constant-Q stack), rosa dct, processing.emphasize."""
    from maua.audiovisual.audioreactive.selfsupervised.features import audio as FA
    from maua.audiovisual.audioreactive.selfsupervised.features import processing as FP
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import spectral

    sr = 30720
    a = synth_audio(4 * sr, sr, 1234)  # the g09 clip: 120 frames
    a12 = synth_audio(12 * sr, sr, 77)  # 360 frames: the sigma = 10 filter of drop_strength needs > 40 frames
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 128, generator=g)
    env = torch.rand(300, 1, generator=g)
    chroma = torch.rand(12, 50, generator=g) + 0.05
    save("g16_features", sr=np.int64(sr), n12=np.int64(12 * sr), seed12=np.int64(77),
         mfcc=FA.mfcc(a, sr), flatness=FA.spectral_flatness(a, sr), contrast=FA.spectral_contrast(a, sr),
         contrast_linear=FA.spectral_contrast(a, sr, linear=True), drop_strength=FA.drop_strength(a12, sr),
         dct_in=x, dct_none=spectral.dct(x), dct_ortho=spectral.dct(x, norm="ortho"),
         emph_in=env, emph_10_50=FP.emphasize(env, 10, 50), emph_3_80=FP.emphasize(env, 3, 80),
         chroma=chroma, tonnetz=FA.tonnetz(a, sr, chroma_fn=lambda a_, sr_: chroma))


def golden_processing():
    """processing.py:102-130 clamp_peaks_percentile / clamp_upper_percentile / clamp_lower_percentile (torch.quantile only; the
    torchaudio biquads of the same file cannot run here) and audioreactive/audio.py:96-112's call into scipy - the reference
    module imports librosa, so its one-line bodies are run as written there: sosfilt(butter(db, f, kind, fs=sr, output="sos"), y)."""
    from scipy import signal
    from maua.audiovisual.audioreactive.selfsupervised.features import processing as FP
    g = torch.Generator().manual_seed(31)
    e1 = torch.rand(400, generator=g) ** 2
    e3 = torch.rand(257, 3, generator=g)
    e3[::7, 1] = e3[3, 1]                      # ties
    sr = 22050
    t = np.arange(2048) / sr                   # a short clip: the whole-length comparisons run against scipy itself in the tests
    rng = np.random.default_rng(5)
    y = np.sin(2 * np.pi * 60 * t) + 0.5 * np.sin(2 * np.pi * 900 * t) + 0.25 * np.sin(2 * np.pi * 6000 * t) + 0.1 * rng.standard_normal(t.size)
    save("g27_processing", e1=e1, e3=e3, sr=np.int64(sr), y=y,
         peaks_1d_90=FP.clamp_peaks_percentile(e1, 90), peaks_3_50=FP.clamp_peaks_percentile(e3, 50),
         upper_1d_75=FP.clamp_upper_percentile(e1, 75), upper_3_20=FP.clamp_upper_percentile(e3, 20),
         lower_1d_30=FP.clamp_lower_percentile(e1, 30), lower_3_95=FP.clamp_lower_percentile(e3, 95),
         low_200_12=signal.sosfilt(signal.butter(12, 200, "low", fs=sr, output="sos"), y),
         low_100_24=signal.sosfilt(signal.butter(24, 100, "low", fs=sr, output="sos"), y),
         high_3000_12=signal.sosfilt(signal.butter(12, 3000, "high", fs=sr, output="sos"), y),
         band_200_3000_12=signal.sosfilt(signal.butter(12, [200, 3000], "band", fs=sr, output="sos"), y))


def golden_pulse():
    """features/audio.py:72-73 pulse = plp(percussive(audio)) (rosa/beat.py:42-75) on a 40 s synthetic clip (1200 frames:
    the tempogram window is 1024 frames)."""
    from maua.audiovisual.audioreactive.selfsupervised.features import audio as FA
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import beat
    sr = 30720
    a = synth_audio(40 * sr, sr, 21)
    env_med = beat.onset_strength(FA.percussive(a), sr, aggregate=lambda *ar, **kw: torch.median(*ar, **kw).values)
    save("g18_pulse", sr=np.int64(sr), n=np.int64(40 * sr), seed=np.int64(21), pulse=FA.pulse(a, sr), env_median=env_med,
         tempo_freqs=beat.fourier_tempo_frequencies(sr))


def golden_pulse_short():
    """pulse on clips shorter than the 1024-frame tempogram window (beat.py:48-49: win_length = len(onset_envelope), an
    even and an odd non-power-of-two transform): 10 s (300 frames) and 277 frames of the g18 clip."""
    from maua.audiovisual.audioreactive.selfsupervised.features import audio as FA
    sr = 30720
    a = synth_audio(40 * sr, sr, 21)
    save("g24_pulse_short", sr=np.int64(sr), n=np.int64(40 * sr), seed=np.int64(21), n_even=np.int64(300 * 1024),
         n_odd=np.int64(277 * 1024), pulse_even=FA.pulse(a[: 300 * 1024], sr), pulse_odd=FA.pulse(a[: 277 * 1024], sr))


SIGNATURES = [  # (reference file under maua/, qualified name there, our module, our qualified name)
    ("audiovisual/generate.py", "generate_audiovisal_from_patch", "maua_amd.audiovisual.generate", "generate_audiovisal_from_patch"),
    ("audiovisual/audioreactive/selfsupervised/sample.py", "generate", "maua_amd.audiovisual.sample", "generate"),
    ("audiovisual/audioreactive/selfsupervised/sample.py", "load_audio", "maua_amd.audio_io", "load_audio"),
    ("audiovisual/audioreactive/selfsupervised/patch.py", "Patch.__init__", "maua_amd.audiovisual.sample", "Patch.__init__"),
    ("audiovisual/audioreactive/selfsupervised/patch.py", "Patch.forward", "maua_amd.audiovisual.sample", "Patch.forward"),
    ("audiovisual/audioreactive/selfsupervised/latent.py", "latent_patch", "maua_amd.latent", "latent_patch"),
    ("audiovisual/audioreactive/selfsupervised/noise.py", "noise_patch", "maua_amd.noise", "noise_patch"),
    ("audiovisual/audioreactive/selfsupervised/mir.py", "retrieve_music_information", "maua_amd.audiovisual.sample", "retrieve_music_information"),
    ("audiovisual/patches/base/__init__.py", "MauaPatch.__init__", "maua_amd.audiovisual.patches.base", "MauaPatch.__init__"),
    ("audiovisual/patches/base/__init__.py", "MauaPatch.force_output_size", "maua_amd.audiovisual.patches.base", "MauaPatch.force_output_size"),
    ("GAN/wrappers/stylegan2.py", "StyleGAN2Synthesizer.__init__", "maua_amd.stylegan2", "StyleGAN2Synthesizer.__init__"),
    ("GAN/wrappers/stylegan2.py", "StyleGAN2Synthesizer.forward", "maua_amd.stylegan2", "StyleGAN2Synthesizer.forward"),
    ("GAN/wrappers/stylegan2.py", "StyleGAN2Synthesizer.change_output_resolution", "maua_amd.stylegan2", "StyleGAN2Synthesizer.change_output_resolution"),
    ("GAN/wrappers/stylegan2.py", "StyleGAN2Synthesizer.make_noise_pyramid", "maua_amd.stylegan2", "StyleGAN2Synthesizer.make_noise_pyramid"),
    ("GAN/wrappers/stylegan.py", "StyleGANMapper.__init__", "maua_amd.stylegan2", "StyleGAN2Mapper.__init__"),
    ("GAN/wrappers/stylegan.py", "StyleGANMapper.forward", "maua_amd.stylegan2", "StyleGAN2Mapper.forward"),
    ("GAN/wrappers/stylegan.py", "StyleGAN.__init__", "maua_amd.stylegan2", "StyleGAN2.__init__"),
    ("GAN/wrappers/stylegan.py", "StyleGAN.get_z_latents", "maua_amd.stylegan2", "StyleGAN2.get_z_latents"),
    ("GAN/wrappers/stylegan.py", "StyleGAN.get_w_latents", "maua_amd.stylegan2", "StyleGAN2.get_w_latents"),
    ("GAN/wrappers/stylegan.py", "StyleGAN.forward", "maua_amd.stylegan2", "StyleGAN2.forward"),
    ("GAN/wrappers/__init__.py", "MauaGenerator.render", "maua_amd.stylegan2", "StyleGAN2.render"),
    ("GAN/wrappers/__init__.py", "get_generator_class", "maua_amd.stylegan2", "get_generator_class"),
    ("GAN/load.py", "load_network", "maua_amd.load", "load_network"),
    ("GAN/load.py", "load_nvidia", "maua_amd.load", "load_nvidia"),
    ("GAN/load.py", "load_nvidia_pt", "maua_amd.load", "load_nvidia_pt"),
    ("GAN/load.py", "load_rosinality2ada", "maua_amd.load", "load_rosinality2ada"),
    ("GAN/wrappers/inference/ops.py", "bias_act", "maua_amd.ops", "bias_act"),
    ("GAN/wrappers/inference/ops.py", "upfirdn2d", "maua_amd.ops", "upfirdn2d"),
    ("GAN/wrappers/inference/ops.py", "upsample2d", "maua_amd.ops", "upsample2d"),
    ("GAN/wrappers/inference/ops.py", "modulated_conv2d", "maua_amd.ops", "modulated_conv2d"),
    ("GAN/wrappers/inference/ops.py", "conv2d_resample", "maua_amd.ops", "conv2d_resample"),
    ("GAN/wrappers/inference/ops.py", "setup_filter", "maua_amd.ops", "setup_filter"),
    ("ops/video.py", "VideoWriter.__init__", "maua_amd.video", "VideoWriter.__init__"),
    ("ops/video.py", "VideoWriter.write", "maua_amd.video", "VideoWriter.write"),
    ("ops/video.py", "write_video", "maua_amd.video", "write_video"),
    ("ops/io.py", "tensor2bytes", "maua_amd.video", "tensor2bytes"),
    ("GAN/wrappers/inference/ops.py", "get_activation_defaults", "maua_amd.ops", "get_activation_defaults"),
    ("GAN/wrappers/inference/ops.py", "activate", "maua_amd.ops", "activate"),
    ("diffusion/processors/guided.py", "GuidedDiffusion.__init__", "maua_amd.diffusion", "GuidedDiffusion.__init__"),
    ("diffusion/processors/guided.py", "GuidedDiffusion.forward", "maua_amd.diffusion", "GuidedDiffusion.forward"),
    ("diffusion/processors/guided.py", "create_models", "maua_amd.diffusion", "create_models"),
    ("diffusion/processors/guided.py", "GradientGuidedConditioning.__init__", "maua_amd.diffusion", "GradientGuidedConditioning.__init__"),
    ("super/image/models/realesrgan.py", "load_model", "maua_amd.super", "load_model"),
    ("super/image/models/realesrgan.py", "upscale", "maua_amd.super", "upscale"),
    ("GAN/wrappers/inference/stylegan2.py", "FullyConnectedLayer.__init__", "maua_amd.modules", "FullyConnectedLayer.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "FullyConnectedLayer.forward", "maua_amd.modules", "FullyConnectedLayer.forward"),
    ("GAN/wrappers/inference/stylegan2.py", "Conv2dLayer.__init__", "maua_amd.modules", "Conv2dLayer.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "Conv2dLayer.forward", "maua_amd.modules", "Conv2dLayer.forward"),
    ("GAN/wrappers/inference/stylegan2.py", "SynthesisLayer.__init__", "maua_amd.modules", "SynthesisLayer.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "SynthesisLayer.forward", "maua_amd.modules", "SynthesisLayer.forward"),
    ("GAN/wrappers/inference/stylegan2.py", "ToRGBLayer.__init__", "maua_amd.modules", "ToRGBLayer.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "ToRGBLayer.forward", "maua_amd.modules", "ToRGBLayer.forward"),
    ("GAN/wrappers/inference/stylegan2.py", "SynthesisBlock.__init__", "maua_amd.modules", "SynthesisBlock.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "SynthesisBlock.forward", "maua_amd.modules", "SynthesisBlock.forward"),
    ("GAN/wrappers/inference/stylegan2.py", "MappingNetwork.__init__", "maua_amd.stylegan2", "MappingNetwork.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "MappingNetwork.forward", "maua_amd.stylegan2", "MappingNetwork.forward"),
    ("GAN/wrappers/inference/stylegan2.py", "SynthesisNetwork.__init__", "maua_amd.stylegan2", "SynthesisNetwork.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "SynthesisNetwork.forward", "maua_amd.stylegan2", "SynthesisNetwork.forward"),
    ("GAN/wrappers/inference/stylegan2.py", "Generator.__init__", "maua_amd.load", "Generator.__init__"),
    ("GAN/wrappers/inference/stylegan2.py", "Generator.forward", "maua_amd.load", "Generator.forward"),
    ("audiovisual/audioreactive/signal.py", "resample", "maua_amd.audiovisual.audioreactive", "resample"),
    ("audiovisual/audioreactive/signal.py", "normalize", "maua_amd.audiovisual.audioreactive", "normalize"),
    ("audiovisual/audioreactive/signal.py", "percentile", "maua_amd.audiovisual.audioreactive", "percentile"),
    ("audiovisual/audioreactive/signal.py", "percentile_clip", "maua_amd.audiovisual.audioreactive", "percentile_clip"),
    ("audiovisual/audioreactive/signal.py", "compress", "maua_amd.audiovisual.audioreactive", "compress"),
    ("audiovisual/audioreactive/signal.py", "expand", "maua_amd.audiovisual.audioreactive", "expand"),
    ("audiovisual/audioreactive/signal.py", "gaussian_filter", "maua_amd.audiovisual.audioreactive", "gaussian_filter"),
    ("audiovisual/audioreactive/latent.py", "single_weighted", "maua_amd.audiovisual.audioreactive", "single_weighted"),
    ("audiovisual/audioreactive/latent.py", "multi_weighted", "maua_amd.audiovisual.audioreactive", "multi_weighted"),
    ("audiovisual/audioreactive/latent.py", "select_modulo", "maua_amd.audiovisual.audioreactive", "select_modulo"),
    ("audiovisual/audioreactive/latent.py", "eerp", "maua_amd.audiovisual.audioreactive", "eerp"),
    ("audiovisual/audioreactive/latent.py", "copeerp", "maua_amd.audiovisual.audioreactive", "copeerp"),
    ("audiovisual/audioreactive/latent.py", "slerp", "maua_amd.audiovisual.audioreactive", "slerp"),
    ("audiovisual/audioreactive/latent.py", "slerp_loops", "maua_amd.audiovisual.audioreactive", "slerp_loops"),
    ("audiovisual/audioreactive/latent.py", "spline_loops", "maua_amd.audiovisual.audioreactive", "spline_loops"),
    ("audiovisual/audioreactive/latent.py", "tempo_loops", "maua_amd.audiovisual.audioreactive", "tempo_loops"),
    ("audiovisual/audioreactive/audio.py", "load_audio", "maua_amd.audiovisual.audioreactive", "load_audio"),
    ("audiovisual/audioreactive/audio.py", "harmonic", "maua_amd.audiovisual.audioreactive", "harmonic"),
    ("audiovisual/audioreactive/audio.py", "percussive", "maua_amd.audiovisual.audioreactive", "percussive"),
    ("audiovisual/audioreactive/audio.py", "low_pass", "maua_amd.audiovisual.audioreactive", "low_pass"),
    ("audiovisual/audioreactive/audio.py", "high_pass", "maua_amd.audiovisual.audioreactive", "high_pass"),
    ("audiovisual/audioreactive/audio.py", "band_pass", "maua_amd.audiovisual.audioreactive", "band_pass"),
    ("audiovisual/audioreactive/mir.py", "onsets", "maua_amd.audiovisual.audioreactive", "onsets"),
    ("audiovisual/audioreactive/selfsupervised/latent.py", "spline_loop_latents", "maua_amd.latent", "spline_loop_latents"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "chromagram", "maua_amd.audio", "chromagram"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "tonnetz", "maua_amd.audio", "tonnetz"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "mfcc", "maua_amd.audio", "mfcc"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "spectral_contrast", "maua_amd.audio", "spectral_contrast"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "spectral_flatness", "maua_amd.audio", "spectral_flatness"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "rms", "maua_amd.audio", "rms"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "drop_strength", "maua_amd.audio", "drop_strength"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "onsets", "maua_amd.audio", "onsets"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "pulse", "maua_amd.audio", "pulse"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "harmonic", "maua_amd.audio", "harmonic"),
    ("audiovisual/audioreactive/selfsupervised/features/audio.py", "percussive", "maua_amd.audio", "percussive"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/spectral.py", "stft", "maua_amd.audio", "stft"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/spectral.py", "istft", "maua_amd.audio", "istft"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/spectral.py", "spectrogram", "maua_amd.audio", "spectrogram"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/spectral.py", "melspectrogram", "maua_amd.audio", "melspectrogram"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/spectral.py", "mel", "maua_amd.audio", "mel"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/spectral.py", "dct", "maua_amd.audio", "dct"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/beat.py", "onset_strength", "maua_amd.audio", "onset_strength"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/beat.py", "plp", "maua_amd.audio", "plp"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/beat.py", "fourier_tempogram", "maua_amd.audio", "fourier_tempogram"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/beat.py", "fourier_tempo_frequencies", "maua_amd.audio", "fourier_tempo_frequencies"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "gaussian_filter", "maua_amd.audio", "gaussian_filter"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "median_filter2d", "maua_amd.audio", "median_filter2d"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "emphasize", "maua_amd.audio", "emphasize"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "normalize", "maua_amd.audio", "normalize"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "clamp_peaks_percentile", "maua_amd.audio", "clamp_peaks_percentile"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "clamp_upper_percentile", "maua_amd.audio", "clamp_upper_percentile"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "clamp_lower_percentile", "maua_amd.audio", "clamp_lower_percentile"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "low_pass", "maua_amd.audio", "low_pass"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "mid_pass", "maua_amd.audio", "mid_pass"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "high_pass", "maua_amd.audio", "high_pass"),
    ("audiovisual/audioreactive/selfsupervised/features/processing.py", "contrast_enhance", "maua_amd.audio", "contrast_enhance"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/constantq.py", "cqt", "maua.audiovisual.audioreactive.selfsupervised.features.rosa.constantq", "cqt"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/constantq.py", "vqt", "maua.audiovisual.audioreactive.selfsupervised.features.rosa.constantq", "vqt"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/constantq.py", "constant_q", "maua_amd.cqt", "constant_q"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/constantq.py", "constant_q_lengths", "maua_amd.cqt", "constant_q_lengths"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/constantq.py", "cqt_frequencies", "maua_amd.cqt", "cqt_frequencies"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/pitch.py", "piptrack", "maua_amd.cqt", "piptrack"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/pitch.py", "estimate_tuning", "maua_amd.cqt", "estimate_tuning"),
    ("audiovisual/audioreactive/selfsupervised/features/rosa/pitch.py", "pitch_tuning", "maua_amd.cqt", "pitch_tuning"),
    # round 6: the text-prompt guidance surface (maua/grad.py, ops/cutouts.py, loss.py, prompt.py)
    ("grad.py", "GradModule.__init__", "maua_amd.grad", "GradModule.__init__"),
    ("grad.py", "GradModule.forward", "maua_amd.grad", "GradModule.forward"),
    ("grad.py", "CLIPGrads.__init__", "maua_amd.grad", "CLIPGrads.__init__"),
    ("grad.py", "CLIPGrads.set_targets", "maua_amd.grad", "CLIPGrads.set_targets"),
    ("grad.py", "CLIPGrads.forward", "maua_amd.grad", "CLIPGrads.forward"),
    ("ops/cutouts.py", "random_cutouts", "maua_amd.grad", "random_cutouts"),
    ("ops/cutouts.py", "MauaCutouts.__init__", "maua_amd.grad", "MauaCutouts.__init__"),
    ("ops/cutouts.py", "MauaCutouts.forward", "maua_amd.grad", "MauaCutouts.forward"),
    ("ops/cutouts.py", "make_cutouts", "maua_amd.grad", "make_cutouts"),
    ("loss.py", "spherical_dist_loss", "maua_amd.grad", "spherical_dist_loss"),
    ("prompt.py", "TextPrompt.__init__", "maua_amd.grad", "TextPrompt.__init__"),
    ("prompt.py", "ImagePrompt.__init__", "maua_amd.grad", "ImagePrompt.__init__"),
    # round 6, second half: the image-prompt grad modules and their perceptors
    ("grad.py", "ColorMatchGrads.__init__", "maua_amd.grad", "ColorMatchGrads.__init__"),
    ("grad.py", "ColorMatchGrads.histogram", "maua_amd.grad", "ColorMatchGrads.histogram"),
    ("grad.py", "ColorMatchGrads.set_targets", "maua_amd.grad", "ColorMatchGrads.set_targets"),
    ("grad.py", "ColorMatchGrads.forward", "maua_amd.grad", "ColorMatchGrads.forward"),
    ("grad.py", "VGGGrads.__init__", "maua_amd.grad", "VGGGrads.__init__"),
    ("grad.py", "VGGGrads.set_targets", "maua_amd.grad", "VGGGrads.set_targets"),
    ("grad.py", "VGGGrads.forward", "maua_amd.grad", "VGGGrads.forward"),
    ("grad.py", "LPIPSGrads.__init__", "maua_amd.grad", "LPIPSGrads.__init__"),
    ("grad.py", "LPIPSGrads.set_targets", "maua_amd.grad", "LPIPSGrads.set_targets"),
    ("grad.py", "LPIPSGrads.forward", "maua_amd.grad", "LPIPSGrads.forward"),
    ("grad.py", "LossGrads.__init__", "maua_amd.grad", "LossGrads.__init__"),
    ("ops/cutouts.py", "DangoCutouts.__init__", "maua_amd.grad", "DangoCutouts.__init__"),
    ("ops/cutouts.py", "DangoCutouts.forward", "maua_amd.grad", "DangoCutouts.forward"),
    ("perceptors/__init__.py", "Perceptor.__init__", "maua_amd.perceptors", "Perceptor.__init__"),
    ("perceptors/__init__.py", "Perceptor.get_target_embeddings", "maua_amd.perceptors", "Perceptor.get_target_embeddings"),
    ("perceptors/__init__.py", "Perceptor.get_loss", "maua_amd.perceptors", "Perceptor.get_loss"),
    ("perceptors/__init__.py", "load_perceptor", "maua_amd.perceptors", "load_perceptor"),
    ("perceptors/vgg_kbc.py", "KBCPerceptor.__init__", "maua_amd.perceptors", "KBCPerceptor.__init__"),
    ("diffusion/image.py", "get_diffusion_model", "maua_amd.diffusion", "get_diffusion_model"),
    ("ops/cutouts.py", "Cutouts.__init__", "maua_amd.grad", "Cutouts.__init__"),
    ("ops/cutouts.py", "Cutouts.forward", "maua_amd.grad", "Cutouts.forward"),
]


def golden_signatures():
    """The call signatures (argument names in order + the source text of their defaults) of every reference function / method
    the host layer mirrors, read from the reference's source with ``ast`` (nothing is imported or executed): the drop-in
    surface as data.  tests/test_cabi_and_host.py holds maua_amd's signatures to it."""
    import ast
    import json
    out = []
    cache = {}
    for path, qual, our_mod, our_qual in SIGNATURES:
        if path not in cache:
            cache[path] = ast.parse((Path(REF) / "maua" / path).read_text())
        node = None
        parts = qual.split(".")
        for top in cache[path].body:
            if len(parts) == 1 and isinstance(top, ast.FunctionDef) and top.name == parts[0]:
                node = top
            if len(parts) == 2 and isinstance(top, ast.ClassDef) and top.name == parts[0]:
                for sub in top.body:
                    if isinstance(sub, ast.FunctionDef) and sub.name == parts[1]:
                        node = sub
        assert node is not None, (path, qual)
        a = node.args
        names = [x.arg for x in a.posonlyargs + a.args]
        defaults = [None] * (len(names) - len(a.defaults)) + [ast.unparse(d) for d in a.defaults]
        args = [[n, d] for n, d in zip(names, defaults)] + [[x.arg, None if d is None else ast.unparse(d)] for x, d in zip(a.kwonlyargs, a.kw_defaults)]
        out.append({"reference": f"maua/{path}:{node.lineno}", "name": qual, "ours": [our_mod, our_qual], "args": args,
                    "varargs": a.vararg.arg if a.vararg else None, "varkw": a.kwarg.arg if a.kwarg else None})
    (HERE / "g25_signatures.json").write_text(json.dumps(out, indent=0))
    print("g25_signatures.json", len(out), "signatures")


def golden_classic():
    """Small classic-API pieces: signal.compress / expand (:84-105), latent.eerp / copeerp (:46-51), audio.low_pass /
    high_pass / band_pass (:96-112; scipy Butterworth on the host)."""
    import sys as _sys
    from maua.audiovisual.audioreactive import latent as RL
    from maua.audiovisual.audioreactive import audio as RA
    RS = _sys.modules["maua.audiovisual.audioreactive.signal"]
    g = torch.Generator().manual_seed(12)
    e = torch.rand(150, generator=g)
    a, b, t = torch.rand(6, 8, generator=g) + 0.1, torch.rand(6, 8, generator=g) + 0.1, torch.rand(6, 1, generator=g)
    x = synth_audio(2048, 30720, 3).numpy()
    unwrap = lambda f: getattr(f, "__wrapped__", f)
    save("g19_classic", e=e, comp_hi=RS.compress(e.clone(), 0.6, 0.5), comp_lo=RS.expand(e.clone(), 0.3, 2.0, invert=True),
         a=a, b=b, t=t, eerp=RL.eerp(a, b, t), copeerp=RL.copeerp(a, b, t), x=x,
         low=unwrap(RA.low_pass)(x, 30720, 200), high=unwrap(RA.high_pass)(x, 30720, 3000),
         band=unwrap(RA.band_pass)(x, 30720, 200, 3000))


def golden_resample():
    """maua/ops/image.py:214-240 resample (lanczos pre-filter + bicubic align_corners=True): the post-process of
    MauaPatch.force_output_size (patches/base/__init__.py:21-25)."""
    from maua.ops import image as OI
    g = torch.Generator().manual_seed(31)
    x = torch.rand(2, 3, 20, 30, generator=g)
    save("g17_resample", x=x, down=OI.resample(x, (16, 24)), down_h=OI.resample(x, (9, 30)), up=OI.resample(x, (25, 40)),
         mixed=OI.resample(x, (28, 17)), short12=OI.resample(x, 12), lanczos_taps=OI.lanczos(OI.ramp(16 / 20, 2), 2))


def golden_patches():
    """The sub-patch graphs of the sampler: selfsupervised/latent.py:16-80 latent_patch and
    selfsupervised/noise.py:89-140 noise_patch, run on explicit features / segmentations.  The permutation each
    latent sub-patch draws and the planes each noise module draws are stored with the outputs, so the fixture does not
    depend on torch's RNG stream ("loop" latent patches need torchcubicspline, un-vendored: pinned by g12_spline)."""
    from maua.audiovisual.audioreactive.selfsupervised import latent as RL
    from maua.audiovisual.audioreactive.selfsupervised import noise as RN
    g = torch.Generator().manual_seed(77)
    T_, P, Lw, D = 40, 9, 18, 16
    palette = torch.randn(P, Lw, D, generator=g)
    base = torch.randn(T_, Lw, D, generator=g)
    features = {"onsets": torch.rand(T_, 1, generator=g), "rms": torch.rand(T_, 1, generator=g),
                "mfcc": torch.rand(T_, 4, generator=g), "chromagram": torch.rand(T_, 3, generator=g)}
    seg = torch.randint(0, 4, (T_,), generator=g)
    segmentations = {(k, 4): seg for k in features}  # (looked up for every patch type, latent.py:35)
    out = {"palette": palette, "base": base, "seg": seg, **{"feat_" + k: v for k, v in features.items()}}
    cases = [("segmentation", "mfcc", "average", "low"), ("segmentation", "onsets", "modulate", "midhigh"),
             ("feature", "onsets", "modulate", "mid"), ("feature", "mfcc", "average", "all"),
             ("feature", "chromagram", "overwrite", "lowmid"), ("feature", "rms", "modulate", "high")]
    for i, (ptype, sf, mt, md) in enumerate(cases):
        rng = torch.Generator("cpu").manual_seed(100 + i)
        perm = torch.randperm(P, generator=torch.Generator("cpu").manual_seed(100 + i))
        lat = RL.latent_patch(rng, base.clone(), palette, segmentations, features, tempo=120.0, fps=24, patch_type=ptype,
                              segments=4, loop_bars=4, seq_feat=sf, seq_feat_weight=0.8, mod_feat="rms",
                              mod_feat_weight=0.6, merge_type=mt, merge_depth=md)
        out[f"lat{i}"] = lat
        out[f"perm{i}"] = perm
    out["cases"] = np.array(["|".join(c) for c in cases])

    # noise graphs: 17 base Loop modules of tiny sizes, two stacked sub-patches; outputs of layers 0, 7, 13, 16
    sizes = [(3 + (l % 3), 4 + (l % 2)) for l in range(17)]
    rng = torch.Generator("cpu").manual_seed(5)
    noise = [RN.Loop(rng, T_, sz, n_loops=2, sigma=3 + l % 4) for l, sz in enumerate(sizes)]
    out["nsizes"] = np.array(sizes)
    for l, m in enumerate(noise):
        out[f"nbase_planes{l}"] = m.noise
    subs = [dict(patch_type="blend", loop_bars=4, seq_feat="mfcc", seq_feat_weight=0.7, mod_feat="onsets",
                 mod_feat_weight=0.9, merge_type="modulate", merge_depth="all", noise_mean=0.1, noise_std=0.8),
            dict(patch_type="multiply", loop_bars=8, seq_feat="chromagram", seq_feat_weight=1.0, mod_feat="rms",
                 mod_feat_weight=1.0, merge_type="average", merge_depth="midhigh", noise_mean=0.0, noise_std=1.2),
            dict(patch_type="loop", loop_bars=16, seq_feat="onsets", seq_feat_weight=1.0, mod_feat="rms",
                 mod_feat_weight=0.5, merge_type="overwrite", merge_depth="low", noise_mean=-0.2, noise_std=0.5)]
    for sub in subs:
        noise = RN.noise_patch(rng, noise, features, 120.0, 24, **sub)

    def planes_of(m, acc):  # every random tensor of the graph, in construction (depth-first, left before right) order
        for name in ("base", "left", "right"):
            if hasattr(m, name):
                planes_of(getattr(m, name), acc)
        if hasattr(m, "noise"):
            acc.append(m.noise)
        return acc
    for l in (0, 7, 13, 16):
        out[f"ny{l}"] = noise[l].forward(5, 6)
        for j, pl in enumerate(planes_of(noise[l], [])):
            out[f"nplanes{l}_{j}"] = pl
    out["subs"] = np.array([repr(sorted(s.items())) for s in subs])
    save("g20_patches", **out)


def golden_cqt():
    """The parts of the constant-Q chain the reference can run here (rosa/constantq.py, rosa/pitch.py, rosa/convert.py):
    filter bank, sparsified FFT basis, the top octave's response, piptrack / estimate_tuning, cq_to_chroma.  The rest
    (torchaudio.resample between octaves, the torchcubicspline coefficients behind spline_quantize) is un-vendored."""
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import spectral as _SP  # noqa: F401 (first: its import cycle)
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import constantq as CQ
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import convert as CV
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import pitch as PT
    a = np.load(HERE / "g09_audio_clip.npz")["audio"]
    y = torch.from_numpy(a)
    sr = 30720
    fmin = torch.tensor(32.70319566257483).float()
    top = CQ.cqt_frequencies(252, fmin, bins_per_octave=36)[-36:]
    filters, lengths = CQ.constant_q(sr, fmin=top.min(), n_bins=36, bins_per_octave=36)
    fft_basis, n_fft, _ = getattr(CQ, "__cqt_filter_fft")(sr, top.min(), 36, 36, 1, 0.01, gamma=0)
    dense = fft_basis.to_dense()
    resp = getattr(CQ, "__cqt_response")(y, n_fft, 1024, fft_basis)
    pitch, mag = PT.piptrack(y, sr)
    tuning = PT.estimate_tuning(y, sr, bins_per_octave=36)
    m = CV.cq_to_chroma(252, "cpu", bins_per_octave=36, n_chroma=12, fmin=fmin)
    nz = torch.nonzero(pitch)
    save("g21_cqt", top_freqs=top, lengths=lengths, filt_rows=torch.view_as_real(filters[[0, 17, 35]]), filt_abs_sum=filters.abs().sum(1),
         n_fft=np.int64(n_fft), basis_nnz=(dense != 0).sum(1), basis_rows=torch.view_as_real(dense[[0, 17, 35]]),
         basis_abs_sum=dense.abs().sum(1), resp=torch.view_as_real(resp), pitch_idx=nz, pitch_val=pitch[nz[:, 0], nz[:, 1]],
         mag_val=mag[nz[:, 0], nz[:, 1]], tuning=np.float32(float(tuning)), cq_to_chroma=m,
         lengths_full=CQ.constant_q_lengths(sr, fmin, n_bins=252, bins_per_octave=36))


def golden_vqt():
    """The variable-Q pieces (gamma != 0) of rosa/constantq.py the reference can run here: filter lengths, filter bank,
    sparsified FFT basis and the top octave's response at the ERB default gamma = 24.7 alpha / 0.108 (constantq.py:53-54)
    and at gamma = 5 (the octave recursion needs the un-vendored torchaudio.resample)."""
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import spectral as _SP  # noqa: F401
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import constantq as CQ
    y = torch.from_numpy(np.load(HERE / "g09_audio_clip.npz")["audio"])
    sr = 30720
    fmin = torch.tensor(32.70319566257483).float()
    out = {}
    for tag, bpo, gamma in (("erb", 36, 24.7 * (2.0 ** (1.0 / 36) - 1) / 0.108), ("g5", 12, 5.0)):
        n_bins = 7 * bpo
        top = CQ.cqt_frequencies(n_bins, fmin, bins_per_octave=bpo)[-bpo:]
        filters, lengths = CQ.constant_q(sr, fmin=top.min(), n_bins=bpo, bins_per_octave=bpo, gamma=gamma)
        fft_basis, n_fft, _ = getattr(CQ, "__cqt_filter_fft")(sr, top.min(), bpo, bpo, 1, 0.01, gamma=gamma)
        dense = fft_basis.to_dense()
        resp = getattr(CQ, "__cqt_response")(y, n_fft, 1024, fft_basis)
        out.update({f"{tag}_gamma": np.float64(gamma), f"{tag}_bpo": np.int64(bpo), f"{tag}_lengths": lengths,
                    f"{tag}_filt_abs_sum": filters.abs().sum(1), f"{tag}_n_fft": np.int64(n_fft),
                    f"{tag}_basis_nnz": (dense != 0).sum(1), f"{tag}_basis_abs_sum": dense.abs().sum(1),
                    f"{tag}_basis_rows": torch.view_as_real(dense[[0, bpo // 2, bpo - 1]]), f"{tag}_resp": torch.view_as_real(resp),
                    f"{tag}_lengths_full": CQ.constant_q_lengths(sr, fmin, n_bins=n_bins, bins_per_octave=bpo, gamma=gamma)})
    save("g23_vqt", **out)


def segment_inputs(seed=3, T=640, C=12, n_sections=5):
    """a feature with section structure (repeated random section templates + noise) and a jittered beat grid"""
    g = torch.Generator().manual_seed(seed)
    templates = torch.randn(3, C, generator=g)
    order = [0, 1, 0, 2, 1]
    bounds = torch.linspace(0, T, n_sections + 1).long()
    env = torch.empty(T, C)
    for s in range(n_sections):
        lo, hi = int(bounds[s]), int(bounds[s + 1])
        env[lo:hi] = templates[order[s]] + 0.3 * torch.randn(hi - lo, C, generator=g)
    beats, b = [], 0
    while True:
        b += int(torch.randint(6, 11, (), generator=g))
        if b >= T - 2:
            break
        beats.append(b)
    return env, beats


def golden_segment():
    """features/rosa/segment.py pieces the reference can run here (torch_geometric / librosa / sklearn are stubs: the
    get_laplacian call of laplacian_segmentation itself cannot run)."""
    from maua.audiovisual.audioreactive.selfsupervised.features.rosa import segment as SG
    env, beats = segment_inputs()
    Csync = torch.stack([torch.median(env[b1:b2], dim=0).values for b1, b2 in zip([0] + beats, beats + [len(env)])])
    R = SG.recurrence_matrix(Csync, width=3, sym=True)
    Rf = SG.timelag_median_filter(R)
    g = torch.Generator().manual_seed(11)
    ev = torch.randn(len(Csync), 16, generator=g)
    evf = SG.median_filter1d(ev.T, k=9, s=1, p=4).T
    out = dict(env=env, beats=np.array(beats), Csync=Csync, R=R, Rf=Rf, ev=ev, evf=evf)
    for k in (2, 6, 16):
        X = torch.randn(len(Csync), k, generator=g) + 2.0 * torch.nn.functional.one_hot(torch.arange(len(Csync)) * k // len(Csync), k)
        Xn = torch.diag(1.0 / torch.norm(X, p=2, dim=1)) @ X
        out[f"km{k}_X"] = X
        out[f"km{k}_init"] = SG.init_plus_plus(Xn.numpy(), k)
        mu, r, dist = SG.differentiable_k_means(X, k, 100)
        out[f"km{k}_mu"], out[f"km{k}_r"], out[f"km{k}_dist"] = mu, r, dist
    save("g22_segment", **out)


def synthetic_rosinality_checkpoint(res=16, n_map=2, seed=7, const_input=True):
    """A random state dict with the key/shape structure of a rosinality StyleGAN2 ``g_ema`` (the structure is what
    maua/GAN/load.py:18-127 consumes); shared with tests/test_load.py, which rebuilds the same tensors."""
    from maua_amd.load import synthetic_rosinality_checkpoint as build
    return build(res, n_map, seed, const_input)


def golden_load():
    """maua/GAN/load.py:18-127 key mapping for both target layouts.  The Generator classes are replaced by a recorder
    (the nv train network is un-vendored; the in-tree inference network is additionally loaded for real to check
    that the produced keys are exactly its state dict).  Stored: per produced key its shape, sum and abs-sum."""
    import json
    import tempfile
    import maua.GAN.load as RL
    from maua.GAN.wrappers.inference import stylegan2 as inf

    class Recorder:
        last = None

        def __init__(self, *a, **k):
            self.args, self.kwargs = a, k

        def load_state_dict(self, sd):
            Recorder.last = (dict(sd), self.args, self.kwargs)

    out = {}
    for const_input in (True,):
        for for_inference in (False, True):
            ck = synthetic_rosinality_checkpoint(const_input=const_input)
            raises = None
            if for_inference:
                # reference quirk (load.py:79-88): with for_inference=True a 'convs.N.noise.weight' key falls into the
                # "not recognized" branch, i.e. the converter raises on every real rosinality checkpoint.  Record that,
                # then pin the inference-layout mapping on the checkpoint without those keys.
                with tempfile.NamedTemporaryFile(suffix=".pt") as f:
                    torch.save(ck, f.name)
                    try:
                        RL.load_rosinality2ada(f.name, for_inference=True)
                        raises = False
                    except Exception as e:
                        raises = "not recognized" in str(e)
                ck["g_ema"] = {k: v for k, v in ck["g_ema"].items() if not (k.startswith("convs.") and k.endswith("noise.weight"))}
            with tempfile.NamedTemporaryFile(suffix=".pt") as f:
                torch.save(ck, f.name)
                real_inf = inf.Generator
                RL.stylegan2_train = MagicMock()
                RL.stylegan2_train.Generator = Recorder
                inf.Generator = Recorder
                try:
                    RL.load_rosinality2ada(f.name, for_inference=for_inference)
                finally:
                    inf.Generator = real_inf
                sd, args, kwargs = Recorder.last
                entry = {k: {"shape": list(v.shape), "sum": float(v.double().sum()), "abs": float(v.double().abs().sum())}
                         for k, v in sd.items()}
                strict_ok = None
                if for_inference:  # the in-tree inference Generator must accept exactly these keys
                    G = real_inf(*args, **kwargs)
                    G.load_state_dict(sd)
                    strict_ok = True
                out[f"rosinality_const{int(const_input)}_inference{int(for_inference)}"] = {
                    "generator_args": [int(a) for a in args], "mapping_layers": int(kwargs["mapping_kwargs"]["num_layers"]),
                    "strict_load_ok": strict_ok, "reference_raises_on_conv_noise_weight": raises, "keys": entry}
    (HERE / "g15_load_keymap.json").write_text(json.dumps(out, indent=0, sort_keys=True))
    print("g15_load_keymap.json", {k: len(v["keys"]) for k, v in out.items()})


def golden_secondary():
    """g28: the reference's in-tree secondary diffusion model (guided.py:68-143) and its default "fast" conditioning
    (:212-274) - forward outputs (v, pred, eps) and the conditioning gradient -J^T g that GradientGuidedConditioning.forward
    returns, computed by the reference's own classes.  Weights: oracle.diffusion.secondary_random_params(seed) loaded with
    strict=True (this also pins the state-dict key plan); the un-vendored guided_diffusion submodule is a stub (guided.py
    imports it at module scope; neither class below touches it)."""
    from types import SimpleNamespace
    import maua.diffusion.processors.guided as RG
    from oracle import diffusion as OD
    seed = 5
    params = OD.secondary_random_params(seed)
    net = RG.SecondaryDiffusionImageNet2()
    missing = net.load_state_dict(params, strict=True)
    net.eval().requires_grad_(False)
    g = torch.Generator().manual_seed(11)
    B, H, W = 2, 64, 96
    x = torch.randn(B, 3, H, W, generator=g)
    tc = torch.tensor([0.15, 0.85])
    out = net(x, tc)
    # the conditioning: a diffusion stand-in carrying exactly the attributes GradientGuidedConditioning reads
    sch = OD.Schedule(1000, "ddim100")
    diffusion = SimpleNamespace(timestep_map=list(sch.timestep_map), sqrt_alphas_cumprod=sch.sqrt_alphas_cumprod,
                                sqrt_one_minus_alphas_cumprod=sch.sqrt_one_minus_alphas_cumprod)
    target = torch.randn(3, H, W, generator=g) * 0.5

    class MSE(torch.nn.Module):   # a grad module in the sense of maua/grad.py:15-25: scale, set_targets, forward(img, t) -> d loss / d img
        scale = 1000.0

        def set_targets(self, prompts):
            pass

        def forward(self, img, t):
            return (2.0 * self.scale / img[0].numel()) * (img - target)
    cond = RG.GradientGuidedConditioning(diffusion, net, [MSE()], speed="fast")
    steps = torch.tensor([7, 61])                                     # indices into the respaced schedule
    t_model = torch.tensor([float(sch.timestep_map[int(i)]) for i in steps])   # what cond_fn receives (rescale_timesteps: the original steps)
    xt = torch.randn(B, 3, H, W, generator=g)
    cond.set_targets([], torch.zeros_like(xt))
    grad = cond(xt, t_model)
    save("g28_secondary", seed=np.int64(seed), x=x, t=tc, v=out.v, pred=out.pred, eps=out.eps, target=target, steps=steps,
         t_model=t_model, xt=xt, cond_grad=grad, mse_scale=np.float32(1000.0))
    print("  strict load:", missing)


def golden_regular():
    """g32: guidance speed "regular" (guided.py:214-218, 236-272) - the gradient the REFERENCE's own GradientGuidedConditioning.forward
    returns when it differentiates through `diffusion.p_mean_variance(model=...)["pred_xstart"]`.  The guided_diffusion submodule is
    empty in the reference checkout, so the diffusion object handed to the reference's class is a stand-in whose p_mean_variance is the
    published arithmetic on the oracle's restated network (respaced index -> model timestep, eps = the first half of the learn_sigma
    output, pred_xstart = sqrt_recip_alphas_cumprod x - sqrt_recipm1_alphas_cumprod eps); everything around it - the timestep
    mapping `timestep_map.index`, img = out * sigma + x * (1 - sigma), the grad modules' sum, the sign, torch.autograd.grad - is the
    reference's code.  Small network (oracle.diffusion.unet_config of the tests' SMALL shape, seed 0: rebuilt from the seed)."""
    from types import SimpleNamespace
    import maua.diffusion.processors.guided as RG
    from oracle import diffusion as OD
    cfg = OD.unet_config(image_size=64, model_channels=32, num_res_blocks=1, attention_resolutions=(16, 8), channel_mult=(1, 2, 2),
                         num_head_channels=32)
    params = OD.init_unet_params(cfg, torch.Generator().manual_seed(0))
    sch = OD.Schedule(1000, "ddim20")

    def p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=None):
        assert not clip_denoised
        out = OD._unet_forward(params, cfg, x, sch.model_timesteps(t.cpu()))
        return {"pred_xstart": OD._ex(sch.sqrt_recip_alphas_cumprod, t, x.shape) * x
                               - OD._ex(sch.sqrt_recipm1_alphas_cumprod, t, x.shape) * out[:, :x.shape[1]]}
    diffusion = SimpleNamespace(timestep_map=list(sch.timestep_map), sqrt_alphas_cumprod=sch.sqrt_alphas_cumprod,
                                sqrt_one_minus_alphas_cumprod=sch.sqrt_one_minus_alphas_cumprod, p_mean_variance=p_mean_variance)
    g = torch.Generator().manual_seed(21)
    B, H, W = 2, 64, 64
    target = torch.randn(3, H, W, generator=g) * 0.5

    class MSE(torch.nn.Module):
        scale = 500.0

        def set_targets(self, prompts):
            pass

        def forward(self, img, t):
            return (2.0 * self.scale / img[0].numel()) * (img - target)
    cond = RG.GradientGuidedConditioning(diffusion, None, [MSE()], speed="regular")
    steps = torch.tensor([12, 5])
    t_model = torch.tensor([float(sch.timestep_map[int(i)]) for i in steps])
    xt = torch.randn(B, 3, H, W, generator=g)
    cond.set_targets([], torch.zeros_like(xt))
    grad = cond(xt, t_model)
    save("g32_regular_conditioning", steps=steps, t_model=t_model, xt=xt, target=target, cond_grad=grad, mse_scale=np.float32(500.0),
         unet_seed=np.int64(0))


def golden_architectures():
    """g29: the "orig" / "resnet" block architectures (inference/stylegan2.py:275-382).  The reference's constructors run, its
    up = 2 forwards do not, so this pins: (i) the constructors' key set, shapes, draw order and num_ws; (ii) the
    reference Conv2dLayer (1 x 1, bias=False: the resnet skip) at up = 1 through its own forward with a gain; (iii) one resnet
    block composed from the reference's own pieces the way SynthesisBlock.forward :354-360 composes them - the up = 2 layers
    as conv_transpose2d + the reference upfirdn2d with the padding conv2d_resample :199-225 computes (3 x 3: (1,1,1,1),
    1 x 1: (2,2,2,2)), conv1 through the reference SynthesisLayer with gain sqrt(.5)."""
    from math import sqrt
    from maua.GAN.wrappers.inference import ops as R
    from maua.GAN.wrappers.inference import stylegan2 as S
    out = {}
    for arch, seed in (("orig", 31), ("resnet", 32)):
        torch.manual_seed(seed)
        net = S.SynthesisNetwork(w_dim=16, img_resolution=32, img_channels=3, channel_base=256, channel_max=16, architecture=arch)
        out[f"{arch}__num_ws"] = np.int64(net.num_ws)
        out[f"{arch}__keys"] = np.array(list(net.state_dict().keys()))
        for k, v in net.state_dict().items():
            out[f"{arch}__" + k.replace(".", "__")] = v
    g = torch.Generator().manual_seed(33)
    B, ci, co, h, wd = 2, 8, 6, 8, 16
    torch.manual_seed(34)
    blk = S.SynthesisBlock(ci, co, w_dim=wd, resolution=2 * h, img_channels=3, is_last=False, architecture="resnet")
    blk.conv0.bias.data.copy_(torch.randn(co, generator=g))
    blk.conv1.bias.data.copy_(torch.randn(co, generator=g))
    x = torch.randn(B, ci, h, h, generator=g)
    ws = torch.randn(B, 2, wd, generator=g)
    f = blk.resample_filter
    # (ii) the skip layer's class at up = 1 (tensor-typed attributes: Q1)
    sk1 = S.Conv2dLayer(ci, co, kernel_size=1, bias=False, up=1)
    sk1.weight.data.copy_(blk.skip.weight.data)
    sk1.padding, sk1.up, sk1.down = T(0), T(1), T(1)
    y_up1 = sk1(x, gain=sqrt(0.5))
    # (iii) y = skip(x, gain sqrt(.5)), up = 2, 1 x 1
    wsk = blk.skip.weight * blk.skip.weight_gain
    t = torch.nn.functional.conv_transpose2d(x, wsk.permute(1, 0, 2, 3), stride=2, padding=0)
    y = R.bias_act(R.upfirdn2d(t, f, padding=T([2, 2, 2, 2]), gain=T(4)), None, act="linear", gain=sqrt(0.5))
    # conv0: styles = affine(w); modulate + demodulate; transposed convolution + FIR; + noise_const; bias_act(lrelu, sqrt 2, 256)
    s = blk.conv0.affine(ws[:, 0])
    w = blk.conv0.weight.unsqueeze(0) * s[:, None, :, None, None]
    w = w / ((w * w).sum((2, 3, 4)) + 1e-8).sqrt()[..., None, None, None]
    wg = w.permute(0, 2, 1, 3, 4).reshape(B * ci, co, 3, 3)
    t = torch.nn.functional.conv_transpose2d(x.reshape(1, B * ci, h, h), wg, stride=2, padding=0, groups=B)
    x0 = R.upfirdn2d(t, f, padding=T([1, 1, 1, 1]), gain=T(4)).reshape(B, co, 2 * h, 2 * h) + blk.conv0.noise_const
    x0 = R.bias_act(x0, blk.conv0.bias, act="lrelu", gain=sqrt(2.0), clamp=256.0)
    blk.conv1.padding, blk.conv1.up = T(1), T(1)
    x1 = blk.conv1(x0, ws[:, 1], "const", gain=sqrt(0.5))
    out.update(blk__x=x, blk__ws=ws, blk__skip_up1=y_up1, blk__skip=y, blk__conv0=x0, blk__conv1=x1, blk__out=y + x1)
    for k, v in blk.state_dict().items():
        out["blk__p__" + k.replace(".", "__")] = v
    save("g29_architectures", **out)


def golden_fp16():
    """g30: the reference's operator layer on float16 tensors (its own render dtype, render/ffmpeg.py:45): modulated_conv2d with
    ops.py:161-165's pre-normalisation branch taken (x.dtype == float16 and demodulate; up = 1 - the up = 2 branch cannot execute
    in-tree), with styles large enough that x * s would leave the half range without it; bias_act and upfirdn2d on
    float16 inputs.  Everything float16 in, float16 out, computed by the reference's functions on the CPU."""
    from maua.GAN.wrappers.inference import ops as R
    g = torch.Generator().manual_seed(300)
    h = torch.float16
    x = (torch.randn(2, 32, 16, 16, generator=g) * 40).clamp(-256, 256).to(h)
    w3 = torch.randn(32, 32, 3, 3, generator=g).to(h)
    s = ((torch.randn(2, 32, generator=g) + 1) * 300).to(h)           # |x s| reaches 1e5 > 65504
    nz = torch.randn(2, 1, 16, 16, generator=g).to(h)
    y_demod = R.modulated_conv2d(x, w3, s, noise=nz, up=T(1), padding=T(1))
    y_small = R.modulated_conv2d(x, w3, (s.float() / 300).to(h), up=T(1), padding=T(1))
    assert y_demod.dtype == h and bool(torch.isfinite(y_demod.float()).all())
    b = torch.randn(32, generator=g).to(h)
    xb = (torch.randn(2, 32, 8, 8, generator=g) * 3).to(h)
    y_ba = R.bias_act(xb, b, act="lrelu", gain=T(sqrt(2)), clamp=T(256.0))
    f = R.setup_filter([1, 3, 3, 1])
    xu = torch.randn(2, 4, 9, 9, generator=g).to(h)
    y_up = R.upfirdn2d(xu, f.to(h), up=T(2), padding=T([2, 1, 2, 1]), gain=T(4))
    save("g30_fp16_ops", x=x, w3=w3, s=s, noise=nz, y_demod=y_demod, y_small=y_small, b=b, xb=xb, y_ba=y_ba, f=f, xu=xu, y_up=y_up)


def golden_offpath():
    """g31: the operator layer OUTSIDE the render path's argument set (VERDICT r4 missing 7).  conv2d_resample with up = 1 and
    paddings other than k // 2 runs in the reference as is (ops.py:228-231); its up > 1 branch cannot execute (Q1), so - like g06 -
    the up-layers with other filters / factors are composed of the same calls by hand: weight regroup (:215-217),
    conv_transpose2d with the padding :218-223 arrive at, the reference's upfirdn2d with the rest (:225)."""
    from maua.GAN.wrappers.inference import ops as R
    g = torch.Generator().manual_seed(310)
    x = torch.randn(2, 8, 10, 12, generator=g)
    w3 = torch.randn(6, 8, 3, 3, generator=g)
    w1 = torch.randn(5, 8, 1, 1, generator=g)
    out = {"x": x, "w3": w3, "w1": w1}
    for p in (0, 2, 3):
        out[f"y3_p{p}"] = R.conv2d_resample(x, w3, padding=T(p))
    out["y1_p2"] = R.conv2d_resample(x, w1, padding=T(2))
    xg = torch.randn(1, 3 * 8, 9, 9, generator=g)
    wg = torch.randn(3 * 4, 8, 3, 3, generator=g)
    out.update(xg=xg, wg=wg, yg_p0=R.conv2d_resample(xg, wg, padding=T(0), groups=T(3)))
    s = torch.randn(2, 8, generator=g) + 1
    out["s"] = s
    B, ci, co = 2, 8, 6
    w = w3.unsqueeze(0) * s[:, None, :, None, None]
    w = w / ((w * w).sum((2, 3, 4)) + 1e-8).sqrt()[..., None, None, None]
    wt = w.reshape(B, co, ci, 3, 3).permute(0, 2, 1, 3, 4).reshape(B * ci, co, 3, 3)
    for name, taps, up in (("f121_up2", [1, 2, 1], 2), ("f11_up2", [1, 1], 2), ("f14641_up2", [1, 4, 6, 4, 1], 2),
                           ("f1331_up4", [1, 3, 3, 1], 4), ("f8_up4", [1, 3, 5, 7, 7, 5, 3, 1], 4), ("f6_up3", [1, 2, 3, 3, 2, 1], 3)):
        f = R.setup_filter(taps, separable=False)
        fw = fh = f.shape[0]
        k, pad = 3, 1
        p0 = pad + (fw + up - 1) // 2 - (k - 1)
        p1 = pad + (fw - up) // 2 - (k - up)
        pt = max(min(-p0, -p1), 0)
        t = torch.nn.functional.conv_transpose2d(x.reshape(1, B * ci, 10, 12), wt, stride=up, padding=pt, groups=B)
        y = R.upfirdn2d(t, f, padding=T([p0 + pt, p1 + pt, p0 + pt, p1 + pt]), gain=T(up * up))
        out["f_" + name] = f
        out["y_" + name] = y.reshape(B, co, 10 * up, 12 * up)
    save("g31_offpath_ops", **out)


def golden_cutouts():
    """g33: the text-prompt guidance path's two in-tree pieces, computed by the reference's own functions.
    (a) maua/loss.py:22-25 spherical_dist_loss on random embeddings (incl. the broadcast shape CLIPGrads uses).
    (b) maua/ops/cutouts.py:8-50 random_cutouts / MauaCutouts on seeded inputs: the ``resize_right`` package is absent from the image,
        so the reference's function runs with oracle.clip.resize (the published algorithm restated) standing in for it - what this
        pins is everything AROUND the resize: the rectangle arithmetic, the draws from torch's global generator and their order, the
        pow schedule over t, the concatenation order.  The rectangles are recovered from the views the reference hands to ``resize``."""
    import maua.loss as RL
    import maua.ops.cutouts as RC
    from oracle import clip as OC
    g = torch.Generator().manual_seed(33)
    x = torch.randn(64, 1, 24, generator=g)
    y = torch.randn(1, 5, 24, generator=g)
    out = {"sd_x": x, "sd_y": y, "sd_out": RL.spherical_dist_loss(x, y)}
    seen = []

    def spy_resize(cutout, out_shape):
        base = cutout._base if cutout._base is not None else cutout
        W = base.shape[-1]
        off = cutout.storage_offset() - base.storage_offset()
        seen.append((cutout.shape[-1], (off // W) % base.shape[-2], off % W))
        return OC.resize(cutout, out_shape)
    RC.resize = spy_resize
    for k, (H, W, cs, cutn, t, seed) in enumerate(((40, 40, 32, 8, 900, 1), (48, 36, 32, 8, 100, 2), (30, 44, 32, 12, 500, 3),
                                                   (256, 256, 224, 32, 981, 4), (24, 24, 32, 8, 300, 5))):
        img = torch.rand(2, 3, H, W, generator=g)
        seen.clear()
        torch.manual_seed(seed)
        cuts = RC.MauaCutouts(cs, cutn)(img, torch.tensor([float(t), 3.0])[[0]].long())   # (grad.py:149: t[[0]].long())
        out[f"cut{k}_cfg"] = np.array([H, W, cs, cutn, t, seed], dtype=np.int64)
        out[f"cut{k}_rects"] = np.array(seen, dtype=np.int64)
        if H <= 64:
            out[f"cut{k}_img"] = img
            out[f"cut{k}_out"] = cuts
        else:   # (the full-size case: rectangles only - what the sampler draws per step at 256^2 / 224)
            out[f"cut{k}_sum"] = cuts.double().sum((1, 2, 3)).float()
    save("g33_cutouts", **out)


def golden_grads():
    """g34: the image-prompt grad modules' in-tree pieces, computed by the reference's own functions.
    (a) maua/grad.py:27-47 differentiable_histogram (values on and between the edges, with and without weights, one value outside).
    (b) maua/grad.py:50-70 ColorMatchGrads.histogram / set_targets / forward with oracle.grads.rgb_to_hsv standing in for the absent
        ``kornia`` - pins the clamp / weighting / histogram / mse / autograd chain around it.
    (c) maua/loss.py:33-80 scaled_mse_loss, feature_loss, gram_matrix.
    (d) maua/perceptors/__init__.py:10-91: the reference's Perceptor hooks + get_loss around the restated vgg19.features (torchvision is
        absent; seeded random weights from oracle.grads.init_vgg_params): the Gram embeddings the hooks store, the loss, and
        torch.autograd.grad back to the image exactly as VGGGrads.forward (grad.py:90-93) asks for it.  ``torch.nested_tensor`` (gone from
        this torch) is replaced by the identity on the list for the duration.
    (e) maua/ops/cutouts.py:101-206 DangoCutouts(skip_augs=True): torchvision's Grayscale / hflip and resize_right replaced by the
        oracle's restatements; pins the rectangle draws and their order, the overview / inner-crop / grey schedule over t.
    (f) maua/ops/image.py:214-240 resample(x, 256) on a 256 x 256 image (LPIPSGrads' pre-step): the identity."""
    import maua.grad as RG
    import maua.loss as RL
    import maua.ops.cutouts as RC
    import maua.ops.image as RI
    import maua.perceptors as RP
    from oracle import clip as OC
    from oracle import grads as OG
    g = torch.Generator().manual_seed(34)
    out = {}
    # (a)
    x = torch.rand(2, 300, generator=g)
    x[0, :8] = torch.tensor([0.0, 1.0, 1 / 254, 2 / 254, 0.5, 253 / 254, 1.002, 0.99999])
    w = torch.rand(2, 300, generator=g)
    out.update(hist_x=x, hist_w=w, hist_out_w=RG.differentiable_histogram(x, w, 255), hist_out=RG.differentiable_histogram(x, None, 255),
               hist_out_17=RG.differentiable_histogram(x, w, 17))
    # (b)
    RG.rgb_to_hsv = OG.rgb_to_hsv
    img = torch.rand(2, 3, 24, 20, generator=g) * 2.2 - 1.1
    style = torch.rand(1, 3, 16, 16, generator=g) * 2 - 1
    for sw in (True, False):
        m = RG.ColorMatchGrads(scale=3.0, saturation_weighting=sw)
        m.register_buffer("target", m.histogram(style))                    # set_targets :65-69 for one StylePrompt
        with torch.enable_grad():
            xi = img.clone().requires_grad_()
            grad = m.forward(xi, None)
        out[f"cm_hist_{int(sw)}"] = m.histogram(img)
        out[f"cm_target_{int(sw)}"] = m.target
        out[f"cm_grad_{int(sw)}"] = grad
    out.update(cm_img=img, cm_style=style)
    # (c)
    a, b = torch.randn(2, 6, 5, 7, generator=g), torch.randn(12, 12, generator=g)
    gm = RL.gram_matrix(a)
    out.update(loss_a=a, loss_b=b, gram_a=gm, scaled_mse=RL.scaled_mse_loss(gm, b), feature_loss=RL.feature_loss(gm, b))
    # (d)
    p = OG.init_vgg_params(OG.VGG19_CFG, 29, generator=torch.Generator().manual_seed(3400))
    layers, i, cin = [], 0, 3
    for v in OG.VGG19_CFG:
        if i > 29:
            break
        if v == "M":
            layers.append(torch.nn.MaxPool2d(2)); i += 1
        else:
            conv = torch.nn.Conv2d(cin, v, 3, padding=1, padding_mode="replicate" if i == 0 else "zeros")
            conv.weight.data.copy_(p[f"{i}.weight"]); conv.bias.data.copy_(p[f"{i}.bias"])
            layers += [conv, torch.nn.ReLU(inplace=True)]; cin = v; i += 2
    per = RP.Perceptor(content_strength=0, content_layers=[], style_strength=2.5, style_layers=list(OG.KBC_STYLE_LAYERS))
    per.net = torch.nn.Sequential(*layers).eval().requires_grad_(False)
    per.preprocess = lambda t: OG.normalize_img(t, OG.IMAGENET_MEAN, OG.IMAGENET_STD)
    per.register_layer_hooks()
    torch.nested_tensor = lambda embs, device=None: list(embs)
    try:
        vimg = torch.rand(1, 3, 32, 32, generator=g) * 2 - 1
        vstyle = torch.rand(1, 3, 32, 32, generator=g)
        targets = [t.clone() for t in per.forward(vstyle)]                 # what get_target_embeddings' forward leaves in the hooks
        with torch.enable_grad():
            xi = vimg.clone().requires_grad_()
            loss = per.get_loss(xi.add(1).div(2), targets)
            grad = torch.autograd.grad(loss, xi)[0]
    finally:
        del torch.nested_tensor
    out.update(vgg_seed=np.int64(3400), vgg_img=vimg, vgg_style=vstyle, vgg_loss=loss.detach(), vgg_grad=grad, vgg_strength=np.float32(2.5))
    for k, t in enumerate(targets):
        if t.numel() <= 128 * 128:
            out[f"vgg_target{k}"] = t
        else:
            out[f"vgg_target{k}_diag"] = t.diagonal().clone()
            out[f"vgg_target{k}_sum"] = t.double().sum().float()
    # (e)
    seen = []

    def spy_resize(cutout, out_shape):
        seen.append(tuple(cutout.shape[-2:]))
        assert list(out_shape[:2]) == [1, 3] and cutout.shape[0] == 1     # (resize_right applies a full-length out_shape to every dimension:
        return OC.resize(cutout, tuple(out_shape[-2:]))                    #  with one image per call only the two spatial ones change)

    class _Gray:
        def __init__(self, n):
            assert n == 3

        def __call__(self, t):
            return OG.grayscale3(t)
    RC.resize = spy_resize
    RC.T.Grayscale = _Gray
    RC.TF.hflip = lambda t: t.flip(-1)
    for k, (H, W, cs, t, seed) in enumerate(((40, 40, 32, 900, 1), (48, 36, 32, 100, 2), (36, 44, 32, 650, 3), (256, 256, 224, 981, 4))):
        dimg = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(340 + k))    # (re-drawn by the tests for the full-size case)
        dc = RC.DangoCutouts(cs, skip_augs=True)
        torch.manual_seed(seed)
        seen.clear()
        cuts = dc(dimg, t)
        out[f"dango{k}_cfg"] = np.array([H, W, cs, t, seed, dc.cut_overview[999 - t], dc.cut_innercut[999 - t]], dtype=np.int64)
        out[f"dango{k}_grey_p"] = np.float32(dc.cut_icgray_p[999 - t])
        out[f"dango{k}_sizes"] = np.array(seen, dtype=np.int64)
        if H <= 64:
            out[f"dango{k}_img"] = dimg
            out[f"dango{k}_out"] = cuts
        else:
            out[f"dango{k}_sum"] = cuts.double().sum((1, 2, 3)).float()
    # (g) cutouts.py:53-98 Cutouts(skip_augs=True) ("normal"): torchvision's Pad replaced by F.pad; the draws (normal_ + two randint per crop)
    class _Pad:
        def __init__(self, n, fill=0):
            self.n, self.fill = n, fill

        def __call__(self, t):
            return torch.nn.functional.pad(t, (self.n,) * 4, value=self.fill)
    RC.T.Pad = _Pad

    def spy2(cutout, out_shape):
        base = cutout._base if cutout._base is not None else cutout
        W_ = base.shape[-1]
        off = cutout.storage_offset() - base.storage_offset()
        seen.append((cutout.shape[-1], (off // W_) % base.shape[-2], off % W_))
        return OC.resize(cutout, tuple(out_shape[-2:]))
    RC.resize = spy2
    for k, (S, cs, cutn, seed) in enumerate(((32, 32, 8, 11), (40, 32, 12, 12))):
        nimg = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(350 + k))
        torch.manual_seed(seed)
        seen.clear()
        cuts = RC.Cutouts(cs, cutn, skip_augs=True)(nimg, None)
        out[f"normal{k}_cfg"] = np.array([S, cs, cutn, seed], dtype=np.int64)
        out[f"normal{k}_rects"] = np.array([(s_ if s_ else S + 2 * (S // 4), y_, x_) for s_, y_, x_ in seen], dtype=np.int64)
        out[f"normal{k}_out"] = cuts
    # (f)
    rx = torch.rand(1, 3, 256, 256, generator=g) * 2 - 1
    out["resample256_maxdiff"] = (RI.resample(rx, 256) - rx).abs().max()
    save("g34_grads", **out)


QUANTILE_NS = [1, 2, 3, 10, 1001, 65536]
QUANTILE_QS = [0.0, 0.01, 0.025, 0.3, 0.5, 0.75, 0.975, 1.0]


def golden_quantile():
    """g35: the reference's compiled efficient_quantile extension (_efficient_quantile(x, q, True, 3)) on randn vectors of
    QUANTILE_NS lengths drawn in turn from one generator (seed 77); the inputs are regenerated by the test, their first
    and last values are stored as a check."""
    ext = sys.modules["maua.audiovisual.audioreactive.selfsupervised.features.efficient_quantile.efficient_quantile"]
    g = torch.Generator().manual_seed(77)
    ref, first, last = [], [], []
    for n in QUANTILE_NS:
        x = torch.randn(n, generator=g)
        ref.append([ext._efficient_quantile(x, torch.FloatTensor([q]), True, 3).squeeze().item() for q in QUANTILE_QS])
        first.append(x[0].item())
        last.append(x[-1].item())
    save("g35_quantile", ns=np.asarray(QUANTILE_NS, dtype=np.int64), qs=np.asarray(QUANTILE_QS, dtype=np.float64),
         ref=np.asarray(ref, dtype=np.float32), x_first=np.asarray(first, dtype=np.float32),
         x_last=np.asarray(last, dtype=np.float32))


if __name__ == "__main__":
    import_reference()
    which = sys.argv[1:] or ["ops", "modules", "audio", "latents", "noise", "io"]
    with torch.no_grad():
        for w in which:
            globals()[f"golden_{w}"]()
