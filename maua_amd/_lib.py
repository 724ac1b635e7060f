"""ctypes binding of libmaua_hip.so — the only thing the Python host code talks to.

There is NO CPU fallback: if the shared library is missing or no HIP device is visible every
operator raises.  (The CPU oracle lives under /oracle and is test infrastructure only.)
"""
import ctypes as C
import functools
import os
import re
import threading
from pathlib import Path

import torch

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MAUA_HIP_LIB", _HERE / "csrc" / "libmaua_hip.so"))
HEADER = _HERE.parent / "include" / "maua_hip.h"

F32, BF16, F16 = 0, 1, 2
F32_SPLIT = 3   # float32 tensors, products as bf16 split products (maua_secondary_create only)
ACTS = {"linear": 0, "relu": 1, "lrelu": 2, "tanh": 3, "sigmoid": 4, "elu": 5, "selu": 6, "softplus": 7, "swish": 8}
PAD_MODES = {"circular": 0, "reflect": 1, "replicate": 2, "constant": 3}
VFEAT_LAYOUTS = {"u8_hwc": 0, "u8_chw": 1, "f32_chw": 2}
CORR_METRICS = {"pearson": 0, "concordance": 1, "autocorrcorr": 2, "rv": 3, "rv2": 4, "r1": 5}


class MauaHipError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()
_ctxs = {}

# ---- the binding: include/maua_hip.h is the one place a signature is written -----------------------------------------------------------
_CTYPES = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "unsigned long long": C.c_ulonglong, "const char*": C.c_char_p}


def ctype_of(ctype, where):
    """A C type of the header as ctypes.  Every pointer but ``const char*`` is c_void_p: it takes ptr(t), None, byref(x), ctypes arrays,
    integer addresses and bytes alike.  An unknown scalar is an error, never an int."""
    t = " ".join(ctype.replace("*", " * ").split()).replace(" *", "*")
    if t not in _CTYPES and not t.endswith("*"):
        raise MauaHipError(f"{where}: no ctypes type for the C type '{t}' (include/maua_hip.h)")
    return _CTYPES.get(t, C.c_void_p)


def declaration(header, name):
    """One function's declaration as the header writes it: (return type, [parameter, ...]).  It is looked up, not tabulated - the first
    ` name(` outside a comment, its return type in front of it on the same line, its parameters up to the `;` - so a process pays for the
    functions it calls and not for the 114 KB header: preprocessor lines, enum blocks and struct bodies are never looked at.  The header is
    searched as bytes, because decoding all of it costs more than the lookups of a whole run."""
    if isinstance(header, str):
        header = header.encode()
    key, at = b" %s(" % name.encode(), -1
    while True:
        at = header.find(key, at + 1)
        if at < 0:
            raise MauaHipError(f"{name} is not declared in include/maua_hip.h")
        if header.rfind(b"/*", 0, at) <= header.rfind(b"*/", 0, at):      # not a mention inside a comment
            break
    ret = header[header.rfind(b"\n", 0, at) + 1:at].decode()
    rest = header[at + len(key):header.find(b";", at)]
    params = b" ".join([piece.partition(b"/*")[0] for piece in rest.split(b"*/")]).decode().rstrip()   # `int aggregate /* 0 = mean */, float* env`
    if not ret.strip() or not params.endswith(")") or "(" in params:
        raise MauaHipError(f"include/maua_hip.h: cannot parse the declaration of {name}: '{ret} {name}({params};'")
    return ret, [] if params[:-1].strip() == "void" else params[:-1].split(",")


def signature(header, name):
    """(restype, [argtypes]) of a function the header (bytes or str) declares; a parameter's type is what stands in front of its name."""
    ret, params = declaration(header, name)
    restype = None if ret.strip() == "void" else ctype_of(ret, name)
    return restype, [ctype_of(p.replace("*", "* ").rsplit(None, 1)[0], name) for p in params]


def declared_names(text):
    """every maua_* name that stands in front of a `(` outside a comment"""
    return sorted(set(re.findall(r"\b(maua_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))


def parse_header(text):
    """name -> (restype, [argtypes]) for every function the header text declares"""
    header = text.encode()
    return {name: signature(header, name) for name in declared_names(text)}


_header = functools.lru_cache(maxsize=None)(lambda: HEADER.read_bytes())


def declared_symbols():
    """Every function the C header declares (used by the export test)."""
    return declared_names(_header().decode())


class _Library(C.CDLL):
    """libmaua_hip.so; a function gets its restype and argtypes from the header when it is first looked up (ctypes keeps it from then on)."""

    def __getitem__(self, name):
        restype, argtypes = signature(_header(), name)
        fn = super().__getitem__(name)
        fn.restype, fn.argtypes = restype, argtypes
        return fn


def lib():
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not LIB_PATH.exists():
                    raise MauaHipError(
                        f"{LIB_PATH} not found: build it with `python -m maua_amd.build` (hipcc, gfx950). "
                        "maua_amd has no CPU fallback.")
                _lib = _Library(str(LIB_PATH))
    return _lib


class host_threads:
    """Context manager / decorator: run host-side tensor prep on at most ``n`` intra-op threads.  The host work of this
    package is small tensors (512 x 512 matrices, filter banks, seeds); on a 128-thread box torch's pool costs ~100 ms to
    spin up and milliseconds of fork/join per tiny operator (measured: MappingNetwork init 100 -> 7 ms, its forward 13 .. 71
    -> 3 ms, get_z_latents 95 -> 6 ms, a CQT's filter banks 290 -> 40 ms); results are identical."""

    def __init__(self, n=1):
        self.n = n

    def __enter__(self):
        self.prev = torch.get_num_threads()
        if self.prev > self.n:
            torch.set_num_threads(self.n)
        return self

    def __exit__(self, *exc):
        if torch.get_num_threads() != self.prev:
            torch.set_num_threads(self.prev)

    def __call__(self, fn):
        import functools

        @functools.wraps(fn)
        def wrapped(*a, **k):
            with host_threads(self.n):
                return fn(*a, **k)
        return wrapped


def check(rc):
    if rc != 0:
        raise MauaHipError(lib().maua_last_error().decode())


def require_device():
    if not torch.cuda.is_available():
        raise MauaHipError("no HIP device visible (torch.cuda.is_available() is False); maua_amd has no CPU fallback")


def ctx(device=None):
    """Per-device context bound to torch's current HIP stream."""
    require_device()
    if device is None:
        dev = torch.cuda.current_device()
    elif isinstance(device, int):
        dev = device
    else:
        dev = torch.device(device).index
        if dev is None:
            dev = torch.cuda.current_device()
    stream = torch.cuda.current_stream(dev).cuda_stream
    c = _ctxs.get(dev)
    if c is None:
        p = C.c_void_p()
        check(lib().maua_ctx_create(dev, stream, C.byref(p)))
        c = _ctxs[dev] = p
    else:
        check(lib().maua_ctx_set_stream(c, stream))
    return c


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def dtype_id(t):
    dt = t if isinstance(t, torch.dtype) else t.dtype
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:   # the reference's own render dtype (render/ffmpeg.py:45): operator layer + synthesis network
        return F16
    raise MauaHipError(f"unsupported dtype {dt}: use float32, bfloat16 or float16")


def dev_tensor(t, dtype=None):
    """contiguous tensor on the current HIP device (uploading if the caller handed a CPU tensor)."""
    require_device()
    if dtype is None:
        dtype = t.dtype
    if t.device.type == "cuda":
        return t.to(dtype=dtype).contiguous()
    return t.to(device="cuda", dtype=dtype).contiguous()


class GemmDesc(C.Structure):
    """maua_gemm_desc (include/maua_hip.h): one GEMM for maua_gemm_nt_route / maua_gemm_nt_ex; pointers as integers."""
    _fields_ = [("a0", C.c_void_p), ("lda0", C.c_long), ("K0", C.c_int),
                ("a1", C.c_void_p), ("lda1", C.c_long), ("K1", C.c_int),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p), ("ldr", C.c_long),
                ("c", C.c_void_p), ("ldc", C.c_long), ("M", C.c_long), ("N", C.c_int),
                ("epi", C.c_int), ("c2", C.c_void_p), ("ldc2", C.c_long), ("aux", C.c_void_p), ("ldaux", C.c_long),
                ("batch", C.c_int), ("a_bstride", C.c_long), ("w_bstride", C.c_long), ("c_bstride", C.c_long)]


class ConvDesc(C.Structure):
    """maua_conv_desc (include/maua_hip.h): one plain 3x3 convolution for maua_conv3x3_route / maua_conv3x3_ex; pointers as integers."""
    _fields_ = [("x", C.c_void_p), ("x_pstride", C.c_int), ("x_bstride", C.c_long),
                ("w", C.c_void_p), ("bias", C.c_void_p),
                ("y", C.c_void_p), ("y_pstride", C.c_int), ("y_coff", C.c_int), ("y_bstride", C.c_long),
                ("res", C.c_void_p), ("res_pstride", C.c_int), ("res_bstride", C.c_long),
                ("res2", C.c_void_p), ("res2_pstride", C.c_int), ("res2_bstride", C.c_long), ("res_gain", C.c_float),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Ci", C.c_int), ("Co", C.c_int),
                ("act", C.c_int), ("alpha", C.c_float), ("gain", C.c_float), ("clamp", C.c_float),
                ("Ci_read", C.c_int), ("x_up2", C.c_int), ("variant", C.c_int),
                ("psum", C.c_void_p)]


class SConvDesc(C.Structure):
    """maua_sconv_desc (include/maua_hip.h): one convolution of the ResNet backbone for maua_conv_strided_ex; pointers as integers."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p), ("y", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Ci", C.c_int), ("Co", C.c_int),
                ("k", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("relu", C.c_int)]


class ModconvDesc(C.Structure):
    """maua_modconv_desc (include/maua_hip.h): one modulated 3x3 layer for maua_modconv_route / maua_modconv_ex; pointers as integers."""
    _fields_ = [("x", C.c_void_p), ("x_bstride", C.c_long),
                ("w", C.c_void_p), ("flip", C.c_int),
                ("s", C.c_void_p), ("d", C.c_void_p),
                ("noise", C.c_void_p), ("noise_bstride", C.c_long), ("noise_strength", C.c_float), ("noise_scale", C.c_void_p),
                ("bias", C.c_void_p),
                ("y", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Ci", C.c_int), ("Co", C.c_int), ("up", C.c_int),
                ("act", C.c_int), ("alpha", C.c_float), ("gain", C.c_float), ("clamp", C.c_float),
                ("out_scale", C.c_void_p), ("y_scaled", C.c_void_p),
                ("rgb_wmod", C.c_void_p), ("rgb_bias", C.c_void_p), ("rgb_prev", C.c_void_p), ("rgb_out", C.c_void_p),
                ("rgb_clamp", C.c_float),
                ("rgb8_out", C.c_void_p), ("rgb_skip_f32", C.c_int),
                ("t", C.c_void_p)]


class AttnDesc(C.Structure):
    """maua_attn_desc (include/maua_hip.h): one attention forward for maua_attention_check / maua_attention_ex; pointers as integers."""
    _fields_ = [("qkv", C.c_void_p), ("out", C.c_void_p), ("lse", C.c_void_p),
                ("B", C.c_int), ("T", C.c_int), ("heads", C.c_int), ("head_ch", C.c_int), ("ld_qkv", C.c_long), ("ld_out", C.c_long),
                ("scale", C.c_float), ("causal", C.c_int), ("dtype", C.c_int)]


class AttnVjpDesc(C.Structure):
    """maua_attn_vjp_desc (include/maua_hip.h): its input gradient for maua_attention_vjp_check / maua_attention_vjp_ex."""
    _fields_ = [("qkv", C.c_void_p), ("out", C.c_void_p), ("d_out", C.c_void_p), ("lse", C.c_void_p), ("d_qkv", C.c_void_p),
                ("delta", C.c_void_p),
                ("B", C.c_int), ("T", C.c_int), ("heads", C.c_int), ("head_ch", C.c_int), ("ld_qkv", C.c_long), ("ld_out", C.c_long),
                ("scale", C.c_float), ("causal", C.c_int), ("dtype", C.c_int)]


class GnDesc(C.Structure):
    """maua_gn_desc (include/maua_hip.h): one fused GroupNorm pass for maua_group_norm_check / _plan / _ex; pointers as integers."""
    _fields_ = [("x0", C.c_void_p), ("C0", C.c_int), ("x1", C.c_void_p), ("C1", C.c_int), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("ss", C.c_void_p), ("ss_ld", C.c_long),
                ("silu", C.c_int), ("mode", C.c_int), ("y", C.c_void_p), ("xr", C.c_void_p),
                ("ps0", C.c_void_p), ("rows0", C.c_int), ("ps1", C.c_void_p), ("rows1", C.c_int),
                ("stats_out", C.c_void_p), ("force_route", C.c_int), ("dtype", C.c_int)]


class GnVjpDesc(C.Structure):
    """maua_gn_vjp_desc (include/maua_hip.h): its input gradient for maua_group_norm_vjp_check / _plan / _ex."""
    _fields_ = [("x0", C.c_void_p), ("C0", C.c_int), ("x1", C.c_void_p), ("C1", C.c_int),
                ("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("ss", C.c_void_p), ("ss_ld", C.c_long),
                ("silu", C.c_int), ("mode", C.c_int), ("dy", C.c_void_p), ("dres", C.c_void_p), ("add0", C.c_void_p),
                ("add1", C.c_void_p), ("dx0", C.c_void_p), ("dx1", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int)]


class FbDesc(C.Structure):
    """maua_farneback_desc (include/maua_hip.h): one estimator run for maua_farneback_check / _pair_ex; pointers as integers."""
    _fields_ = [("im_a", C.c_void_p), ("im_b", C.c_void_p), ("H", C.c_int), ("W", C.c_int),
                ("flow_ab", C.c_void_p), ("flow_ba", C.c_void_p),
                ("level_hi", C.c_int), ("level_lo", C.c_int), ("iterations", C.c_int),
                ("init_ab", C.c_void_p), ("init_ba", C.c_void_p),
                ("gray", C.c_void_p), ("blur", C.c_void_p), ("level", C.c_void_p), ("coef", C.c_void_p), ("flow_in", C.c_void_p),
                ("mat", C.c_void_p)]


class NcaDesc(C.Structure):
    """maua_nca_desc (include/maua_hip.h); pointers as integers."""
    _fields_ = [("x", C.c_void_p), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p),
                ("n_steps", C.c_int), ("rate", C.c_float), ("rate_map", C.c_void_p), ("u", C.c_void_p),
                ("seed", C.c_ulonglong), ("stream", C.c_ulonglong), ("step0", C.c_ulonglong),
                ("col0", C.c_int), ("W_sub", C.c_int), ("margin", C.c_int), ("steps_per_launch", C.c_int)]


# routes of maua_modconv_route / maua_modconv_ex and of maua_synth_get_plan (csrc/synth.hip's Route enum; UPFIR: the FIR / epilogue pass alone)
ROUTES = {"lowres": 0, "generic": 1, "dma_conv1": 2, "hires": 3, "upwalk": 4, "fused_walk": 5, "walk_done": 6, "tconv_fir": 7,
          "tconv_dma": 8, "tconv2": 9, "upfir": 10}
