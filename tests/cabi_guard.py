"""Guarded buffers and calls for the tests that drive the C ABI directly (tests/test_gpu_audio_kernels.py,
tests/test_gpu_latent_kernels.py, tests/test_gpu_segment_kernels.py, tests/test_gpu_diffusion_kernels.py): G = 4096 guard elements on both sides of every buffer (NaN around
inputs, a sentinel bit pattern in outputs), so that after a call the guards are intact, the body is fully written and no NaN leaked
in.  A plain module, imported by name; it holds no test and no fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

DEV = "cuda"
G = 4096                                            # guard elements on either side of every buffer
SENT = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Buf:
    """n elements between guard regions.  Inputs (data given): `guard` (NaN) around them.  Outputs: a sentinel bit pattern everywhere;
    check() wants the guards as they were, and of an output every element written and no NaN."""

    def __init__(self, n, dtype=torch.float32, data=None, guard=float("nan")):
        self.n, self.out = int(n), data is None
        self.full = torch.empty((2 * G + self.n,), dtype=dtype, device=DEV)
        self.es = self.full.element_size()
        if data is None:
            self._bits().fill_(SENT[self.es])
        else:
            self.full.fill_(guard)
            if self.n:
                self.full[G:G + self.n] = torch.as_tensor(np.ascontiguousarray(data)).reshape(-1).to(dtype).to(DEV)
        b = self._bits()
        self.guards = (b[:G].clone(), b[G + self.n:].clone())
        self.ptr = C.c_void_p(self.full.data_ptr() + G * self.es)

    def _bits(self):
        return self.full.view(BITS[self.es])

    def get(self):
        body = self.full[G:G + self.n]
        return (body.float() if body.dtype == torch.bfloat16 else body).cpu().numpy()      # (numpy has no bfloat16: its float32 value)

    def check(self, what, nan_ok=False, written=None):
        b = self._bits()
        assert torch.equal(b[:G], self.guards[0]) and torch.equal(b[G + self.n:], self.guards[1]), f"{what}: a store outside the buffer"
        if self.out if written is None else written:
            assert bool((b[G:G + self.n] != SENT[self.es]).all()), f"{what}: elements of the result were never written"
        if self.out and not nan_ok and self.full.is_floating_point():
            assert not bool(torch.isnan(self.full[G:G + self.n]).any()), f"{what}: NaN in the result (a guard was read)"

    def untouched(self):
        return bool((self._bits() == SENT[self.es]).all())


def inp(a, dtype=torch.float32, **kw):
    a = np.asarray(a)
    return Buf(a.size, dtype, data=a, **kw)


def cbuf(z):
    """a complex array as interleaved float32 (the values must be float32 numbers)"""
    z = np.asarray(z)
    ri = np.stack((z.real, z.imag), -1).astype(np.float32)
    assert np.array_equal(ri.astype(np.float64), np.stack((z.real, z.imag), -1).astype(np.float64))
    return inp(ri)


def call(name, *args):
    L.check(getattr(L.lib(), name)(L.ctx(), *args))
    torch.cuda.synchronize()


def refused(name, *args):
    """the entry point returns an error (a host-side check, before any launch) and L.check raises it"""
    rc = getattr(L.lib(), name)(L.ctx(), *args)
    assert rc != 0, f"{name} accepted {args}"
    with pytest.raises(L.MauaHipError):
        L.check(rc)
    torch.cuda.synchronize()


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.isfinite(err).all()
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0


def same(got, want):
    """bit for bit up to the sign of zero; NaN equals NaN"""
    return np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)
