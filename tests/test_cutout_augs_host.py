"""Host side of the augmented "normal" / "dango" cutouts (maua/ops/cutouts.py:53-206 with skip_augs=False, their default): the plans
maua_amd.grad draws from torch's global generator against the draws the REFERENCE's own classes made (tests/golden/g36_cutout_augs.npz,
tests/golden/make_golden_augs.py), the generator's end state, the CPU restatement of torchvision against the reference's outputs, and
the library's refusal of bad records (checked on the host, before any device is touched)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import torchvision_augs_ref as TA  # noqa: E402
from oracle import clip as OC  # noqa: E402


def g36():
    z = np.load(Path(__file__).resolve().parent / "golden" / "g36_cutout_augs.npz")
    return {k: z[k] for k in z.files}


def test_normal_plan_equals_the_reference_draws():
    from maua_amd.grad import Cutouts
    g = g36()
    for k in range(2):
        S, cs, cutn, seed = (int(v) for v in g[f"normal{k}_cfg"])
        P = S + 2 * Cutouts.pad_of(S)
        torch.manual_seed(seed)
        rects, augs = Cutouts(cs, cutn).plan(P, P)
        after = torch.rand(4)
        assert np.array_equal(np.asarray(rects), g[f"normal{k}_rects"]), k
        assert augs.shape == (cutn, TA.AUG_REC) and augs.dtype == np.float32
        assert np.array_equal(augs, g[f"normal{k}_augs"]), (k, np.abs(augs - g[f"normal{k}_augs"]).max())
        assert torch.equal(after, torch.from_numpy(g[f"normal{k}_rand_after"])), k


def test_dango_plan_equals_the_reference_draws():
    from maua_amd.grad import DangoCutouts
    g = g36()
    for k in range(2):
        S, cs, t, seed, overview, inner = (int(v) for v in g[f"dango{k}_cfg"])
        dc = DangoCutouts(cs)
        torch.manual_seed(seed)
        rects, augs = dc.aug_plan(S, S, t)
        after = torch.rand(4)
        assert len(rects) == overview + inner
        inner_seen = g[f"dango{k}_sizes"][-inner:]
        mine = np.array([(r[0] & ((1 << 24) - 1), r[1], r[2]) for r in rects[overview:]])
        grey = np.array([(r[0] & (1 << 30)) != 0 for r in rects[overview:]])
        assert grey.any() and np.array_equal(mine[:, 0], inner_seen[:, 0]), k
        # (a grey crop reaches the resize as a new tensor: its offsets are not recoverable from the view)
        assert np.array_equal(mine[~grey], inner_seen[~grey]), k
        assert np.array_equal(augs, g[f"dango{k}_augs"]), k
        assert torch.equal(after, torch.from_numpy(g[f"dango{k}_rand_after"])), k


def test_the_restatement_reproduces_the_reference_outputs():
    """The CPU pipeline (tests/torchvision_augs_ref.py) applied with g36's draws, crops and Philox noise gives the reference's outputs."""
    g = g36()
    for k in range(2):
        S, cs, cutn, seed = (int(v) for v in g[f"normal{k}_cfg"])
        img = torch.from_numpy(g[f"normal{k}_img"])
        key = int(g[f"normal{k}_key"])
        p = S // 4
        padded = torch.nn.functional.pad(img, (p,) * 4)
        outs = []
        for j, ((s, y, x), rec) in enumerate(zip(g[f"normal{k}_rects"], g[f"normal{k}_augs"])):
            crop = padded[:, :, y:y + s, x:x + s]
            outs.append(OC.resize(TA.augment(crop, rec, TA.philox_noise(key, j, crop.shape)), (cs, cs)))
        got = torch.cat(outs)
        assert float((got - torch.from_numpy(g[f"normal{k}_out"])).abs().max()) <= 1e-6, k
    for k in range(2):
        S, cs, t, seed, overview, inner = (int(v) for v in g[f"dango{k}_cfg"])
        from maua_amd.grad import DangoCutouts
        from oracle import grads as OG
        img = torch.from_numpy(g[f"dango{k}_img"])
        torch.manual_seed(seed)
        plan = DangoCutouts(cs, skip_augs=True).plan(S, S, t)
        cuts = OG.dango_cutouts(img, plan, cs, OC.resize)
        got = TA.augment(cuts, g[f"dango{k}_augs"][0], TA.philox_noise(int(g[f"dango{k}_key"]), 0, cuts.shape))
        assert float((got - torch.from_numpy(g[f"dango{k}_out"])).abs().max()) <= 1e-6, k


def test_skip_augs_plans_are_unchanged():
    """skip_augs=True draws exactly what it drew before: the crops only, in the same order, leaving the generator in the same state."""
    from maua_amd.grad import Cutouts, DangoCutouts
    torch.manual_seed(5)
    rects, augs = Cutouts(32, 8, skip_augs=True).plan(60, 60)
    a1 = torch.rand(3)
    torch.manual_seed(5)
    want = []
    for ch in range(8):
        if ch > 8 - 2:
            want.append((60, 0, 0))
        else:
            size = int(60 * torch.zeros(1,).normal_(mean=0.8, std=0.3).clip(float(32 / 60), 1.0))
            ox = int(torch.randint(0, abs(60 - size + 1), ()))
            oy = int(torch.randint(0, abs(60 - size + 1), ()))
            want.append((size, oy, ox))
    assert augs is None and rects == want and torch.equal(a1, torch.rand(3))
    dc = DangoCutouts(32, skip_augs=True)
    torch.manual_seed(6)
    r1, a = dc.aug_plan(48, 48, 300)
    s1 = torch.rand(2)
    torch.manual_seed(6)
    assert a is None and r1 == dc.rects(48, 48, 300) and torch.equal(s1, torch.rand(2))


def test_constructors_take_the_reference_defaults():
    from maua_amd.grad import CLIPGrads, Cutouts, DangoCutouts, make_cutouts
    assert not Cutouts(32, 8).skip_augs and not DangoCutouts(32).skip_augs
    assert not make_cutouts("normal", 32, 8).skip_augs
    for mode in ("None", "2D", "3D"):
        with pytest.raises(NotImplementedError, match="ColorJitter"):
            DangoCutouts(32, animation_mode=mode)
        DangoCutouts(32, animation_mode=mode, skip_augs=True)
    # augmented cutouts are never merged; the plain rule is unchanged
    r = np.array([[[40, 0, 0]] * 2 + [[20 + i, 1, 2] for i in range(6)]], dtype=np.int32)
    assert CLIPGrads.merge_identical(r)[1] is not None
    assert CLIPGrads.merge_identical(r, np.zeros((1, 8, 17), np.float32))[1] is None


def _refusal(rec):
    """maua_cutouts_aug with a NULL context: the records are checked first, so a bad one is named; a good one reaches the ctx check."""
    from maua_amd import _lib as L
    rects = np.array([[8, 0, 0]], dtype=np.int32)
    augs = np.ascontiguousarray(np.asarray(rec, dtype=np.float32).reshape(1, 17))
    one3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    rc = L.lib().maua_cutouts_aug(None, C.c_void_p(16), 1, 8, 8, rects.ctypes.data_as(C.c_void_p), 1, 8, C.c_float(1.0), C.c_float(0.0),
                                  one3, one3, augs.ctypes.data_as(C.c_void_p), C.c_ulonglong(1), 0, C.c_void_p(16))
    return rc, L.lib().maua_last_error().decode()


def test_bad_records_are_refused():
    good = np.zeros(17, np.float32)
    good[1:7] = [1, 0, 0, 0, 1, 0]
    rc, msg = _refusal(good)
    assert rc != 0 and "ctx" in msg and "record" not in msg
    bad = []
    r = good.copy(); r[0] = 0.5; bad.append(r)                       # flip not a bit
    r = good.copy(); r[16] = 2; bad.append(r)                        # grey not a bit
    r = good.copy(); r[7] = -1; bad.append(r)                        # perspective flag not a bit
    r = good.copy(); r[3] = np.nan; bad.append(r)                    # non-finite matrix
    r = good.copy(); r[1:7] = 0; bad.append(r)                       # singular matrix
    r = good.copy(); r[7] = 1; r[8:16] = [1, 0, 0, 0, 1, 0, np.inf, 0]; bad.append(r)   # non-finite coefficients
    for b in bad:
        rc, msg = _refusal(b)
        assert rc != 0 and "record 0" in msg, msg
