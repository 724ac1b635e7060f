"""Generate tests/golden/g41_metrics.npz by IMPORTING the reference's maua/GAN/metrics/{frechet,kernel,prdc}.py by file path (authoring
container only; the tests consume the committed .npz).  This script holds no reference code: it runs the reference's own functions on the
CPU, on the ``.double()`` copies of float32 features, and records what they return.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py <reference checkout>

Recorded:
  {a,b,c}_f1, _f2      float32 feature pairs (tests/metrics_ref.py gaussian_pair): a (96, 96, d 24), b (200, 180, d 70), c (64, 80, d 16)
  {a,b,c}_frechet      frechet_distance(f1.double(), f2.double())
  {a,b,c}_kid, _kid_idx, _kid_seed   kernel_distance under np.random.seed(seed) and the indices its np.random.choice calls returned,
                       [S, 2, m] in call order; (S, m) = a (4, 50), b (2, 100), c (3, 64: every row of feats1 is drawn)
  {a,b,c}_prdc         [3, 4]: prdc(f1.double(), f2.double(), k) for k = 1, 3, 5
  lat_*, dup_*         integer lattices in [-8, 8], d 32, 80 and 72 rows (dup_: three rows of each set repeat another): features,
                       prdc for k = 3 (lat_) and k = 1 (dup_), and the twin's integer counts
  signatures           JSON: the reference's argument lists (names and defaults) read from its source with ast, and the command line's
                       flags with their defaults
The script refuses inputs on which the reference alone would be ambiguous: a Newton-Schulz error within 1 % of 1e-5 or an error ratio
within 1 % of 1 before the stop, a relative margin |dist - radius| / radius below 1e-9 on the Gaussian pairs, or a twin that disagrees
with the reference.
"""
import ast
import importlib.util
import json
import sys
from pathlib import Path
from unittest.mock import patch

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import metrics_ref as MR  # noqa: E402

OUT = HERE / "g41_metrics.npz"
PAIRS = {"a": (41, 96, 96, 24, 4, 50), "b": (42, 200, 180, 70, 2, 100), "c": (43, 64, 80, 16, 3, 64)}      # seed, N1, N2, d, S, m
KID_SEED = 1234


def load(root, name):
    spec = importlib.util.spec_from_file_location(f"_ref_metrics_{name}", root / "maua" / "GAN" / "metrics" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def literal(node):
    try:
        return ast.literal_eval(node)
    except ValueError:
        return ast.unparse(node)


def signatures(root):
    out = {}
    for name in ("frechet", "kernel", "prdc", "compute"):
        tree = ast.parse((root / "maua" / "GAN" / "metrics" / f"{name}.py").read_text())
        for fn in (n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and not n.name.startswith("_")):
            args, defaults = [a.arg for a in fn.args.args], [literal(d) for d in fn.args.defaults]
            if args[:1] != ["self"]:
                out[f"{name}.{fn.name}"] = {"args": args, "defaults": dict(zip(args[len(args) - len(defaults):], defaults))}
        if name == "compute":
            flags = {}
            for call in (n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "add_argument"):
                kw = {k.arg: literal(k.value) for k in call.keywords}
                flags[ast.literal_eval(call.args[0])] = {k: kw[k] for k in ("default", "required", "action", "nargs", "choices") if k in kw}
            out["compute.flags"] = flags
    return out


def main():
    root = Path(sys.argv[1])
    fre, ker, prd = load(root, "frechet"), load(root, "kernel"), load(root, "prdc")
    rec = {}
    for tag, (seed, n1, n2, d, S, m) in PAIRS.items():
        f1, f2 = MR.gaussian_pair(seed, n1, n2, d)
        t1, t2 = torch.from_numpy(f1).double(), torch.from_numpy(f2).double()
        rec[f"{tag}_f1"], rec[f"{tag}_f2"] = f1, f2
        rec[f"{tag}_frechet"] = np.float64(fre.frechet_distance(t1, t2))
        info = MR.frechet_info(f1, f2)
        e = np.array(info["errors"], dtype=np.float64)
        assert not info["retried"] and abs(info["distance"] - rec[f"{tag}_frechet"]) <= 1e-9 * info["scale"], (tag, info["distance"])
        assert (np.abs(e / 1e-5 - 1) > 0.01).all() and (np.abs(e[1:] / e[:-1] - 1) > 0.01).all() and e[-1] <= 1e-5, (tag, e)
        print(tag, "frechet", rec[f"{tag}_frechet"], "iterations", info["iterations"], "last errors", e[-2:])

        drawn, choice = [], np.random.choice

        def recording(*a, **k):
            drawn.append(choice(*a, **k))
            return drawn[-1]

        np.random.seed(KID_SEED)
        with patch.object(np.random, "choice", recording):
            rec[f"{tag}_kid"] = np.float64(ker.kernel_distance(t1, t2, num_subsets=S, max_subset_size=m))
        rec[f"{tag}_kid_idx"] = np.stack(drawn).reshape(S, 2, -1).astype(np.int64)
        rec[f"{tag}_kid_seed"] = np.int64(KID_SEED)
        twin = MR.kernel_info(f1, f2, rec[f"{tag}_kid_idx"])
        assert abs(twin["kid"] - rec[f"{tag}_kid"]) <= 1e-10 * abs(twin["abs_sums"]).max() / rec[f"{tag}_kid_idx"].shape[2] ** 2, (tag, twin["kid"])
        print(tag, "kid", rec[f"{tag}_kid"], "subset size", rec[f"{tag}_kid_idx"].shape[2])

        rows = []
        for k in (1, 3, 5):
            rows.append(prd.prdc(t1, t2, nearest_k=k))
            pi = MR.prdc_info(f1, f2, k)
            assert pi["margin"] > 1e-9 and MR.prdc_from_counts(pi["counts"], n1, n2, k) == tuple(rows[-1]), (tag, k, pi["margin"], rows[-1])
            print(tag, "prdc k", k, rows[-1], "margin", pi["margin"])
        rec[f"{tag}_prdc"] = np.array(rows, dtype=np.float64)

    for tag, seed, k, dup in (("lat", 51, 3, 0), ("dup", 52, 1, 3)):
        real, fake = MR.lattice_pair(seed, 80, 72, 32, duplicates=dup)
        out = prd.prdc(torch.from_numpy(real).double(), torch.from_numpy(fake).double(), nearest_k=k)
        pi = MR.prdc_info(real, fake, k)
        assert MR.prdc_from_counts(pi["counts"], 80, 72, k) == tuple(out), (tag, out, pi["counts"])
        rec[f"{tag}_real"], rec[f"{tag}_fake"], rec[f"{tag}_k"] = real.astype(np.int8), fake.astype(np.int8), np.int64(k)
        rec[f"{tag}_prdc"], rec[f"{tag}_counts"] = np.array(out, dtype=np.float64), np.array(pi["counts"], dtype=np.int64)
        print(tag, "prdc", out, "counts", pi["counts"], "zero radii", int((pi["r_real"] == 0).sum()))

    rec["signatures"] = np.array(json.dumps(signatures(root), sort_keys=True))
    np.savez_compressed(OUT, **rec)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
