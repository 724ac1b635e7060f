"""GAN evaluation metrics on the device (drop-in for maua/GAN/metrics/{frechet,kernel,prdc,compute}.py).

Frechet distance, kernel distance (KID) and precision / recall / density / coverage (PRDC) between the features of real images and of
generated ones.  Everything runs in float64 on the library's f64 matrix-core GEMM (csrc/gemm_f64.hip): float32 features are widened on
load, float64 features are taken as they are.  Features are device tensors and stay there; only scalars come back.  There is no CPU path:
without a device every function raises ``MauaHipError``.

Extractors of ``compute``: a callable, a (module, size) pair, ``"CLIP:<tower>"`` and ``"SwAV:<checkpoint>"`` (``"SwAV-bf16:<checkpoint>"``
in bfloat16) - the reference's SwAV ResNet-50 (maua_amd.resnet) with the weights read from a local file: they are not bundled, like CLIP's.

Not built (each raises ``NotImplementedError`` by name): ``symsqrtm`` (an SVD, unused by ``frechet_distance``), the ``"Inception"`` extractor
(its Inception-v3 forward is not part of this build; its checkpoint is a TorchScript archive) and the bare ``"SwAV"`` spelling, which
would have to download its weights.
"""
import ctypes as C
import glob as _glob
import os
from pathlib import Path
from zipfile import ZipFile

import numpy as np
import torch

from . import _lib as L

MAX_NEAREST_K = 15
SIZE = 224      # compute.py:22: what a folder's images are resized to when the extractor states no size of its own
EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp", "npy"}
UNBUILT_EXTRACTORS = {"SwAV": "its weights (swav_800ep_pretrain.pth.tar) are not bundled and are never downloaded: name a local file as "
                              "'SwAV:<checkpoint>' ('SwAV-bf16:<checkpoint>' in bfloat16)",
                      "Inception": "its Inception-v3 forward (extractors/inception.py) is not part of this build"}


def _features(t, name):
    """[rows, d] device tensor, float32 or float64, contiguous -> (tensor, f64 flag)"""
    L.require_device()
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    if t.dim() != 2:
        raise ValueError(f"{name}: features must be [rows, d], got {tuple(t.shape)}")
    t = L.dev_tensor(t, torch.float64 if t.dtype == torch.float64 else torch.float32)
    return t, int(t.dtype == torch.float64)


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device), int(nbytes)


def gemm_f64(a, b, transa=False, transb=False, alpha=1.0, beta=0.0, out=None, M=None, N=None, K=None, lda=None, ldb=None, ldc=None):
    """``out = alpha * op(a) @ op(b) + beta * out`` in float64 (maua_gemm_f64).  a and b are 2-D float64 device tensors as stored;
    M, N, K and the leading dimensions default to what their shapes say, and may be given to multiply a corner of wider storage."""
    L.require_device()
    a, b = L.dev_tensor(a, torch.float64), L.dev_tensor(b, torch.float64)
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError("gemm_f64: a and b must be 2-D")
    lda = int(a.shape[1]) if lda is None else int(lda)
    ldb = int(b.shape[1]) if ldb is None else int(ldb)
    M = int(a.shape[1] if transa else a.shape[0]) if M is None else int(M)
    K = int(a.shape[0] if transa else a.shape[1]) if K is None else int(K)
    N = int(b.shape[0] if transb else b.shape[1]) if N is None else int(N)
    need_a = ((K - 1) * lda + M) if transa else ((M - 1) * lda + K)
    need_b = ((N - 1) * ldb + K) if transb else ((K - 1) * ldb + N)
    if min(M, N, K) < 1 or need_a > a.numel() or need_b > b.numel():
        raise ValueError(f"gemm_f64: M, N, K = {M}, {N}, {K} with lda = {lda}, ldb = {ldb} do not fit a {tuple(a.shape)} and b {tuple(b.shape)}")
    if out is None:
        if beta != 0.0:
            raise ValueError("gemm_f64: beta != 0 needs out=")
        out = torch.empty((M, N), dtype=torch.float64, device=a.device)
    ldc = int(out.shape[1]) if ldc is None else int(ldc)
    if out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous() or out.dim() != 2 or (M - 1) * ldc + N > out.numel():
        raise ValueError("gemm_f64: out must be a contiguous float64 device tensor that holds M rows of ldc")
    L.check(L.lib().maua_gemm_f64(L.ctx(a.device), int(bool(transa)), int(bool(transb)), M, N, K, float(alpha), L.ptr(a), lda, L.ptr(b), ldb,
                                  float(beta), L.ptr(out), ldc))
    return out


def moments(feats):
    """(mean [d], cov [d, d]) in float64: ``torch.mean(feats, axis=0)`` and ``torch.cov(feats.T)`` (frechet.py:73-74)."""
    x, f64 = _features(feats, "moments")
    N, d = map(int, x.shape)
    lib = L.lib()
    ws, nbytes = _workspace(lib.maua_metrics_moments_workspace(N, d), x.device)
    mean = torch.empty(d, dtype=torch.float64, device=x.device)
    cov = torch.empty((d, d), dtype=torch.float64, device=x.device)
    L.check(lib.maua_metrics_moments(L.ctx(x.device), L.ptr(x), f64, N, d, L.ptr(ws), nbytes, L.ptr(mean), L.ptr(cov)))
    return mean, cov


def sqrtm_info(matrix, num_iters=100):
    """The Newton-Schulz square root with its record: (S float64 [d, d], [error of every iteration run], iterations)."""
    L.require_device()
    if matrix.dim() != 2:
        raise ValueError(f"Input dimension equals {matrix.dim()}, expected 2")
    if num_iters <= 0:
        raise ValueError(f"Number of iteration equals {num_iters}, expected greater than 0")
    m = L.dev_tensor(matrix, torch.float64)
    d = int(m.shape[0])
    if int(m.shape[1]) != d:
        raise ValueError(f"sqrtm: the matrix must be square, got {tuple(m.shape)}")
    lib = L.lib()
    ws, nbytes = _workspace(lib.maua_sqrtm_workspace(d), m.device)
    s = torch.empty_like(m)
    errors, iters = (C.c_double * int(num_iters))(), C.c_int()
    L.check(lib.maua_sqrtm_newton_schulz(L.ctx(m.device), L.ptr(m), d, int(num_iters), L.ptr(ws), nbytes, L.ptr(s), errors, C.byref(iters)))
    return s, list(errors[:iters.value]), iters.value


def sqrtm(matrix, num_iters=100):
    """frechet.py:4-46: square root of a matrix by the Newton-Schulz iteration, in float64, returned in the matrix's dtype."""
    return sqrtm_info(matrix, num_iters)[0].to(matrix.dtype)


def symsqrtm(matrix):
    """Not built: frechet.py:49-58 is a singular value decomposition, and the library has none (frechet_distance does not use it)."""
    raise NotImplementedError("symsqrtm is not built: it needs a singular value decomposition (frechet.py:49-58), and the library has none; "
                              "sqrtm (Newton-Schulz) is what frechet_distance uses")


def frechet_info(feats1, feats2, eps=1e-6, num_iters=100):
    """frechet_distance with its record: a dict of distance, the Newton-Schulz errors, iterations and whether the eps retry ran."""
    x1, f64 = _features(feats1, "frechet_distance")
    x2, f64b = _features(feats2, "frechet_distance")
    if f64 != f64b:
        x1, x2, f64 = x1.double(), x2.double(), 1
    assert x1.shape[1] == x2.shape[1], "Training and test mean vectors have different lengths"
    N1, N2, d = int(x1.shape[0]), int(x2.shape[0]), int(x1.shape[1])
    lib = L.lib()
    ws, nbytes = _workspace(lib.maua_frechet_workspace(N1, N2, d), x1.device)
    dist, errors, iters, retried = C.c_double(), (C.c_double * int(num_iters))(), C.c_int(), C.c_int()
    L.check(lib.maua_frechet_distance(L.ctx(x1.device), L.ptr(x1), N1, L.ptr(x2), N2, d, f64, float(eps), int(num_iters), L.ptr(ws), nbytes,
                                      C.byref(dist), errors, C.byref(iters), C.byref(retried)))
    if retried.value:
        print(f"Frechet distance calculation produced singular product; adding {eps} to diagonal of cov estimates")
    return {"distance": dist.value, "errors": list(errors[:iters.value]), "iterations": iters.value, "retried": bool(retried.value)}


def frechet_distance(feats1, feats2, eps=1e-6):
    """frechet.py:61-94: ``|mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2))`` between the Gaussians fitted to two feature sets -> float."""
    return frechet_info(feats1, feats2, eps)["distance"]


def draw_subsets(n1, n2, num_subsets=100, max_subset_size=1000):
    """kernel.py:9-13's draws, in its call order (the feats2 subset first, then feats1's) -> int64 [num_subsets, 2, m].  Under the same
    ``np.random.seed`` these are the reference's subsets."""
    m = min(min(n1, n2), max_subset_size)
    idx = np.empty((num_subsets, 2, m), dtype=np.int64)
    for s in range(num_subsets):
        idx[s, 0] = np.random.choice(n2, m, replace=False)
        idx[s, 1] = np.random.choice(n1, m, replace=False)
    return idx


def kernel_info(feats1, feats2, num_subsets=100, max_subset_size=1000, indices=None):
    """kernel_distance with its record: a dict of kid, the indices drawn [S, 2, m] and per subset the sums ``a.sum()``, ``a.diag().sum()``,
    ``b.sum()`` of kernel.py:14-16 (float64 [S, 3], on the host)."""
    x1, f64 = _features(feats1, "kernel_distance")
    x2, f64b = _features(feats2, "kernel_distance")
    if f64 != f64b:
        x1, x2, f64 = x1.double(), x2.double(), 1
    if x1.shape[1] != x2.shape[1]:
        raise ValueError(f"kernel_distance: feature widths differ, {x1.shape[1]} and {x2.shape[1]}")
    N1, N2, d = int(x1.shape[0]), int(x2.shape[0]), int(x1.shape[1])
    if indices is None:
        indices = draw_subsets(N1, N2, num_subsets, max_subset_size)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    S, two, m = indices.shape
    if two != 2 or indices[:, 0].min() < 0 or indices[:, 0].max() >= N2 or indices[:, 1].min() < 0 or indices[:, 1].max() >= N1:
        raise ValueError("kernel_distance: indices must be [S, 2, m] with rows of feats2 in [:, 0] and rows of feats1 in [:, 1]")
    lib = L.lib()
    idx = torch.from_numpy(indices).to(x1.device)
    ws, nbytes = _workspace(lib.maua_kernel_distance_workspace(m, d), x1.device)
    out = torch.empty(1 + 3 * S + 6 * S, dtype=torch.float64, device=x1.device)
    kid, sums, raw = out[:1], out[1:1 + 3 * S], out[1 + 3 * S:]
    L.check(lib.maua_kernel_distance(L.ctx(x1.device), L.ptr(x1), N1, L.ptr(x2), N2, d, f64, L.ptr(idx), S, m, L.ptr(ws), nbytes,
                                     L.ptr(kid), L.ptr(sums), L.ptr(raw)))
    host = out.cpu().numpy()
    return {"kid": float(host[0]), "indices": indices, "sums": host[1:1 + 3 * S].reshape(S, 3).copy()}


def kernel_distance(feats1, feats2, num_subsets=100, max_subset_size=1000):
    """kernel.py:4-18: the KID score of two feature sets -> float.  The subsets are drawn on the host with ``np.random.choice``."""
    return kernel_info(feats1, feats2, num_subsets, max_subset_size)["kid"]


def pairwise_distances(x, y=None):
    """prdc.py:10-24: [N, M] squared distances ``|x_i|^2 + |y_j|^2 - 2 x_i . y_j`` (NaN -> 0, clamped at 0) as a float64 device tensor.
    The one function here that writes the matrix; prdc and nearest_neighbor_distances never do."""
    a, f64 = _features(x, "pairwise_distances")
    b, f64b = (a, f64) if y is None else _features(y, "pairwise_distances")
    if f64 != f64b:
        a, b, f64 = a.double(), b.double(), 1
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"pairwise_distances: feature widths differ, {a.shape[1]} and {b.shape[1]}")
    N, M, d = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    lib = L.lib()
    ws, nbytes = _workspace(lib.maua_prdc_workspace(N, M, d), a.device)
    dist = torch.empty((N, M), dtype=torch.float64, device=a.device)
    L.check(lib.maua_pairwise_distances(L.ctx(a.device), L.ptr(a), N, L.ptr(b), M, d, f64, L.ptr(ws), nbytes, L.ptr(dist)))
    return dist


def _check_k(name, nearest_k):
    if int(nearest_k) != nearest_k or not 1 <= int(nearest_k) <= MAX_NEAREST_K:
        raise ValueError(f"{name}: nearest_k must be 1 .. {MAX_NEAREST_K} (the kernel keeps nearest_k + 1 <= 16 values per row), "
                         f"got nearest_k={nearest_k}")
    return int(nearest_k)


def nearest_neighbor_distances(input_features, nearest_k):
    """prdc.py:27-37: the distance of every row to its nearest_k-th nearest neighbour (the row itself counts as the first of the
    nearest_k + 1 smallest, as in the reference) -> float64 device tensor [N]."""
    k = _check_k("nearest_neighbor_distances", nearest_k)
    x, f64 = _features(input_features, "nearest_neighbor_distances")
    N, d = map(int, x.shape)
    lib = L.lib()
    ws, nbytes = _workspace(lib.maua_prdc_workspace(N, 1, d), x.device)
    radii = torch.empty(N, dtype=torch.float64, device=x.device)
    L.check(lib.maua_knn_radii(L.ctx(x.device), L.ptr(x), N, d, f64, k, L.ptr(ws), nbytes, L.ptr(radii)))
    return radii


def prdc_info(real_features, fake_features, nearest_k=5):
    """prdc with its record: a dict of the four integer counts (precise fakes, recalled reals, the sum of the density counts, covered
    reals) and the two radius vectors (float64 device tensors)."""
    k = _check_k("prdc", nearest_k)
    x, f64 = _features(real_features, "prdc")
    y, f64b = _features(fake_features, "prdc")
    if f64 != f64b:
        x, y, f64 = x.double(), y.double(), 1
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"prdc: feature widths differ, {x.shape[1]} and {y.shape[1]}")
    N, M, d = int(x.shape[0]), int(y.shape[0]), int(x.shape[1])
    lib = L.lib()
    ws, nbytes = _workspace(lib.maua_prdc_workspace(N, M, d), x.device)
    counts = torch.empty(4, dtype=torch.int64, device=x.device)
    r_real = torch.empty(N, dtype=torch.float64, device=x.device)
    r_fake = torch.empty(M, dtype=torch.float64, device=x.device)
    L.check(lib.maua_prdc(L.ctx(x.device), L.ptr(x), N, L.ptr(y), M, d, f64, k, L.ptr(ws), nbytes, L.ptr(counts), L.ptr(r_real), L.ptr(r_fake)))
    return {"counts": tuple(int(c) for c in counts.cpu()), "r_real": r_real, "r_fake": r_fake, "N": N, "M": M, "nearest_k": k}


def prdc_counts(real_features, fake_features, nearest_k=5):
    """The integers behind prdc: (fakes inside some real ball, reals inside some fake ball, sum over the fakes of the real balls they
    lie in, reals whose nearest fake lies inside their own ball)."""
    return prdc_info(real_features, fake_features, nearest_k)["counts"]


def prdc_from_counts(counts, N, M, nearest_k):
    """The reference's float32 arithmetic on the integer counts (prdc.py:56-59: ``.float().mean()``, density ``/ nearest_k``)."""
    precise, recalled, density, covered = (np.float32(c) for c in counts)
    return (float(precise / np.float32(M)), float(recalled / np.float32(N)), float(density / np.float32(M) / np.float32(nearest_k)),
            float(covered / np.float32(N)))


def prdc(real_features, fake_features, nearest_k=5):
    """prdc.py:40-61: precision, recall, density and coverage of two manifolds -> four floats.

    The four values are formed from exact integer counts with the reference's float32 divisions, so wherever every comparison
    ``dist < radius`` falls as in the reference the tuple is bit-equal to the reference's.  Beyond 2^24 true pairs ours is the exact
    count rounded once to float32, where the reference's float32 sum rounds on the way."""
    info = prdc_info(real_features, fake_features, nearest_k)
    return prdc_from_counts(info["counts"], info["N"], info["M"], info["nearest_k"])


# ---- compute(): features of real and generated images, then the metrics (compute.py) ---------------------------------------------------
def resize_single_channel(x_np, size):
    from PIL import Image
    img = Image.fromarray(x_np.astype(np.float32))      # a float32 array is PIL mode "F"
    img = img.resize((size, size), resample=Image.BILINEAR)
    return np.asarray(img).clip(0, 255).reshape(size, size, 1)


def resize_clean(x, size):
    """compute.py:25-34: PIL mode "F" bilinear per channel, on the host (data loading) -> float32 [size, size, 3] in [0, 1]."""
    x = [resize_single_channel(x[:, :, idx], size) for idx in range(3)]
    return np.concatenate(x, axis=2).astype(np.float32) / 255.0


class FolderImages(torch.utils.data.Dataset):
    """compute.py:37-75: the images of a folder (recursively) or of a zip, resize_clean'ed to ``size`` -> float32 [3, size, size]."""

    def __init__(self, input_dir, n_images, size):
        super().__init__()
        input_dir = str(input_dir)
        if ".zip" in input_dir:
            files = sorted(set(ZipFile(input_dir).namelist()))
            files = [x for x in files if os.path.splitext(x)[1].lower()[1:] in EXTENSIONS]
        else:
            files = sorted([file for ext in EXTENSIONS for file in _glob.glob(os.path.join(input_dir, f"**/*.{ext}"), recursive=True)])
        if len(files) < n_images:
            raise ValueError(f"{input_dir} holds {len(files)} images, fewer than the {n_images} samples asked for")
        files = np.array(files)
        if n_images < len(files):
            files = files[np.random.permutation(len(files))[:n_images]]
        self.files, self.n_images, self.input_dir, self.size = files, n_images, input_dir, size

    def __getitem__(self, index):
        from PIL import Image
        path = str(self.files[index])
        if ".zip" in self.input_dir:
            with ZipFile(self.input_dir).open(path, "r") as f:
                image_np = np.load(f) if path.endswith(".npy") else np.array(Image.open(f).convert("RGB"))
        elif path.endswith(".npy"):
            image_np = np.load(path)
        else:
            image_np = np.array(Image.open(path).convert("RGB"))
        return torch.from_numpy(np.ascontiguousarray(resize_clean(image_np, self.size).transpose(2, 0, 1)))

    def __len__(self):
        return self.n_images


class GeneratorImages:
    """compute.py:78-91: ``n_images`` batches of ``G()`` mapped to [0, 1] and resized with the library's resize."""

    def __init__(self, G, n_images, size):
        self.n_images, self.G, self.size = n_images, G, size

    def __getitem__(self, index):
        from .image import resize
        if index >= self.n_images:
            raise IndexError(index)
        tensor = self.G().float().add(1).div(2)
        if self.size is None or tuple(tensor.shape[-2:]) == (self.size, self.size):
            return tensor
        return resize(tensor, out_shape=(self.size, self.size))

    def __len__(self):
        return self.n_images


def default_num_workers():
    return min(8, torch.multiprocessing.cpu_count())


class _ClipExtractor:
    def __init__(self, tower, allow_random_init):
        from . import clip
        self.model = clip.load(tower, allow_random_init=allow_random_init, text_tower=False)[0]
        self.size = int(self.model.visual.input_resolution)

    def __call__(self, batch):
        from .clip import CLIP_MEAN, CLIP_STD
        mean = torch.tensor(CLIP_MEAN, device=batch.device).reshape(1, 3, 1, 1)
        std = torch.tensor(CLIP_STD, device=batch.device).reshape(1, 3, 1, 1)
        return self.model.encode_image((batch.float() - mean) / std).float()


def get_extractor(extractor, allow_random_init=False):
    """-> (callable batch [B, 3, size, size] in [0, 1] -> features [B, d], size or None, name).  A callable or a (module, size) pair is
    taken as it is; ``"CLIP:<tower>"`` is one of maua_amd.clip's image towers; ``"SwAV:<checkpoint>"`` is the reference's SwAV ResNet-50
    with the weights of that local file (``"SwAV-bf16:<checkpoint>"``: in bfloat16; ``"SwAV:random"`` with ``allow_random_init``: the
    reference's initialisation) - it takes the batch in [0, 1] as it is (compute.py:147) and reports under the name ``SwAV``; the bare
    ``"SwAV"`` (nothing is downloaded) and ``"Inception"`` are not built."""
    if isinstance(extractor, (tuple, list)) and len(extractor) == 2 and callable(extractor[0]):
        return extractor[0], int(extractor[1]), getattr(extractor[0], "__name__", type(extractor[0]).__name__)
    if callable(extractor):
        return extractor, None, getattr(extractor, "__name__", type(extractor).__name__)
    if extractor in UNBUILT_EXTRACTORS:
        raise NotImplementedError(f"extractor {extractor!r} is not built: {UNBUILT_EXTRACTORS[extractor]}; pass a callable, a "
                                  "(module, size) pair, 'CLIP:<tower>' or 'SwAV:<checkpoint>'")
    if isinstance(extractor, str) and extractor.startswith("CLIP:"):
        ex = _ClipExtractor(extractor[len("CLIP:"):], allow_random_init)
        return ex, ex.size, extractor
    if isinstance(extractor, str) and extractor.startswith(("SwAV:", "SwAV-bf16:")):
        from .resnet import SwAV
        spelling, _, checkpoint = extractor.partition(":")
        dtype = torch.bfloat16 if spelling == "SwAV-bf16" else torch.float32
        return SwAV(checkpoint, dtype=dtype, allow_random_init=allow_random_init), SIZE, "SwAV"
    raise ValueError(f"unknown extractor {extractor!r}: pass a callable, a (module, size) pair, 'CLIP:<tower>' or 'SwAV:<checkpoint>'")


@torch.inference_mode()
def compute(real_samples, fake_samples, n_samples=10_000, extractor="SwAV", metrics=("frechet", "kernel", "prdc"), batch_size=32,
            num_workers=None, device=None, ignore_cache=False, verbose=True, return_features=False, allow_random_init=False,
            cache_dir="cache"):
    """compute.py:94-185.  ``real_samples``: a folder, a zip or an iterable of [B, 3, H, W] batches in [0, 1]; ``fake_samples``: a callable
    returning a batch in [-1, 1].  The real features are cached in ``cache_dir`` under the reference's file name.  Features stay on the
    device.  -> the dict of results under the reference's keys; with ``return_features`` also the two feature tensors."""
    L.require_device()
    for metric in metrics:
        if metric not in ("frechet", "kernel", "prdc"):
            raise ValueError(f"Unknown metric: {metric}")
    model, size, name = get_extractor(extractor, allow_random_init)
    device = torch.device("cuda" if device is None else device)
    num_workers = default_num_workers() if num_workers is None else num_workers
    from_path = isinstance(real_samples, (str, Path))
    cache_file = None
    if from_path:
        cache_file = os.path.join(cache_dir, f"{Path(real_samples).stem}_real_{name.replace('/', '-')}_features.npz")
    use_cache = cache_file is not None and os.path.exists(cache_file) and not ignore_cache
    n_batches = n_samples // batch_size
    if from_path and not use_cache:
        real_loader = torch.utils.data.DataLoader(FolderImages(real_samples, n_samples, SIZE if size is None else size),
                                                  batch_size=batch_size, num_workers=num_workers)
    elif use_cache:
        real_loader = range(n_batches)
    else:
        real_loader = real_samples
    fake_loader = GeneratorImages(fake_samples, n_batches, size)
    pairs = zip(real_loader, fake_loader)
    if verbose:
        try:
            from tqdm import tqdm
            pairs = tqdm(pairs, total=n_batches, unit_scale=batch_size, unit="images")
        except ImportError:
            pass
    real_features, fake_features = [], []
    for real_batch, fake_batch in pairs:
        fake_batch = fake_batch.to(device)
        if not use_cache:
            real_batch = real_batch.to(device).float()
            if real_batch.shape[-2:] != fake_batch.shape[-2:]:
                from .image import resize
                real_batch = resize(real_batch, out_shape=tuple(fake_batch.shape[-2:]))
            assert real_batch.shape[0] == fake_batch.shape[0]
            feats = model(torch.cat((real_batch, fake_batch))).float()
            real_feats, fake_feats = feats.chunk(2)
            real_features.append(real_feats)
            fake_features.append(fake_feats)
        else:
            fake_features.append(model(fake_batch).float())
    fake_features = torch.cat(fake_features)
    if use_cache:
        with np.load(cache_file) as data:
            real_features = torch.from_numpy(data["real_features"]).to(device)
    else:
        real_features = torch.cat(real_features)
        if cache_file is not None:
            os.makedirs(os.path.dirname(cache_file) or ".", exist_ok=True)
            np.savez_compressed(cache_file, real_features=real_features.cpu().numpy())

    res = {}
    for metric in metrics:
        if metric == "frechet":
            res[f"Frechet {name} Distance"] = frechet_distance(real_features, fake_features)
        elif metric == "kernel":
            res[f"Kernel {name} Distance"] = kernel_distance(real_features, fake_features)
        else:
            (res[f"Precision ({name})"], res[f"Recall ({name})"], res[f"Density ({name})"],
             res[f"Coverage ({name})"]) = prdc(real_features, fake_features)
    return (res, real_features, fake_features) if return_features else res


def parser():
    """compute.py:193-203's flags, with --extractor widened to the names get_extractor takes and --allow_random_init added."""
    import argparse
    p = argparse.ArgumentParser(prog="python -m maua.GAN.metrics.compute")
    p.add_argument("--data_dir", type=str, required=True)
    p.add_argument("--checkpoint", type=str, required=True)
    p.add_argument("--n_samples", type=int, default=10_000)
    p.add_argument("--extractor", type=str, default="SwAV", help="SwAV:<checkpoint> (SwAV-bf16:<checkpoint> in bfloat16), CLIP:<tower>, e.g. CLIP:ViT-B/32; bare SwAV and Inception are not built")
    p.add_argument("--metrics", type=str, nargs="+", default=["frechet", "kernel", "prdc"], choices=["frechet", "kernel", "prdc"])
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--num_workers", type=int, default=default_num_workers())
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--ignore_cache", action="store_true")
    p.add_argument("--allow_random_init", action="store_true", help="a CLIP tower without weights gets CLIP's own initialisation; SwAV:random the reference's")
    return p


def main(argv=None):
    import json
    args = parser().parse_args(argv)
    if args.extractor in UNBUILT_EXTRACTORS:
        get_extractor(args.extractor)      # raises by name before a checkpoint is read
    from .load import load_network
    G = load_network(args.checkpoint).eval().to(args.device)

    def fake_samples(*a, **kw):
        return G(z=torch.randn((args.batch_size, 512), device=args.device), c=None)

    res = compute(real_samples=args.data_dir, fake_samples=fake_samples, n_samples=args.n_samples, extractor=args.extractor,
                  metrics=args.metrics, batch_size=args.batch_size, num_workers=args.num_workers, device=args.device,
                  ignore_cache=args.ignore_cache, allow_random_init=args.allow_random_init)
    print(json.dumps(res, indent=4))
    return res
