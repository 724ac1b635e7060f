"""Neural cellular automata (maua/nca/train.py + generate.py, after znah's gitart_kunstformen_ca): the 12-channel texture automaton whose
update rule is a circular 3 x 3 perception stencil and two 1 x 1 convolutions behind a random per-pixel update mask.

The update runs in csrc/nca.hip, one launch per step or per 2 or 4 (include/maua_hip.h: maua_nca_*).  ``CA`` holds the reference's parameter names and
shapes, so its checkpoints load; it is not autograd-aware.  The update masks are drawn inside the kernel from the build-owned Philox
stream (``seed``, ``stream``) addressed by step and pixel - not from torch's generator - unless the caller hands the
uniforms in.

Built here: the step, forward_keep and the steps' gradient, loading / saving, generate()'s three videos, and train(): the VGG-16 Gram loss
of the batch-mean Gram matrices (maua_vgg_gram_mean_grad, csrc/perceptor.hip) walked back through the kept steps.
"""
import ctypes as C
import os
import pickle
from pathlib import Path

import numpy as np
import torch

from . import _lib as L

STEP_DTYPES = {"f32": L.F32, "split": L.F32_SPLIT}
RENDER_STEPS_PER_LAUNCH = {"f32": 1, "split": 2}      # generate()'s default per product mode, as measured (scripts/bench_nca.py)


NcaDesc = L.NcaDesc


def perception(x):
    """train.py:167-169: [B, C, H, W] -> [B, 4 C, H, W], per channel the circular 3 x 3 stencils {identity, sobel_x, sobel_x^T, laplacian}
    with un-normalised taps, feature 4 c + f (the step kernel forms these in registers; this is the operator for callers)."""
    x = L.dev_tensor(x, torch.float32)
    if x.ndim != 4:
        raise ValueError("perception expects a [B, C, H, W] tensor")
    b, c, h, w = x.shape
    out = torch.empty(b, 4 * c, h, w, dtype=torch.float32, device=x.device)
    L.check(L.lib().maua_nca_perception(L.ctx(x.device), L.ptr(x), b, c, h, w, L.ptr(out)))
    return out


def to_rgb(x):
    """train.py:191-193: the first three channels (the starting state is black)"""
    return x[..., :3, :, :]


# ---- the two frame schedules and the fade of generate.py (host arithmetic) -----------------------------------------------------------------

def evolution_steps(k):
    """generate.py:17: steps of frame k of the evolution video"""
    return min(2 ** (k // 30), 32)


def ratemap_steps(k):
    """generate.py:55: steps of frame k of the rate-map video"""
    return min(int(2 ** (k / 30)), 32)


def fade(k):
    """generate.py:59: the rate-map video's fade-out from frame 400"""
    return min(1.0 - (k - 400) / 100, 1.0)


def inject_seed(i):
    """train.py:218: the empty state replaces the first sample of the batch only at these iterations"""
    return i % 32 == 0


class _Handle:
    def __init__(self, chn, hidden, dtype, device):
        self.p = C.c_void_p()
        self.device = device
        L.check(L.lib().maua_nca_create(L.ctx(device), chn, hidden, dtype, C.byref(self.p)))

    def __del__(self):
        try:
            if self.p:
                L.lib().maua_nca_destroy(self.p)
        except Exception:
            pass


class CA(torch.nn.Module):
    """train.py:172-188.  forward / step update ``x`` through the library; ``products``: "f32" (exact v_mfma_f32_32x32x2_f32, the parity
    mode) or "split" (hi / lo bf16, three products: what rendering uses)."""

    def __init__(self, chn=12, hidden_n=96, products="split", seed=0, stream=0, steps_per_launch=1):
        super().__init__()
        if products not in STEP_DTYPES:
            raise ValueError(f"products must be one of {sorted(STEP_DTYPES)}")
        if steps_per_launch not in (1, 2, 4):
            raise ValueError("steps_per_launch must be 1, 2 or 4")
        self.steps_per_launch = steps_per_launch      # of step() outside window mode; the result has the same bits
        self.chn, self.hidden_n, self.products = chn, hidden_n, products
        self.w1 = torch.nn.Conv2d(chn * 4, hidden_n, 1)
        self.w2 = torch.nn.Conv2d(hidden_n, chn, 1, bias=False)
        self.w2.weight.data.zero_()
        self.rng_seed, self.rng_stream, self.steps_done = int(seed), int(stream), 0
        self._handles = {}

    def __getstate__(self):
        """the library handles belong to this object: a copy (copy.deepcopy, torch.save of the module) makes its own on first use"""
        d = self.__dict__.copy()
        d["_handles"] = {}
        return d

    def seed(self, n, sz=128):
        return torch.zeros(n, self.chn, sz, sz, device=self.w1.weight.device)

    def _handle(self, device):
        key = (self.products, device.index)
        if key not in self._handles:
            self._handles[key] = _Handle(self.chn, self.hidden_n, STEP_DTYPES[self.products], device)
        return self._handles[key]

    def _desc(self, x, n, update_rate, u, step0, window):
        L.require_device()
        if x.device.type != "cuda" or x.dtype != torch.float32 or not x.is_contiguous() or x.ndim != 4 or x.shape[1] != self.chn:
            raise ValueError(f"the state must be a contiguous float32 [B, {self.chn}, H, W] tensor on the device")
        dev = x.device
        L.ctx(dev)          # the handle's context follows torch's current stream
        b, _, h, w = x.shape
        keep = [self.w1.weight.detach().to(dev, torch.float32).contiguous(), self.w1.bias.detach().to(dev, torch.float32).contiguous(),
                self.w2.weight.detach().to(dev, torch.float32).contiguous()]
        d = NcaDesc(x=x.data_ptr(), B=b, H=h, W=w, w1=keep[0].data_ptr(), b1=keep[1].data_ptr(), w2=keep[2].data_ptr(), n_steps=n,
                    seed=self.rng_seed, stream=self.rng_stream, step0=self.steps_done if step0 is None else int(step0))
        if torch.is_tensor(update_rate):
            m = update_rate.to(dev, torch.float32).contiguous()
            if tuple(m.shape) != (h, w):
                raise ValueError(f"a rate map must be [H, W] = [{h}, {w}], got {tuple(m.shape)}")
            keep.append(m)
            d.rate_map = m.data_ptr()
        else:
            d.rate = float(update_rate)
        if u is not None:
            uu = u.to(dev, torch.float32).contiguous()
            if uu.numel() != n * b * h * w:
                raise ValueError(f"u must hold [n_steps, B, H, W] = [{n}, {b}, {h}, {w}] uniforms")
            keep.append(uu)
            d.u = uu.data_ptr()
        if window is not None:
            d.col0, d.W_sub, d.margin = (int(v) for v in window)
        return d, keep

    @torch.no_grad()
    def step(self, x, n=1, update_rate=0.5, u=None, step0=None, window=None):
        """n updates of x in place (one library call).  u: [n, B, H, W] uniforms instead of the Philox draws; step0: the Philox step index of
        the first update (default: this module's running count, which the call advances); window = (col0, W_sub, margin)."""
        d, keep = self._desc(x, n, update_rate, u, step0, window)
        if window is None:
            d.steps_per_launch = self.steps_per_launch
        L.check(L.lib().maua_nca_step(self._handle(x.device).p, C.byref(d)))
        if step0 is None:
            self.steps_done += n
        return x

    @torch.no_grad()
    def forward(self, x, update_rate=0.5):
        """train.py:180-185: one update; returns a new tensor as the reference does"""
        return self.step(x.clone(), 1, update_rate)

    @torch.no_grad()
    def forward_keep(self, x, n, update_rate=0.5, u=None, step0=None):
        """[n + 1, B, chn, H, W]: x and the state after each of n updates (what the gradient walks back through)"""
        d, keep = self._desc(x, n, update_rate, u, step0, None)
        states = torch.empty((n + 1,) + tuple(x.shape), dtype=torch.float32, device=x.device)
        L.check(L.lib().maua_nca_forward_keep(self._handle(x.device).p, C.byref(d), L.ptr(states)))
        if step0 is None:
            self.steps_done += n
        return states

    @torch.no_grad()
    def backward(self, states, g_last, update_rate=0.5, u=None, *, step0=None):
        """The gradient of the n = len(states) - 1 updates forward_keep stored: (dL/dx_0, dL/dw1.weight, dL/dw1.bias, dL/dw2.weight)
        from g_last = dL/dx_n.  update_rate, u and step0 must be forward_keep's.  step0, the Philox step index forward_keep's first update
        had (``steps_done`` before that call, unless it was given one), has no default: with drawn masks a wrong one silently gives the
        gradient of other masks.  With the caller's uniforms ``u`` it is not used."""
        n = states.shape[0] - 1
        if step0 is None:
            if u is None:
                raise ValueError("CA.backward: pass step0, the Philox step index forward_keep's first update had")
            step0 = 0
        g_last = L.dev_tensor(g_last, torch.float32)
        if states.dtype != torch.float32 or not states.is_contiguous() or tuple(g_last.shape) != tuple(states.shape[1:]):
            raise ValueError("states must be forward_keep's contiguous float32 [n + 1, B, chn, H, W] and g_last one state's shape")
        d, keep = self._desc(states[0], n, update_rate, u, step0, None)
        g_first = torch.empty_like(g_last)
        dw1, db1, dw2 = (torch.empty_like(p, dtype=torch.float32, device=states.device) for p in (self.w1.weight, self.w1.bias, self.w2.weight))
        L.check(L.lib().maua_nca_vjp(self._handle(states.device).p, C.byref(d), L.ptr(states), L.ptr(g_last), L.ptr(g_first), L.ptr(dw1),
                                     L.ptr(db1), L.ptr(dw2)))
        return g_first, dw1, db1, dw2


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------

class _CaUnpickler(pickle.Unpickler):
    """Reads what the reference writes, ``torch.save(module)`` of a class named CA (train.py:249), executing nothing: the globals an
    nn.Module pickle of two Conv2d needs resolve to maua_amd.load's allow-list or to inert stand-ins; anything else raises."""
    MODULE_CLASSES = {"CA", "Conv2d"}

    def __init__(self, file, storages):
        super().__init__(file)
        self.storages = storages

    def find_class(self, module, name):
        from .load import _NetworkUnpickler, _PickledObject
        if (module, name) in _NetworkUnpickler.ALLOWED or (module in ("builtins", "__builtin__") and name in _NetworkUnpickler.BUILTINS):
            return pickle.Unpickler.find_class(self, "builtins", name) if module == "__builtin__" else pickle.Unpickler.find_class(self, module, name)
        if module == "torch" and (name.endswith("Storage") or isinstance(getattr(torch, name, None), torch.dtype)):
            return getattr(torch, name)
        if name in self.MODULE_CLASSES and (name == "CA" or module.startswith("torch.nn.modules")):
            return _PickledObject
        raise pickle.UnpicklingError(f"an NCA checkpoint may not reference {module}.{name}")

    def persistent_load(self, pid):
        # torch's zip format: ('storage', storage_type, key, location, numel)
        if not (isinstance(pid, tuple) and len(pid) == 5 and pid[0] == "storage"):
            raise pickle.UnpicklingError("unknown persistent id in an NCA checkpoint")
        import warnings
        _, stype, key, _, numel = pid
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)      # TypedStorage's deprecation notice: _rebuild_tensor_v2 still takes one
            dtype = getattr(stype, "dtype", None) or torch.float32
            if key not in self.storages:
                self.storages[key] = torch.frombuffer(bytearray(self.read_record(key)), dtype=dtype)[:numel].untyped_storage()
            return torch.storage.TypedStorage(wrap_storage=self.storages[key], dtype=dtype, _internal=True)


def _module_pickle_state_dict(path):
    import zipfile
    from .load import _module_state_dict
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        pkl = [n for n in names if n.endswith("/data.pkl")]
        if len(pkl) != 1:
            raise ValueError(f"{path}: not a torch.save archive")
        root = pkl[0][:-len("data.pkl")]
        import io
        up = _CaUnpickler(io.BytesIO(z.read(pkl[0])), {})
        up.read_record = lambda key: z.read(f"{root}data/{key}")
        obj = up.load()
    sd = _module_state_dict(obj)
    chn = getattr(obj, "chn", None)
    return {k: torch.as_tensor(v).float() for k, v in sd.items()}, chn


def load_ca(path, products="split", device=None, steps_per_launch=1):
    """A CA from a state dict (what ``save`` writes) or from the reference's ``torch.save(ca)`` (read without running anything the file
    names; a pickle that references any other global raises)."""
    path = str(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such NCA checkpoint")
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:              # a pickled module: torch's weights-only loader refuses the class it names
        sd, _ = _module_pickle_state_dict(path)
    if not isinstance(sd, dict) or not {"w1.weight", "w1.bias", "w2.weight"} <= set(sd):
        raise ValueError(f"{path}: not an NCA checkpoint (w1.weight, w1.bias, w2.weight)")
    hidden, k1 = sd["w1.weight"].shape[:2]
    ca = CA(k1 // 4, hidden, products=products, steps_per_launch=steps_per_launch)
    ca.load_state_dict({k: sd[k] for k in ("w1.weight", "w1.bias", "w2.weight")})
    if device is not None:
        ca = ca.to(device)
    return ca


def save(ca, path):
    torch.save({k: v.detach().cpu() for k, v in ca.state_dict().items()}, str(path))


# ---- rendering (generate.py) --------------------------------------------------------------------------------------------------------------

def zoom2(img):
    """train.py:85-88 with scale 2 on a [B, C, H, W] tensor: nearest neighbour"""
    return img.repeat_interleave(2, -2).repeat_interleave(2, -1)


def frame_bytes(x, gain=1.0):
    """One video frame: the first three channels of x[0], zoomed x 2, clamped to [0, 1] and packed to u8 [1, 2H, 2W, 3] on the device"""
    from .video import tensor2bytes_device
    img = to_rgb(x[:1])
    if gain != 1.0:
        img = img * gain
    return tensor2bytes_device(zoom2(img), (0, 1))


def text_rate_map(s="WΛV", font_file="DejaVuSans.ttf", size=256, pad=64):
    """generate.py:38-49: the blurred text as an update-rate map in [0.05, 0.65]"""
    import PIL.Image
    import PIL.ImageDraw
    import PIL.ImageFilter
    import PIL.ImageFont
    try:
        font = PIL.ImageFont.truetype(font_file, size)
    except OSError as e:
        raise FileNotFoundError(f"text_rate_map needs the font file {font_file!r}") from e
    l, t, r, b = font.getbbox(s)
    w, h = r, b
    im = PIL.Image.new("L", (w + pad * 2, h + pad * 2))
    PIL.ImageDraw.Draw(im).text((pad, pad), s, fill=255, font=font)
    p = np.float32(im.filter(PIL.ImageFilter.GaussianBlur(5)))
    return torch.from_numpy(p / p.max() * 0.6 + 0.05)


def render_evolution(ca, write, num_frames=600, size=256):
    """generate.py:14-21: min(2 ** (k // 30), 32) steps per frame from a zero state"""
    x, t = ca.seed(1, size), 0              # the video's own step count addresses the masks: a render does not depend on earlier calls
    for k in range(num_frames):
        ca.step(x, evolution_steps(k), step0=t)
        t += evolution_steps(k)
        write(frame_bytes(x))
    return x


def render_checkgrid(models, write, num_frames=600, strip=128, rows=512, rounds=8, x=None, seed=0):
    """generate.py:25-36: every checkpoint on its own strip of one grid; a model updates its strip through a window one column wider on
    either side, whose interior it replaces, so each sees its left neighbour's fresh column.  The Philox step index counts rounds."""
    chn = models[0].chn
    dev = models[0].w1.weight.device
    if x is None:
        g = torch.Generator().manual_seed(seed)
        x = (torch.rand(1, chn, rows, strip * len(models) + 2, generator=g) * 0.1).to(dev)
    t = 0
    for _ in range(num_frames):
        for _ in range(rounds):
            for ci, f in enumerate(models):
                f.step(x, 1, step0=t, window=(ci * strip, strip + 2, 1))
            t += 1
        write(frame_bytes(x))
    return x


def render_ratemap(ca, rate_map, write, num_frames=600):
    """generate.py:51-60: min(int(2 ** (k / 30)), 32) steps per frame under a per-pixel update rate, fading out from frame 400"""
    rate_map = rate_map.to(ca.w1.weight.device, torch.float32).contiguous()
    h, w = rate_map.shape
    x, t = torch.zeros(1, ca.chn, h, w, device=rate_map.device), 0
    for k in range(num_frames):
        ca.step(x, ratemap_steps(k), rate_map, step0=t)
        t += ratemap_steps(k)
        write(frame_bytes(x, fade(k)))
    return x


def generate(model_file, out_dir, num_frames=600, checkpoints=None, rate_map=None, fps=30.0, products="split", writer=None, size=256,
             grid=(512, 128)):
    """The reference's three videos of a trained rule.  checkpoints: the files of the checkpoint grid (default: the ``*.pt`` beside
    model_file, without the first and last two, generate.py:26); rate_map: any [h, w] tensor (default text_rate_map()).  writer:
    ``writer(path, (w, h), fps)`` returns the context manager that takes the frames (default maua_amd.video.VideoWriter).  size: the side
    of the evolution video's state; grid = (rows, strip): the checkpoint grid's rows and the columns of each model's strip."""
    from .video import VideoWriter
    L.require_device()
    writer = writer or (lambda path, size, fps: VideoWriter(path, size, fps))
    model_file, out_dir = Path(model_file), Path(out_dir)
    stem = model_file.stem
    style, _, tag = stem.rpartition("_")
    style = style or stem
    # two steps per launch measured 12 % faster than one in split mode on the 256 x 256 render and slower in exact f32; same bits
    ca = load_ca(model_file, products, "cuda", steps_per_launch=RENDER_STEPS_PER_LAUNCH[products])
    rows, strip = grid
    with writer(out_dir / f"{style}_{tag}.mp4", (2 * size, 2 * size), fps) as vid:
        render_evolution(ca, vid.write, num_frames, size)
    if checkpoints is None:
        checkpoints = sorted(str(p) for p in model_file.parent.glob(f"{style}*.pt"))[2:-2]
    if checkpoints:
        models = [load_ca(p, products, "cuda") for p in checkpoints]
        with writer(out_dir / f"{style}_checkgrid.mp4", (2 * (strip * len(models) + 2), 2 * rows), fps) as vid:
            render_checkgrid(models, vid.write, num_frames, strip, rows)
    if rate_map is None:
        rate_map = text_rate_map()
    h, w = rate_map.shape
    with writer(out_dir / f"{style}-{tag}-wav.mp4", (2 * w, 2 * h), fps) as vid:
        render_ratemap(ca, rate_map, vid.write, num_frames)


# ---- training (train.py:118-142, 196-251) ----------------------------------------------------------------------------------------------------

STYLE_LAYERS = (1, 6, 11, 18, 25)       # train.py:123, ReLUs of torchvision's vgg16.features


class StyleLoss:
    """calc_styles + ``g.mean(0)`` + style_loss (train.py:122-142, 228-229) and the loss's gradient with respect to the images, in one
    library call (maua_vgg_gram_mean_grad).  ``net``: a perceptors.VGGFeatures built with in_mul 1, in_add 0, ImageNet mean / std and
    zero padding; ``layers``: features indices of its taps."""

    def __init__(self, net, layers=STYLE_LAYERS):
        self.net, self.layers = net, tuple(layers)
        self.targets = None

    @classmethod
    def vgg16(cls, state_dict=None, allow_random_init=False, dtype=torch.bfloat16, generator=None):
        from .perceptors import IMAGENET_MEAN, IMAGENET_STD, VGG16_CFG, VGGFeatures, _load_weights
        net = VGGFeatures(VGG16_CFG, STYLE_LAYERS[-1], (1.0, 0.0, IMAGENET_MEAN, IMAGENET_STD), dtype=dtype, generator=generator)
        _load_weights(net, state_dict, "vgg16", allow_random_init)
        return cls(net)

    def calc_styles(self, imgs):
        """[B, 3, H, W] in [0, 1] -> the taps' Gram matrices F F^T / (h w), [B, C, C] each"""
        self.net.forward(imgs)
        out = []
        for l in self.layers:
            _, h, w = self.net._grid(self.net.op_of(l))
            out.append(self.net.gram(l) / float(h * w))
        return out

    def set_target(self, style_img):
        """the style image's Gram matrices (train.py:199); one image"""
        self.targets = [g[0].contiguous() for g in self.calc_styles(style_img)]
        return self.targets

    def loss_grad(self, imgs, targets=None):
        """(loss: one device float, d loss / d imgs)"""
        from .perceptors import _ptr_array
        tg = [L.dev_tensor(t, torch.float32).contiguous() for t in (self.targets if targets is None else targets)]
        if len(tg) != len(self.layers):
            raise ValueError(f"{len(tg)} targets for {len(self.layers)} style layers")
        imgs = self.net._check(imgs.contiguous())
        for t, l in zip(tg, self.layers):
            c = self.net.channels(l)
            if tuple(t.shape) != (c, c):
                raise ValueError(f"style target of features[{l}]: shape {tuple(t.shape)}, expected ({c}, {c})")
        B, _, H, W = imgs.shape
        taps = (C.c_int * len(tg))(*[self.net.op_of(l) for l in self.layers])
        grad = torch.empty_like(imgs)
        loss = torch.empty(1, dtype=torch.float32, device=imgs.device)
        L.check(L.lib().maua_vgg_gram_mean_grad(self.net._handle(), L.ptr(imgs), B, H, W, taps, len(tg), _ptr_array(tg), L.ptr(grad), L.ptr(loss)))
        self.net._shape = tuple(imgs.shape)
        return loss, grad


def load_style(style_file, max_size=128, multiple=16):
    """train.py:197 (imread with max_size: PIL's thumbnail under the filter the reference calls ANTIALIAS, LANCZOS in current PIL), then a
    central crop to sides that are multiples of ``multiple``, which the perceptor needs.  -> [1, 3, h, w] in [0, 1]"""
    import PIL.Image
    img = PIL.Image.open(style_file).convert("RGB")
    img.thumbnail((max_size, max_size), PIL.Image.LANCZOS)
    a = np.float32(img) / 255.0
    h, w = (a.shape[0] // multiple) * multiple, (a.shape[1] // multiple) * multiple
    if h == 0 or w == 0:
        raise ValueError(f"{style_file}: the style image must be at least {multiple} pixels on either side after the thumbnail")
    y0, x0 = (a.shape[0] - h) // 2, (a.shape[1] - w) // 2
    return torch.from_numpy(np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w].transpose(2, 0, 1)))[None]


def train_step(ca, x, step_n, style, opt, targets=None, trace=None):
    """One iteration of train.py:221-236 on the batch x: step_n updates keeping every state, the style loss of the RGB slice, its
    gradient walked back through the steps, each parameter gradient divided by its norm + 1e-8, the optimiser's step.  Returns (the new
    batch, the loss as a device float).  trace: a dict that receives the intermediates (tests)."""
    step0 = ca.steps_done
    states = ca.forward_keep(x, step_n)
    loss, dimg = style.loss_grad(to_rgb(states[-1]).contiguous(), targets)
    g_last = torch.zeros_like(states[-1])
    g_last[:, :3] = dimg
    g_first, dw1, db1, dw2 = ca.backward(states, g_last, step0=step0)
    if trace is not None:
        trace.update(states=states, loss=loss, g_last=g_last, g_first=g_first, dw1=dw1.clone(), db1=db1.clone(), dw2=dw2.clone(), step0=step0)
    for p, g in ((ca.w1.weight, dw1), (ca.w1.bias, db1), (ca.w2.weight, dw2)):
        p.grad = (g / (g.norm() + 1e-8)).to(p.device).reshape(p.shape)
    opt.step()
    opt.zero_grad()
    return states[-1], loss


def train(style_file, out_dir, steps=7500, vgg_weights=None, pool_size=1024, batch=4, size=128, step_range=(32, 96), save_every=500, seed=0,
          dtype=torch.bfloat16, style=None, lr=1e-3):
    """train.py:196-251.  vgg_weights: a torchvision vgg16 state-dict file (default: torchvision's cache; MAUA_ALLOW_RANDOM_INIT=1 in the
    environment trains against a randomly initialised network).  Pool indices and step counts come from numpy's generator seeded with
    ``seed``, the update masks from the module's Philox stream.  Returns (the CA, the list of losses)."""
    import PIL.Image
    L.require_device()
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    name = Path(style_file).stem
    if style is None:
        sd = torch.load(str(vgg_weights), map_location="cpu", weights_only=True) if vgg_weights else None
        style = StyleLoss.vgg16(sd, os.environ.get("MAUA_ALLOW_RANDOM_INIT") == "1", dtype)
    style.set_target(load_style(style_file).cuda())
    with torch.random.fork_rng(devices=[]):             # w1's initialisation from ``seed`` too, the global generator left alone
        torch.manual_seed(seed)
        ca = CA(products="f32", seed=seed)
    ca = ca.cuda()
    opt = torch.optim.Adam(ca.parameters(), lr)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [2000, 4000], 0.3)
    pool = ca.seed(pool_size, size)
    rng = np.random.default_rng(seed)
    losses = []
    for i in range(steps):
        idx = torch.from_numpy(rng.choice(pool_size, batch, replace=False)).cuda()
        x = pool[idx]
        if inject_seed(i):
            x[:1] = ca.seed(1, size)
        x, loss = train_step(ca, x, int(rng.integers(*step_range)), style, opt)
        sched.step()
        pool[idx] = x
        losses.append(loss)
        if len(losses) % save_every == 0 or len(losses) == steps:
            save(ca, out_dir / f"{name}_{len(losses)}.pt")
            strip = frame_strip(x)
            PIL.Image.fromarray(strip).save(out_dir / f"{name}_{len(losses)}.png")
    return ca, [float(v) for v in torch.cat(losses).cpu()] if losses else []


def frame_strip(x):
    """train.py:250-251: the batch's RGB images side by side, u8 [H, B W, 3]"""
    from .video import tensor2bytes_device
    b = tensor2bytes_device(to_rgb(x).contiguous(), (0, 1)).cpu().numpy()
    return np.hstack(list(b))


def _parser(prog):
    import argparse
    ap = argparse.ArgumentParser(prog=prog)
    ap.add_argument("style_file")
    ap.add_argument("out_dir")
    return ap


def generate_parser():
    ap = _parser("python -m maua.nca.generate")
    ap.add_argument("--model-file", default=None, help="default: OUT_DIR/<style name>_7500.pt (generate.py:9)")
    ap.add_argument("--num-frames", type=int, default=600)
    ap.add_argument("--products", choices=sorted(STEP_DTYPES), default="split")
    return ap


def train_parser():
    ap = _parser("python -m maua.nca.train")
    ap.add_argument("--steps", type=int, default=7500)
    ap.add_argument("--vgg-weights", default=None, help="torchvision vgg16 state dict")
    return ap


def generate_main(argv=None):
    a = generate_parser().parse_args(argv)
    model = a.model_file or os.path.join(a.out_dir, f"{Path(a.style_file).stem}_7500.pt")
    generate(model, a.out_dir, a.num_frames, products=a.products)


def train_main(argv=None):
    a = train_parser().parse_args(argv)
    train(a.style_file, a.out_dir, a.steps, vgg_weights=a.vgg_weights)
