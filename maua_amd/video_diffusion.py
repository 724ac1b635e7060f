"""The optical-flow video pipeline around guided diffusion (maua/diffusion/video.py:38-427): a video is stylised frame by frame - the
previous output is warped along the optical flow, blended into the next input frame under the forward / backward consistency mask,
noised, and handed to ``diffusion.forward``.

Same names, keyword arguments, defaults and order of operations as the reference.  What differs, on purpose:
  * the optical flow is estimated on the device (``maua_amd.flow``: Farneback's algorithm restated, both directions of a pair batched;
    the reference calls OpenCV on the host twice per frame); parity with OpenCV itself is unpinned;
  * ``VideoFrames`` reads a directory or glob of image files, a ``.npy`` / array / tensor of frames, or - through an ``ffmpeg``
    executable on PATH - a video file; decord is not used, and frames are resized by the library's cubic ``resize``, not by decord's
    swscale filter;
  * frames, flows and consistency maps stay on the device for the run as float32 (``FramesOnDisk`` keeps the reference's interface);
    ``persist=True`` also writes the reference's JPEG / ``.mflo`` files under ``workspace/<name>/`` from a writer thread, and a valid
    flow cache is re-used by the reference's rule.  The reads inside the loop come from the device copies: the reference's 8-bit JPEG
    round trip of flows and frames and its read-before-write race are not reproduced;
  * the injected noise comes from the library's Philox streams (key: one ``torch.randint`` draw per frame, so ``constant_seed``
    repeats it); the reference's ``randn_like`` values are not reproduced;
  * with no hook between fade and noise the whole composition is one launch; with ``turbo=1`` the in-between step is the identity it is
    in the reference (``prev * 0 + next * 1``) and launches nothing, so the composition kernel is the only launch between two sampler
    calls (``ContentPrompt``'s own arithmetic on the content frame aside);
  * the last step of the loop (``f_n >= N + wrap_around``) only flushes the turbo in-betweens and ends there; the reference goes on,
    indexes ``loop_fade`` past its end (:268-269) and raises IndexError before its sampler call;
  * ``diffusion``: "guided" or a processor instance; the latent / stable / glide / glid3xl processors raise by name before any work.
"""
import os
import random
import shutil
import subprocess
from functools import partial, reduce
from glob import glob
from pathlib import Path
from queue import Empty, Queue
from threading import Thread
from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch

from .diffusion import get_diffusion_model
from .flow import (check_consistency, compose, decode_mflo, draw_noise_key, encode_mflo, get_flow_model, resize_bilinear,  # noqa: F401
                   turbo_step)
from .grad import ContentPrompt, ImagePrompt, StylePrompt, TextPrompt
from .image import OTHER_PROCESSORS, build_output_name, match_histogram, resize, round64, sharpen, width_height  # noqa: F401
from .video import write_video

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")
ACCEPTS = ("a directory or glob of image files, a .npy file or an array / tensor of frames ([N, 3, H, W] or [N, H, W, 3], uint8), or a video "
           "file when an ffmpeg executable is on PATH")


def seed_everything(seed):
    """maua/utility.py:57-61."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


# ======================================================================================================== frames
def _frames_u8(a, what):
    a = torch.as_tensor(a)
    if a.dim() != 4 or a.dtype != torch.uint8 or (a.shape[1] != 3 and a.shape[3] != 3):
        raise ValueError(f"VideoFrames: {what} must hold uint8 frames [N, 3, H, W] or [N, H, W, 3], got {a.dtype} {tuple(a.shape)}; it accepts {ACCEPTS}")
    return a if a.shape[3] == 3 and a.shape[1] != 3 else a.permute(0, 2, 3, 1)


def _parse_ppm_stream(buf, what):
    """Concatenated binary PPM images (``P6 <width> <height> <maxval>`` and the pixels: what ``ffmpeg -f image2pipe -vcodec ppm`` writes,
    each frame carrying its own size) -> uint8 tensor [N, H, W, 3]."""
    frames, pos, n = [], 0, len(buf)
    while pos < n:
        fields = []
        while len(fields) < 4:                       # magic, width, height, maxval: whitespace-separated, '#' starts a comment
            while pos < n and buf[pos:pos + 1].isspace():
                pos += 1
            if pos < n and buf[pos:pos + 1] == b"#":
                while pos < n and buf[pos:pos + 1] != b"\n":
                    pos += 1
                continue
            start = pos
            while pos < n and not buf[pos:pos + 1].isspace():
                pos += 1
            if start == pos:
                raise RuntimeError(f"VideoFrames: truncated PPM header in the frames of {what}")
            fields.append(bytes(buf[start:pos]))
        pos += 1                                      # the single whitespace byte that ends the header
        if fields[0] != b"P6" or fields[3] != b"255":
            raise RuntimeError(f"VideoFrames: unexpected frame format {fields[0]!r} (maxval {fields[3]!r}) in the frames of {what}")
        w, h = int(fields[1]), int(fields[2])
        if w <= 0 or h <= 0 or pos + h * w * 3 > n:
            raise RuntimeError(f"VideoFrames: truncated frame in the frames of {what}")
        frames.append(np.frombuffer(buf, dtype=np.uint8, count=h * w * 3, offset=pos).reshape(h, w, 3))
        pos += h * w * 3
    if not frames or any(f.shape != frames[0].shape for f in frames):
        raise RuntimeError(f"VideoFrames: no frames, or frames of different sizes, in {what}")
    return torch.from_numpy(np.stack(frames))


def read_frames(source):
    """-> uint8 tensor [N, H, W, 3] on the host."""
    if isinstance(source, (np.ndarray, torch.Tensor)):
        return _frames_u8(source, "the array")
    src = str(source)
    if src.endswith(".npy") and os.path.isfile(src):
        return _frames_u8(np.load(src), src)
    files = None
    if os.path.isdir(src):
        files = sorted(f for f in glob(os.path.join(src, "*")) if f.lower().endswith(IMAGE_SUFFIXES))
    elif any(ch in src for ch in "*?["):
        files = sorted(glob(src))
    if files is not None:
        if not files:
            raise FileNotFoundError(f"VideoFrames: no image files in {src}; it accepts {ACCEPTS}")
        from PIL import Image
        frames = [np.asarray(Image.open(f).convert("RGB")) for f in files]
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError(f"VideoFrames: the image files of {src} differ in size")
        return torch.from_numpy(np.stack(frames))
    if os.path.isfile(src) and shutil.which("ffmpeg") is not None:
        # PPM frames through a pipe: every frame carries its own size, so ffmpeg alone is enough (no ffprobe)
        r = subprocess.run([shutil.which("ffmpeg"), "-v", "error", "-i", src, "-f", "image2pipe", "-vcodec", "ppm", "-"], capture_output=True)
        if r.returncode != 0 or len(r.stdout) == 0:
            raise RuntimeError(f"VideoFrames: ffmpeg could not decode {src}: {r.stderr.decode(errors='replace').strip()}")
        return _parse_ppm_stream(r.stdout, src)
    raise RuntimeError(f"VideoFrames: cannot read {src!r}: it accepts {ACCEPTS}")


class VideoFrames(torch.utils.data.Dataset):
    """diffusion/video.py:38-50: frame ``idx`` -> [1, 3, height, width] in [-1, 1] on ``device``.  Every frame is prepared once, when
    the object is built, and indexing hands out views: nothing launches when the loop reads a frame."""

    def __init__(self, filename, height, width, device):
        super().__init__()
        u8 = read_frames(filename)
        data = u8.to(device).permute(0, 3, 1, 2).float().div(127.5).sub(1)
        if tuple(data.shape[2:]) != (height, width):
            data = resize(data, out_shape=(height, width))          # the library's cubic resize (device only)
        self.data = data.contiguous()

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, idx):
        if isinstance(idx, (list, np.ndarray, torch.Tensor)):
            return torch.stack([self.data[int(i):int(i) + 1] for i in idx])
        idx = int(idx) % len(self)
        return self.data[idx:idx + 1]


class WriteThread(Thread):
    """diffusion/video.py:53-80: consistency maps and frames as JPEG, flows as ``.mflo``."""

    def __init__(self, queue: Queue, basename: str, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.queue = queue
        self.basename = basename
        self.done = False

    def run(self):
        from PIL import Image
        while True:
            try:
                item, idx = self.queue.get(timeout=0.05)
            except Empty:
                if self.done:
                    return
                continue
            if isinstance(item, torch.Tensor):
                item = item.detach().cpu().numpy()
            if len(item.shape) < 4:
                item = item[None]
            shape = item.shape
            if tuple(shape[:2]) == (1, 1):
                consistency = np.round(item.squeeze() * 255).astype(np.uint8)
                Image.fromarray(consistency).save(f"{self.basename}{idx}.jpg", quality=95)
            elif shape[-1] == 2:
                mflo = encode_mflo(item.squeeze())
                Image.fromarray(mflo).save(f"{self.basename}{idx}.mflo", format="JPEG", quality=95)
            else:
                img = np.clip(np.round((item.squeeze().transpose(1, 2, 0) + 1) * 127.5), 0, 255).astype(np.uint8)
                Image.fromarray(img).save(f"{self.basename}{idx}.jpg", quality=95)


class FramesOnDisk(torch.utils.data.Dataset):
    """diffusion/video.py:83-122 with the items held on the device: ``insert`` / indexing / ``len`` / ``finalize`` as there.
    ``persist=True`` also writes the reference's files (and reads the ones a previous run left)."""

    def __init__(self, basename, device, persist=False):
        super().__init__()
        self.basename = basename
        self.device = device
        self.persist = persist
        self.items = {}
        self.length = len(glob(f"{basename}*")) if persist else 0
        self.write_queue = Queue()
        self.write_thread = None
        if persist:
            self.write_thread = WriteThread(self.write_queue, self.basename, daemon=True)
            self.write_thread.start()

    def __len__(self):
        return self.length

    def _read(self, i):
        from PIL import Image
        file = f"{self.basename}{i}.jpg"
        if os.path.exists(file.replace(".jpg", ".mflo")):
            mflo = np.asarray(Image.open(file.replace(".jpg", ".mflo")))
            return torch.tensor(decode_mflo(mflo))[None]
        image = Image.open(file)
        a = np.asarray(image)
        tensor = torch.from_numpy(a.reshape(*a.shape[:2], -1).copy()).permute(2, 0, 1).float().div(255)
        if image.mode == "RGB":  # mode "L" (consistency map) is left with value range (0, 1)
            tensor = tensor.mul(2).sub(1)
        return tensor[None]

    def __getitem__(self, idx):
        if not isinstance(idx, (list, np.ndarray)):
            idx = [idx]
        tensors = []
        for i in idx:
            i = int(i)
            if i not in self.items:
                if not self.persist:
                    raise IndexError(f"{self.basename}{i} was never inserted")
                self.items[i] = self._read(i).to(self.device)
            tensors.append(self.items[i])
        return tensors[0] if len(tensors) == 1 else torch.cat(tensors)

    def insert(self, item, idx=None):
        idx = idx if idx is not None else len(self)
        self.items[int(idx)] = item.detach()
        if self.persist:
            self.write_queue.put((item, idx))
        self.length += 1

    def close(self):
        """Let the writer thread drain its queue and end (a no-op without ``persist``)."""
        if self.write_thread is not None:
            self.write_thread.done = True
            self.write_thread.join()
            self.write_thread = None

    def finalize(self):
        """-> the items in index order as one tensor [N, ...] (what ``write_video`` takes)."""
        self.length -= 1
        self.close()
        return torch.cat([self.items[i] for i in sorted(self.items)])


class Cache(dict):
    """easydict.EasyDict's role: a dict whose keys read as attributes."""
    __getattr__ = dict.__getitem__


def initialize_cache_files(names, out_name, device, persist=False):
    if persist:
        os.makedirs(f"workspace/{out_name}", exist_ok=True)
    return Cache({name: FramesOnDisk(f"workspace/{out_name}/{name}", device, persist) for name in names})


@torch.inference_mode()
def initialize_optical_flow(cache, init, consistency_trust, width, height, device):
    """diffusion/video.py:130-158: per frame the forward and the backward flow (one batched estimator pass), clamped; the consistency
    map of the pair; both resized to the synthesis size (the flow times the reference's multiplier, as written there)."""
    flow_model = get_flow_model()
    frames = VideoFrames(init, height=min(height, 512), width=min(width, 512), device=device)
    N = len(frames)

    if len(cache.flow) == N and tuple(cache.flow[0].shape[1:3]) == (height, width):
        print("Optical flow cache seems valid, re-using...")
        return
    else:
        cache.flow.length = cache.consistency.length = 0

    for f_n in range(N):
        prev = frames[(f_n - 1) % N].add(1).div(2)
        curr = frames[f_n].add(1).div(2)

        forward, backward = flow_model.pair(curr, prev)
        maxflow = max(forward.shape[0], forward.shape[1])

        if consistency_trust > 0:
            consistency = check_consistency(forward, backward, clamp=maxflow)
            consistency = resize_bilinear(consistency, (height, width))
            cache.consistency.insert(consistency.unsqueeze(1))

        multiplier = float(np.mean((width / forward.shape[1], height / forward.shape[2])))
        cache.flow.insert(resize_bilinear(forward, (height, width), multiplier=multiplier, clamp=maxflow))


# ======================================================================================================== processor
class VideoFlowDiffusionProcessor(torch.nn.Module):
    def forward(
        self,
        diffusion,
        init: str,
        text: Optional[str] = None,
        image: Optional[str] = None,
        style: Optional[str] = None,
        size: Tuple[int] = (256, 256),
        first_skip: float = 0.4,
        first_frame_init: Optional[str] = None,
        skip: float = 0.7,
        blend: float = 2,
        consistency_trust: float = 0.75,
        wrap_around: int = 0,
        turbo: int = 1,
        noise_injection: float = 0.02,
        flow_exaggeration: float = 1.0,
        pre_hook: Optional[Callable] = None,
        post_hook: Optional[Callable] = None,
        hist_persist: bool = False,
        constant_seed: Optional[int] = None,
        device: str = "cuda",
        preview: bool = False,
        persist: bool = False,
    ):
        # process user inputs
        height, width = [round64(s) for s in size]

        # load init video
        frames = VideoFrames(init, height, width, device)
        N = len(frames)

        # initialize cache
        cache = initialize_cache_files(names=["frame", "flow", "consistency"],
                                       out_name=build_output_name(init if isinstance(init, (str, Path)) else None, unique=False), device=device,
                                       persist=persist)
        cache.frame.length = 0
        initialize_optical_flow(cache, init, consistency_trust, width, height, device)  # calculate optical flow

        if first_frame_init is not None:
            out_img = ImagePrompt(path=first_frame_init, size=(height, width)).img.to(device)
            cache.frame.insert(out_img)
            hist_img = out_img.clone()
        else:
            out_img = None

        loop_fade = torch.sqrt(torch.linspace(1, 0, wrap_around)).tolist()
        turbo_blend = torch.linspace(0, 1, turbo + 1)[1:].tolist()
        turbo_prev_img = turbo_next_img = None

        # the prompts that do not change from frame to frame are built once (the reference builds them per frame from the same arguments)
        fixed_prompts = []
        if style is not None:
            fixed_prompts.append(StylePrompt(path=style, size=(height, width)))
        if text is not None:
            fixed_prompts.append(TextPrompt(text))
        if image is not None:
            fixed_prompts.append(ImagePrompt(path=image))

        try:
            for f_n in range(0, N + wrap_around + turbo, turbo):

                if constant_seed:
                    seed_everything(constant_seed)

                if f_n >= N + wrap_around:
                    turbo_next_img = cache.frame[f_n % N]
                if f_n > 0:  # apply turbo blending
                    for t, f_t in enumerate(range(f_n - turbo, f_n)):
                        if turbo == 1:
                            img = turbo_next_img        # prev * (1 - 1) + next * 1, and the warped prev is dropped below: no launch
                        else:
                            warp_next = t != 0 and f_n < N + wrap_around
                            if turbo_prev_img is None and not warp_next:
                                img = turbo_next_img
                            else:
                                turbo_prev_img, turbo_next_img, img = turbo_step(turbo_prev_img, turbo_next_img, cache.flow[f_t % N],
                                                                                 flow_exaggeration, warp_next, turbo_blend[t])
                        cache.frame.insert(img, f_t % N)
                    out_img = turbo_next_img

                if f_n >= N + wrap_around:
                    break       # the step that only flushes the in-betweens; the reference goes on and raises IndexError at its fade (:268-269)

                prompts = [ContentPrompt(frames[f_n % N])] + fixed_prompts

                init_img = frames[f_n % N]

                prev_img = flow_mask = None
                if blend > 0:
                    if consistency_trust > 0:
                        flow_mask = cache.consistency[f_n % N]
                    prev_img = frames[(f_n - 1) % N] if f_n == 0 else out_img

                wrap = f_n / N >= 1
                late_noise = bool(pre_hook) or (hist_persist and f_n > 0)
                key = draw_noise_key() if (noise_injection != 0 and not late_noise) else 0
                init_img = compose(init_img, prev_img, cache.flow[f_n % N] if prev_img is not None else None, flow_mask,
                                   cache.frame[f_n % N] if wrap else None, flow_exaggeration=flow_exaggeration,
                                   consistency_trust=consistency_trust, blend=blend, fade=loop_fade[f_n % N] if wrap else 1.0,
                                   noise_injection=0.0 if late_noise else noise_injection, seed=key)

                if late_noise:
                    if pre_hook:
                        init_img = pre_hook(init_img)

                    if hist_persist and f_n > 0:
                        init_img = match_histogram(init_img, hist_img)

                    if noise_injection != 0:
                        init_img = compose(init_img, noise_injection=noise_injection, seed=draw_noise_key())

                out_img = diffusion.forward(init_img, prompts, first_skip if f_n == 0 else skip, verbose=False)

                if hist_persist and f_n == 0:
                    hist_img = out_img.clone()

                if post_hook:
                    out_img = post_hook(out_img)

                if preview:
                    import matplotlib.pyplot as plt
                    plt.imshow(out_img.squeeze().add(1).div(2).clamp(0, 1).permute(1, 2, 0).cpu().numpy())
                    plt.axis("off")
                    plt.show(block=False)
                    plt.pause(0.5)

                cache.frame.insert(out_img, f_n % N)

                turbo_prev_img = turbo_next_img
                turbo_next_img = out_img

        except KeyboardInterrupt:
            print("KeyboardInterrupt: saving and quiting...")

        except BaseException:
            for store in cache.values():      # no writer thread outlives a failed run
                store.close()
            raise

        for store in (cache.flow, cache.consistency):        # their writer threads end too (persist=True), with everything written
            store.close()
        return cache.frame.finalize()


@torch.no_grad()
def video_sample(
    diffusion,
    init: str,
    text: Optional[str] = None,
    image: Optional[str] = None,
    style: Optional[str] = None,
    size: Tuple[int] = (256, 256),
    timesteps: int = 50,
    first_skip: float = 0.4,
    first_frame_init: str = None,
    skip: float = 0.7,
    blend: float = 2,
    consistency_trust: float = 0.75,
    wrap_around: int = 0,
    turbo: int = 1,
    noise_injection: float = 0.02,
    flow_exaggeration: float = 1,
    sampler: str = "plms",
    guidance_speed: str = "fast",
    clip_scale: float = 0.0,
    lpips_scale: float = 0.0,
    style_scale: float = 0.0,
    color_match_scale: float = 0.0,
    cfg_scale: float = 5.0,
    match_hist: bool = False,
    hist_persist: bool = False,
    sharpness: float = 1.0,
    constant_seed: Optional[int] = None,
    device: str = "cuda",
    preview: bool = False,
    guided_kwargs=None,
    text_encoder=None,
    clip_models=None,
    persist: bool = False,
):
    """diffusion/video.py:304-379.  ``guided_kwargs`` / ``text_encoder`` / ``clip_models`` reach ``get_diffusion_model`` as in
    ``image_sample``; ``persist``: also write the cache files under ``workspace/``."""
    if isinstance(diffusion, str) and diffusion in OTHER_PROCESSORS:
        raise NotImplementedError(f'diffusion="{diffusion}": the latent / stable / glide / glid3xl processors are not built; "guided" or a '
                                  f'processor instance')
    if isinstance(diffusion, str):
        diffusion = get_diffusion_model(
            diffusion=diffusion,
            timesteps=timesteps,
            sampler=sampler,
            guidance_speed=guidance_speed,
            clip_scale=clip_scale,
            lpips_scale=lpips_scale,
            style_scale=style_scale,
            color_match_scale=color_match_scale,
            cfg_scale=cfg_scale,
            image=image,
            guided_kwargs=guided_kwargs,
            text_encoder=text_encoder,
            clip_models=clip_models,
            text=text,
        )

    pre_hook = partial(match_histogram, source_tensor=StylePrompt(path=style).img) if match_hist else None

    post_fns = []
    if sharpness != 1.0:
        post_fns.append(partial(sharpen, strength=sharpness))
    post_hook = (lambda img: reduce(lambda i, f: f(i), post_fns, img)) if len(post_fns) > 0 else None

    video = VideoFlowDiffusionProcessor()(
        diffusion=diffusion,
        init=init,
        text=text,
        image=image,
        style=style,
        size=size,
        first_skip=first_skip,
        first_frame_init=first_frame_init,
        skip=skip,
        blend=blend,
        consistency_trust=consistency_trust,
        wrap_around=wrap_around,
        turbo=turbo,
        noise_injection=noise_injection,
        flow_exaggeration=flow_exaggeration,
        pre_hook=pre_hook,
        post_hook=post_hook,
        hist_persist=hist_persist,
        constant_seed=constant_seed,
        device=device,
        preview=preview,
        persist=persist,
    )
    return video


def build_parser():
    # fmt:off
    import argparse
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, allow_abbrev=True)
    parser.add_argument("--init", type=str, default="random", help='How to initialize the image "random", "perlin", or a path to an image file.')
    parser.add_argument("--text", type=str, default=None, help='A text prompt to visualize.')
    parser.add_argument("--image", type=str, default=None, help='An image prompt to use (overrides --text and uses Justin Pinkney\'s image conditioned Stable Diffusion model).')
    parser.add_argument("--style", type=str, default=None, help='An image whose style should be optimized for in the output image (only works with "guided" diffusion at the moment, see --style-scale).')
    parser.add_argument("--size", type=width_height, default=(512, 512), help='Size to synthesize the video at.')
    parser.add_argument("--skip", type=float, default=0.85, help='Lower fractions will stray further from the original image, while higher fractions will hallucinate less detail.')
    parser.add_argument("--first-skip", type=float, default=0.4, help='Separate skip fraction for the first frame.')
    parser.add_argument("--first-frame-init", type=str, default=None, help='Image file to initialize the first frame with (will over-rule --first-skip).')
    parser.add_argument("--timesteps", type=int, default=50, help='Number of timesteps to sample the diffusion process at. Higher values will take longer but are generally of higher quality.')
    parser.add_argument("--blend", type=float, default=2, help='Factor with which to blend previous frames into the next frame. Higher values will stay more consistent over time (e.g. --blend 20 means 20:1 ratio of warped previous frame to new input frame).')
    parser.add_argument("--consistency-trust", type=float, default=0.75, help='How strongly to trust flow consistency mask. Lower values will lead to more consistency over time. Higher values will respect occlusions of the background more.')
    parser.add_argument("--wrap-around", type=int, default=0, help='Number of extra frames to continue for, looping back to start. This allows for seamless transitions back to the start of the video.')
    parser.add_argument("--turbo", type=int, default=1, help='Only apply diffusion every --turbo\'th frame, otherwise just warp the previous frame with optical flow. Can be much faster for high factors at the cost of some visual detail.')
    parser.add_argument("--noise-injection", type=float, default=0.02, help='Inject a little bit of extra noise between each frame. Helps counteract loss of detail and formation of large empty regions.')
    parser.add_argument("--flow-exaggeration", type=float, default=1, help='Factor to multiply optical flow with. Higher values lead to more extreme movements in the final video.')
    parser.add_argument("--diffusion", type=str, default="stable", help='Which diffusion model to use. Options: "guided", "latent", "glide", "glid3xl", "stable" or a /path/to/stable-diffusion.ckpt')
    parser.add_argument("--sampler", type=str, default="lms", choices=["p", "ddim", "plms", "euler", "euler_ancestral", "heun", "dpm_fast", "dpm_adaptive", "dpm_2", "dpm_2_ancestral", "lms"], help='Which sampling method to use. "p", "ddim", and "plms" work for all diffusion models, the rest are currently only supported with "stable" diffusion.')
    parser.add_argument("--guidance-speed", type=str, default="fast", choices=["regular", "fast"], help='How to perform "guided" diffusion. "regular" is slower but can be higher quality, "fast" corresponds to the secondary model method (a.k.a. Disco Diffusion).')
    parser.add_argument("--clip-scale", type=float, default=0.0, help='Controls strength of CLIP guidance when using "guided" diffusion.')
    parser.add_argument("--lpips-scale", type=float, default=0.0, help='Controls the apparent influence of the content image when using "guided" diffusion and a --content image.')
    parser.add_argument("--style-scale", type=float, default=0.0, help='When using "guided" diffusion and a --style image, a higher --style-scale enforces textural similarity to the style, while a lower value will be conceptually similar to the style.')
    parser.add_argument("--color-match-scale", type=float, default=0.0, help='When using "guided" diffusion, the --color-match-scale guides the output\'s colors to match the --style image.')
    parser.add_argument("--cfg-scale", type=float, default=7.5, help='Classifier-free guidance strength. Higher values will match the text prompt more closely at the cost of output variability.')
    parser.add_argument("--match-hist", action="store_true", help='Match the color histogram of the initialization image to the --style image before starting diffusion.')
    parser.add_argument("--hist-persist", action="store_true", help='Match the color histogram of subsequent frames to the first diffused frame (helps alleviate oversaturation).')
    parser.add_argument("--sharpness", type=float, default=1.0, help='Sharpen the image by this amount after each diffusion scale (a value of 1.0 will leave the image unchanged, higher values will be sharper).')
    parser.add_argument("--constant-seed", type=int, default=None, help='Use a fixed noise seed for all frames (None to disable).')
    parser.add_argument("--device", type=str, default="cuda", help='Which device to use (e.g. "cpu" or "cuda:1")')
    parser.add_argument("--preview", action="store_true", help='Show frames as they\'re rendered (moderately slower).')
    parser.add_argument("--fps", type=int, default=12, help='Framerate of output video.')
    parser.add_argument("--out-dir", type=str, default="output/", help='Directory to save output images to.')
    # fmt:on
    return parser


def main(argv=None):
    """``python -m maua.diffusion.video``: the reference's flags (:382-426); the video goes to ``--out-dir`` (the reference writes to
    ``output/`` whatever the flag says).  Not in the reference: MAUA_ALLOW_RANDOM_INIT=1 in the environment runs with randomly
    initialised networks when the guided-diffusion checkpoints are missing (smoke runs)."""
    args = build_parser().parse_args(argv)
    if args.sampler == "lms" and args.diffusion == "guided":
        args.sampler = "plms"      # the CLI's default sampler is a "stable"-only one; video_sample's own default for "guided"
    out_name = build_output_name(args.init, args.style, args.text, args.image)[:222]
    out_dir, fps = args.out_dir, args.fps
    del args.out_dir, args.fps
    kw = vars(args)
    if os.environ.get("MAUA_ALLOW_RANDOM_INIT") == "1":
        kw["guided_kwargs"] = dict(allow_random_init=True)
    video = video_sample(**kw)
    Path(out_dir).mkdir(parents=True, exist_ok=True)
    path = f"{out_dir}/{Path(args.diffusion).stem}_{out_name}.mp4"
    write_video(video, path, fps=fps, value_range=(-1, 1))
    print(path)


if __name__ == "__main__":
    main()
