"""Score a render's audio-reactivity: matrix correlations between the audio features and the video features of the same frames.

No reference counterpart: the reference holds the instruments (features/video.py, features/correlation.py) and its thesis evaluation
combined them by hand.  Here they are one call on the device:

    table = audiovisual_score(audio_features, video_features)          # dicts of [T, F] device tensors
    python -m maua_amd.audiovisual.score --audio_file clip.wav --frames frames.npy --fps 30

The video features come from ``maua_amd.video_features.VideoAnalyzer`` (what ``FFMPEG.__call__(..., analyzer=...)`` fills during a
render), the audio features from ``sample.retrieve_music_information``.
"""
import argparse

import numpy as np
import torch

from .. import correlation as CR

ALL = "all"


def audiovisual_score(audio_features, video_features, metrics=("rv2", "autocorrcorr")):
    """``audio_features`` / ``video_features``: {name: [T, F]} over the same frames (when the two sides differ in length, as a hop-aligned
    audio analysis and a render may by a frame, both are cut to the shorter).  Returns {"audio": row names, "video": column names,
    metric: float32 tensor [rows, columns] on the host, ...}: every audio feature against every video feature, with a last row and column
    ``"all"`` for the concatenation of the side's features.  Metrics that need Fx == Fy (pearson, concordance, r1) raise on a pair of
    unequal widths."""
    if not audio_features or not video_features:
        raise ValueError("audiovisual_score: both sides need at least one feature")
    for m in metrics:
        if m not in CR.METRICS:
            raise ValueError(f"audiovisual_score: unknown metric {m!r}: the metrics are {list(CR.METRICS)}")

    a = {k: (m if m.dim() > 1 else m.unsqueeze(-1)).float() for k, m in audio_features.items()}
    v = {k: (m if m.dim() > 1 else m.unsqueeze(-1)).float() for k, m in video_features.items()}
    T = min(min(m.shape[0] for m in a.values()), min(m.shape[0] for m in v.values()))
    a = {k: m[:T].reshape(T, -1).contiguous() for k, m in a.items()}
    v = {k: m[:T].reshape(T, -1).contiguous() for k, m in v.items()}
    a[ALL] = torch.cat(list(a.values()), dim=1)
    v[ALL] = torch.cat(list(v.values()), dim=1)
    table = {"audio": list(a), "video": list(v)}
    for m in metrics:
        cells = [CR.correlation(m, x, y) for x in a.values() for y in v.values()]
        table[m] = torch.stack(cells).reshape(len(a), len(v)).cpu()
    return table


def format_table(table):
    lines = []
    for m in (k for k in table if k not in ("audio", "video")):
        w = max(len(n) for n in table["audio"]) + 2
        lines.append(f"{m}".ljust(w) + " ".join(c.rjust(15) for c in table["video"]))
        for name, row in zip(table["audio"], table[m]):
            lines.append(name.ljust(w) + " ".join(f"{float(x):15.4f}" for x in row))
        lines.append("")
    return "\n".join(lines)


def score_frames(audio_file, frames, fps=30, metrics=("rv2", "autocorrcorr"), bins=32, batch_size=16, audio_offset=0, audio_duration=None):
    """Score a MemMap render (``frames``: the path of its uint8 [T, 3, H, W] ``.npy``, or such an array) against its audio."""
    from ..audio_io import load_audio
    from ..video_features import VideoAnalyzer
    from .sample import retrieve_music_information
    if isinstance(frames, str):
        frames = np.load(frames, mmap_mode="r")
    if frames.ndim != 4 or frames.shape[1] != 3 or frames.dtype != np.uint8:
        raise ValueError(f"frames must be uint8 [T, 3, H, W] (render/memmap.py), got {frames.dtype} {frames.shape}")
    audio, sr = load_audio(audio_file, audio_offset, audio_duration, fps)
    features, _, _ = retrieve_music_information(audio, sr)
    an = VideoAnalyzer(frames.shape[2], frames.shape[3], bins=bins, max_batch=batch_size)
    for i in range(0, frames.shape[0], batch_size):
        an.push(torch.from_numpy(np.ascontiguousarray(frames[i:i + batch_size])))
    table = audiovisual_score(features, an.features(), metrics)
    an.close()
    return table


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="score a MemMap render (uint8 [T, 3, H, W] .npy) against its audio")
    ap.add_argument("--audio_file", required=True)
    ap.add_argument("--frames", required=True, help="the render's frames_memmap.npy")
    ap.add_argument("--fps", type=float, default=30)
    ap.add_argument("--metrics", nargs="+", default=["rv2", "autocorrcorr"], choices=list(CR.METRICS))
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--audio_offset", type=float, default=0)
    ap.add_argument("--audio_duration", type=float, default=None)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    table = score_frames(a.audio_file, a.frames, a.fps, tuple(a.metrics), a.bins, a.batch_size, a.audio_offset, a.audio_duration)
    print(format_table(table))
    return table


if __name__ == "__main__":
    main()
