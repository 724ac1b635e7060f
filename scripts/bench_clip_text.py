"""CLIP's text tower (CLIP.encode_text, csrc/clip_text.hip + the causal attention of csrc/attention.hip) on one GPU: device-event time of
one ``TextTransformer`` forward at the ViT-B/16 text config (77 tokens, width 512, 12 layers, 8 heads), bf16, random init, for 1 / 16
/ 64 prompts after warm-up.  ``--profile``: the same run again in a child process under ``rocprofv3 --kernel-trace --stats``, and the
causal attention kernel's share of the summed kernel time.  Not part of bench.py: the tower runs once per prompt set, off the loop.
``python scripts/bench_clip_text.py [--reps 20] [--profile] [--out DIR]``"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def time_encode(sizes, reps, warmup):
    import torch
    from maua_amd.clip import TEXT_CONFIGS, TextTransformer
    cfg = TEXT_CONFIGS["ViT-B/16"]
    tt = TextTransformer(*cfg, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(1)
    res = {}
    for n in sizes:
        tok = torch.randint(1, cfg[1] - 2, (n, cfg[0]), generator=g, dtype=torch.int32)
        tok[:, 0] = cfg[1] - 2
        eot = torch.randint(2, cfg[0], (n,), generator=g)
        for r in range(n):
            tok[r, eot[r]] = cfg[1] - 1
            tok[r, eot[r] + 1:] = 0
        tok = tok.cuda()
        for _ in range(warmup):
            tt(tok)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = []
        for _ in range(reps):
            ev[0].record()
            tt(tok)
            ev[1].record()
            ev[1].synchronize()
            times.append(ev[0].elapsed_time(ev[1]))
        times.sort()
        res[n] = dict(median_ms=times[len(times) // 2], min_ms=times[0], per_prompt_us=1e3 * times[len(times) // 2] / n)
    return res


def kernel_share(stats_csv):
    """(causal attention ns, all kernels ns, {kernel: ns}) from rocprofv3's kernel_stats.csv."""
    tot, att, per = 0.0, 0.0, {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            tot += ns
            per[row["Name"]] = ns
            if "attention_kernel" in row["Name"] and "true" in row["Name"]:
                att += ns
    return att, tot, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="also run once under rocprofv3 --kernel-trace --stats (a child process)")
    ap.add_argument("--out", default="build/clip_text_prof")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.profile:
        a.out = os.path.abspath(a.out)
        os.makedirs(a.out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out, "-o", "clip_text", "--",
               sys.executable, os.path.abspath(__file__), "--sizes", a.sizes, "--reps", "5", "--warmup", "1"]
        r = subprocess.run(cmd, cwd=ROOT)
        if r.returncode != 0:
            sys.exit(f"rocprofv3 run failed ({r.returncode})")
        found = glob.glob(os.path.join(a.out, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            sys.exit("no kernel_stats.csv written")
        att, tot, per = kernel_share(found[0])
        top = sorted(per.items(), key=lambda kv: -kv[1])[:8]
        print(json.dumps(dict(causal_attention_ms=att / 1e6, all_kernels_ms=tot / 1e6, causal_attention_share=att / max(tot, 1.0),
                              top_kernels_ms={k[:90]: v / 1e6 for k, v in top})))
        return
    res = time_encode(sizes, a.reps, a.warmup)
    print(json.dumps({"clip_text_encode_ViT-B/16_bf16": res}))


if __name__ == "__main__":
    main()
