#!/usr/bin/env python3
"""Wall time of ``GPTQ.fasterquant`` per layer: the HIP column loop against the torch-op loop.

    python tools/bench_gptq.py [--shapes 3840x1280 1280x1280 5120x1280 1280x5120] [--groupsizes -1 128]
                               [--tokens 2048] [--reps 3] [--out gptq.jsonl]

For each (rows x K, groupsize): a seeded random weight and a Hessian accumulated from ``--tokens`` random
token rows; ``fasterquant(backend="torch")`` and the automatic pick (the kernel) alternate ``--reps`` times
after one warm-up of each, timed on the host clock between device synchronisations.  ``prepare`` (dead
columns, damping, the two Cholesky calls) is timed on its own: both paths pay it, ``loop_*`` is the total
minus that share.  ``same_codes`` is the share of integer codes on which the two paths agree on that layer.
One JSON line per point (medians, seconds), appended to ``--out`` as it is measured.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))

import torch  # noqa: E402


def timed(dev, fn):
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def point(rows, k, gs, tokens, reps, dev):
    from samq.gptq import GPTQ
    g = torch.Generator(device="cpu").manual_seed(rows * 7 + k)
    w0 = (0.02 * torch.randn((rows, k), generator=g)).to(dev)
    x = torch.randn((tokens, k), generator=g).to(dev)
    lin = torch.nn.Linear(k, rows, bias=False).to(dev)
    q = GPTQ(lin)
    q.add_batch(x)
    h0 = q.H.clone()

    def fresh():
        lin.weight.data = w0.clone()
        q.H = h0.clone()

    t = {"prepare": [], "torch": [], "hip": []}
    codes = {}
    for rep in range(reps + 1):
        for path in ("prepare", "hip", "torch"):
            fresh()
            if path == "prepare":
                dt, _ = timed(dev, lambda: q.prepare(0.01, False))
            else:
                backend = "auto" if path == "hip" else "torch"
                dt, (s, z) = timed(dev, lambda: q.fasterquant(groupsize=gs, backend=backend))
                rep_g = k // s.shape[1]
                c = torch.round(lin.weight.data / s.repeat_interleave(rep_g, 1)) + z.repeat_interleave(rep_g, 1)
                codes[path] = c
            if rep:   # rep 0 is the warm-up
                t[path].append(dt)
    same = float((codes["hip"] == codes["torch"]).float().mean())   # share of identical codes, hip vs torch
    dist = float((codes["hip"] - codes["torch"]).abs().max())
    med = {p: statistics.median(v) for p, v in t.items()}
    return dict(rows=rows, K=k, groupsize=gs, prepare_s=round(med["prepare"], 5), torch_s=round(med["torch"], 5),
                hip_s=round(med["hip"], 5), loop_torch_s=round(med["torch"] - med["prepare"], 5),
                loop_hip_s=round(med["hip"] - med["prepare"], 5), hip_min_s=round(min(t["hip"]), 5),
                hip_max_s=round(max(t["hip"]), 5), torch_min_s=round(min(t["torch"]), 5),
                torch_max_s=round(max(t["torch"]), 5), same_codes=round(same, 6), max_code_distance=dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["3840x1280", "1280x1280", "5120x1280", "1280x5120"])
    ap.add_argument("--groupsizes", nargs="+", type=int, default=[-1, 128])
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gptq: no GPU visible; timings are taken on the GPU only")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    for shape in a.shapes:
        rows, k = (int(v) for v in shape.split("x"))
        for gs in a.groupsizes:
            res = dict(point(rows, k, gs, a.tokens, a.reps, dev), tokens=a.tokens, reps=a.reps, device=name)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
