"""Micro-benchmark of the W8A8 (fq_vit) attention kernels on the vit_b geometry (64 x 64 grid,
12 heads of 64, windows of 14 and global) or, ``--model vit_h``, the vit_h one (16 heads of 80), HIP
events on the launch stream; outputs of every run compared with the first (determinism).
``SAMQ_LIB`` selects a variant library.  ``--side`` / ``--window`` reach the generic kernel: a global grid
below 64 x 64 (streaming) and windows other than 14 (resident keys; 8 runs 13 waves, 16 runs 16).

    python tools/bench_attn_q8.py [--model vit_b] [--batch 1] [--iters 20] [--side 32] [--window 8 16 0]
"""
import argparse
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))
from samq import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("vit_b", "vit_h"), default="vit_b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window-only", action="store_true")
    ap.add_argument("--global-only", action="store_true")
    ap.add_argument("--side", type=int, default=64, help="token grid side")
    ap.add_argument("--window", type=int, nargs="+", help="window sizes to time (0 = global); default 14 and 0")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    heads, d = {"vit_b": (12, 64), "vit_h": (16, 80)}[args.model]
    b, side = args.batch, args.side
    c = heads * d
    qkv = torch.randint(-100, 100, (b, side, side, 3 * c), generator=g, device=dev, dtype=torch.int8)
    bias = torch.randn(3 * c, generator=g, device=dev) * 0.1
    stream = torch.cuda.current_stream()
    for window in args.window or ((14,) if args.window_only else ((0,) if args.global_only else (14, 0))):
        s = 2 * (window or side) - 1
        rh = torch.randn(s, d, generator=g, device=dev) * 0.1
        rw = torch.randn(s, d, generator=g, device=dev) * 0.1

        # the fp16 copy of V is read by the 64 x 64 global kernel only
        v16 = qkv[..., 2 * c:].to(torch.float16).contiguous() if window == 0 and side == 64 else None

        def run(v=None):
            return ops.rel_attention_q8(qkv, bias if window else None, rh, rw, heads, window, d ** -0.5, 0.05, 0.08,
                                        0.1, 0.03, v16=v)
        ref = run()
        if v16 is not None:   # the global kernel staging V from the fp16 copy (the engine's path)
            assert torch.equal(run(v16), ref)
            b16 = 1e9
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.iters):
                    run(v16)
                e1.record(stream)
                torch.cuda.synchronize()
                b16 = min(b16, e0.elapsed_time(e1) / args.iters * 1e3)
            print(f"attention_q8 {args.model} side={side} window= 0 B={b} with fp16 V: {b16:8.1f} us", flush=True)
        best = 1e9
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.iters):
                run()
            e1.record(stream)
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / args.iters * 1e3)
        same = torch.equal(run(), ref)
        keys = (window * window) if window else side * side
        nq = b * side * side
        gop = 2 * 2 * nq * keys * d * heads / 1e9
        print(f"attention_q8 {args.model} side={side} window={window:2d} B={b}: {best:8.1f} us  {gop / best * 1e3:7.1f} TOPS (q.k + p.v)  "
              f"deterministic: {same}", flush=True)


if __name__ == "__main__":
    main()
