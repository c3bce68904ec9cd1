#!/usr/bin/env python3
"""The click simulator's next click per call: ``ops.next_click`` against the host composition it replaces.

    python tools/bench_clicker.py [--reps 7] [--out clicker.jsonl]

Masks at 1024 x 1024, ``n = 1`` and ``n = 16`` per call, three scenes: ``rim`` (the prediction is the seeded blob
ground truth moved by 6 pixels: thin error rims of both kinds), ``half`` (the prediction misses everything left
of the image's middle: an error region half the image wide) and ``canvas`` (all ground truth, nothing predicted:
one false-negative region over the whole image, the row search's worst case).  The host composition downloads
both masks, takes ``scipy.ndimage.distance_transform_edt`` of the two padded error masks per mask, crops, and
takes the maxima and the first arg-max (always scipy, so that the baseline is the same on every machine;
OpenCV's ``distanceTransform``, which the upstream clicker calls, is not timed).  The two paths alternate
``--reps`` times after a warm-up of each; a timed run is ``inner`` back-to-back calls on the host clock between device
synchronisations (the HIP path ends in its one host read).  One JSON line per point: medians per call in ms,
min / max of the runs, and whether click, sign and both maxima agree."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))
sys.path.insert(0, str(REPO / "tools"))

import torch  # noqa: E402

from bench_amg import compare  # noqa: E402


def host_edt():
    from scipy.ndimage import distance_transform_edt
    return "scipy.ndimage", distance_transform_edt


def host_next_click(pred, gt, edt):
    pred, gt = pred.cpu().numpy(), gt.cpu().numpy()
    rows = []
    for p, g in zip(pred, gt):
        obj, keep = g == 1, g != -1
        fn, fp = (edt(np.pad(m, 1))[1:-1, 1:-1] for m in (obj & ~p & keep, ~obj & p & keep))
        pos = fn.max() > fp.max()
        ys, xs = np.where(fn == fn.max()) if pos else np.where(fp == fp.max())
        rows.append([int(pos), int(ys[0]), int(xs[0]), int(round(fn.max() ** 2)), int(round(fp.max() ** 2)),
                     int((p & obj & keep).sum()), int(((p | obj) & keep).sum()), 0])
    return rows


def scene(kind, n, size, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:size, 0:size]
    gt = np.zeros((n, size, size), np.int8)
    for i in range(n):
        for cy, cx, r in zip(rng.uniform(0, size, 6), rng.uniform(0, size, 6), rng.uniform(0.05, 0.25, 6) * size):
            gt[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    if kind == "canvas":
        return np.zeros(gt.shape, dtype=bool), np.ones_like(gt)
    if kind == "half":
        gt[:, :, : size // 2] = 1
        pred = gt == 1
        pred[:, :, : size // 2] = False
        return pred, gt
    return np.roll(gt == 1, (6, 6), (1, 2)), gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clicker: no GPU visible; timings are taken on the GPU only")
    from samq import ops
    dev = torch.device("cuda:0")
    name, edt = host_edt()
    for kind in ("rim", "half", "canvas"):
        for n in (1, 16):
            pred, gt = (torch.from_numpy(v).to(dev) for v in scene(kind, n, a.size, n))
            res, out = compare({"host": lambda: host_next_click(pred, gt, edt),
                                "hip": lambda: ops.next_click(pred, gt).tolist()}, a.reps)
            line = json.dumps(dict(op="next_click", scene=kind, n=n, size=a.size, **res, host=name,
                                   fn_fp_max_d2=[r[3:5] for r in out["hip"]][:2], equal=out["hip"] == out["host"],
                                   reps=a.reps, device=torch.cuda.get_device_name(0)))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
