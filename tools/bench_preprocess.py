#!/usr/bin/env python3
"""Wall time of ``SamPredictor.set_image`` from a numpy image to features ready, with the resize on the host
(PIL, as ``ResizeLongestSide.apply_image``) and on the device (``ops.resize_u8``).

    python tools/bench_preprocess.py [--reps 7] [--models w4a16_vit_h,w8a8_vit_b] [--out preprocess.jsonl]

Per model (random weights: W4A16 ViT-H through the uint8 patch-embedding entry, W8A8 fq_vit vit_b through the
float variant) and image size (1500 x 2250, 480 x 640, seeded uniform bytes), four timed paths that alternate
``--reps`` times after a warm-up of each, on the host clock between device synchronisations:

  pil      the host resize alone (no device work)
  host     resize on the host, upload of the resized image, ``set_torch_image``: ``set_image`` before the kernel
  hip      ``set_image``: upload of the raw image, ``ops.resize_u8``, encoder
  kernel   ``ops.resize_u8`` alone on a resident image (uint8 variant)

One JSON line per point: medians in ms, min / max of the runs and whether ``host`` and ``hip`` leave equal features.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(name, dev):
    from samq.build_sam import Sam
    from samq.synthetic import random_fq_encoder, random_quant_encoder
    enc = random_quant_encoder("vit_h", device=dev) if name == "w4a16_vit_h" else random_fq_encoder("vit_b", device=dev)
    return Sam(enc).to(dev).eval()


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def point(name, pred, size, reps):
    from samq import ops
    dev = pred.device
    img = np.random.Generator(np.random.PCG64(size[0])).integers(0, 256, size + (3,), dtype=np.uint8)
    hw = pred.transform.get_preprocess_shape(*size, pred.transform.target_length)
    resident = torch.from_numpy(img).to(dev)

    def host():
        inp = pred.transform.apply_image(img)
        pred.set_torch_image(torch.as_tensor(inp, device=dev).permute(2, 0, 1).contiguous()[None], size)

    paths = {"pil": lambda: pred.transform.apply_image(img), "host": host, "hip": lambda: pred.set_image(img),
             "kernel": lambda: ops.resize_u8(resident, hw)}
    inner, t = {}, {k: [] for k in paths}
    for k, fn in paths.items():
        timed(fn, 1)
        inner[k] = max(1, min(200, int(40.0 / max(timed(fn, 1), 1e-3))))
    for _ in range(reps):
        for k, fn in paths.items():
            t[k].append(timed(fn, inner[k]))
    host()
    ref = pred.get_image_embedding().clone()
    pred.set_image(img)
    rec = dict(model=name, size=list(size), resized=list(hw), inner=inner,
               equal=bool(torch.equal(ref, pred.get_image_embedding())))
    for k, v in t.items():
        rec[f"{k}_ms"] = round(statistics.median(v), 4)
        rec[f"{k}_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--models", default="w4a16_vit_h,w8a8_vit_b")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_preprocess: no GPU visible; timings are taken on the GPU only")
    import samq
    dev = torch.device("cuda:0")
    for name in a.models.split(","):
        pred = samq.SamPredictor(build(name, dev))
        for size in ((1500, 2250), (480, 640)):
            line = json.dumps(dict(point(name, pred, size, a.reps), reps=a.reps, device=torch.cuda.get_device_name(0)))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
