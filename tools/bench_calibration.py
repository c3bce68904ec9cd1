#!/usr/bin/env python3
"""Wall time of fq_vit calibration per activation observer: HIP observers vs the torch-op path.

    python tools/bench_calibration.py [--img 1024] [--images 3] [--methods minmax ema percentile omse]
                                      [--paths hip torch] [--out calib.jsonl]

For each (path, method): a fresh random vit_b encoder (same seed), ``calibrate_with`` of ``--images``
seeded images on the GPU, timed on the host clock between device synchronisations.  ``torch`` forces
the observer classes onto their torch ops (``MinmaxObserver.use_hip = False``): the reference's
behaviour, np.percentile on the host above 2**24 elements included.  One JSON line per result
(appended to ``--out`` as it is measured, so a slow configuration cannot lose the earlier ones).
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "sam-quantization_amd"))

import torch  # noqa: E402


def build(method, img, seed=0):
    from samq import fq_vit
    cfg = fq_vit.Config(False, False, method)
    cfg.BIT_TYPE_A = fq_vit.BIT_TYPE_DICT["int8"]
    enc = fq_vit.build_fq_image_encoder("vit_b", img_size=img, cfg=cfg)
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if name.endswith(("norm1.weight", "norm2.weight")) or name in ("neck.1.weight", "neck.3.weight"):
                p.copy_(1 + 0.05 * torch.randn(p.shape, generator=g))
            elif "rel_pos" in name or name == "pos_embed":
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return enc.cuda().eval(), g


def run(method, path, img, images):
    from samq import fq_vit
    fq_vit.MinmaxObserver.use_hip = path == "hip"
    enc, g = build(method, img)
    imgs = [torch.randn((1, 3, img, img), generator=g).cuda() for _ in range(images)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc.calibrate_with(imgs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    scales = [float(m.quantizer.scale) for m in fq_vit.act_quantizers(enc).values()]
    return dt, sum(scales)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=1024)
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--methods", nargs="+", default=["minmax", "ema", "percentile", "omse"])
    ap.add_argument("--paths", nargs="+", default=["hip", "torch"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    try:
        rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
    except OSError:
        rev = ""
    import hashlib
    from samq import _lib
    lib = hashlib.sha256(_lib.LIB_PATH.read_bytes()).hexdigest()[:12]      # the build that was measured
    dev = torch.cuda.get_device_name(0)
    run("minmax", "hip", a.img, 1)      # warm-up: library load, allocator, rocBLAS
    for path in a.paths:
        for method in a.methods:
            dt, chk = run(method, path, a.img, a.images)
            line = json.dumps(dict(method=method, path=path, img=a.img, images=a.images, seconds=round(dt, 3),
                                   scale_sum=chk, device=dev, torch=torch.__version__, rev=rev, lib_sha256=lib))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
