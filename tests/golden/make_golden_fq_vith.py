"""Generate ``fq_vith_d2_img256.npz``: the reference's fq_vit W8A8 encoder at ViT-H dims.

``make_golden.py``'s ``make_fq`` at embed 1280, 16 heads (head dim 80), depth 2 with block 1 global
(``global_attn_indexes=[1]``), img 256: minmax calibration on the images of seeds 21 / 22, quant
forward on the image of seed 23.  Same keys as ``fq_vitb_img256.npz`` (output codes, the 30 QAct
scales with their names, every per-channel weight scale, meta JSON) -- data only.

Run where a checkout of the reference is available, never on the GPU box:

    python tests/golden/make_golden_fq_vith.py --reference <path to the reference checkout>
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from functools import partial
from pathlib import Path

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))

from oracle import synth  # noqa: E402

IMG, DEPTH, GLOBAL, SEED = 256, 2, (1,), 200 + 256
CALIB_SEEDS, TEST_SEED = (21, 22), 23
OUT = HERE / "fq_vith_d2_img256.npz"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SAMQ_REFERENCE"), required="SAMQ_REFERENCE" not in os.environ,
                    help="the reference checkout (or $SAMQ_REFERENCE)")
    ref = Path(ap.parse_args().reference)
    sys.path.insert(0, str(ref))
    sys.path.insert(0, str(ref / "fq_vit"))
    from fq_vit.models.sam.image_encoder import ImageEncoderViT as FQEnc
    from fq_vit.models.ptq.layers import QIntLayerNorm
    from fq_vit.models.ptq import QAct, QConv2d, QLinear, QIntSoftmax
    from fq_vit.config import Config
    from models import BIT_TYPE_DICT
    torch.manual_seed(0)
    cfgq = Config(False, False, "minmax")
    cfgq.BIT_TYPE_A = BIT_TYPE_DICT["int8"]
    cfg = synth.encoder_config("vit_h", depth=DEPTH, global_attn_indexes=GLOBAL, img_size=IMG)
    assert cfg["embed_dim"] == 1280 and cfg["num_heads"] == 16
    enc = FQEnc(depth=DEPTH, embed_dim=1280, img_size=IMG, mlp_ratio=4, norm_layer=partial(QIntLayerNorm, eps=1e-6),
                num_heads=16, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=list(GLOBAL),
                window_size=14, out_chans=256, quant=False, calibrate=False, cfg=cfgq)
    state = {k: v.astype(np.float16).astype(np.float32) for k, v in synth.make_encoder_state(cfg, seed=SEED).items()}
    missing, unexpected = enc.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(("quantizer" in m) or ("qact" in m) for m in missing), missing
    enc.eval()
    imgs = [synth.make_images(1, IMG, seed=s) for s in CALIB_SEEDS]
    test_img = synth.make_images(1, IMG, seed=TEST_SEED)
    mods = [m for m in enc.modules() if type(m) in (QConv2d, QLinear, QAct, QIntSoftmax)]
    t0 = time.time()
    with torch.no_grad():
        for m in mods:
            m.calibrate = True
        for i, im in enumerate(imgs):
            if i == len(imgs) - 1:
                for m in mods:
                    m.last_calibrate = True
            enc(torch.from_numpy(im))
        for m in mods:
            m.calibrate = False
            m.quant = True
        out = enc(torch.from_numpy(test_img)).numpy()
    print(f"fq vit_h depth {DEPTH} img {IMG}: {time.time() - t0:.1f}s absmax {np.abs(out).max():.3f}")
    scales = {name: float(m.quantizer.scale.reshape(-1)[0]) for name, m in enc.named_modules() if isinstance(m, QAct)}
    wscales = {name: m.quantizer.scale.reshape(-1).numpy() for name, m in enc.named_modules()
               if isinstance(m, (QLinear, QConv2d))}
    s_out = scales["qacts.3"]
    codes = np.round(out / s_out)
    assert np.abs(codes * s_out - out).max() < 1e-5 * max(1.0, np.abs(out).max())
    np.savez_compressed(OUT, codes=codes.astype(np.int8), out_scale=np.float32(s_out),
                        act_scale_names=np.array(list(scales.keys())),
                        act_scales=np.array(list(scales.values()), np.float32),
                        **{"wscale:" + k: v for k, v in wscales.items()},
                        meta=json.dumps(dict(img_size=IMG, seed=SEED, calib_seeds=list(CALIB_SEEDS), test_seed=TEST_SEED,
                                             model="vit_h", depth=DEPTH, global_attn_indexes=list(GLOBAL),
                                             torch=torch.__version__)))
    print("wrote", OUT, OUT.stat().st_size, "bytes,", len(scales), "QActs")


if __name__ == "__main__":
    main()
