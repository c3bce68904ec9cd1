"""Generate ``fq_observers.npz``: what the reference's ema / percentile / omse observers compute.

Run where the reference checkout is available (read-only, see ``make_golden.py``); never on the
GPU box.  Inputs come from ``tests/_observer_ref.py`` (seeded), so the fixture holds only running
statistics, scales, zero points, chosen omse candidates and the module-level scales / codes:

* ``obs:<method>:<case>:max`` / ``:min`` -- running ``max_val`` / ``min_val`` after each of the three
  updates (stacked), ``:scale`` / ``:zp`` -- the final quantisation parameters; for omse also
  ``:idx`` (the chosen candidate) and ``:gap`` (float64 relative gap to the runner-up).  The script
  asserts that the reference's pick (f32 ``.mean()``) equals the float64 pick on every omse input.
* ``mod:<method>:scales`` (140, in ``act_scale_names`` order), ``mod:omse:zps``, ``mod:omse:codes``
  (``round(out / s_out)`` of the quant forward on the test image) -- vit_b at img 256 with the state
  of ``fq_vitb_img256.npz``, calibrated on three images.
"""
from __future__ import annotations

import json
import sys
import time
from functools import partial
from pathlib import Path

sys.dont_write_bytecode = True

import numpy as np
import torch

REF = Path("/root/reference")
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REF))
sys.path.insert(0, str(REF / "fq_vit"))

from oracle import synth  # noqa: E402
import _observer_ref as R  # noqa: E402


def observer_level(out: dict):
    from models import BIT_TYPE_DICT
    from models.ptq.observer.build import build_observer
    bt = BIT_TYPE_DICT["int8"]
    for method, cases in R.METHOD_CASES.items():
        for case in cases:
            module_type, mode, _, permute, _ = R.OBSERVER_CASES[case]
            obs = build_observer(method, module_type, bt, mode, permute=permute)
            maxs, mins = [], []
            xs = R.case_inputs(case)
            for x in xs:
                obs.update(x)
                maxs.append(obs.max_val.clone().numpy())
                mins.append(obs.min_val.clone().numpy())
            key = f"obs:{method}:{case}"
            if method == "omse":
                idx, cands, _, gap = R.omse_pick_f64(xs[-1], obs.max_val, obs.min_val, bt.lower_bound, bt.upper_bound)
                scale, zp = obs.get_quantization_params(xs[-1])
                # the reference's f32 .mean() pick must be the exact-sum pick on every fixture input
                assert float(scale) == float(cands[idx][2]) and float(zp) == float(cands[idx][3]), (case, idx)
                assert float(obs.max_val) == float(cands[idx][0]), (case, idx)
                out[key + ":idx"] = np.int64(idx)
                out[key + ":gap"] = np.float64(gap)
                out[key + ":best_max"] = obs.max_val.numpy()
                out[key + ":best_min"] = obs.min_val.numpy()
                print(f"{key}: candidate {idx}, float64 gap to runner-up {gap:.3e}")
            else:
                scale, zp = obs.get_quantization_params()
            out[key + ":max"] = np.stack(maxs)
            out[key + ":min"] = np.stack(mins)
            out[key + ":scale"] = scale.numpy()
            out[key + ":zp"] = zp.numpy()


def module_level(out: dict, meta: dict):
    from fq_vit.models.sam.image_encoder import ImageEncoderViT as FQEnc
    from fq_vit.models.ptq.layers import QIntLayerNorm
    from fq_vit.models.ptq import QAct, QConv2d, QLinear, QIntSoftmax
    from fq_vit.config import Config
    from models import BIT_TYPE_DICT
    img_size = 256
    g = np.load(HERE / "fq_vitb_img256.npz", allow_pickle=False)
    gmeta = json.loads(str(g["meta"]))
    names = [str(n) for n in g["act_scale_names"]]
    cfg = synth.encoder_config("vit_b", img_size=img_size)
    state = {k: v.astype(np.float16).astype(np.float32)
             for k, v in synth.make_encoder_state(cfg, seed=gmeta["seed"]).items()}
    sd = {k: torch.from_numpy(v) for k, v in state.items()}
    imgs = [synth.make_images(1, img_size, seed=s) for s in R.MODULE_CALIB_SEEDS]
    test_img = synth.make_images(1, img_size, seed=R.MODULE_TEST_SEED)
    for method in ("ema", "percentile", "omse"):
        cfgq = Config(False, False, method)
        cfgq.BIT_TYPE_A = BIT_TYPE_DICT["int8"]
        enc = FQEnc(depth=12, embed_dim=768, img_size=img_size, mlp_ratio=4,
                    norm_layer=partial(QIntLayerNorm, eps=1e-6), num_heads=12, patch_size=16, qkv_bias=True,
                    use_rel_pos=True, global_attn_indexes=[2, 5, 8, 11], window_size=14, out_chans=256, quant=False,
                    calibrate=False, cfg=cfgq)
        missing, unexpected = enc.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        enc.eval()
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
            qa = {n: m for n, m in enc.named_modules() if isinstance(m, QAct)}
            assert list(qa) == names
            out[f"mod:{method}:scales"] = np.array([float(qa[n].quantizer.scale.reshape(-1)[0]) for n in names],
                                                   np.float32)
            zps = np.array([float(qa[n].quantizer.zero_point.reshape(-1)[0]) for n in names], np.float32)
            if method == "omse":
                y = enc(torch.from_numpy(test_img)).numpy()
                s_out = float(out["mod:omse:scales"][names.index("qacts.3")])
                codes = np.round(y / s_out)
                assert np.abs(codes * s_out - y).max() < 1e-5 * max(1.0, np.abs(y).max())
                assert np.abs(codes).max() < 2 ** 15
                out["mod:omse:zps"] = zps
                out["mod:omse:codes"] = codes.astype(np.int16)
            else:
                assert not zps.any()
        print(f"module {method}: {time.time() - t0:.1f}s")
    meta.update(img_size=img_size, seed=gmeta["seed"], calib_seeds=list(R.MODULE_CALIB_SEEDS),
                test_seed=R.MODULE_TEST_SEED)


def main():
    torch.manual_seed(0)
    out: dict = {}
    meta = dict(torch=torch.__version__, numpy=np.__version__)
    observer_level(out)
    module_level(out, meta)
    np.savez_compressed(HERE / "fq_observers.npz", meta=json.dumps(meta), **out)
    print("wrote", HERE / "fq_observers.npz", (HERE / "fq_observers.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
