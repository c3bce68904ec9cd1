"""Writes tests/golden/fq_ptf.npz from the reference's ``PtfObserver`` and SAM image encoder.

Run where the reference package is importable (its root and its ``fq_vit`` directory on ``sys.path``):

    python tests/golden/make_golden_ptf.py <reference root>

The fixture holds data only: for every observer case of ``tests/_ptf_ref.py`` and both activation bit
types the running min / max after each of the three updates, the final per-channel scale, the zero
point and the picks; for the model of ``_ptf_ref.MODEL`` (vit_b, depth 2, img 256, the default ``Config()``,
seeded weights, three calibration images) every activation scale and zero point, the quant-mode output
codes on the test image and the names of the QActs that carry a ``PtfObserver``; the smallest relative gap
between a channel's best and second-best float64 score.

The generator asserts, for every channel of every case and of every PTF QAct of the model, that the reference's f32-mean pick equals the
float64-sum pick and that this gap exceeds 1e-6 (``_ptf_ref.MIN_GAP``): the HIP observer, which ranks
float64 sums, then makes the reference's picks.  A seed that violates this is replaced, not the bound.
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import _ptf_ref as P  # noqa: E402


def main(ref_root: str) -> None:
    from functools import partial
    sys.path.insert(0, str(HERE.parent.parent))
    sys.path.insert(0, ref_root)
    sys.path.insert(0, str(Path(ref_root) / "fq_vit"))
    from fq_vit.config import Config
    from fq_vit.models.ptq import QAct, QConv2d, QIntSoftmax, QLinear
    from fq_vit.models.ptq.bit_type import BIT_TYPE_DICT
    from fq_vit.models.ptq.layers import QIntLayerNorm
    from fq_vit.models.ptq.observer.ptf import PtfObserver
    from fq_vit.models.sam.image_encoder import ImageEncoderViT
    from oracle import synth

    def encoder(cfg, img_size):
        return ImageEncoderViT(depth=P.MODEL["depth"], embed_dim=768, img_size=img_size, mlp_ratio=4,
                               norm_layer=partial(QIntLayerNorm, eps=1e-6), num_heads=12, patch_size=16, qkv_bias=True,
                               use_rel_pos=True, global_attn_indexes=list(P.MODEL["global_attn_indexes"]),
                               window_size=14, out_chans=256, quant=False, calibrate=False, cfg=cfg)

    def ptf_names(enc):
        return [n for n, m in enc.named_modules() if isinstance(m, QAct) and isinstance(m.quantizer.observer, PtfObserver)]

    out, min_gap = {}, np.inf
    for case, (shape, permute, _) in P.OBSERVER_CASES.items():
        xs = P.observer_inputs(case)
        for bt in P.BIT_TYPES:
            obs = PtfObserver("activation", BIT_TYPE_DICT[bt], "channel_wise", permute=permute)
            for i, x in enumerate(xs):
                obs.update(x)
                out[f"{case}:{bt}:max{i}"] = obs.max_val.numpy().copy()
                out[f"{case}:{bt}:min{i}"] = obs.min_val.numpy().copy()
            scale, zp = obs.get_quantization_params(xs[-1])
            assert scale.dim() == 1 and zp.dim() == 0
            qmin, qmax = P.BIT_TYPES[bt]
            # scale1 itself (a channel may not pick it): scale8 / 8 from the layer range
            scale8 = (obs.max_val.max() - obs.min_val.min()) / float(qmax - qmin)
            s1_ref = float(scale8 / 2 / 2 / 2)
            picks = torch.log2(scale / s1_ref).round().to(torch.int64).numpy()
            sums = P.scores64(P.channel_last(xs[-1], permute).numpy(), s1_ref, float(zp), qmin, qmax)
            assert np.array_equal(sums.argmin(1), picks), (case, bt, "f32-mean pick != float64-sum pick")
            srt = np.sort(sums, axis=1)
            gap = float(((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min())
            assert gap > P.MIN_GAP, (case, bt, gap)
            min_gap = min(min_gap, gap)
            out[f"{case}:{bt}:scale"] = scale.numpy()
            out[f"{case}:{bt}:zp"] = np.float32(zp)
            out[f"{case}:{bt}:picks"] = picks.astype(np.int8)
            out[f"{case}:{bt}:scale1"] = np.float32(s1_ref)

    # the calibrated model: vit_b, depth 2, one global block, img 256, the default Config() (uint8, ptf, lis)
    img_size = P.MODEL["img_size"]
    enc = encoder(Config(), img_size)
    assert not ptf_names(encoder(Config(False, False, "minmax"), 64))
    missing, unexpected = enc.load_state_dict(P.model_state(synth), strict=False)
    assert not unexpected and all("quantizer" in k for k in missing)
    enc.eval()
    mods = [m for m in enc.modules() if type(m) in (QConv2d, QLinear, QAct, QIntSoftmax)]
    acts = [(n, m) for n, m in enc.named_modules() if isinstance(m, QAct)]
    caught = {}
    hooks = [m.register_forward_hook(lambda mod, inp, o, n=n: caught.__setitem__(n, inp[0].detach()))
             for n, m in acts if isinstance(m.quantizer.observer, PtfObserver)]
    with torch.no_grad():
        for m in mods:
            m.calibrate = True
        seeds = P.MODEL["calib_seeds"]
        for i, sd in enumerate(seeds):
            if i == len(seeds) - 1:
                for m in mods:
                    m.last_calibrate = True
            enc(torch.from_numpy(synth.make_images(1, img_size, seed=sd)))
        for h in hooks:
            h.remove()
        for m in mods:
            m.calibrate = False
            m.quant = True
        y = enc(torch.from_numpy(synth.make_images(1, img_size, seed=P.MODEL["test_seed"])))
    for n, m in acts:     # the float64-sum pick is the reference's on the model's own activations too
        q = m.quantizer
        out[f"model:scale:{n}"] = q.scale.numpy()
        out[f"model:zp:{n}"] = np.float32(q.zero_point)
        if n in caught:
            obs = q.observer
            s1 = float((obs.max_val.max() - obs.min_val.min()) / 255.0 / 2 / 2 / 2)
            sums = P.scores64(P.channel_last(caught[n], obs.permute).numpy(), s1, float(q.zero_point), 0, 255)
            assert np.array_equal(sums.argmin(1), torch.log2(q.scale / s1).round().to(torch.int64).numpy()), n
            srt = np.sort(sums, axis=1)
            gap = float(((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min())
            assert gap > P.MIN_GAP, (n, gap)
            min_gap = min(min_gap, gap)
    s3, z3 = float(acts[-1][1].quantizer.scale), float(acts[-1][1].quantizer.zero_point)
    assert acts[-1][0] == "qacts.3"
    codes = torch.round(y / s3 + z3)
    assert codes.min() >= 0 and codes.max() <= 255 and torch.equal((codes - z3) * s3, y)
    out["model:codes"] = codes.numpy().astype(np.uint8)
    out["act_names"] = np.array([n for n, _ in acts])
    out["ptf_names"] = np.array(ptf_names(enc))
    out["meta"] = np.array(json.dumps(dict(P.MODEL, min_gap=min_gap, config="Config()")))
    np.savez_compressed(HERE / "fq_ptf.npz", **out)
    print("wrote", HERE / "fq_ptf.npz", "min gap", min_gap, "ptf", out["ptf_names"].tolist())


if __name__ == "__main__":
    main(sys.argv[1])
