"""Generate ``fq_decoder.npz``: the reference's fq_vit W8A8 prompt encoder + mask decoder.

The reference's ``PromptEncoder`` / ``MaskDecoder`` / ``TwoWayTransformer`` inside its ``Sam`` (a
stub in place of the image encoder) at a 16 x 16 embedding grid (input 256), with the seeded
fp16-rounded weights of ``tests/_fq_decoder_ref.decoder_state``: minmax calibration through the
five ``Sam`` switches on three (image embedding, two points + box) sets, then quant mode on a
held-out embedding with both prompt shapes (one point: 5 + 2 tokens; two points + box: 5 + 4).

Stored (data only): the sorted state-dict keys before and after calibration, every activation and
weight scale, the int8 codes + scale of the taps (``qact_embed1``, ``qact_embed2``,
``pos_src_qact``, each block's ``queries`` / ``keys``, the transformer's final ``queries`` -- its
``keys`` are the last block's -- and the low-res masks ``qact1``), ``iou_pred`` and, for the two
points + box set, the codes of every transformer QAct on the token rows (``act:<module name>``).

Run where a checkout of the reference is available, on the CPU:

    python tests/golden/make_golden_fq_decoder.py --reference <path to the reference checkout>
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import _fq_decoder_ref as R  # noqa: E402

OUT = HERE / "fq_decoder.npz"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SAMQ_REFERENCE"), required="SAMQ_REFERENCE" not in os.environ,
                    help="the reference checkout (or $SAMQ_REFERENCE)")
    ref = Path(ap.parse_args().reference)
    sys.path.insert(0, str(ref))
    sys.path.insert(0, str(ref / "fq_vit"))
    from fq_vit.config import Config
    from fq_vit.models.ptq import QAct, QConv2d, QLinear
    from fq_vit.models.sam.mask_decoder import MaskDecoder
    from fq_vit.models.sam.prompt_encoder import PromptEncoder
    from fq_vit.models.sam.sam import Sam
    from fq_vit.models.sam.transformer import TwoWayTransformer
    from models import BIT_TYPE_DICT

    torch.manual_seed(0)
    cfg = Config(False, False, "minmax")
    cfg.BIT_TYPE_A = BIT_TYPE_DICT["int8"]
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(R.GRID, R.GRID), input_image_size=(R.IMG, R.IMG),
                       mask_in_chans=16, quant=False, calibrate=False, cfg=cfg)
    md = MaskDecoder(num_multimask_outputs=3,
                     transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8, quant=False,
                                                   calibrate=False, cfg=cfg),
                     transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256, quant=False, calibrate=False,
                     cfg=cfg)
    enc = torch.nn.Identity()
    enc.img_size = R.IMG
    sam = Sam(image_encoder=enc, prompt_encoder=pe, mask_decoder=md, cfg=cfg)
    sam.eval()

    def sub_state():
        return {k: v for k, v in sam.state_dict().items() if k.startswith(("prompt_encoder.", "mask_decoder."))}
    keys_built = sorted(sub_state())
    state = R.decoder_state({k: tuple(v.shape) for k, v in sub_state().items()})
    missing, unexpected = sam.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)

    def run(seed, shape, taps=None, acts=None):
        emb = torch.from_numpy(R.image_embedding(seed))
        pt, lab, box = R.prompt_set(seed, shape)
        hooks = []
        if acts is not None:
            for name, mod in md.named_modules():
                if isinstance(mod, QAct) and (name.startswith("transformer.") or name == "qact_embed1"):
                    hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: acts.__setitem__(name, o)))
        if taps is not None:
            def grab(name):
                return lambda m, i, o: taps.__setitem__(name, o)
            for name, mod in (("qact_embed1", md.qact_embed1), ("qact_embed2", md.qact_embed2),
                              ("pos_src_qact", md.pos_src_qact), ("qact1", md.qact1), ("transformer", md.transformer),
                              ("layers.0", md.transformer.layers[0]), ("layers.1", md.transformer.layers[1])):
                hooks.append(mod.register_forward_hook(grab(name)))
        with torch.no_grad():
            sparse, dense = pe(points=(torch.from_numpy(pt), torch.from_numpy(lab)),
                               boxes=None if box is None else torch.from_numpy(box), masks=None)
            masks, iou = md.predict_masks(image_embeddings=emb, image_pe=pe.get_dense_pe(),
                                          sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense)
        for h in hooks:
            h.remove()
        return masks, iou

    sam.model_open_calibrate()
    for i, seed in enumerate(R.CALIB_SEEDS):
        if i == len(R.CALIB_SEEDS) - 1:
            sam.model_open_last_calibrate()
        run(seed, "point_box")
    sam.model_close_calibrate()
    sam.model_quant()
    keys_cal = sorted(sub_state())

    named = {n: m for n, m in sam.named_modules() if n.startswith(("prompt_encoder.", "mask_decoder."))}
    # prompt-encoder mask-branch QActs never ran (no mask input): they have no scale
    ascales = {n: float(m.quantizer.scale.reshape(-1)[0]) for n, m in named.items()
               if isinstance(m, QAct) and m.quantizer.scale is not None}
    wscales = {n: m.quantizer.scale.reshape(-1).numpy() for n, m in named.items()
               if isinstance(m, (QLinear, QConv2d)) and m.quantizer.scale is not None}
    T = "mask_decoder.transformer."
    tap_scale = {"qact_embed1": "mask_decoder.qact_embed1", "qact_embed2": "mask_decoder.qact_embed2",
                 "pos_src_qact": "mask_decoder.pos_src_qact", "qact1": "mask_decoder.qact1",
                 "layers.0.queries": T + "layers.0.qact10", "layers.0.keys": T + "layers.0.qact14",
                 "layers.1.queries": T + "layers.1.qact10", "layers.1.keys": T + "layers.1.qact14",
                 "queries": T + "qact4"}
    arrays = {}
    for shape in R.PROMPT_SHAPES:
        taps, acts = {}, {}
        masks, iou = run(R.TEST_SEED, shape, taps, acts if shape == R.STAGE_SHAPE else None)
        # every transformer QAct on the token rows (fewer than STAGE_ROWS_MAX codes): the inputs and
        # references of the stage-local GPU test, where one code is more than the 1e-4 bound allows
        # and the module graph's own fp32 matmul rounding differs from machine to machine
        for name, v in acts.items():
            if v.numel() <= R.STAGE_ROWS_MAX:
                s = ascales["mask_decoder." + name]
                codes = np.round(v.numpy() / s)
                assert np.abs(codes * s - v.numpy()).max() < 1e-5 * max(1.0, np.abs(v.numpy()).max()), name
                arrays["act:" + name] = codes.astype(np.int8)
        vals = {k: taps[k] for k in ("qact_embed1", "qact_embed2", "pos_src_qact", "qact1")}
        for i in (0, 1):
            vals[f"layers.{i}.queries"], vals[f"layers.{i}.keys"] = taps[f"layers.{i}"]
        vals["queries"], final_keys = taps["transformer"]
        assert torch.equal(final_keys, vals["layers.1.keys"])
        assert torch.equal(masks, vals["qact1"])
        for name, v in vals.items():
            s = ascales[tap_scale[name]]
            codes = np.round(v.numpy() / s)
            assert np.abs(codes * s - v.numpy()).max() < 1e-5 * max(1.0, np.abs(v.numpy()).max()), name
            assert np.abs(codes).max() <= 128
            if name in ("qact_embed2", "pos_src_qact"):   # the same for both prompt shapes
                if "tap:" + name in arrays:
                    assert np.array_equal(arrays["tap:" + name], codes.astype(np.int8))
                arrays["tap:" + name] = codes.astype(np.int8)
            else:
                arrays[f"tap:{shape}:{name}"] = codes.astype(np.int8)
        arrays[f"iou_pred:{shape}"] = iou.numpy().astype(np.float32)
        print(shape, "tokens", vals["qact_embed1"].shape[1], "iou_pred", iou.numpy().round(4),
              "mask>0", float((masks > 0).float().mean()))
    np.savez_compressed(OUT, keys_built=np.array(keys_built), keys_calibrated=np.array(keys_cal),
                        act_scale_names=np.array(list(ascales)), act_scales=np.array(list(ascales.values()), np.float32),
                        tap_scale_names=np.array(list(tap_scale)), tap_scale_of=np.array(list(tap_scale.values())),
                        **{"wscale:" + k: v for k, v in wscales.items()}, **arrays,
                        meta=json.dumps(dict(grid=R.GRID, img=R.IMG, state_seed=R.STATE_SEED,
                                             calib_seeds=list(R.CALIB_SEEDS), test_seed=R.TEST_SEED,
                                             calib_prompt="point_box", prompt_shapes=list(R.PROMPT_SHAPES),
                                             torch=torch.__version__)))
    print("wrote", OUT, OUT.stat().st_size, "bytes,", len(ascales), "QAct scales,", len(wscales), "weight scales")


if __name__ == "__main__":
    main()
