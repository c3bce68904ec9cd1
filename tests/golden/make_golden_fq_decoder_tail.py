"""Generate ``fq_decoder_tail.npz``: the tail of the reference's fq_vit W8A8 mask decoder.

The same model, seeds, calibration and two prompt shapes as ``make_golden_fq_decoder.py`` (the
reference's ``PromptEncoder`` / ``MaskDecoder`` inside its ``Sam`` at a 16 x 16 grid, the seeded
weights of ``tests/_fq_decoder_ref.decoder_state``, minmax calibration on three sets, quant mode on
the held-out embedding).  Stored per prompt shape, as int8 codes (data only):

* ``<shape>:upscaling.qacts.<i>`` (i = 0..4): the outputs of ``MaskDecoder.qacts[i]``, NCHW;
* ``<shape>:mlp.<j>.<qact>`` (j = 0..3 the hypernetwork MLPs, 4 the IoU head; qact one of
  ``qacts1.0``, ``qacts2.0``, ``qacts1.1``, ``qacts2.1``, ``qact3``): every MLP QAct's output;
* ``<shape>:hyper_in``: the stacked ``qact3`` codes of the four hypernetwork MLPs (each at its own scale).

The scales, ``qact1``, ``iou_pred`` and the transformer's ``queries`` / ``keys`` are in ``fq_decoder.npz``.

Run where a checkout of the reference is available, on the CPU:

    python tests/golden/make_golden_fq_decoder_tail.py --reference <path to the reference checkout>
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

OUT = HERE / "fq_decoder_tail.npz"
MLP_QACTS = ("qacts1.0", "qacts2.0", "qacts1.1", "qacts2.1", "qact3")


def mlp_module_name(j: int) -> str:
    return f"output_hypernetworks_mlps.{j}" if j < 4 else "iou_prediction_head"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SAMQ_REFERENCE"), required="SAMQ_REFERENCE" not in os.environ,
                    help="the reference checkout (or $SAMQ_REFERENCE)")
    ref = Path(ap.parse_args().reference)
    sys.path.insert(0, str(ref))
    sys.path.insert(0, str(ref / "fq_vit"))
    from fq_vit.config import Config
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
    sub = {k: v for k, v in sam.state_dict().items() if k.startswith(("prompt_encoder.", "mask_decoder."))}
    state = R.decoder_state({k: tuple(v.shape) for k, v in sub.items()})
    missing, unexpected = sam.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)

    named = dict(md.named_modules())
    watch = {f"upscaling.qacts.{i}": f"qacts.{i}" for i in range(5)}
    for j in range(5):
        for q in MLP_QACTS:
            watch[f"mlp.{j}.{q}"] = f"{mlp_module_name(j)}.{q}"

    def run(seed, shape, acts=None):
        emb = torch.from_numpy(R.image_embedding(seed))
        pt, lab, box = R.prompt_set(seed, shape)
        hooks = []
        if acts is not None:
            for key, name in watch.items():
                hooks.append(named[name].register_forward_hook(lambda m, i, o, key=key: acts.__setitem__(key, o)))
        with torch.no_grad():
            sparse, dense = pe(points=(torch.from_numpy(pt), torch.from_numpy(lab)),
                               boxes=None if box is None else torch.from_numpy(box), masks=None)
            out = md.predict_masks(image_embeddings=emb, image_pe=pe.get_dense_pe(),
                                   sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense)
        for h in hooks:
            h.remove()
        return out

    sam.model_open_calibrate()
    for i, seed in enumerate(R.CALIB_SEEDS):
        if i == len(R.CALIB_SEEDS) - 1:
            sam.model_open_last_calibrate()
        run(seed, "point_box")
    sam.model_close_calibrate()
    sam.model_quant()

    arrays = {}
    for shape in R.PROMPT_SHAPES:
        acts = {}
        run(R.TEST_SEED, shape, acts)
        for key, name in watch.items():
            s = float(named[name].quantizer.scale.reshape(-1)[0])
            v = acts[key].numpy()
            codes = np.round(v / s)
            assert np.abs(codes * s - v).max() < 1e-5 * max(1.0, np.abs(v).max()), key
            assert np.abs(codes).max() <= 128
            arrays[f"{shape}:{key}"] = codes.astype(np.int8)
        arrays[f"{shape}:hyper_in"] = np.stack([arrays[f"{shape}:mlp.{j}.qact3"] for j in range(4)], axis=1)
        print(shape, {k: arrays[f"{shape}:{k}"].shape for k in ("upscaling.qacts.0", "upscaling.qacts.4", "hyper_in")})
    np.savez_compressed(OUT, **arrays, meta=json.dumps(dict(grid=R.GRID, prompt_shapes=list(R.PROMPT_SHAPES),
                                                            test_seed=R.TEST_SEED, torch=torch.__version__)))
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
