"""The float mask decoder's fused tail (``MaskDecoder.use_fused_tail``: ``samq_decoder_mlps_f32`` +
``samq_upscale_masks_f32``) against the module itself in float64 on the CPU.

Error measure ``e(x) = max|x - ref64| / max|ref64|`` per output; condition ``e(fused) <= 4 e(fp32 module on the
CPU) + 2^-22`` (a different fp32 summation order over K = 256, 64, 32; a dropped low plane or a single fp16
operand would sit near 2^-11).  The upscaling kernel's tile is 64 input pixels: 1 x 1 is one pixel, 3 x 5 a
partial tile (with B = 3 three prompts in one tile), 5 x 13 = 65 pixels crosses a tile (with B = 3 the prompt
boundaries fall inside tiles), 16 x 16 is four whole tiles.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _decoder_tail_f32_ref as R


CASES = [(h, w, b, nt, 1.0) for h, w in ((1, 1), (3, 5), (5, 13), (16, 16)) for b in (1, 3) for nt in (7, 9)]
CASES += [(5, 13, 3, 9, 2.0 ** -10), (5, 13, 3, 9, 2.0 ** 10)]   # the scale of keys, at one shape


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,b,n_tokens,scale", CASES)
def test_fused_tail_against_float64_module(cuda, h, w, b, n_tokens, scale):
    from samq import ops
    dec, masks64, iou64, hyper64 = R.tail_case(100 * h + w, b, n_tokens, h, w, scale)
    m32, i32 = R.run(dec, b, n_tokens, h, w)                 # the fp32 module tail on the CPU
    with torch.no_grad():
        h32 = torch.stack([m(dec.transformer.hs[:, 1 + i]) for i, m in enumerate(dec.output_hypernetworks_mlps)], 1)
    gpu = copy.deepcopy(dec).to(cuda)
    gpu.use_fused_tail = True
    masks, iou = R.run(gpu, b, n_tokens, h, w)
    assert masks.shape == (b, 4, 4 * h, 4 * w) and iou.shape == (b, 4)
    t = gpu._tail
    hyper, _ = ops.decoder_mlps_f32(gpu.transformer.hs, t["w1"], t["w2"], t["w3"], t["b1"], t["b2"], t["b3"])
    R.check("masks", masks, m32, masks64)
    R.check("iou", iou, i32, iou64)
    R.check("hyper", hyper, h32, hyper64)
    again = R.run(gpu, b, n_tokens, h, w)
    assert torch.equal(again[0], masks) and torch.equal(again[1], iou)


@pytest.mark.gpu
def test_predict_torch_with_fused_tail(cuda):
    import samq
    from samq.build_sam import Sam, build_image_encoder
    torch.manual_seed(3)
    sam = Sam(build_image_encoder(768, 2, 12, [1], img_size=256)).eval().to(cuda)
    pred = samq.SamPredictor(sam)
    pred.set_image(np.random.Generator(np.random.PCG64(0)).integers(0, 256, (200, 160, 3), dtype=np.uint8))
    pts = torch.tensor([[[80.0, 100.0]], [[30.0, 150.0]]], device=cuda)
    lab = torch.ones((2, 1), dtype=torch.int, device=cuda)
    _, iou_off, low_off = pred.predict_torch(pts, lab)
    sam.mask_decoder.use_fused_tail = True
    _, iou, low = pred.predict_torch(pts, lab)
    _, iou2, low2 = pred.predict_torch(pts, lab)
    assert low.shape == (2, 3, 64, 64) and torch.equal(low2, low) and torch.equal(iou2, iou)
    # the whole prompt encoder + decoder in float64 on the CPU, on the same features
    s64 = copy.deepcopy(sam).cpu().double()
    with torch.no_grad():
        sparse, dense = s64.prompt_encoder(points=(pts.cpu().double(), lab.cpu()), boxes=None, masks=None)
        low64, iou64 = s64.mask_decoder(pred.features.cpu().double(), s64.prompt_encoder.get_dense_pe(), sparse, dense,
                                        True)
    R.check("predict_torch low_res_logits", low, low_off, low64)
    R.check("predict_torch iou_predictions", iou, iou_off, iou64)


@pytest.mark.gpu
def test_fused_tail_refusal_and_refresh(cuda):
    from samq.sam_decoder import MaskDecoder, TwoWayTransformer
    odd = MaskDecoder(transformer_dim=256, iou_head_depth=2,
                      transformer=TwoWayTransformer(depth=1, embedding_dim=256, mlp_dim=64, num_heads=8)).to(cuda)
    assert R.run(odd, 1, 7, 2, 2)[0].shape == (1, 4, 8, 8)
    odd.use_fused_tail = True
    with pytest.raises(NotImplementedError, match="iou_prediction_head.*depth 2"):
        R.run(odd, 1, 7, 2, 2)
    # new weights (a state dict, an in-place update) reach the packed snapshot
    a, b = (R.tail_case(s, 1, 7, 3, 5)[0].to(cuda) for s in (1, 2))
    a.use_fused_tail = b.use_fused_tail = True
    first, want = R.run(a, 1, 7, 3, 5), R.run(b, 1, 7, 3, 5)
    a.load_state_dict(b.state_dict())
    got = R.run(a, 1, 7, 3, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], first[0])
    with torch.no_grad():
        a.output_upscaling[3].bias.add_(1.0)
    assert not torch.equal(R.run(a, 1, 7, 3, 5)[0], got[0])


def test_cpu_model_with_the_flag_takes_the_module_path():
    dec = R.tail_case(5, 2, 7, 3, 5)[0]
    want = R.run(dec, 2, 7, 3, 5)
    dec.use_fused_tail = True
    got = R.run(dec, 2, 7, 3, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_c_abi_argument_checks():
    """Every case returns before a launch, so this runs without a GPU."""
    from samq import _lib
    lib = _lib.load()
    p, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)

    def mlps(B=1, nt=7, C=256, hs=p, out=p):
        return lib.samq_decoder_mlps_f32(hs, p, p, p, p, p, p, out, p, B, nt, C, None), lib.samq_last_error().decode()

    def masks(B=1, h=4, w=4, C=256, keys=p, out=p):
        return (lib.samq_upscale_masks_f32(keys, p, p, p, p, p, p, p, out, B, h, w, C, 1e-6, None),
                lib.samq_last_error().decode())

    for call, name, arg in ((mlps, "decoder_mlps_f32", "hs"), (masks, "upscale_masks_f32", "keys")):
        assert call(B=0, **{arg: None, "out": None})[0] == _lib.SAMQ_OK
        assert call(B=-1) == (_lib.SAMQ_ERR_INVALID, f"{name}: negative size")
        assert call(**{arg: None}) == (_lib.SAMQ_ERR_INVALID, f"{name}: null pointer")
        assert call(out=None) == (_lib.SAMQ_ERR_INVALID, f"{name}: null pointer")
        assert call(C=128) == (_lib.SAMQ_ERR_UNSUPPORTED, f"{name}: the transformer width must be 256")
        assert call(**{arg: odd}) == (_lib.SAMQ_ERR_INVALID, f"{name}: pointers must be 16-byte aligned")
    assert mlps(nt=4)[0] == _lib.SAMQ_ERR_INVALID and masks(h=0, keys=None)[0] == _lib.SAMQ_OK
