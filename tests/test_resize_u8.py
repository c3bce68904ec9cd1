"""``ops.resize_u8`` (``samq_resize_u8``) against Pillow itself, ``np.array(Image.fromarray(a).resize((w, h),
Image.BILINEAR))``, with ``torch.equal``: the op, a window with and without the channel flip, the float variant
against ``Sam.preprocess``, ``SamPredictor.set_image`` through it, and the C entry's argument checks."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from samq.sam_decoder import ResizeLongestSide

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def pil(a, hw):
    return torch.from_numpy(np.array(Image.fromarray(np.ascontiguousarray(a)).resize((hw[1], hw[0]), Image.BILINEAR)))


def image(shape, seed, binary=False):
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, shape + (3,), dtype=np.uint8)
    return (a >> 7) * np.uint8(255) if binary else a     # {0, 255}: reaches the clamp and the half-way rounding


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("H,W,L", [(37, 53, 64), (150, 225, 64), (191, 166, 64), (65, 3, 64), (3, 65, 64), (64, 48, 64),
                                   (1, 1, 64), (1000, 999, 1024), (1500, 2250, 1024)])
def test_op_equals_pil(cuda, H, W, L, binary):
    from samq import ops
    a = image((H, W), H * W + L, binary)
    hw = ResizeLongestSide.get_preprocess_shape(H, W, L)
    out = ops.resize_u8(torch.from_numpy(a).to(cuda), hw)
    assert out.shape == (3,) + hw and out.dtype == torch.uint8
    assert torch.equal(out.cpu(), pil(a, hw).permute(2, 0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_window_and_flip(cuda, flip):
    from samq import ops
    a = image((300, 400), 5)
    x0, y0, x1, y1 = box = (57, 31, 313, 222)
    hw = ResizeLongestSide.get_preprocess_shape(y1 - y0, x1 - x0, 64)
    crop = a[y0:y1, x0:x1, ::-1] if flip else a[y0:y1, x0:x1]
    assert torch.equal(ops.resize_u8(torch.from_numpy(a).to(cuda), hw, box=box, flip=flip).cpu(),
                       pil(crop, hw).permute(2, 0, 1))


@pytest.mark.gpu
def test_float_variant_is_sam_preprocess(cuda):
    from samq import ops
    a = image((150, 225), 6)
    hw = ResizeLongestSide.get_preprocess_shape(150, 225, 64)
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    x = (pil(a, hw).permute(2, 0, 1).float() - mean) / std
    ref = F.pad(x, (0, 64 - hw[1], 0, 64 - hw[0]), value=0)
    out = ops.resize_u8(torch.from_numpy(a).to(cuda), hw, norm=(mean.to(cuda), std.to(cuda)), pad_to=64)
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("encoder", ["gptq", "fq_vit"])
def test_predictor_features_equal_host_resize(cuda, encoder):
    """``set_image(np_image)`` leaves the features of ``set_torch_image`` on the PIL-resized, uploaded image: through
    the uint8 patch-embedding entry of a GPTQ encoder and through the float variant for an fq_vit one."""
    import samq
    if encoder == "gptq":
        from _encoder_helpers import oracle_vith, product_encoder
        from samq.build_sam import Sam
        cfg, st, names, q = oracle_vith(2, seed=7, name="vit_b", img_size=256, global_idx=(1,))
        sam = Sam(product_encoder(cfg, st, names, q, -1, cuda)).to(cuda).eval()
    else:
        from samq import fq_sam
        torch.manual_seed(3)
        sam = fq_sam.build_fq_sam("vit_b", img_size=256, depth=1).to(cuda).eval()
    pred = samq.SamPredictor(sam)
    a = image((200, 160), 7)
    pred.set_image(a)
    feat, sizes = pred.get_image_embedding().clone(), (pred.original_size, pred.input_size)
    host = pil(a, ResizeLongestSide.get_preprocess_shape(200, 160, 256)).to(cuda).permute(2, 0, 1).contiguous()[None]
    pred.set_torch_image(host, (200, 160))
    assert sizes == (pred.original_size, pred.input_size) == ((200, 160), (256, 205))
    assert torch.equal(feat, pred.get_image_embedding())


def test_arguments_rejected_before_any_device_call():
    from samq import _lib
    lib, p = _lib.load(), ctypes.c_void_p(16)

    def call(img, H, W, box, out_hw):
        return lib.samq_resize_u8(img, H, W, *box, *out_hw, 0, p, 0, None, None, 0, None)

    assert call(p, 1025, 64, (0, 0, 64, 1025), (64, 4)) == _lib.SAMQ_ERR_UNSUPPORTED      # fs = 1025 / 64 > 16
    assert call(p, 64, 64, (0, 0, 65, 64), (32, 32)) == _lib.SAMQ_ERR_INVALID             # window outside the image
    assert call(p, 2, 1000, (0, 0, 1000, 2), (0, 64)) == _lib.SAMQ_ERR_INVALID            # get_preprocess_shape(2, 1000, 64)
    assert ResizeLongestSide.get_preprocess_shape(2, 1000, 64) == (0, 64)
    assert call(None, 0, 0, (0, 0, 0, 0), (0, 64)) == _lib.SAMQ_OK                        # null image, zero output area
