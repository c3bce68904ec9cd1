"""``ops.mask_postprocess`` (``samq_mask_postprocess``) and ``SamPredictor.predict_torch_scored`` against the
float64 ``postprocess_masks`` on the CPU (``_mask_post_ref``).

Exact cases: logits that are multiples of 1/4 on dyadic scales make every weight, product and sum exact in
fp32 and float64, so masks and all seven statistics are compared with ``torch.equal``, ties at the thresholds
included.  General cases: a pixel is *undecided* for a threshold t when ``|ref64 - t| <= eps`` with
``eps = 2^-12 max|low|`` (an fp32 source coordinate below 2048 carries at most 2^-13 absolute error, times a
slope of at most ``max|low| / 2`` per padded-input pixel, over two stages; factor 2 margin; the value
arithmetic adds ~2^-20 max|low|).  Decided pixels must match; counts and boxes are bracketed by the decided
and the undecided sets; the fused reductions must equal what torch recomputes from the returned mask.
"""
import numpy as np
import pytest
import torch

from _mask_post_ref import boxes, count, ref_stats, ref_values

pytestmark = pytest.mark.gpu

EXACT = [((64, 64), (64, 64)), ((128, 128), (64, 64)), ((32, 32), (64, 64)), ((32, 16), (64, 32)),
         ((128, 64), (64, 32)), ((16, 32), (32, 64))]


@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("orig,inp", EXACT)
def test_exact_dyadic(cuda, orig, inp, n):
    from samq import ops
    g = torch.Generator().manual_seed(1000 * n + 10 * orig[0] + orig[1])
    low = torch.randint(-16, 17, (n, 16, 16), generator=g).float() / 4
    v = ref_values(low, 64, inp, orig)
    assert (v == 0).any() and (v.abs() == 1).any()          # ties at all three thresholds occur
    mask, st = ops.mask_postprocess(low.to(cuda), 64, inp, orig)
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), v > 0)
    assert torch.equal(st.cpu(), ref_stats(v, 0.0, 1.0))


def test_exact_empty_full_and_blob(cuda):
    from samq import ops
    low = torch.full((5, 16, 16), -4.0)
    low[2:4] = 4.0
    low[4, 9, 3] = 4.0
    v = ref_values(low, 64, (64, 32), (128, 64))
    mask, st = ops.mask_postprocess(low.to(cuda), 64, (64, 32), (128, 64))
    st = st.cpu()
    assert torch.equal(mask.cpu(), v > 0) and torch.equal(st, ref_stats(v, 0.0, 1.0))
    assert not st[:2].any()                                   # empty: union 0 and box 0, 0, 0, 0
    assert st[2:4].tolist() == [[128 * 64] * 3 + [0, 0, 63, 127, 0]] * 2
    assert 0 < st[4, 2] < 128 * 64 and (st[4, 3:5] > 0).all()


GENERAL = [(16, (96, 64), 3, 0.0, 1.0), (16, (40, 30), 7, 0.0, 1.0), (64, (300, 417), 3, 0.0, 1.0),
           (64, (131, 77), 2, 0.0, 1.0), (256, (683, 1024), 2, 0.0, 1.0), (256, (1200, 1800), 1, 0.0, 1.0),
           (64, (300, 417), 3, 0.5, 0.25)]


@pytest.mark.parametrize("lh,orig,n,thr,off", GENERAL)
def test_general_against_float64(cuda, lh, orig, n, thr, off):
    from samq import ops
    from samq.sam_decoder import ResizeLongestSide
    g = torch.Generator().manual_seed(lh + orig[0] + orig[1] + n)
    low = 4 * torch.randn((n, lh, lh), generator=g)
    inp = ResizeLongestSide.get_preprocess_shape(orig[0], orig[1], 4 * lh)
    v = ref_values(low, 4 * lh, inp, orig)
    eps = 2.0 ** -12 * low.abs().max().item()
    und = {t: (v - t).abs() <= eps for t in (thr, thr + off, thr - off)}
    share = (und[thr] | und[thr + off] | und[thr - off]).double().mean().item()
    print(f"\n[mask_post] lh {lh} -> {orig} n {n}: eps {eps:.2e}, undecided share {share:.2e}")
    assert share <= 1e-2                                      # a condition on the inputs

    d_low = low.to(cuda)
    mask, st = ops.mask_postprocess(d_low, 4 * lh, inp, orig, thr, off)
    mask, st = mask.cpu(), st.cpu()
    dec = ~und[thr]
    assert torch.equal(mask[dec], (v > thr)[dec])
    for col, t in ((0, thr + off), (1, thr - off), (2, thr)):
        sure = count((v > t) & ~und[t])
        assert (sure <= st[:, col]).all() and (st[:, col] <= sure + count(und[t])).all()
    inner, outer = boxes((v > thr) & dec), boxes((v > thr) | und[thr])
    assert (st[:, 3:5] <= inner[:, :2]).all() and (st[:, 5:7] >= inner[:, 2:]).all()
    assert (st[:, 3:5] >= outer[:, :2]).all() and (st[:, 5:7] <= outer[:, 2:]).all()
    # the fused reductions against the kernel's own mask
    assert torch.equal(st[:, 2], count(mask)) and torch.equal(st[:, 3:7], boxes(mask)) and not st[:, 7].any()
    for col, t in ((0, thr + off), (1, thr - off)):
        assert torch.equal(st[:, col], count(ops.mask_postprocess(d_low, 4 * lh, inp, orig, t, 0.0)[0].cpu()))
    none, st2 = ops.mask_postprocess(d_low, 4 * lh, inp, orig, thr, off, masks=False)
    assert none is None and torch.equal(st2.cpu(), st)


def test_fp16_batched_input_and_guards(cuda):
    from samq import ops
    g = torch.Generator().manual_seed(5)
    low = (4 * torch.randn((2, 3, 16, 16), generator=g)).half().to(cuda)
    for inp, orig in (((64, 43), (96, 64)), ((64, 64), (64, 64))):
        m16, s16 = ops.mask_postprocess(low, 64, inp, orig)
        m32, s32 = ops.mask_postprocess(low.float(), 64, inp, orig)
        assert m16.shape == (2, 3) + orig and s16.shape == (2, 3, 8)
        assert torch.equal(m16, m32) and torch.equal(s16, s32)
    ok = dict(img_size=64, input_size=(64, 43), original_size=(96, 64), masks=False)
    for bad in (dict(img_size=60), dict(input_size=(0, 43)), dict(input_size=(64, 65)), dict(original_size=(96, 0)),
                dict(original_size=(65536, 32768))):
        with pytest.raises(AssertionError):
            ops.mask_postprocess(low, **{**ok, **bad})
    with pytest.raises(AssertionError):
        ops.mask_postprocess(low[..., :8].contiguous(), **ok)   # lh != lw


def test_predict_torch_scored(cuda):
    import samq
    from samq.build_sam import Sam, build_image_encoder
    torch.manual_seed(3)
    sam = Sam(build_image_encoder(768, 2, 12, [1], img_size=256)).eval()
    cpu = samq.SamPredictor(sam)
    cpu.features, cpu.is_image_set = torch.zeros((1, 256, 16, 16)), True
    with pytest.raises(NotImplementedError):
        cpu.predict_torch_scored(torch.zeros((2, 1, 2)), torch.ones((2, 1), dtype=torch.int))
    pred = samq.SamPredictor(sam.to(cuda))
    pred.set_image(np.random.Generator(np.random.PCG64(0)).integers(0, 256, (200, 160, 3), dtype=np.uint8))
    pts = torch.tensor([[[80.0, 100.0]], [[30.0, 150.0]]], device=cuda)
    lab = torch.ones((2, 1), dtype=torch.int, device=cuda)
    out = pred.predict_torch_scored(pts, lab, multimask_output=True)
    masks, iou, low = pred.predict_torch(pts, lab, multimask_output=True)
    assert out["masks"].shape == (2, 3, 200, 160) and out["masks"].dtype == torch.bool
    assert all(out[k].shape == (2, 3) for k in ("iou_predictions", "stability_score", "areas"))
    assert out["boxes"].shape == (2, 3, 4)
    low = out["low_res_logits"]      # a second decoder run repeats the first only up to torch's fp32 summation order
    _, st = samq.ops.mask_postprocess(low, 256, pred.input_size, pred.original_size, sam.mask_threshold, 1.0, False)
    torch.testing.assert_close(out["stability_score"], st[..., 0].float() / st[..., 1].float(), rtol=0, atol=0,
                               equal_nan=True)
    assert torch.equal(out["areas"], out["masks"].flatten(2).sum(2).int())
    assert torch.equal(out["boxes"].reshape(6, 4).cpu(), boxes(out["masks"].reshape(6, 200, 160).cpu()))
    v = ref_values(low.reshape(6, 64, 64), 256, pred.input_size, pred.original_size).reshape(2, 3, 200, 160)
    dec = (v - sam.mask_threshold).abs() > 2.0 ** -12 * low.abs().max().item()
    assert torch.equal(out["masks"].cpu()[dec], masks.cpu()[dec])
    assert pred.predict_torch_scored(pts, lab, return_masks=False)["masks"] is None
