"""``ops.mask_rle`` (``samq_mask_rle_count`` / ``samq_mask_rle_write``) against the numpy definition: paste the
mask on a zero canvas, flatten in Fortran order, take the run lengths (``_amg_ref.rle_ref``).  Exact.

The kernel's band is 64 rows per wave, four bands per workgroup: (300, 130) has five bands (seams at 64, 128,
192, 256) in two workgroup rows; (67, 259) and (3, 1030) reach the second and the fifth 256-column tile with a
ragged last lane and unaligned rows."""
import numpy as np
import pytest
import torch

from _amg_ref import rle_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 7), (64, 64), (67, 259), (300, 130), (3, 1030)]
# name -> (x0, y0, H - h, W - w)
PLACES = {"none": None, "interior": (3, 5, 9, 7), "bottom_right": (5, 3, 3, 5), "full_height": (4, 0, 0, 6),
          "top_left": (0, 0, 4, 3)}
CASES = [(s, "none") for s in SHAPES] + [(s, p) for s in ((64, 64), (67, 259)) for p in list(PLACES)[1:]]


def make_masks(h, w):
    rng = np.random.Generator(np.random.PCG64(h * 1000 + w))
    yy, xx = np.mgrid[:h, :w]
    corners = np.zeros((h, w), dtype=bool)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    seam = np.zeros((h, w), dtype=bool)       # a column that ends set, the next one starts set
    seam[-1, w // 2 - (w > 1)] = seam[0, w // 2] = True
    blob = ((yy - h / 2) / (h / 3 + 1)) ** 2 + ((xx - 0.4 * w) / (w / 4 + 1)) ** 2 < 1
    return np.stack([rng.random((h, w)) < 0.5, np.zeros((h, w), dtype=bool), np.ones((h, w), dtype=bool), corners,
                     seam, blob])


@pytest.mark.parametrize("shape,place", CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_mask_rle(cuda, shape, place):
    from samq import ops
    h, w = shape
    masks = make_masks(h, w)
    x0, y0, dh, dw = PLACES[place] or (0, 0, 0, 0)
    H, W = h + dh, w + dw
    kw = {} if place == "none" else dict(crop_box=[x0, y0, x0 + w, y0 + h], orig_size=(H, W))
    dev = torch.from_numpy(masks).to(cuda)
    for sel, t in ((None, dev), ([4, 0, 5, 0, 2], dev.to(torch.uint8))):
        st = None if sel is None else torch.tensor(sel, device=cuda)
        offsets, counts = ops.mask_rle(t, st, **kw)
        assert offsets.dtype == torch.int64 and counts.dtype == torch.int32
        ref = [rle_ref(masks[i], x0, y0, H, W) for i in (sel or range(len(masks)))]
        assert np.array_equal(offsets.cpu().numpy(), np.cumsum([0] + [len(r) for r in ref]))
        assert np.array_equal(counts.cpu().numpy(), np.concatenate(ref))
        assert all(r.sum() == H * W for r in np.split(counts.cpu().numpy(), offsets.cpu().numpy()[1:-1]))


def test_mask_rle_empty_selection_and_guards(cuda):
    from samq import ops
    masks = torch.ones((2, 8, 12), dtype=torch.bool, device=cuda)
    offsets, counts = ops.mask_rle(masks, torch.empty(0, dtype=torch.int64, device=cuda))
    assert offsets.tolist() == [0] and counts.numel() == 0
    for bad in (dict(crop_box=[4, 0, 16, 8], orig_size=(8, 15)),        # x0 + w > W
                dict(crop_box=[0, 2, 12, 10], orig_size=(9, 12)),       # y0 + h > H
                dict(crop_box=[-1, 0, 11, 8], orig_size=(8, 12)),
                dict(crop_box=[0, 0, 12, 8], orig_size=(65536, 32768))):
        with pytest.raises(AssertionError):
            ops.mask_rle(masks, None, **bad)
    with pytest.raises(AssertionError):
        ops.mask_rle(masks[:, :, ::2])
