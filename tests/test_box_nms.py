"""``ops.box_nms`` (``samq_box_nms``) against a float64 greedy loop with a stable rank (``_amg_ref.nms_ref``).

Why exact equality holds.  Corner coordinates are integers below 256 (family "int") or multiples of 1/8 below
128 (family "eighth"), so every area, intersection and union is exact in fp32: a product is below 2^22 with at
most 22 significant bits.  The true IoU is a rational p / q and for t in {1/2, 3/4}, p / q != t gives
|p / q - t| = |4 p - 4 t q| / (4 q) >= 1 / (4 q).  Integer family: q < 2^17, a gap above 2^-19, far more than
half an ulp of a quotient below 1 (2^-25).  Eighth family: scale by 64, q < 2^21 with coordinates below 128, a gap
above 2^-23, still four times half an ulp.  So the correctly rounded fp32 quotient lies on the same side of t as
the float64 one, and an IoU of exactly t is not above t in either.  Zero-area pairs give 0 / 0 = NaN: kept.

Sizes: one tile, the tile edge (63, 64, 65), three tiles, and 1000 / 4200 boxes (16 / 66 column words: the
sweep's second wave of column-word threads; its capacity, 32768 boxes, is the entry's own limit)."""
import numpy as np
import pytest
import torch

from _amg_ref import nms_ref

pytestmark = pytest.mark.gpu

CRAFTED = np.array([[0, 0, 2, 2], [0, 0, 2, 1],            # IoU exactly 1/2
                    [10, 10, 14, 14], [10, 10, 14, 13],    # IoU exactly 3/4
                    [20, 20, 20, 25], [20, 20, 20, 25],    # zero area: NaN, both kept
                    [30, 30, 40, 40], [30, 30, 40, 40]],   # identical boxes, identical scores: the lower index wins
                   dtype=np.float64)


def make_boxes(n, family, rng):
    unit, top = (1.0, 256) if family == "int" else (0.125, 128)
    centres = rng.uniform(0.2 * top, 0.8 * top, (5, 2))
    c = centres[rng.integers(0, 5, n)] + rng.normal(0, 0.04 * top, (n, 2))
    half = rng.uniform(0.02 * top, 0.15 * top, (n, 2))
    b = np.concatenate([c - half, c + half], axis=1)
    b = np.clip(np.round(b / unit) * unit, 0, top - unit)
    if n >= len(CRAFTED):
        b[:len(CRAFTED)] = CRAFTED
    return b


@pytest.mark.parametrize("thr", [0.5, 0.75])
@pytest.mark.parametrize("family", ["int", "eighth"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 1000, 4200])
def test_box_nms(cuda, n, family, thr):
    from samq import ops
    rng = np.random.Generator(np.random.PCG64(n))
    boxes = make_boxes(n, family, rng)
    for scores in (np.round(rng.random(n) * 16) / 16, np.ones(n)):      # many ties; all equal: index order
        keep = ops.box_nms(torch.from_numpy(boxes).float().to(cuda), torch.from_numpy(scores).float().to(cuda), thr)
        assert keep.dtype == torch.int64
        ref = nms_ref(boxes, scores, thr)
        assert np.array_equal(keep.cpu().numpy(), ref)
        rank = np.argsort(np.argsort(-scores, kind="stable"), kind="stable")
        assert np.all(np.diff(rank[ref]) > 0)
        if n >= len(CRAFTED) and scores.min() == 1:
            assert {0, 1, 4, 5, 6}.issubset(ref.tolist()) and 7 not in ref
            assert (3 in ref) == (thr == 0.75)      # 3/4 is above 0.5 only


def test_box_nms_empty_and_limit(cuda):
    from samq import ops
    keep = ops.box_nms(torch.zeros((0, 4), device=cuda), torch.zeros(0, device=cuda), 0.5)
    assert keep.dtype == torch.int64 and keep.numel() == 0
    with pytest.raises(NotImplementedError):
        ops.box_nms(torch.zeros((32769, 4), device=cuda), torch.zeros(32769, device=cuda), 0.5)
