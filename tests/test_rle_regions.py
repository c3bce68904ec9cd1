"""``ops.rle_remove_small_regions`` (``samq_rle_regions_*``) and ``SamAutomaticMaskGenerator.postprocess_small_regions``
against the numpy / flood-fill reference of ``_regions_ref``.  Every comparison is exact integer equality."""
import ctypes

import numpy as np
import pytest
import torch

from _amg_ref import nms_ref
from _regions_ref import clean, csr, regions_ref
from test_automatic_mask_generator import sam  # noqa: F401  (the tiny model fixture)


def paint(H, W, *cells):
    m = np.zeros((H, W), dtype=bool)
    for y, x in cells:
        m[y, x] = True
    return m


H2, W2 = 9, 10
DIAG = paint(H2, W2, (1, 1), (1, 2), (2, 1), (3, 2), (3, 3), (4, 3))          # two L's of 3 touching at a corner
SERPENTINE = np.zeros((H2, W2), dtype=bool)
SERPENTINE[::2] = True
SERPENTINE[1::4, -1] = SERPENTINE[3::4, 0] = True
FULL = np.ones((H2, W2), dtype=bool)
# name -> (mask, unchanged at min_area 4, area at min_area 4): the one thing each is there for
CRAFTED = {
    "diagonal_islands": (DIAG, True, 6),                                     # one component of 6, not two of 3
    "diagonal_holes": (~DIAG, True, 84),
    "column_seam": (paint(H2, W2, (7, 4), (8, 4), (0, 5), (1, 5), (2, 5), (3, 5)), False, 4),   # one run, 2 + 4
    "border_hole": (FULL & ~paint(H2, W2, (0, 4), (0, 5)), False, 90),
    "small_outer_background": (FULL & ~paint(H2, W2, (0, 0), (0, 1), (1, 0)), False, 90),
    "unique_largest": (paint(H2, W2, (0, 0), (1, 0), (4, 2), (5, 2), (6, 2), (5, 3), (4, 6), (4, 7), (4, 8)), False, 4),
    "tie": (paint(H2, W2, (5, 1), (6, 1), (7, 1), (0, 6), (1, 6), (2, 6)), False, 3),   # column 1 wins
    "single_small": (paint(H2, W2, (4, 4), (4, 5), (5, 5)), False, 3),       # flagged, run lengths identical
    "empty": (~FULL, True, 0), "full": (FULL, True, 90), "serpentine": (SERPENTINE, True, 54),
}
LINE = [np.array(list(row)) == "#" for row in ("....###.###....", "#.#.#.#.#.#.#.#", "." * 15, "#" * 15, "#" + "." * 13 + "#")]
# canvas -> masks; in one column the islands of "....###.###...." meet through the filled hole of that column only
CANVASES = {"2d": [m for m, _, _ in CRAFTED.values()], "one_row": [r[None, :] for r in LINE],
            "one_column": [r[:, None] for r in LINE], "one_pixel": [FULL[:1, :1], ~FULL[:1, :1]]}


def check(cuda, masks, min_area):
    from samq import ops
    offsets, counts = (torch.from_numpy(v).to(cuda) for v in csr(masks))
    got = ops.rle_remove_small_regions(offsets, counts, masks[0].shape, min_area)
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32, torch.int32, torch.bool]
    ref, filled, dropped = regions_ref(masks, min_area)
    for name, g, r in zip(("offsets", "counts", "boxes", "areas", "unchanged"), got, ref):
        assert np.array_equal(g.cpu().numpy(), r), name
    return ref, filled, dropped


@pytest.mark.gpu
@pytest.mark.parametrize("min_area", [1, 4, 10, 1000])
@pytest.mark.parametrize("canvas", list(CANVASES))
def test_crafted(cuda, canvas, min_area):
    ref, _, _ = check(cuda, CANVASES[canvas], min_area)
    offsets, counts = csr(CANVASES[canvas])
    if min_area == 1:       # nothing is below 1: the input comes back
        assert np.array_equal(ref[0], offsets) and np.array_equal(ref[1], counts) and ref[4].all()
    if canvas == "2d" and min_area == 4:
        assert [(bool(u), int(a)) for u, a in zip(ref[4], ref[3])] == [(u, a) for _, u, a in CRAFTED.values()]
        i = list(CRAFTED).index("single_small")
        assert np.array_equal(ref[1][ref[0][i]:ref[0][i + 1]], counts[offsets[i]:offsets[i + 1]])
    if canvas == "2d" and min_area == 10:      # all small: the 4 of "unique_largest" stays, column 1 of "tie"
        assert [ref[2][list(CRAFTED).index(k)].tolist() for k in ("unique_largest", "tie")] == [[2, 4, 3, 6], [1, 5, 1, 7]]
    if canvas in ("one_row", "one_column") and min_area == 4:      # holes first: 3 + 1 + 3 is one island of 7
        assert ref[3][0] == 7 and not ref[4][0]


def random_masks(kind, H, W, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind != "blob":
        return list(rng.random((n, H, W)) < kind)
    f = np.cumsum(np.cumsum(rng.standard_normal((n, H + 5, W + 5)), axis=1), axis=2)      # 5 x 5 box sums
    f = f[:, 5:, 5:] - f[:, :-5, 5:] - f[:, 5:, :-5] + f[:, :-5, :-5]
    return list(f > 2.0)


SIZES = [(5, 64), (64, 5), (33, 47), (130, 70)]
# (kind, canvas, masks per call, min_area, seed): the seeds are the first at which the reference fills a hole and
# drops an island in the noise cases (asserted below)
SEEDS = {(0.3, (130, 70)): 1, (0.7, (5, 64)): 157, (0.7, (33, 47)): 1, (0.7, (130, 70)): 1}
RANDOM = [(d, s, 3, (2, 5, 40)[(di + si) % 3], SEEDS.get((d, s), 0))
          for di, d in enumerate((0.3, 0.5, 0.7)) for si, s in enumerate(SIZES)]
RANDOM += [("blob", s, 3, (40, 5, 2, 40)[si], 0) for si, s in enumerate(SIZES)]
RANDOM += [(0.5, (5, 64), 70, 5, 0), (0.5, (64, 5), 1, 2, 0), (0.3, (33, 47), 1, 5, 0), (0.7, (5, 64), 70, 40, 3),
           ("blob", (33, 47), 70, 5, 0), ("blob", (130, 70), 1, 40, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,n,min_area,seed", RANDOM,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_random(cuda, kind, size, n, min_area, seed):
    _, filled, dropped = check(cuda, random_masks(kind, *size, n, seed), min_area)
    assert kind == "blob" or (filled >= 1 and dropped >= 1)


@pytest.mark.gpu
def test_both_memory_tiers(cuda):
    """Parents and areas live in LDS up to RGN_LDS_SEGS = 16384 segments (csrc/rle_regions.hip), in the workspace
    above: one mask on either side in one call, 256 x 256 noise, the smaller one in 120 columns only."""
    rng = np.random.Generator(np.random.PCG64(7))
    big = rng.random((256, 256)) < 0.5
    small = big & (np.arange(256) < 120)
    segments = [m.shape[1] + int((m[1:] != m[:-1]).sum()) for m in (big, small)]
    assert segments[0] > 2 * 16384 > 16384 >= segments[1] > 15000, segments
    _, filled, dropped = check(cuda, [big, small], 5)
    assert filled >= 1 and dropped >= 1


@pytest.mark.gpu
def test_generator_with_planted_masks(cuda, sam):
    """``generate`` with ``min_mask_region_area = 30`` set on the constructed generator, on planted masks
    (``test_crops_with_planted_masks``'s scheme): per prompt a disc of radius 5 with a pinhole, a clean disc of
    radius 10 and the same disc with a 2 x 2 speck 25 px to its right (too wide a box for the crop's NMS to pair
    the two; cleaned they are one disc and the untouched one has to stay).  Expected: the reference's steps in numpy."""
    import samq
    from samq.automatic_mask_generator import build_point_grid, generate_crop_boxes
    H, W = 200, 160
    crop_boxes = generate_crop_boxes((H, W), 1, 512 / 1500)[0]
    grids = [np.array([[.25, .25], [.75, .25], [.25, .75], [.75, .75]]), build_point_grid(3)]
    gen = samq.SamAutomaticMaskGenerator(sam.to(cuda), points_per_side=None, point_grids=grids, points_per_batch=5,
                                         crop_n_layers=1)
    yy, xx = np.mgrid[:H, :W]
    planted = []    # (crop box, canvas, full-image xyxy box)
    def box(m):
        ys, xs = np.nonzero(m)
        return [xs.min(), ys.min(), xs.max(), ys.max()]
    def plant(points, crop_size, crop_box, orig_size):
        x0, y0, x1, y1 = crop_box
        first = len(planted)
        for px, py in points:
            cx, cy = int(px + x0), int(py + y0)
            disc = lambda r: (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
            speck = (abs(xx - cx - 25.5) < 1) & (abs(yy - cy - 0.5) < 1)
            for canvas in (disc(5) & ~disc(0), disc(10), disc(10) | speck):
                canvas = canvas & (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
                planted.append((crop_box, canvas, box(canvas)))
        new = planted[first:]
        boxes = torch.tensor(np.array([p[2] for p in new]) - [x0, y0, x0, y0], dtype=torch.int32, device=cuda)
        iou = (0.9 + torch.arange(first, len(planted), device=cuda) / 1024).view(-1, 3)
        res = {"masks": torch.tensor(np.stack([p[1][y0:y1, x0:x1] for p in new]), device=cuda).unflatten(0, (-1, 3)),
               "iou_predictions": iou, "stability_score": torch.ones_like(iou), "boxes": boxes.view(-1, 3, 4)}
        return gen._select(res, points, crop_box, orig_size)
    gen._process_batch = plant
    cand = gen.candidates(np.zeros((H, W, 3), dtype=np.uint8))
    gen.candidates = lambda image: cand         # both runs on the same candidates: one pass of the encoder
    recs = {}
    for gen.min_mask_region_area in (30, 0):
        recs[gen.min_mask_region_area] = [(round((r["predicted_iou"] - 0.9) * 1024), r["segmentation"], r["area"],
                                           r["bbox"]) for r in gen.generate(np.zeros((H, W, 3), dtype=np.uint8))]
    got, plain = recs[30], recs[0]
    kept = []
    for cb in crop_boxes:      # edge filter and the crop's NMS
        idx = [i for i, p in enumerate(planted) if p[0] == cb and not (
            (np.abs(np.subtract(p[2], cb)) <= 20) & ~(np.abs(np.subtract(p[2], [0, 0, W, H])) <= 20)).any()]
        kept += [idx[k] for k in nms_ref([planted[i][2] for i in idx], idx, 0.7)]
    crop_area = [(planted[i][0][2] - planted[i][0][0]) * (planted[i][0][3] - planted[i][0][1]) for i in kept]
    final = [kept[k] for k in nms_ref([planted[i][2] for i in kept], 1 / np.array(crop_area), 0.7)]
    def expect(i, m):
        b = box(m)
        return (i, m, m.sum(), [b[0], b[1], b[2] - b[0], b[3] - b[1]])
    def same(a, b):
        assert [x[0] for x in a] == [y[0] for y in b]
        for x, y in zip(a, b):
            assert np.array_equal(x[1], y[1]) and x[2:] == y[2:], (x[0], x[2:], y[2:])
    same(plain, [expect(i, planted[i][1]) for i in final])
    cleaned = [clean(planted[i][1], 30) for i in final]
    keep = nms_ref([box(c[0]) for c in cleaned], [float(c[3]) for c in cleaned], 0.7)
    same(got, [expect(final[k], cleaned[k][0]) for k in keep])
    ids = [g[0] for g in got]
    pairs = [i for i in final if i % 3 == 1 and i + 1 in final]     # a clean disc and its speckled twin survived
    assert pairs and all(i in ids and i + 1 not in ids for i in pairs)
    assert any(i % 3 == 0 for i in ids) and len({tuple(planted[i][0]) for i in ids}) >= 3


def test_c_entries_check_sizes_on_the_host():
    """``n == 0`` is a no-op before any pointer check; a bad size is refused before anything reaches the device."""
    from samq import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def label(n=2, total=8, H=8, W=8, min_area=4, ptr=p):
        return lib.samq_rle_regions_label(ptr, ptr, n, total, H, W, min_area, ptr, ptr, ptr, 1 << 20, None)

    assert label(n=0, ptr=None) == _lib.SAMQ_OK
    assert lib.samq_rle_regions_write(None, 0, 0, 8, 8, None, None, 0, None, 0, None) == _lib.SAMQ_OK
    for bad in (dict(min_area=0), dict(H=65536, W=32768), dict(n=-1), dict(total=1), dict(ptr=None)):
        assert label(**bad) == _lib.SAMQ_ERR_INVALID, bad
    assert lib.samq_rle_regions_write(p, -1, 8, 8, 8, p, p, 1 << 20, p, 8, None) == _lib.SAMQ_ERR_INVALID
    assert lib.samq_rle_regions_workspace(2, 8, 65536, 32768) == 0 and lib.samq_rle_regions_workspace(2, 8, 8, 8) > 0
    assert label(total=(1 << 31) - 4) == _lib.SAMQ_ERR_UNSUPPORTED
