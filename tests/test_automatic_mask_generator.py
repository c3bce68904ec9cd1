"""``SamAutomaticMaskGenerator`` on the tiny float model of ``test_predict_torch_scored``: the records against the
numpy helpers and against each other.  Two decoder runs repeat each other only up to fp32 summation order, so
both output modes are built from ONE ``candidates`` run.

Random weights: the logits stay below 0.5 in magnitude, the predicted IoUs fall into two groups (below 0.07 and
above 0.13; float model, plain torch path on the CPU), and the masks are noise whose boxes span their crop.  Hence
``stability_score_offset=0.02`` (scores from 0.33 up), ``pred_iou_thresh=0.1`` (drops two masks of three) and
``stability_score_thresh=0.3``; in the sub-crops of ``crop_n_layers=1`` every candidate of the model touches an
inner crop edge, so ``test_generate`` reaches the crop loop with full-image survivors only, and
``test_crops_with_planted_masks`` covers sub-crop survivors with masks of its own."""
import numpy as np
import pytest
import torch

from _amg_ref import iou_rows, nms_ref, rle_to_mask

pytestmark = pytest.mark.gpu

KEYS = ["segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"]


@pytest.fixture(scope="module")
def sam():
    from samq.build_sam import Sam, build_image_encoder
    torch.manual_seed(3)
    return Sam(build_image_encoder(768, 2, 12, [1], img_size=256)).eval()


def max_pair_iou(boxes):
    b = np.asarray(boxes, dtype=np.float64)
    b[:, 2:] += b[:, :2]
    return max([np.nanmax(iou_rows(b[i], b[i + 1:]), initial=0.0) for i in range(len(b) - 1)], default=0.0)


@pytest.mark.parametrize("layers", [0, 1])
def test_generate(cuda, sam, layers):
    import samq
    from samq.automatic_mask_generator import generate_crop_boxes
    image = np.random.Generator(np.random.PCG64(0)).integers(0, 256, (200, 160, 3), dtype=np.uint8)
    gen = samq.SamAutomaticMaskGenerator(sam.to(cuda), points_per_side=4, points_per_batch=5, pred_iou_thresh=0.1,
                                         stability_score_thresh=0.3, stability_score_offset=0.02,
                                         crop_n_layers=layers, output_mode="uncompressed_rle")
    cand = gen.candidates(image)
    rles = gen.records(cand, (200, 160))
    gen.output_mode = "binary_mask"
    recs = gen.records(cand, (200, 160))
    crop_boxes = [[x0, y0, x1 - x0, y1 - y0] for x0, y0, x1, y1 in generate_crop_boxes((200, 160), layers, 512 / 1500)[0]]
    assert 1 <= len(recs) < 16 * 3 * len(crop_boxes) and len(rles) == len(recs)
    for rle, rec in zip(rles, recs):
        assert list(rec) == KEYS and list(rle) == KEYS
        mask = rec["segmentation"]
        assert mask.dtype == bool and mask.shape == (200, 160)
        assert rle["segmentation"]["size"] == [200, 160]
        assert np.array_equal(rle_to_mask(rle["segmentation"]["counts"], 200, 160), mask)
        assert type(rec["area"]) is int and rec["area"] == mask.sum()
        ys, xs = np.nonzero(mask)
        assert rec["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()]
        assert all(type(rec[k]) is float for k in ("predicted_iou", "stability_score"))
        assert rec["predicted_iou"] > 0.1 and rec["stability_score"] >= 0.3
        assert rec["crop_box"] in crop_boxes
        (px, py), (cx, cy, cw, ch) = rec["point_coords"][0], rec["crop_box"]
        assert len(rec["point_coords"]) == 1 and cx <= px <= cx + cw and cy <= py <= cy + ch
    for cb in crop_boxes:
        assert max_pair_iou([r["bbox"] for r in recs if r["crop_box"] == cb] or [[0, 0, 1, 1]]) <= 0.7
    assert max_pair_iou([r["bbox"] for r in recs]) <= 0.7


def test_crops_with_planted_masks(cuda, sam):
    """Records of sub-crops.  ``_process_batch`` is replaced by one that plants discs of radius 5, 9 and 10 around
    every prompt (clipped to the crop, stability 1, predicted IoU 0.9 + index / 1024) and hands them to ``_select``,
    so the edge filter, ``ops.mask_rle`` at a placement, both NMS calls and the uncropping run on known masks.  The
    expected list is the numpy composition of the same steps on the uncropped canvas.  The fifth full-image prompt
    is the centre of the first sub-crop, whose discs (planted 27 .. 29) therefore repeat 12 .. 14: the NMS across
    crops has to keep the sub-crop's."""
    import samq
    from samq.automatic_mask_generator import build_point_grid, generate_crop_boxes
    H, W = 200, 160
    crop_boxes = generate_crop_boxes((H, W), 1, 512 / 1500)[0]
    grids = [np.array([[.25, .25], [.75, .25], [.25, .75], [.75, .75],
                       [crop_boxes[1][2] / 2 / W, crop_boxes[1][3] / 2 / H]]), build_point_grid(3)]
    gen = samq.SamAutomaticMaskGenerator(sam.to(cuda), points_per_side=None, point_grids=grids, points_per_batch=5,
                                         crop_n_layers=1)
    yy, xx = np.mgrid[:H, :W]
    planted = []    # (crop box, full-image prompt, canvas, full-image xyxy box of the disc)

    def plant(points, crop_size, crop_box, orig_size):
        x0, y0, x1, y1 = crop_box
        first = len(planted)
        for px, py in points:
            for r in (5, 9, 10):
                canvas = (xx - int(px + x0)) ** 2 + (yy - int(py + y0)) ** 2 <= r * r
                canvas &= (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
                ys, xs = np.nonzero(canvas)
                planted.append((crop_box, [px + x0, py + y0], canvas, [xs.min(), ys.min(), xs.max(), ys.max()]))
        new = planted[first:]
        boxes = torch.tensor(np.array([p[3] for p in new]) - [x0, y0, x0, y0], dtype=torch.int32, device=cuda)
        iou = (0.9 + torch.arange(first, len(planted), device=cuda) / 1024).view(-1, 3)
        res = {"masks": torch.tensor(np.stack([p[2][y0:y1, x0:x1] for p in new]), device=cuda).unflatten(0, (-1, 3)),
               "iou_predictions": iou, "stability_score": torch.ones_like(iou), "boxes": boxes.view(-1, 3, 4)}
        return gen._select(res, points, crop_box, orig_size)

    gen._process_batch = plant
    recs = gen.generate(np.zeros((H, W, 3), dtype=np.uint8))
    kept = []
    for cb in crop_boxes:      # edge filter and the crop's NMS
        idx = [i for i, p in enumerate(planted) if p[0] == cb and not (
            (np.abs(np.subtract(p[3], cb)) <= 20) & ~(np.abs(np.subtract(p[3], [0, 0, W, H])) <= 20)).any()]
        kept += [idx[k] for k in nms_ref([planted[i][3] for i in idx], idx, 0.7)]
    crop_area = [(planted[i][0][2] - planted[i][0][0]) * (planted[i][0][3] - planted[i][0][1]) for i in kept]
    final = [kept[k] for k in nms_ref([planted[i][3] for i in kept], 1 / np.array(crop_area), 0.7)]
    assert [round((r["predicted_iou"] - 0.9) * 1024) for r in recs] == final
    assert np.array_equal(planted[12][2], planted[27][2]) and {27, 29} <= set(final) and not {12, 13, 14} & set(final)
    assert len({tuple(planted[i][0]) for i in final}) >= 3
    for rec, i in zip(recs, final):
        cb, point, canvas, box = planted[i]
        assert rec["crop_box"] == [cb[0], cb[1], cb[2] - cb[0], cb[3] - cb[1]] and rec["point_coords"] == [point]
        assert np.array_equal(rec["segmentation"], canvas) and rec["area"] == canvas.sum()
        assert rec["bbox"] == [box[0], box[1], box[2] - box[0], box[3] - box[1]]


def test_generator_errors(sam):
    import samq
    with pytest.raises(NotImplementedError):
        samq.SamAutomaticMaskGenerator(sam, min_mask_region_area=1)
    with pytest.raises(ImportError):
        samq.SamAutomaticMaskGenerator(sam, output_mode="coco_rle")
    gen = samq.SamAutomaticMaskGenerator(sam.cpu(), points_per_side=2)
    with pytest.raises(NotImplementedError):
        gen.generate(np.zeros((64, 48, 3), dtype=np.uint8))
