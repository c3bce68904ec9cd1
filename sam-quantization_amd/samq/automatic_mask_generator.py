"""``SamAutomaticMaskGenerator``: "segment everything" over a grid of point prompts, with the constructor,
the defaults and the output records of ``segment_anything/automatic_mask_generator.py``, on the HIP path:

* per batch of points ONE ``SamPredictor.predict_torch_scored`` call (decoder, then ``ops.mask_postprocess``:
  masks, stability scores, boxes, areas), the three filters as one boolean tensor on the device, and
  ``ops.mask_rle`` of the surviving masks straight onto the full-image canvas (no ``uncrop_masks`` copy);
* per crop ``ops.box_nms`` on the predicted IoUs, across crops ``ops.box_nms`` on ``1 / crop area``;
* with ``min_mask_region_area > 0`` ``ops.rle_remove_small_regions`` on the run lengths of the survivors (no mask is
  decoded) and a third ``ops.box_nms`` that prefers the masks it left untouched (``postprocess_small_regions``);
* the image is uploaded once; every crop is resized from the resident copy (``SamPredictor.set_image`` with a
  ``box``: ``ops.resize_u8`` on a window), not sliced, resized and uploaded again on the host;
* host lists are built once per crop from the CSR tensors (one device-to-host copy per field), not once per mask.

Host round trips, none of which grows with the number of masks.  Per batch: two reads (the size of the
selection from ``nonzero``, the RLE total inside ``ops.mask_rle``) and two small uploads (the crop / image
boxes of the edge filter, the batch's points).  Per crop: two reads (the kept count inside ``ops.box_nms``, the
kept rows' RLE total), two small uploads (the crop's shift and box) and the six copies of the result.  Per image
with more than one crop: the kept count of the NMS across crops and its index list.  Per image with
``min_mask_region_area > 0``: the cleaned rows' RLE total, the kept count of that NMS, one small upload (the
survivors' row indices) and the copies of the result.
GPU only, with any ``Sam`` the predictor accepts (GPTQ, fq_sam or float).
"""
from __future__ import annotations

import math
from itertools import product
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .sam_decoder import SamPredictor


def build_point_grid(n_per_side: int) -> np.ndarray:
    """An n x n grid of (x, y) points in [0, 1]^2, cell centres, row by row."""
    pts = np.linspace(1 / (2 * n_per_side), 1 - 1 / (2 * n_per_side), n_per_side)
    return np.stack(np.meshgrid(pts, pts), axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side: int, n_layers: int, scale_per_layer: int) -> List[np.ndarray]:
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def generate_crop_boxes(im_size: Tuple[int, int], n_layers: int, overlap_ratio: float):
    """The whole image, then for layer i a (2^(i+1))^2 grid of overlapping crops.  Returns (xyxy boxes, layers)."""
    im_h, im_w = im_size
    boxes, layers = [[0, 0, im_w, im_h]], [0]
    for layer in range(n_layers):
        n = 2 ** (layer + 1)
        overlap = int(overlap_ratio * min(im_h, im_w) * (2 / n))
        crop_w = int(math.ceil((overlap * (n - 1) + im_w) / n))
        crop_h = int(math.ceil((overlap * (n - 1) + im_h) / n))
        xs = [int((crop_w - overlap) * i) for i in range(n)]
        ys = [int((crop_h - overlap) * i) for i in range(n)]
        for x0, y0 in product(xs, ys):
            boxes.append([x0, y0, min(x0 + crop_w, im_w), min(y0 + crop_h, im_h)])
            layers.append(layer + 1)
    return boxes, layers


def rle_to_mask(rle: Dict[str, Any]) -> np.ndarray:
    """A bool (h, w) mask from an uncompressed RLE record {"size": [h, w], "counts": [...]}."""
    h, w = rle["size"]
    ends = np.cumsum(np.asarray(rle["counts"], dtype=np.int64))
    flat = np.zeros(h * w + 1, dtype=np.int8)
    np.add.at(flat, ends[:-1:2], 1)       # a run of ones starts where an even-indexed run ends
    np.add.at(flat, ends[1::2], -1)
    return np.cumsum(flat[:-1]).astype(bool).reshape(w, h).T


def coco_encode_rle(rle: Dict[str, Any]) -> Dict[str, Any]:
    from pycocotools import mask as mask_utils
    h, w = rle["size"]
    out = mask_utils.frPyObjects(rle, h, w)
    out["counts"] = out["counts"].decode("utf-8")
    return out


def _xywh(box: List[int]) -> List[int]:
    return [box[0], box[1], box[2] - box[0], box[3] - box[1]]


def _gather_rows(lens: torch.Tensor, counts: torch.Tensor, rows: torch.Tensor, total: Optional[int]):
    """Rows ``rows`` of a CSR batch (row lengths ``lens``, entries ``counts``) as a new CSR batch ``(offsets,
    counts)``, on the device.  ``total``: the number of entries gathered, read from the device when ``None``."""
    starts = torch.cumsum(lens, 0) - lens
    klen = lens[rows]
    koff = torch.cat([klen.new_zeros(1), torch.cumsum(klen, 0)])
    if total is None:
        total = int(koff[-1])
    src = torch.repeat_interleave(starts[rows] - koff[:-1], klen, output_size=total) \
        + torch.arange(total, device=counts.device)
    return koff, counts[src]


class SamAutomaticMaskGenerator:
    def __init__(self, model, points_per_side: Optional[int] = 32, points_per_batch: int = 64,
                 pred_iou_thresh: float = 0.88, stability_score_thresh: float = 0.95,
                 stability_score_offset: float = 1.0, box_nms_thresh: float = 0.7, crop_n_layers: int = 0,
                 crop_nms_thresh: float = 0.7, crop_overlap_ratio: float = 512 / 1500,
                 crop_n_points_downscale_factor: int = 1, point_grids: Optional[List[np.ndarray]] = None,
                 min_mask_region_area: int = 0, output_mode: str = "binary_mask") -> None:
        assert (points_per_side is None) != (point_grids is None), \
            "Exactly one of points_per_side or point_grid must be provided."
        if points_per_side is not None:
            self.point_grids = build_all_layer_point_grids(points_per_side, crop_n_layers,
                                                           crop_n_points_downscale_factor)
        else:
            self.point_grids = point_grids
        assert output_mode in ("binary_mask", "uncompressed_rle", "coco_rle"), f"Unknown output_mode {output_mode}."
        if output_mode == "coco_rle":
            from pycocotools import mask as mask_utils  # noqa: F401
        if min_mask_region_area > 0:
            raise NotImplementedError("min_mask_region_area > 0 needs OpenCV's connected components: not supported")
        self.predictor = SamPredictor(model)
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_n_layers = crop_n_layers
        self.crop_nms_thresh = crop_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.min_mask_region_area = min_mask_region_area
        self.output_mode = output_mode

    @torch.no_grad()
    def generate(self, image: np.ndarray) -> List[Dict[str, Any]]:
        """Mask records for an HWC uint8 image: ``segmentation``, ``area``, ``bbox`` (xywh), ``predicted_iou``,
        ``point_coords``, ``stability_score``, ``crop_box`` (xywh)."""
        cand = self.candidates(image)
        if self.min_mask_region_area > 0:
            cand = self.postprocess_small_regions(cand, image.shape[:2], self.min_mask_region_area,
                                                  max(self.box_nms_thresh, self.crop_nms_thresh))
        return self.records(cand, image.shape[:2])

    @torch.no_grad()
    def candidates(self, image: np.ndarray):
        """The forward half of ``generate``: per crop the host copy of what survived the filters and the crop's
        NMS, and the (crop, row) pairs that survive the NMS across crops, in output order."""
        orig_size = tuple(image.shape[:2])
        crop_boxes, layers = generate_crop_boxes(orig_size, self.crop_n_layers, self.crop_overlap_ratio)
        if self.predictor.device.type == "cuda":
            # one upload; every crop is resized from the resident image (ops.resize_u8 on a window)
            image = torch.as_tensor(np.ascontiguousarray(image), device=self.predictor.device)
        crops = [self._process_crop(image, box, layer, orig_size) for box, layer in zip(crop_boxes, layers)]
        crops = [c for c in crops if c is not None]
        where = [(ci, r) for ci, c in enumerate(crops) for r in range(len(c["boxes"]))]
        if len(crop_boxes) > 1 and where:
            # prefer masks of smaller crops; all masks of a crop tie, which box_nms ranks by index
            boxes = torch.cat([c["boxes"] for c in crops])
            area = torch.cat([c["crop_box_t"].expand(len(c["boxes"]), 4) for c in crops]).float()
            scores = 1 / ((area[:, 2] - area[:, 0]) * (area[:, 3] - area[:, 1]))
            where = [where[g] for g in ops.box_nms(boxes.float(), scores, self.crop_nms_thresh).tolist()]
        return crops, where

    def records(self, candidates, orig_size) -> List[Dict[str, Any]]:
        """The host half of ``generate``: the output records of ``candidates(image)`` in ``self.output_mode``."""
        crops, where = candidates
        out = []
        for ci, r in where:
            c = crops[ci]
            counts = c["counts"][c["offsets"][r]:c["offsets"][r + 1]]
            rle = {"size": [orig_size[0], orig_size[1]], "counts": counts.tolist()}
            if self.output_mode == "coco_rle":
                seg = coco_encode_rle(rle)
            elif self.output_mode == "binary_mask":
                seg = rle_to_mask(rle)
            else:
                seg = rle
            out.append({"segmentation": seg, "area": int(counts[1::2].sum()), "bbox": _xywh(c["boxes_l"][r]),
                        "predicted_iou": c["iou_l"][r], "point_coords": [c["points_l"][r]],
                        "stability_score": c["stab_l"][r], "crop_box": _xywh(c["crop_box"])})
        return out

    @staticmethod
    @torch.no_grad()
    def postprocess_small_regions(candidates, orig_size, min_area: int, nms_thresh: float):
        """Holes and islands below ``min_area`` removed from every surviving mask, then a box NMS that ranks the
        masks this left untouched first (score 1 against 0), as the reference's method of this name.  Takes what
        ``candidates(image)`` returns and gives back the same structure for ``records``: one entry per crop, all
        sharing the arrays of the cleaned survivors (row ``k`` is ``where[k]``), and the kept ``(crop, row)``
        pairs in the NMS's order.  Host reads: the cleaned rows' RLE total and the kept count of the NMS."""
        crops, where = candidates
        if not where:
            return candidates
        dev = crops[0]["boxes"].device
        # the survivors' rows out of the crops' device CSR copies, in `where` order; their total from the host copy
        base = np.concatenate([[0], np.cumsum([len(c["boxes_l"]) for c in crops])])
        rows = torch.tensor([int(base[ci]) + r for ci, r in where], device=dev)
        total = sum(int(crops[ci]["offsets"][r + 1] - crops[ci]["offsets"][r]) for ci, r in where)
        offsets, counts = _gather_rows(torch.cat([c["offsets_d"].diff() for c in crops]),
                                       torch.cat([c["counts_d"] for c in crops]), rows, total)
        offsets, counts, new_boxes, _, unchanged = ops.rle_remove_small_regions(offsets, counts, orig_size, min_area)
        keep = ops.box_nms(new_boxes.float(), unchanged.float(), nms_thresh)
        # a row that nothing changed equals its input, so the cleaned rows serve for every mask; the box is
        # replaced for the changed ones only
        boxes = torch.where(unchanged[:, None], torch.cat([c["boxes"] for c in crops])[rows], new_boxes.long())
        merged = {"boxes": boxes, "boxes_l": boxes.tolist(), "offsets": offsets.cpu().numpy(),
                  "counts": counts.cpu().numpy(), "offsets_d": offsets, "counts_d": counts}
        for field in ("iou_l", "stab_l", "points_l"):
            merged[field] = [crops[ci][field][r] for ci, r in where]
        out = [{**merged, "crop_box": c["crop_box"], "crop_box_t": c["crop_box_t"]} for c in crops]
        return out, [(where[k][0], k) for k in keep.tolist()]

    def _process_crop(self, image, crop_box, layer, orig_size):
        x0, y0, x1, y1 = crop_box
        crop_size = (y1 - y0, x1 - x0)
        self.predictor.set_image(image, box=crop_box)
        points = self.point_grids[layer] * np.array(crop_size)[None, ::-1]
        batches = []
        for b in range(0, len(points), self.points_per_batch):
            d = self._process_batch(points[b:b + self.points_per_batch], crop_size, crop_box, orig_size)
            if d is not None:
                batches.append(d)
        self.predictor.reset_image()
        if not batches:
            return None
        dev = batches[0]["boxes"].device
        shift = torch.tensor([x0, y0, x0, y0], device=dev)
        boxes = torch.cat([d["boxes"] for d in batches])
        iou = torch.cat([d["iou"] for d in batches])
        stab = torch.cat([d["stab"] for d in batches])
        pts = torch.cat([d["points"] for d in batches])
        lens = torch.cat([d["offsets"].diff() for d in batches])
        counts = torch.cat([d["counts"] for d in batches])
        keep = ops.box_nms(boxes.float(), iou, self.box_nms_thresh)
        # the kept rows' run lengths, gathered on the device in keep order; the total is the crop's second host
        # read (the first is box_nms's kept count)
        koff, kcounts = _gather_rows(lens, counts, keep, None)
        # to the host once per crop, one copy per field
        full = boxes[keep] + shift
        return {"crop_box": list(crop_box), "crop_box_t": torch.tensor([crop_box], device=dev),
                "boxes": full, "boxes_l": full.tolist(), "iou_l": iou[keep].tolist(), "stab_l": stab[keep].tolist(),
                "points_l": (pts[keep] + shift[:2]).tolist(), "offsets": koff.cpu().numpy(),
                "counts": kcounts.cpu().numpy(), "offsets_d": koff, "counts_d": kcounts}

    def _process_batch(self, points, crop_size, crop_box, orig_size):
        """One batch of points of one crop -> the device tensors of its surviving candidates (or ``None``)."""
        dev = self.predictor.device
        coords = torch.as_tensor(self.predictor.transform.apply_coords(points, crop_size), dtype=torch.float,
                                 device=dev)
        labels = torch.ones(coords.shape[0], dtype=torch.int, device=dev)
        res = self.predictor.predict_torch_scored(coords[:, None, :], labels[:, None], multimask_output=True,
                                                  stability_score_offset=self.stability_score_offset)
        return self._select(res, points, crop_box, orig_size)

    def _select(self, res, points, crop_box, orig_size):
        """Filter the candidates of ``predict_torch_scored`` and run-length encode the survivors."""
        masks = res["masks"].flatten(0, 1)
        iou, stab = res["iou_predictions"].flatten().float(), res["stability_score"].flatten()
        boxes = res["boxes"].flatten(0, 1)
        dev = masks.device
        per_point = res["masks"].shape[1]
        x0, y0, x1, y1 = crop_box
        # near a crop edge that is not an image edge (both within 20 px, on the uncropped box)
        shift_t, crop_t, image_t = torch.tensor([[x0, y0, x0, y0], [x0, y0, x1, y1], [0, 0, orig_size[1], orig_size[0]]],
                                                dtype=torch.float, device=dev)
        full = boxes.float() + shift_t
        near = ((full - crop_t).abs() <= 20.0) & ~((full - image_t).abs() <= 20.0)
        ok = ~near.any(dim=1)
        if self.pred_iou_thresh > 0.0:
            ok &= iou > self.pred_iou_thresh
        if self.stability_score_thresh > 0.0:
            ok &= stab >= self.stability_score_thresh
        sel = ok.nonzero().flatten()      # sync 1 of 2: the size of the selection
        if sel.numel() == 0:
            return None
        offsets, counts = ops.mask_rle(masks, sel, crop_box, orig_size)     # sync 2 of 2: the RLE total
        pts = torch.as_tensor(np.asarray(points, dtype=np.float64).repeat(per_point, axis=0), device=dev)
        return {"boxes": boxes[sel].long(), "iou": iou[sel], "stab": stab[sel], "points": pts[sel],
                "offsets": offsets, "counts": counts}
