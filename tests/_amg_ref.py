"""numpy references of the automatic mask generator's pieces: Fortran-order RLE, greedy NMS, box IoU."""
import numpy as np


def rle_ref(mask, x0, y0, H, W):
    """Run lengths of `mask` pasted at (x0, y0) on a zero H x W canvas, Fortran order, zeros first."""
    canvas = np.zeros((H, W), dtype=bool)
    canvas[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]] = mask
    flat = canvas.flatten(order="F")
    bounds = np.concatenate([[0], np.flatnonzero(np.diff(flat.astype(np.int8))) + 1, [H * W]])
    counts = np.diff(bounds)
    return np.concatenate([[0], counts]) if flat[0] else counts


def rle_to_mask(counts, H, W):
    return np.repeat(np.arange(len(counts)) % 2 == 1, counts).reshape(W, H).T


def iou_rows(box, others):
    """float64 IoU of one xyxy box against (n, 4); 0 / 0 is NaN."""
    w = np.maximum(np.minimum(box[2], others[:, 2]) - np.maximum(box[0], others[:, 0]), 0)
    h = np.maximum(np.minimum(box[3], others[:, 3]) - np.maximum(box[1], others[:, 1]), 0)
    area = (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return w * h / ((box[2] - box[0]) * (box[3] - box[1]) + area - w * h)


def nms_ref(boxes, scores, thr):
    """Greedy NMS in float64: descending score, equal scores by ascending index; kept indices in rank order."""
    boxes = np.asarray(boxes, dtype=np.float64)
    order = np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")
    ranked = boxes[order]
    dead = np.zeros(len(order), dtype=bool)
    keep = []
    for i in range(len(order)):
        if not dead[i]:
            keep.append(order[i])
            dead[i + 1:] |= iou_rows(ranked[i], ranked[i + 1:]) > thr
    return np.asarray(keep, dtype=np.int64)
