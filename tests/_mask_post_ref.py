"""Float64 reference of ``ops.mask_postprocess``: the project's ``postprocess_masks`` on ``low.double()`` on
the CPU, and the thresholds, sums and ``batched_mask_to_box`` rule (``segment_anything/utils/amg.py``) on it."""
import torch

from samq.sam_decoder import postprocess_masks


def ref_values(low, img_size, input_size, original_size):
    """(N, H, W) float64 from (N, lh, lw) logits."""
    return postprocess_masks(low.detach().double().cpu()[:, None], img_size, input_size, original_size)[:, 0]


def boxes(mask):
    """Inclusive xyxy int32 (N, 4) of bool (N, H, W) masks; 0, 0, 0, 0 for an empty one."""
    _, h, w = mask.shape
    rows, cols = mask.any(2), mask.any(1)
    ys, xs = torch.arange(h), torch.arange(w)
    out = torch.stack([(cols * xs + w * ~cols).min(1).values, (rows * ys + h * ~rows).min(1).values,
                       (cols * xs).max(1).values, (rows * ys).max(1).values], 1)
    return (out * rows.any(1)[:, None]).int()


def count(pred):
    return pred.flatten(1).sum(1).int()


def ref_stats(v, thr, off):
    """int32 (N, 8): inter, union, area, box, 0."""
    m = v > thr
    cnt = torch.stack([count(v > thr + off), count(v > thr - off), count(m)], 1)
    return torch.cat([cnt, boxes(m), torch.zeros((len(v), 1), dtype=torch.int32)], 1)
