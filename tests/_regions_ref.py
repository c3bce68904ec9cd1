"""Reference of ``remove_small_regions`` (holes, then islands): an 8-neighbour flood fill in place of OpenCV."""
import numpy as np

from _amg_ref import rle_ref, rle_to_mask


def components(mask):
    """8-connected components of the set pixels, numbered by first pixel in column-major order: (labels, areas)."""
    (H, W), areas = mask.shape, []
    labels = np.full((H, W), -1, dtype=np.int32)
    for x, y in zip(*np.nonzero(mask.T)):       # column-major order
        if labels[y, x] >= 0:
            continue
        labels[y, x] = len(areas)
        stack, area = [(y, x)], 0
        while stack:
            cy, cx = stack.pop()
            area += 1
            for ny in range(max(cy - 1, 0), min(cy + 2, H)):
                for nx in range(max(cx - 1, 0), min(cx + 2, W)):
                    if mask[ny, nx] and labels[ny, nx] < 0:
                        labels[ny, nx] = len(areas)
                        stack.append((ny, nx))
        areas.append(area)
    return labels, np.asarray(areas, dtype=np.int64)


def clean(mask, min_area):
    """(cleaned mask, holes filled, islands dropped, unchanged)."""
    labels, areas = components(~mask)
    holes = np.flatnonzero(areas < min_area)
    mask = mask | np.isin(labels, holes)
    labels, areas = components(mask)
    small = np.flatnonzero(areas < min_area)
    dropped = 0
    if len(small):
        keep = np.flatnonzero(areas >= min_area)
        if not len(keep):
            keep = [int(np.argmax(areas))]      # the first of the largest: the earliest in column-major order
        dropped = len(areas) - len(keep)
        mask = np.isin(labels, keep)
    return mask, len(holes), dropped, not len(holes) and not len(small)


def csr(masks):
    rows = [rle_ref(m, 0, 0, *m.shape) for m in masks]
    return np.cumsum([0] + [len(r) for r in rows]), np.concatenate(rows).astype(np.int32)


def regions_ref(masks, min_area):
    """Expected ``ops.rle_remove_small_regions`` of ``csr(masks)``, holes filled and islands dropped in the batch."""
    offsets, counts = csr(masks)
    H, W = masks[0].shape
    out, boxes, filled, dropped = [], [], 0, 0
    for i in range(len(masks)):
        m, f, d, same = clean(rle_to_mask(counts[offsets[i]:offsets[i + 1]], H, W), min_area)
        ys, xs = np.nonzero(m)
        boxes.append([xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) else [0, 0, 0, 0])
        out.append((m, same))
        filled, dropped = filled + f, dropped + d
    new_offsets, new_counts = csr([m for m, _ in out])
    return (new_offsets, new_counts, np.asarray(boxes), np.asarray([m.sum() for m, _ in out]),
            np.asarray([s for _, s in out])), filled, dropped
