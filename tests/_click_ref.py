"""Numpy / scipy reference of ``ops.next_click``: ``Clicker._get_next_click`` with padding on squared integer
distances, the counts of ``get_iou``, and a seeded blob painter."""
import numpy as np
from scipy.ndimage import distance_transform_edt


def d2_ref(m):
    """Squared distance to the nearest zero of ``m`` padded by a one-pixel ring of zeros, int64."""
    return np.rint(distance_transform_edt(np.pad(m, 1))[1:-1, 1:-1] ** 2).astype(np.int64)


def next_click_ref(pred, gt, clicked=(), ignore=-1):
    """One mask: (the row ``[is_positive, y, x, fn_max, fp_max, inter, union, 0]``, the maps (2, H, W))."""
    pred, obj, keep = pred.astype(bool), gt == 1, gt != ignore
    maps = np.stack([d2_ref(obj & ~pred & keep), d2_ref(~obj & pred & keep)])
    dt = maps.copy()
    for y, x in clicked:
        if 0 <= y < dt.shape[1] and 0 <= x < dt.shape[2]:
            dt[:, y, x] = 0
    fn_max, fp_max = int(dt[0].max()), int(dt[1].max())
    pos = fn_max > fp_max
    ys, xs = np.where(dt[0] == fn_max) if pos else np.where(dt[1] == fp_max)
    return [int(pos), int(ys[0]), int(xs[0]), fn_max, fp_max, int((pred & obj & keep).sum()),
            int(((pred | obj) & keep).sum()), 0], maps


def blobs(H, W, seed, discs=5):
    """(pred bool, gt int8) of one seeded scene: ``gt`` a union of discs with a disc-shaped hole and a diagonal
    ignore band; ``pred`` misses the last disc (a thick false-negative region) and has the others and the hole
    moved diagonally (thin rims of both kinds)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W]
    side = max(H, W)
    cys, cxs, rs = rng.uniform(0, H, discs), rng.uniform(0, W, discs), rng.uniform(0.08, 0.3, discs) * side
    hy, hx = rng.uniform(0, H), rng.uniform(0, W)

    def paint(shift, count):
        m = np.zeros((H, W), dtype=bool)
        for cy, cx, r in zip(cys[:count], cxs[:count], rs[:count]):
            m |= (yy - cy - shift) ** 2 + (xx - cx + shift) ** 2 <= r * r
        return m & ((yy - hy - shift) ** 2 + (xx - hx + shift) ** 2 > (0.06 * side) ** 2)

    gt = paint(0.0, discs).astype(np.int8)
    gt[np.abs(yy - xx - (H - W) // 2) <= side // 40] = -1
    return paint(0.07 * side, discs - 1), gt
