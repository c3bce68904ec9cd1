"""``ops.next_click`` (``samq_next_click``), ``samq.Clicker`` and ``click_eval.evaluate_sample`` against the numpy /
scipy reference of ``_click_ref``.  Every comparison is exact integer equality."""
import ctypes

import numpy as np
import pytest
import torch

from _click_ref import blobs, next_click_ref
from test_automatic_mask_generator import sam  # noqa: F401  (the tiny model fixture)


def check(cuda, pred, gt, clicked=None, ignore=-1):
    """Maps and rows of one call on (n, H, W) arrays against the per-mask reference; returns the rows."""
    from samq import ops
    d_pred, d_gt = torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda)
    d_clicked = None if clicked is None else torch.tensor(clicked, dtype=torch.int32, device=cuda)
    out, d2 = ops.next_click(d_pred, d_gt, d_clicked, ignore, dist=True)
    assert out.dtype == torch.int32 and d2.dtype == torch.int32 and tuple(d2.shape) == (len(pred), 2) + pred.shape[1:]
    assert torch.equal(ops.next_click(d_pred, d_gt, d_clicked, ignore), out)      # the click path writes no maps
    for i in range(len(pred)):
        row, maps = next_click_ref(pred[i], gt[i], () if clicked is None else clicked[i], ignore)
        assert np.array_equal(d2[i].cpu().numpy(), maps), i
        assert out[i].tolist() == row, i
    return out.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("n,H,W,kind", [(1, 1, 1, "blobs"), (1, 1, 37, "blobs"), (1, 37, 1, "blobs"), (1, 1, 101, "blobs"),
                                        (1, 9, 10, "blobs"), (2, 40, 131, "blobs"), (2, 201, 70, "blobs"),
                                        (1, 130, 131, "noise"), (2, 1024, 1024, "blobs")])
def test_maps_and_click(cuda, n, H, W, kind, seed):
    """W = 131 crosses the row pass's lane stride (64) and two column tiles (NC_COLS = 64) with a ragged tail of
    3; H = 201 spans three column segments (NC_SEG = 64) plus 9 rows, H = 130 two plus 2 (csrc/next_click.hip).
    Noise makes many short searches and first-index ties; blobs make long ones.  With n H W odd the workspace's
    last region (the count rows, after 4 n H W bytes of g) starts 4 bytes off an 8-byte boundary: (1, 1, 101)
    has two count rows there and a size of 2052 bytes before rounding."""
    if kind == "noise":
        rng = np.random.Generator(np.random.PCG64(seed))
        pred, gt = rng.random((n, H, W)) < 0.5, (rng.integers(0, 8, (n, H, W)) > 1).astype(np.int8)
        gt[rng.random((n, H, W)) < 0.05] = -1
    else:
        pred, gt = (np.stack(v) for v in zip(*(blobs(H, W, 2 * seed + i) for i in range(n))))
    check(cuda, pred, gt)


S = 12
FULL, NONE = np.ones((1, S, S), np.int8), np.zeros((1, S, S), dtype=bool)
BOX = np.zeros((1, S, S), np.int8)
BOX[:, 2:9, 3:11] = 1
HALF = np.zeros((1, S, S), np.int8)
HALF[:, :, :S // 2] = 1
BAND = FULL.copy()
BAND[:, :, 5:7] = -1
TWO = np.zeros((1, S, S), np.int8)
TWO[0, 3, 4] = TWO[0, 7, 9] = 1
# name -> (pred, gt, clicked, the row's first five and the counts it is there for)
CRAFTED = {
    "pred_equals_gt": (BOX == 1, BOX, None, [0, 0, 0, 0, 0, 56, 56]),
    "all_fn_four_centres_tie": (NONE, FULL, None, [1, 5, 5, 36, 0, 0, 144]),
    "mirror_halves_tie_is_negative": (HALF == 0, HALF, None, [0, 2, 8, 9, 9, 0, 144]),
    "ignore_band_separates": (NONE, BAND, None, [1, 2, 2, 9, 0, 0, 120]),
    "argmax_already_clicked": (NONE, FULL, [[[5, 5]]], [1, 5, 6, 36, 0, 0, 144]),
    "every_error_pixel_clicked": (NONE, TWO, [[[3, 4], [7, 9]]], [0, 0, 0, 0, 0, 0, 2]),
    "unused_slots": (NONE, FULL, [[[-1, 5], [5, 5], [-1, -1], [5, 6]]], [1, 6, 5, 36, 0, 0, 144]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CRAFTED))
def test_crafted(cuda, name):
    pred, gt, clicked, want = CRAFTED[name]
    assert check(cuda, pred, gt, clicked)[0][:7] == want


@pytest.mark.gpu
def test_batch_equals_single_calls(cuda):
    """Different masks, sizes of error and click lists in one call: every row equals its own call's."""
    pred, gt = (np.stack(v) for v in zip(*(blobs(70, 90, s) for s in range(3))))
    clicked = [[[y, x], [-1, 0]] for _, y, x, *_ in check(cuda, pred, gt)]
    rows = check(cuda, pred, gt, clicked)
    assert rows == [check(cuda, pred[i:i + 1], gt[i:i + 1], clicked[i:i + 1])[0] for i in range(3)]
    assert len({tuple(r) for r in rows}) == 3


@pytest.mark.gpu
def test_clicker_episode(cuda):
    import samq
    preds, gts = zip(*(blobs(64, 96, s) for s in range(6)))
    gt = gts[0]
    clicker, clicked = samq.Clicker(gt_mask=gt, device=cuda, click_indx_offset=3), []
    for step, pred in enumerate(preds):
        clicker.make_next_click(pred if step % 2 else torch.from_numpy(pred).to(cuda))
        row, _ = next_click_ref(pred, gt, clicked)
        click = clicker.get_clicks()[-1]
        assert (int(click.is_positive), *click.coords_and_indx) == (row[0], row[1], row[2], 3 + step)
        assert clicker.last_counts == (row[5], row[6]) and len(clicker) == step + 1
        clicked.append(click.coords)
    state, last = clicker.get_state(), clicker.get_clicks()[-1]
    clicker._remove_last_click()
    clicker.make_next_click(preds[5])
    assert clicker.get_clicks()[-1].coords_and_indx == last.coords_and_indx
    clicker.set_state(state[:3])
    clicker.make_next_click(preds[3])
    assert clicker.get_clicks(4)[-1].coords_and_indx == state[3].coords_and_indx
    assert (clicker.num_pos_clicks, clicker.num_neg_clicks) == (sum(c.is_positive for c in state[:4]),
                                                                sum(not c.is_positive for c in state[:4]))


@pytest.mark.gpu
def test_evaluate_sample(cuda, sam):
    import samq
    from samq.click_eval import get_iou
    image = np.random.Generator(np.random.PCG64(0)).integers(0, 256, (200, 160, 3), dtype=np.uint8)
    gt = blobs(200, 160, 4)[1]
    predictor, seen = samq.SamPredictor(sam.to(cuda)), []
    clicks, ious, mask = samq.evaluate_sample(image, gt, predictor, 2.0, max_clicks=4,
                                              callback=lambda im, g, pred, i, cl: seen.append(pred.cpu().numpy()))
    assert len(clicks) == len(seen) == 4 and ious.dtype == np.float32 and np.array_equal(mask.cpu().numpy(), seen[-1])
    prev = [np.zeros_like(seen[0])] + seen[:-1]
    for i, click in enumerate(clicks):
        row, _ = next_click_ref(prev[i], gt, [c.coords for c in clicks[:i]])
        assert (int(click.is_positive), *click.coords_and_indx) == (row[0], row[1], row[2], i)
        assert ious[i] == np.float32(get_iou(torch.from_numpy(gt), torch.from_numpy(seen[i])).double())
    clicks, ious, _ = samq.evaluate_sample(image, gt, predictor, 0.0, min_clicks=2, max_clicks=4)
    assert len(clicks) == len(ious) == 2


def test_compute_noc_metric():
    from samq.click_eval import compute_noc_metric
    table = [np.array([0.5, 0.86, 0.8, 0.95]), np.array([0.1, 0.2]), np.array([0.9])]
    noc, over = compute_noc_metric(table, [0.85, 0.9, 0.99], max_clicks=4)
    assert noc == [(2 + 4 + 1) / 3, (4 + 4 + 1) / 3, 4.0] and over == [1, 2, 3]


def test_arguments_rejected_before_any_launch():
    from samq import _lib, ops
    with pytest.raises(RuntimeError):
        ops.next_click(torch.zeros((4, 4), dtype=torch.bool), torch.zeros((4, 4), dtype=torch.int8))
    lib, p = _lib.load(), ctypes.c_void_p(64)
    assert lib.samq_next_click_workspace(1, 8, 8) > 0 and lib.samq_next_click_workspace(0, 8, 8) == 0
    assert lib.samq_next_click_workspace(1, 1, 101) == 2056        # 2052 bytes of regions, a multiple of 8 out
    assert lib.samq_next_click(None, None, None, 0, 0, 8, 8, -1, None, None, None, 0, None) == _lib.SAMQ_OK
    for n, H, W, K in [(1, 4097, 8, 0), (1, 8, 4097, 0), (1, 0, 8, 0), (1, 8, 8, 65), (1, 8, 8, -1), (-1, 8, 8, 0)]:
        assert lib.samq_next_click_workspace(n, H, W) == 0 or K != 0
        assert lib.samq_next_click(p, p, p, K, n, H, W, -1, p, None, p, 1 << 30, None) == _lib.SAMQ_ERR_INVALID
    assert lib.samq_next_click(p, p, p, 1, 1, 8, 8, -1, p, None, p, 8, None) == _lib.SAMQ_ERR_INVALID   # short workspace
