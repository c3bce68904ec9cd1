"""The click simulator of the RITM interactive-segmentation protocol (reference ``inference/clicker.py``) on the
device: the same ``Click`` / ``Clicker`` surface, with the next click taken by ``ops.next_click`` (exact
distance transform of the error regions in HIP) instead of ``cv2.distanceTransform`` on the host.

The ground truth is uploaded once, in the constructor.  ``make_next_click`` costs one kernel call and one host
read of eight integers; no mask and no distance image is copied to the host.  Where the reference keeps a
``not_clicked_map`` image, this clicker keeps the list of clicked pixels (at most 64 clicks per episode, the
kernel's limit; the protocol uses 20).
"""
from __future__ import annotations

from copy import deepcopy

import numpy as np
import torch

MAX_CLICKS = 64


class Click:
    def __init__(self, is_positive, coords, indx=None):
        self.is_positive = is_positive
        self.coords = coords          # (y, x)
        self.indx = indx

    @property
    def coords_and_indx(self):
        return (*self.coords, self.indx)

    def copy(self, **kwargs):
        c = deepcopy(self)
        for k, v in kwargs.items():
            setattr(c, k, v)
        return c


def _mask_tensor(mask, dtype, device):
    t = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
    assert t.dim() == 2, "Clicker: masks are (H, W)"
    return t.to(device=device, dtype=dtype)


class Clicker:
    def __init__(self, gt_mask=None, init_clicks=None, ignore_label=-1, click_indx_offset=0, device=None):
        self.click_indx_offset = click_indx_offset
        self.ignore_label = int(ignore_label)
        self.last_counts = None       # (inter, union) of the prediction last given to make_next_click
        self.last_max_d2 = None       # (fn_max, fp_max) squared distances of that prediction
        if gt_mask is not None:
            if device is None:
                device = gt_mask.device if isinstance(gt_mask, torch.Tensor) else torch.device("cuda")
            self.gt_mask = _mask_tensor(gt_mask, torch.int8, device)
        else:
            self.gt_mask = None
        self.reset_clicks()
        if init_clicks is not None:
            for click in init_clicks:
                self.add_click(click)

    def make_next_click(self, pred_mask):
        assert self.gt_mask is not None
        self.add_click(self._get_next_click(pred_mask))

    def get_clicks(self, clicks_limit=None):
        return self.clicks_list[:clicks_limit]

    def _get_next_click(self, pred_mask):
        from . import ops
        assert len(self.clicks_list) <= MAX_CLICKS, "Clicker: more than 64 clicks in one episode"
        dev = self.gt_mask.device
        pred = _mask_tensor(pred_mask, torch.bool, dev)
        clicked = None
        if self.clicks_list:
            clicked = torch.tensor([[list(c.coords) for c in self.clicks_list]], dtype=torch.int32).to(dev)
        row = ops.next_click(pred, self.gt_mask, clicked, self.ignore_label)[0].tolist()   # the one host read
        self.last_counts = (row[5], row[6])
        self.last_max_d2 = (row[3], row[4])
        return Click(is_positive=bool(row[0]), coords=(row[1], row[2]))

    def add_click(self, click):
        click.indx = self.click_indx_offset + self.num_pos_clicks + self.num_neg_clicks
        if click.is_positive:
            self.num_pos_clicks += 1
        else:
            self.num_neg_clicks += 1
        self.clicks_list.append(click)

    def _remove_last_click(self):
        click = self.clicks_list.pop()
        if click.is_positive:
            self.num_pos_clicks -= 1
        else:
            self.num_neg_clicks -= 1

    def reset_clicks(self):
        self.num_pos_clicks = 0
        self.num_neg_clicks = 0
        self.clicks_list = []

    def get_state(self):
        return deepcopy(self.clicks_list)

    def set_state(self, state):
        self.reset_clicks()
        for click in state:
            self.add_click(click)

    def __len__(self):
        return len(self.clicks_list)
