"""Peaked-softmax inputs for the fp16 attention kernels, their float64 oracle, and a float64 model
of the kernels' lazily moved exponent offset (tests/test_attn_softmax_range.py).

TEST INFRASTRUCTURE.  The kernels stream the keys one grid row at a time and keep an online softmax
whose exp2 offset ``m`` moves only when a row max leaves a band above it
(``csrc/attention_glob80.h`` softmax lambda, ``csrc/attention_rel.h`` soft lambda).  Inputs a few
units wide never leave the band; the inputs built here carry a staircase of row maxima that walks
every branch of both rules, and ``streamed_softmax_f64`` counts the branches it takes.

A case is ``(b, h, w, heads, d, window)`` like ``test_rel_attention``'s; ``window == 0`` is a
global (square) grid.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import sam_ref

LOG2E = 1.4426950408889634

# per-key-row steps of the staircase in exp2 units (for a query with b = 1): steps in (0, 8],
# (8, 15] and above 15, deep drops and late spikes
STEPS = (5, 10, 20, 5, 12, 18, -40, 30, 25, 3, 3, 9, 16, -60, 45, -20)
B_CYCLE = (1.0, -1.0, 0.0, 0.5)

FAULTS = ("no_rescale_on_recompute", "no_rescale_on_deferred", "move_not_baked_into_next_row",
          "denominator_not_rescaled")


def staircase(rows: int) -> np.ndarray:
    """a(key row): the cumulative sum of STEPS (repeated), exp2 units at b = 1."""
    reps = -(-rows // len(STEPS))
    return np.cumsum(np.tile(np.asarray(STEPS, np.float64), reps))[:rows]


@functools.lru_cache(maxsize=None)
def peaked_attn_inputs(case, seed):
    """fp16 ``qkv`` (B, H, W, 3C) built directly (no projection), ``qkv_bias`` (3C,), and the two
    rel-pos tables (2 side - 1, d).  q, k ~ 0.5 N(0,1); tables ~ 0.1 N(0,1); v uniform in [-2, 2]
    (so every output is a convex combination with |o| <= 2); channel 0 of every head carries the
    staircase: k = a(key row) / (4 scale log2e) on one key in eight of each key row and 0 elsewhere,
    q = 4 b(query) with b cycling through B_CYCLE over consecutive queries, tables 0."""
    b, h, w, heads, d, window = case
    rng = np.random.Generator(np.random.PCG64(seed))
    c = heads * d
    side = window if window else h
    q = 0.5 * rng.standard_normal((b, h, w, heads, d))
    k = 0.5 * rng.standard_normal((b, h, w, heads, d))
    v = rng.uniform(-2.0, 2.0, (b, h, w, heads, d))
    bias = np.concatenate([0.5 * rng.standard_normal(2 * c), rng.uniform(-2.0, 2.0, c)])
    rph = 0.1 * rng.standard_normal((2 * side - 1, d))
    rpw = 0.1 * rng.standard_normal((2 * side - 1, d))
    rph[:, 0] = 0.0
    rpw[:, 0] = 0.0
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    krow, kcol = (ys % side, xs % side)          # the key's row / column inside its window (or grid)
    a = staircase(side)[krow] / (4.0 * d ** -0.5 * LOG2E)
    k[..., 0] = np.where(kcol % 8 == 0, a, 0.0)[None, :, :, None]
    bq = np.asarray(B_CYCLE)[(ys * w + xs) % len(B_CYCLE)]
    q[..., 0] = (4.0 * bq)[None, :, :, None]
    qkv = np.concatenate([t.reshape(b, h, w, c) for t in (q, k, v)], axis=-1).astype(np.float16)
    assert np.isfinite(qkv).all() and np.abs(qkv[..., 2 * c:].astype(np.float32)).max() <= 2.0
    return qkv, bias.astype(np.float16), rph.astype(np.float16), rpw.astype(np.float16)


def _t64(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float64)


def _partition(case, qkv, bias):
    """float64 (B', side, side, 3C) units of a case: the grid itself, or its windows with the pad
    tokens set to the bias (the pad mask is a partitioned tensor of ones)."""
    window = case[5]
    x = _t64(qkv)
    if not window:
        return x, None
    xw, pad_hw = sam_ref.window_partition(x, window)
    real, _ = sam_ref.window_partition(torch.ones(x.shape[:3] + (1,), dtype=torch.float64), window)
    return torch.where(real > 0, xw, _t64(bias)), pad_hw


def _per_head(fn, xw, heads, d):
    """fn on one head at a time (the (units, L, L) float64 scores of a 64 x 64 grid are 134 MB)."""
    u, s1, s2, _ = xw.shape
    x5 = xw.view(u, s1, s2, 3, heads, d)
    return torch.cat([fn(x5[:, :, :, :, i].reshape(u, s1, s2, 3 * d)) for i in range(heads)], dim=-1)


@functools.lru_cache(maxsize=None)
def oracle_f64(case, seed):
    """``oracle.sam_ref.attention_core`` in float64 on the fp16 input values -> (B, H, W, C) float64."""
    b, h, w, heads, d, window = case
    qkv, bias, rph, rpw = peaked_attn_inputs(case, seed)
    xw, pad_hw = _partition(case, qkv, bias)
    o = _per_head(lambda x: sam_ref.attention_core(x, 1, _t64(rph), _t64(rpw)), xw, heads, d)
    if window:
        o = sam_ref.window_unpartition(o, window, pad_hw, (h, w))
    out = o.numpy()
    out.flags.writeable = False
    return out


def _f16(x):
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def scores_log2(x, rph, rpw, kernel_rounding=False):
    """exp2-domain scores of one head: x float64 (U, S, S, 3d) -> (U, S*S, S, S) [query, key row, key
    column] and v (U, S, S, d).  ``kernel_rounding``: q enters as fp16(fp32(q) scale log2e) and the
    TH / TW terms, (Qs . R) / scale, are rounded through fp16 -- the input roundings the kernels
    document (TW stays in f32 in the kernels, TH in the general kernel too: this is the outer case)."""
    u, s, _, d3 = x.shape
    d = d3 // 3
    q, k, v = x.view(u, s, s, 3, d).unbind(3)
    scale = d ** -0.5
    if kernel_rounding:
        qs = (q.to(torch.float32) * torch.tensor(scale * LOG2E, dtype=torch.float32)).to(torch.float16).to(torch.float64)
    else:
        qs = q * (scale * LOG2E)
    rh = sam_ref.rel_pos_table(s, s, _t64(rph))
    rw = sam_ref.rel_pos_table(s, s, _t64(rpw))
    th = torch.einsum("uijd,ikd->uijk", qs, rh) / scale      # log2e q.Rh, table row by the query ROW
    tw = torch.einsum("uijd,ikd->uijk", qs, rw) / scale
    if kernel_rounding:
        th, tw = _f16(th), _f16(tw)
    sc = torch.einsum("uijd,uyxd->uijyx", qs, k) + th[..., :, None] + tw[..., None, :]
    return sc.reshape(u, s * s, s, s), v


def _softmax2_out(x, rph, rpw, kernel_rounding):
    sc, v = scores_log2(x, rph, rpw, kernel_rounding)
    u, n, s, _ = sc.shape
    sc = sc.reshape(u, n, n)
    p = torch.exp2(sc - sc.amax(-1, keepdim=True))
    o = (p @ v.reshape(u, n, -1)) / p.sum(-1, keepdim=True)
    return o.view(u, s, s, -1)


@functools.lru_cache(maxsize=None)
def input_rounding_distance(case, seed):
    """max |oracle with the kernels' input roundings - oracle_f64|: what the fp16 q scaling and the
    fp16 rel-pos terms cost at this case's scores, before any rounding inside the softmax."""
    b, h, w, heads, d, window = case
    qkv, bias, rph, rpw = peaked_attn_inputs(case, seed)
    xw, pad_hw = _partition(case, qkv, bias)
    o = _per_head(lambda x: _softmax2_out(x, rph, rpw, True), xw, heads, d)
    if window:
        o = sam_ref.window_unpartition(o, window, pad_hw, (h, w))
    return float((o.numpy() - oracle_f64(case, seed)).__abs__().max())


def one_head_unit(case, seed, head=0, unit=0):
    """(scores_log2 (N, S, S), v (S, S, d), oracle (N, d)) of one (window or image, head)."""
    b, h, w, heads, d, window = case
    qkv, bias, rph, rpw = peaked_attn_inputs(case, seed)
    xw, _ = _partition(case, qkv, bias)
    u, s, _, _ = xw.shape
    x = xw[unit:unit + 1].view(1, s, s, 3, heads, d)[:, :, :, :, head].reshape(1, s, s, 3 * d)
    sc, v = scores_log2(x, rph, rpw)
    ref = sam_ref.attention_core(x, 1, _t64(rph), _t64(rpw)).reshape(s * s, d)
    return sc[0].numpy(), v[0].numpy(), ref.numpy()


def streamed_softmax_f64(scores, v, rule, fault=None):
    """float64 emulation of the kernels' per-key-row softmax state machine.

    scores (N, R, K) exp2-domain scores of N queries against R key rows of K keys, v (R, K, d).
    rule "glob80" (csrc/attention_glob80.h): P of a row is formed with the offset of the previous
    rows; a row max past m + 15 rescales O and recomputes P with the new offset at once; one past
    m + 8 defers the move to the start of the next row, and the moved offset is baked into that
    row's scores.  rule "rel" (csrc/attention_rel.h): the offset moves at once when the row max
    passes m + 8.  ``fault`` (one of FAULTS) breaks one step of the machine.

    Returns (out (N, d), counts, pmax): counts of (query, key row) steps after row 0 per regime,
    of 32-query groups in which a branch is taken by some queries and not by others, and the largest
    P that entered a P.V product."""
    assert rule in ("glob80", "rel") and (fault is None or fault in FAULTS)
    if rule == "rel" and fault in ("no_rescale_on_recompute", "move_not_baked_into_next_row"):
        raise ValueError(f"the rel rule has no step for {fault}")
    n, rows, _ = scores.shape
    o = np.zeros((n, v.shape[-1]))
    l = np.zeros(n)
    m = np.full(n, -np.inf)
    moff = np.zeros(n)             # glob80: the offset baked into the current row's scores
    m_pend = np.full(n, -np.inf)
    pend = np.zeros(n, bool)
    cnt = dict(stay=0, deferred=0, recompute=0, deferred_then_recompute=0, low14=0, low24=0, mixed_groups=0)
    pmax = 0.0

    def mixed(flag):
        g = np.add.reduceat(flag.astype(np.int64), np.arange(0, n, 32))
        size = np.diff(np.append(np.arange(0, n, 32), n))
        return int(((g > 0) & (g < size)).sum())

    def rescale(alpha, num=True):
        nonlocal o, l
        if num:
            o = o * alpha[:, None]
        if fault != "denominator_not_rescaled":
            l = l * alpha

    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rows):
            s = scores[:, r, :]
            mrow = s.max(-1)
            if rule == "glob80":
                was_pend = pend.copy()
                if pend.any():   # last row's deferred move
                    alpha = np.where(pend, np.exp2(m - m_pend), 1.0)
                    m = np.where(pend, m_pend, m)
                    rescale(alpha, num=fault != "no_rescale_on_deferred")
                    pend[:] = False
                low = m - mrow
                p = np.exp2(s - moff[:, None])
                unsafe = ~(mrow <= m + 15.0)
                if unsafe.any():
                    mnew = np.where(unsafe, mrow, m)
                    alpha = np.where(unsafe, np.exp2(m - mnew), 1.0)
                    alpha = np.where(np.isnan(alpha), 0.0, alpha)
                    m = mnew
                    rescale(alpha, num=fault != "no_rescale_on_recompute" or r == 0)
                    p = np.where(unsafe[:, None], np.exp2(s - m[:, None]), p)
                pend = mrow > m + 8.0
                m_pend = mrow.copy()
                moff = m if fault == "move_not_baked_into_next_row" else np.where(pend, m_pend, m)
                if r:
                    cnt["stay"] += int((~pend & ~unsafe).sum())
                    cnt["deferred"] += int(pend.sum())
                    cnt["recompute"] += int(unsafe.sum())
                    cnt["deferred_then_recompute"] += int((was_pend & unsafe).sum())
                    cnt["mixed_groups"] += mixed(pend) + mixed(unsafe) + mixed(was_pend)
            else:
                low = m - mrow
                up = mrow > m + 8.0
                mnew = np.where(up, mrow, m)
                alpha = np.where(up, np.exp2(m - mnew), 1.0)
                m = mnew
                rescale(alpha, num=fault != "no_rescale_on_deferred" or r == 0)
                p = np.exp2(s - m[:, None])
                if r:
                    cnt["stay"] += int((~up).sum())
                    cnt["deferred"] += int(up.sum())   # the rel rule's only move
                    cnt["mixed_groups"] += mixed(up)
            if r:
                cnt["low14"] += int((low > 14.0).sum())
                cnt["low24"] += int((low > 24.0).sum())
            pmax = max(pmax, float(p.max()))
            o = o + p @ v[r]
            l = l + p.sum(-1)
    return o / l[:, None], cnt, pmax


def precomputed_bias(case, seed):
    """fp16 (rel_h, rel_w) (B heads, S, S, S) of a global case, from float64 q . R: the tensors
    ``fused_attention.forward`` takes."""
    b, h, w, heads, d, window = case
    assert not window and h == w
    qkv, _, rph, rpw = peaked_attn_inputs(case, seed)
    x = _t64(qkv).view(b, h, w, 3, heads, d)
    q = x[:, :, :, 0].permute(0, 3, 1, 2, 4).reshape(b * heads, h, w, d)
    rel_h, rel_w = sam_ref.rel_bias(q, _t64(rph), _t64(rpw), h, w)
    return rel_h.to(torch.float16).contiguous(), rel_w.to(torch.float16).contiguous()


def regime_line(cnt):
    return " ".join(f"{k}={v}" for k, v in cnt.items())


assert math.isclose(LOG2E, math.log2(math.e))
