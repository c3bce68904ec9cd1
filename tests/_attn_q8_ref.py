"""Reference and inputs of the W8A8 attention tests at any head dim.

``attn_ref`` is ``test_w8a8._attn_ref`` with the softmax scale as an argument (that one hard-codes
``d ** -0.5``; exact-tie inputs at d = 80 need 2^-3) -- bit for bit the same graph at d = 64,
which test_w8a8_hd80.py checks.  ``q8_inputs`` / ``exact_attn_inputs`` are the recipes of
``test_w8a8._q8_inputs`` / ``_exact_attn_inputs`` with the head dim as a parameter.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import fq_ref, sam_ref

Q8_SCALES = (np.float32(0.02), np.float32(2.0 / 127.5), np.float32(6.0 / 127.5), np.float32(2.6 / 127.5))


def attn_ref(qkv_codes, bias, relh, relw, heads, window, sm_scale, s_qkv, s1, s2, s_o, dtype=torch.float32, fq1=None,
             fq2=None, codes2=None):
    """fq_vit Attention core (oracle F semantics) on fake-quant qkv values, with windowing; the
    arguments of ``test_w8a8._attn_ref`` plus ``sm_scale`` (the factor on q before q.k)."""
    b, h, w, c3 = qkv_codes.shape
    c = c3 // 3
    d = c // heads
    fq1, fq2 = fq1 or fq_ref.fake_quant, fq2 or fq_ref.fake_quant
    ts = lambda s: torch.tensor(float(s), dtype=dtype)   # the scales are fp32 values: exact in either dtype
    qkv = torch.from_numpy(qkv_codes.astype(np.float32)).to(dtype) * ts(s_qkv)
    if window > 0:
        # pad tokens project the zero-padded LN output: qkv = bias, then attn.qact1
        pad_val = fq_ref.fake_quant(torch.from_numpy(bias).to(dtype) if bias is not None else
                                    torch.zeros(c3, dtype=dtype), ts(s_qkv))
        hp, wp = -(-h // window) * window, -(-w // window) * window
        full = pad_val.expand(b, hp, wp, c3).clone()
        full[:, :h, :w] = qkv
        qkv, _ = sam_ref.window_partition(full, window)
    bq, hh, ww, _ = qkv.shape
    n, ll = bq * heads, hh * ww
    t = qkv.reshape(bq, ll, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = t.reshape(3, n, ll, d).unbind(0)
    rph, rpw = torch.from_numpy(relh).to(dtype), torch.from_numpy(relw).to(dtype)
    o = torch.empty((n, ll, d), dtype=dtype)
    step = max(1, (1 << 24) // (ll * ll))
    for i in range(0, n, step):
        qi, ki, vi = q[i:i + step], k[i:i + step], v[i:i + step]
        m = qi.shape[0]
        sc = (qi * sm_scale) @ ki.transpose(-2, -1)
        sc = fq1(sc, ts(s1))
        rh, rw = sam_ref.rel_bias(qi.reshape(m, hh, ww, d), rph, rpw, hh, ww)
        sc = (sc.view(m, hh, ww, hh, ww) + rh[..., :, None] + rw[..., None, :]).view(m, ll, ll)
        sc = fq2(sc, ts(s2))
        if codes2 is not None:
            codes2.append(torch.round(sc / ts(s2)).to(torch.int16))
        o[i:i + step] = torch.softmax(sc, -1) @ vi
    o = o.view(bq, heads, hh, ww, d).permute(0, 2, 3, 1, 4).reshape(bq, hh, ww, c)
    if window > 0:
        o = sam_ref.window_unpartition(o, window, (hp, wp), (h, w))
    return np.clip(np.round((o / ts(s_o)).numpy()), -128, 127)


def q8_inputs(b, h, w, heads, window, seed, d):
    """Random full-range codes, N(0, 0.5) tables, N(0, 0.3) bias (``test_w8a8._q8_inputs`` at head dim d);
    used with Q8_SCALES."""
    c = heads * d
    rng = np.random.Generator(np.random.PCG64(seed))
    qkv = rng.integers(-128, 128, (b, h, w, 3 * c), dtype=np.int8)
    side = window or h
    relh = (rng.standard_normal((2 * side - 1, d), dtype=np.float32) * 0.5).astype(np.float32)
    relw = (rng.standard_normal((2 * side - 1, d), dtype=np.float32) * 0.5).astype(np.float32)
    bias = (rng.standard_normal(3 * c, dtype=np.float32) * 0.3).astype(np.float32)
    return qkv, bias, relh, relw


EXACT_SM_SCALE = 2.0 ** -3

# Sharp-softmax variants of the "saturating" codes: the kernels move their exp2 offset only when a
# score code exceeds it by more than lazyc = min(floor(8 / (s_a2 log2e)), 255) codes and index the
# P table by c - m.  At s_a2 = 2^-6 lazyc is capped at 255 (the offset never moves after its first
# value) and at 2^-4 it is 88; a real checkpoint calibrates s_a2 to a few tenths.
#   "peaked": s_a2 = 2^-1, lazyc = 11;   "needle": s_a2 = 2^1, lazyc = 2 (near one-hot rows).
# s_out is not a power of two: with one-hot rows a power-of-two s_out puts o / s_out on exact ties
# that the fp32 and fp64 references resolve differently.
PEAKED_VARIANTS = ("peaked", "needle")
PEAKED_S_A2 = {"peaked": 2.0 ** -1, "needle": 2.0 ** 1}
PEAKED_LAZYC = {"peaked": 11, "needle": 2}
PEAKED_S_OUT = np.float32(0.0371)


def lazy_codes(s_a2):
    """lazyc of csrc/attention_q8_util.h (q8_ptab_lazy), in the kernel's fp32 arithmetic."""
    k2 = np.float32(s_a2) * np.float32(1.4426950408889634)
    return int(min(np.floor(np.float32(8.0) / k2), 255))


def offset_moves_after_row0(codes2, side, lazyc):
    """Replay of the lazy offset over the key rows of the second quantiser's codes ((n, L, L) int16
    tensors, L = side^2): how often m moves (a row max above m + lazyc) after the first key row."""
    moves = 0
    for t in codes2:
        rowmax = t.view(t.shape[0], t.shape[1], side, side).amax(-1).to(torch.int32)   # (n, L, key row)
        m = rowmax[..., 0].clone()
        for r in range(1, side):
            up = rowmax[..., r] > m + lazyc
            m = torch.where(up, rowmax[..., r], m)
            moves += int(up.sum())
    return moves


def exact_attn_inputs(b, h, w, heads, window, variant, seed, d):
    """``test_w8a8._exact_attn_inputs`` at head dim d, to be used with sm_scale = 2^-3 and
    s_qkv = 2^-5: q.k * scale = int * 2^-13 with |int| <= d * 2^14 (< 2^21 at d = 80), rel_h, rel_w =
    int * 2^-9 with |int| <= d * 2^10 (< 2^17) -- every score-side value is exact in fp32 in any
    summation order.  Variants "fine", "saturating", "peaked" and "needle" as there.
    Returns (qkv, bias, relh, relw, (s_qkv, s_a1, s_a2, s_out))."""
    c = heads * d
    side = window or h
    rng = np.random.Generator(np.random.PCG64(seed))
    relh = (rng.integers(-8, 9, (2 * side - 1, d)) * 2.0 ** -4).astype(np.float32)
    relw = (rng.integers(-8, 9, (2 * side - 1, d)) * 2.0 ** -4).astype(np.float32)
    s_qkv = np.float32(2.0 ** -5)
    kb = rng.integers(-40, 41, 3 * c).astype(np.float64)
    far = rng.random(3 * c) < 1.0 / 16
    kb[far] = rng.choice(np.array([-141.0, -130.0, -129.0, 128.0, 129.0, 140.0]), int(far.sum()))
    bias = ((2 * kb + 1) / 2 * 2.0 ** -5).astype(np.float32)
    if variant == "fine":
        qkv = rng.integers(-128, 128, (b, h, w, 3 * c), dtype=np.int8)
        qkv[..., :2 * c] = rng.integers(-16, 16, (b, h, w, 2 * c), dtype=np.int8)
        scales = (s_qkv, np.float32(2.0 ** -9), np.float32(2.0 ** -6), np.float32(2.0 ** -3 / side))
    else:
        assert variant in ("saturating",) + PEAKED_VARIANTS
        qkv = rng.integers(-128, 128, (b, h, w, 3 * c), dtype=np.int8)
        tok = qkv.reshape(b, h * w, 3 * c)
        tok[:, 0:3, :2 * c] = 127
        tok[:, 3:5, :2 * c] = -128
        scales = (s_qkv, np.float32(2.0 ** -6), np.float32(2.0 ** -4), np.float32(2.0 ** -6))
        if variant in PEAKED_VARIANTS:
            scales = (s_qkv, scales[1], np.float32(PEAKED_S_A2[variant]), PEAKED_S_OUT)
    return qkv, bias, relh, relw, scales


def q8_launch(cuda, qkv, bias, relh, relw, heads, window, sm_scale, scales, **kw):
    from samq import ops
    dev = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(cuda)
    return ops.rel_attention_q8(dev(qkv), dev(bias), dev(relh), dev(relw), heads, window, float(sm_scale),
                                *(float(s) for s in scales), **kw)
