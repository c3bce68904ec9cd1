"""CPU reference of the W8A8 attention on codes with zero points (test_attn_zp.py): the fq_vit
Attention core of ``test_w8a8._attn_ref`` with every QAct a quantiser (scale, zp),
``code = clamp(round(x / s + zp), -128, 127)``, value ``(code - zp) * s``.

``wrong`` selects a deliberately wrong variant, to show what the test inputs can see:
  "after"  the zero points added after the rounding (round(x / s) + zp);
  "ksum"   the key-sum term of sum (q - z)(k - z) = q.k - z (qsum + ksum) + D z^2 dropped;
  "qsum"   the query-sum term dropped;
  "pad0"   pad tokens carry the code 0 instead of the code of their value.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import sam_ref

ZP_SETS = ((23, -9, 17, -31), (-19, 40, -60, 75))       # (qkv, a1, a2, out)
Q8_SCALES = (np.float32(0.02), np.float32(2.0 / 127.5), np.float32(6.0 / 127.5), np.float32(2.6 / 127.5))


def _codes(x, s, z, after=False):
    r = x / s
    r = torch.round(r) + z if after else torch.round(r + z)
    return torch.clamp(r, -128, 127)


def attn_ref_zp(qkv_codes, bias, relh, relw, heads, window, scales, zps, dtype=torch.float32, wrong=None,
                sm_scale=None, codes1=None):
    """Output codes (B, H, W, C) as a float array.  ``codes1``: a list that receives the share of the
    first score quantiser's codes that sit on a clamp end."""
    s_qkv, s1, s2, s_o = scales
    z, z1, z2, z_o = (float(v) for v in zps)
    after = wrong == "after"
    b, h, w, c3 = qkv_codes.shape
    c = c3 // 3
    d = c // heads
    sm = d ** -0.5 if sm_scale is None else sm_scale
    ts = lambda s: torch.tensor(float(s), dtype=dtype)
    full = torch.from_numpy(qkv_codes.astype(np.float32)).to(dtype)
    hp, wp = h, w
    if window > 0:
        bv = torch.from_numpy(bias).to(dtype) if bias is not None else torch.zeros(c3, dtype=dtype)
        pad = torch.zeros(c3, dtype=dtype) if wrong == "pad0" else _codes(bv, ts(s_qkv), z, after)
        hp, wp = -(-h // window) * window, -(-w // window) * window
        padded = pad.expand(b, hp, wp, c3).clone()
        padded[:, :h, :w] = full
        full, _ = sam_ref.window_partition(padded, window)
    bq, hh, ww, _ = full.shape
    n, ll = bq * heads, hh * ww
    t = full.reshape(bq, ll, 3, heads, d).permute(2, 0, 3, 1, 4)
    qc, kc, vc = t.reshape(3, n, ll, d).unbind(0)
    q, k, v = (qc - z) * ts(s_qkv), (kc - z) * ts(s_qkv), (vc - z) * ts(s_qkv)
    rph, rpw = torch.from_numpy(relh).to(dtype), torch.from_numpy(relw).to(dtype)
    o = torch.empty((n, ll, d), dtype=dtype)
    step = max(1, (1 << 24) // (ll * ll))
    for i in range(0, n, step):
        qi, ki, vi = q[i:i + step], k[i:i + step], v[i:i + step]
        m = qi.shape[0]
        sc = (qi * sm) @ ki.transpose(-2, -1)
        unit = ts(s_qkv) * ts(s_qkv) * sm
        if wrong == "ksum":      # q.k - z qsum + D z^2: the -z ksum term missing
            sc = sc + z * kc[i:i + step].sum(-1)[:, None, :] * unit
        elif wrong == "qsum":
            sc = sc + z * qc[i:i + step].sum(-1)[:, :, None] * unit
        c1 = _codes(sc, ts(s1), z1, after)
        if codes1 is not None:
            codes1.append(float(((c1 == -128) | (c1 == 127)).float().mean()))
        sc = (c1 - z1) * ts(s1)
        rh, rw = sam_ref.rel_bias(qi.reshape(m, hh, ww, d), rph, rpw, hh, ww)
        sc = (sc.view(m, hh, ww, hh, ww) + rh[..., :, None] + rw[..., None, :]).view(m, ll, ll)
        sc = (_codes(sc, ts(s2), z2, after) - z2) * ts(s2)
        o[i:i + step] = torch.softmax(sc, -1) @ vi
    o = o.view(bq, heads, hh, ww, d).permute(0, 2, 3, 1, 4).reshape(bq, hh, ww, c)
    if window > 0:
        o = sam_ref.window_unpartition(o, window, (hp, wp), (h, w))
    return _codes(o, ts(s_o), z_o, after).numpy()


def inputs(b, h, w, heads, d, window, zp_qkv, seed):
    """``test_w8a8._q8_inputs`` at head dim d with codes zp_qkv + U[-105, 104] (no value clips),
    N(0, 0.5) tables, N(0, 0.3) bias."""
    c = heads * d
    rng = np.random.Generator(np.random.PCG64([seed, d, zp_qkv & 0xFF]))
    qkv = (zp_qkv + rng.integers(-105, 105, (b, h, w, 3 * c))).astype(np.int8)
    side = window or h
    relh = (rng.standard_normal((2 * side - 1, d), dtype=np.float32) * 0.5).astype(np.float32)
    relw = (rng.standard_normal((2 * side - 1, d), dtype=np.float32) * 0.5).astype(np.float32)
    bias = (rng.standard_normal(3 * c, dtype=np.float32) * 0.3).astype(np.float32)
    return qkv, bias, relh, relw


EXACT_ZPS = (23, -9, 17, -31)          # all odd: every exact tie rounds differently with the zp added late


def exact_inputs(b, h, w, heads, window, seed):
    """The "fine" variant of ``test_w8a8._exact_attn_inputs`` shifted by the zero point: d = 64,
    sm_scale = 2^-3, s_qkv = 2^-5, q / k codes zp + [-16, 16), v codes zp + U[-105, 104], tables
    integers / 16, bias half-integers * s_qkv (pad codes on ties; a few beyond the clamp), s_a1 = 2^-9,
    s_a2 = 2^-6, s_out = 2^-3 / S: every score-side value is exact in fp32 in any order, 1/16 of the
    first quantiser's arguments and 1/8 of the second's are exact ties."""
    d, z = 64, EXACT_ZPS[0]
    c = heads * d
    side = window or h
    rng = np.random.Generator(np.random.PCG64([seed, 4242]))
    relh = (rng.integers(-8, 9, (2 * side - 1, d)) * 2.0 ** -4).astype(np.float32)
    relw = (rng.integers(-8, 9, (2 * side - 1, d)) * 2.0 ** -4).astype(np.float32)
    s_qkv = np.float32(2.0 ** -5)
    kb = rng.integers(-40, 41, 3 * c).astype(np.float64)
    far = rng.random(3 * c) < 1.0 / 16
    kb[far] = rng.choice(np.array([-170.0, -160.0, 120.0, 140.0]), int(far.sum()))
    bias = ((2 * kb + 1) / 2 * 2.0 ** -5).astype(np.float32)
    qkv = (z + rng.integers(-105, 105, (b, h, w, 3 * c))).astype(np.int8)
    qkv[..., :2 * c] = (z + rng.integers(-16, 16, (b, h, w, 2 * c))).astype(np.int8)
    scales = (s_qkv, np.float32(2.0 ** -9), np.float32(2.0 ** -6), np.float32(2.0 ** -3 / side))
    return qkv, bias, relh, relw, scales
