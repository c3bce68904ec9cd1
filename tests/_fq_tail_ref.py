"""numpy float64 restatements of the three fused stages of the fq_vit W8A8 mask decoder tail
(``csrc/decoder_tail.hip``), from input codes to output codes, for ``test_fq_decoder_tail.py``.

Every function returns ``{name: codes}`` and ``{name: pre-rounding quotient}`` (float64): a position
whose quotient lies within ``TIE_EPS`` of a half-integer may round either way in fp32 and is left out
of equality checks (``near_tie``).  Each quantiser's restatement takes the codes of the one before it
as an optional argument, so a stage can be checked from the kernel's own input codes."""
from __future__ import annotations

import math

import numpy as np

TIE_EPS = 1e-3


def q8(x, s):
    """(codes, quotient) of UniformQuantizer (zero point 0, int8): round half to even, clamp."""
    quot = np.asarray(x, np.float64) / float(s)
    return np.clip(np.rint(quot), -128, 127), quot


def near_tie(quot):
    return np.abs(np.abs(quot - np.floor(quot)) - 0.5) < TIE_EPS


def gelu_codes(codes, s):
    """GELU (erf form) of the fake-quant values codes * s, through the 256-entry table of the codes."""
    v = np.arange(-128, 128, dtype=np.float64) * float(s)
    table = np.array([0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0))) for x in v])
    return table[np.asarray(codes, np.int64) + 128]


def convt_k2s2(x, weight):
    """x (B, h, w, Cin) NHWC, weight (Cin, Cout, 2, 2) as nn.ConvTranspose2d -> (B, 2h, 2w, Cout)."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    b, h, w, _ = x.shape
    y = np.einsum("byxi,iokl->bykxlo", x, weight)
    return y.reshape(b, 2 * h, 2 * w, weight.shape[1])


def upscale0_ref(x, s_in, weight, bias, gamma, beta, eps, s0, s1, s2, c0=None, c1=None):
    """convT 256 -> 64 + qacts[0] | LayerNorm2D + qacts[1] | GELU + qacts[2].  x (B, h, w, Cin) codes."""
    codes, quot = {}, {}
    y = convt_k2s2(np.asarray(x, np.float64) * float(s_in), weight) + np.asarray(bias, np.float64)
    codes["q0"], quot["q0"] = q8(y, s0)
    v = (codes["q0"] if c0 is None else np.asarray(c0, np.float64)) * float(s0)
    u = v.mean(-1, keepdims=True)
    var = ((v - u) ** 2).mean(-1, keepdims=True)
    y = (v - u) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    codes["q1"], quot["q1"] = q8(y, s1)
    codes["q2"], quot["q2"] = q8(gelu_codes(codes["q1"] if c1 is None else c1, s1), s2)
    return codes, quot


def upscale1_masks_ref(x, s_in, weight, bias, hyper, s_hyper, s3, s4, s_q1, c3=None, c4=None):
    """convT 64 -> 32 + qacts[3] | GELU + qacts[4] | hyper_in @ x + qact1.  x (B, H, W, Cin) codes,
    hyper (B, M, 32) codes with scales s_hyper (M,).  ``masks`` (B, M, 2H, 2W)."""
    codes, quot = {}, {}
    y = convt_k2s2(np.asarray(x, np.float64) * float(s_in), weight) + np.asarray(bias, np.float64)
    codes["q3"], quot["q3"] = q8(y, s3)
    codes["q4"], quot["q4"] = q8(gelu_codes(codes["q3"] if c3 is None else c3, s3), s4)
    x4 = np.asarray(codes["q4"] if c4 is None else c4, np.int64)
    dot = np.einsum("bmc,byxc->bmyx", np.asarray(hyper, np.int64), x4)        # exact integers
    sc = np.asarray(s_hyper, np.float32).astype(np.float64)[None, :, None, None] * float(s4)
    codes["masks"], quot["masks"] = q8(dot.astype(np.float64) * sc, s_q1)
    return codes, quot


def mlp_ref(x, s_in, layers, s1, s2, s3):
    """One 3-layer MLP on codes x (B, C): layers = [(weight codes (N, K), s_w, bias (N,))] * 3, s1 / s2 the
    scales of qacts1 / qacts2 of the two hidden layers.  Names: ``q1.<i>``, ``q2.<i>`` (i = 0, 1), ``q3``."""
    codes, quot = {}, {}
    c, s = np.asarray(x, np.int64), float(s_in)
    for i, (w, s_w, bias) in enumerate(layers):
        acc = (c @ np.asarray(w, np.int64).T).astype(np.float64)
        y = acc * (s * float(s_w)) + np.asarray(bias, np.float64)
        if i < 2:
            codes[f"q1.{i}"], quot[f"q1.{i}"] = q8(y, s1[i])
            r = np.maximum(codes[f"q1.{i}"], 0.0) * float(s1[i])
            codes[f"q2.{i}"], quot[f"q2.{i}"] = q8(r, s2[i])
            c, s = codes[f"q2.{i}"].astype(np.int64), float(s2[i])
        else:
            codes["q3"], quot["q3"] = q8(y, s3)
    return codes, quot


def compare(out, ref, quot, what=""):
    """(max |dcode|, share of codes that differ, share of near-tie positions, differing codes outside
    the near-tie set) of kernel codes against a restatement."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    d = np.abs(out - ref)
    tie = near_tie(quot)
    return float(d.max()), float((d > 0).mean()), float(tie.mean()), int(((d > 0) & ~tie).sum())
