"""CPU references for the kernels that take activation zero points (test_zp_kernels.py).

A quantiser is ``(scale, zp)``: ``code = clamp(rint(fl(fl(x / s) + zp)), -128, 127)``, value
``(code - zp) * s`` (fq_vit quantizer/uniform.py:23-45) -- the zero point joins the fp32 quotient
BEFORE the round-half-even.  ``quant32`` evaluates exactly that chain in fp32 (numpy's fp32 division
and addition are correctly rounded), ``quant64`` the same formula in float64; ``after=True`` is the
deliberately wrong ``rint(q) + zp`` the tests must be able to see.

The GEMM inputs are those of ``_i8_ref.problem("w8", K)`` (every fp32 step of the dequantisation
exact, a large share of exact-tie quotients), with one weight row made all positive so that
``zp_a * sum_k w`` is large against the sum itself, and an input zero point that is a multiple of 16
so that the offset stays on the problem's coarse grid and the ties survive.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import _i8_ref as R

F32 = np.float32


def quant32(x, s, zp, after=False):
    """The contract, step by step in fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.asarray(x).astype(F32) / F32(s)
        r = np.rint(q) + F32(zp) if after else np.rint(q + F32(zp))
    return np.clip(r, -128, 127).astype(np.int8)


def quant64(x, s, zp, after=False):
    q = np.asarray(x, np.float64) / np.float64(s)
    r = np.rint(q) + zp if after else np.rint(q + zp)
    return np.clip(r, -128, 127).astype(np.int8)


def fake32(codes, s, zp):
    return (codes.astype(F32) - F32(zp)) * F32(s)


# ----------------------------------------------------------------------------- quantiser operands
QUANT_ZPS = (-128, -37, 0, 5, 127)
QUANT_N = 4099
TIE_SCALE = F32(2.0 ** -4)


def quant_operands(dtype):
    """4099 values: every exact tie (k + 0.5) s for k in [-300, 299] (s = 2^-4: exact in fp32 and
    fp16), both saturated ends (+-40, +-1000, +-inf in fp32), +-0, and Gaussians over the code range."""
    rng = np.random.Generator(np.random.PCG64(41))
    ties = (np.arange(-300, 300) + 0.5) * float(TIE_SCALE)
    ends = [40.0, -40.0, 1000.0, -1000.0, 0.0, -0.0] + ([np.inf, -np.inf, 3e38, -3e38] if dtype == np.float32 else
                                                       [65504.0, -65504.0])
    rest = rng.standard_normal(QUANT_N - ties.size - len(ends)) * 6.0
    v = np.concatenate([ties, ends, rest]).astype(dtype)
    assert v.size == QUANT_N
    return v


# ----------------------------------------------------------------------------- LayerNorm
LN_ROWS = 37
LN_ZPS = (-128, -3, 0, 90)
LN_IN_SCALE = F32(3 * 2.0 ** -5)


@functools.lru_cache(maxsize=None)
def ln_problem(c: int):
    g = torch.Generator().manual_seed(7000 + c)
    codes = torch.randint(-128, 128, (LN_ROWS, c), generator=g).to(torch.int8)
    gamma = 1 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    return codes, gamma, beta


def ln64(codes, zp_in, gamma, beta, eps):
    """LayerNorm in float64 of the dequantised rows (code - zp_in) * in_scale."""
    x = (codes.double() - zp_in) * float(LN_IN_SCALE)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma.double(), beta.double(), eps).numpy()


# ----------------------------------------------------------------------------- GEMM
GEMM_M = 77
ZP_A, ZP_MID, ZP_RES, ZP_OUT = -48, -21, 11, 37      # distinct, non-zero; mid and out odd (ties)
RMOD = 13
POS_ROW = 3                                          # the all-positive weight row


class GemmProblem:
    """M = 77 rows of ``_i8_ref.problem('w8', k)`` with weight row 3 all positive; y is the exact
    float64 value of float(acc + col_offset) * csc + bias."""

    def __init__(self, k: int):
        p = R.problem("w8", k)
        self.p, self.k = p, k
        self.a = p.a[:GEMM_M]
        assert self.a.min() == -128 and self.a.max() == 127
        w = p.w.copy()
        w[POS_ROW] = np.maximum(np.abs(w[POS_ROW].astype(np.int16)), 16).clip(16, 112).astype(np.int8)
        assert (w[POS_ROW] > 0).all()
        self.w = w
        self.wsum = w.astype(np.int64).sum(1)
        self.acc = self.a.astype(np.float64) @ w.astype(np.float64).T          # sum a w, exact
        self.col_offset = (-ZP_A * self.wsum).astype(np.int32)
        assert abs(int(self.col_offset[POS_ROW])) > 2 * np.abs(self.acc[:, POS_ROW]).mean()
        self.res_i8 = p.res_i8[:GEMM_M]
        self.scales = p.scales["fine"]

    def y(self, col_offset=None):
        coff = self.col_offset if col_offset is None else col_offset
        tot = self.acc + coff.astype(np.float64)[None, :] + self.p.b_int[None, :]
        assert np.abs(tot).max() < 2 ** 24
        return tot * self.p.csc[None, :]

    def residual(self, rmod: int):
        return self.res_i8[np.arange(GEMM_M) % rmod] if rmod else self.res_i8


@functools.lru_cache(maxsize=None)
def gemm_problem(k: int) -> GemmProblem:
    return GemmProblem(k)


def q8_res(y, r, mid, res, out, zp_mid, zp_res, zp_out, after=False):
    """Q8_RES with zero points, every step in fp32 as the kernel takes it: the mid fake quantiser
    (mid > 0), the residual (r - zp_res) * res, their sum, the output quantiser."""
    x = np.asarray(y).astype(F32)
    if mid > 0:
        x = fake32(quant32(x, mid, zp_mid, after), mid, zp_mid)
    rv = (r.astype(F32) - F32(zp_res)) * F32(res)
    return quant32(rv + x, out, zp_out, after)


def check_gelu_q8_zp(got, g, out_scale, zp):
    """Q8_GELU under a zero point, by the rule of ``_i8_ref.check_gelu_q8``: a code may differ from
    clamp(rint(g / s + zp)) by one step, and only where g / s + zp lies within
    GELU_E / s + 2 ulp32(|g / s|) + ulp32(|g / s + zp|) of the midpoint between the two codes -- the
    documented error of the approximate GELU, the reciprocal-multiply quotient (<= 1.5 ulp) and the
    one fp32 rounding of the sum.  Returns (share differing, violations)."""
    q = g / np.float64(out_scale)
    t = q + zp
    ref = np.clip(np.rint(t), -128, 127).astype(np.int64)
    gi = got.astype(np.int64)
    diff = gi != ref
    if not diff.any():
        return 0.0, 0
    go, rf, td, qd = gi[diff], ref[diff], t[diff], q[diff]
    tol = (R.GELU_E / np.float64(out_scale) + 2 * np.spacing(np.abs(qd).astype(F32)).astype(np.float64) +
           np.spacing(np.abs(td).astype(F32)).astype(np.float64))
    bad = (np.abs(go - rf) != 1) | (np.abs(td - (go + rf) / 2.0) > tol)
    return float(diff.mean()), int(bad.sum())


# ----------------------------------------------------------------------------- convolutions
def conv_problem(mode: int, b: int, cin: int, side: int, n: int):
    """Exact conv inputs by the rules of ``_i8_ref``: codes mostly multiples of 16 with full-range
    channels, a_scale * wscale[n] a power of two, bias an integer multiple of it."""
    rng = np.random.Generator(np.random.PCG64([mode, b, cin, side, 99]))
    g = side // 16 if mode == 1 else side
    x = (rng.integers(-8, 8, (b, cin, side, side)) * 16).astype(np.int8)
    x[:, ::3, ::5] = rng.integers(-128, 128, x[:, ::3, ::5].shape, dtype=np.int8)
    kk = 16 if mode == 1 else 3
    w = (rng.integers(-8, 8, (n, cin, kk, kk)) * 16).astype(np.int8)
    w[5::8] = rng.integers(-128, 128, w[5::8].shape, dtype=np.int8)
    w[POS_ROW] = np.maximum(np.abs(w[POS_ROW].astype(np.int16)), 16).clip(16, 112).astype(np.int8)
    e_col = -9 - rng.integers(0, 3, n)
    csc = np.float64(R.A_SCALE) * np.float64(2.0) ** e_col
    b_int = 256 * rng.integers(-12, 13, n)
    pos = rng.integers(-128, 128, (g * g, n), dtype=np.int8)
    return x, w, (np.float64(2.0) ** e_col).astype(F32), b_int, csc, pos, g


def conv_acc(x, w, mode: int, zp_a: int, pad_code=None):
    """sum (x - zp_a) w of the convolution in float64, (B, G, G, N).  ``pad_code``: the code the
    padding holds (default zp_a: a padded 0.0); mode 1 has no padding."""
    import torch.nn.functional as F
    xt, wt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64))
    if mode == 1:
        return F.conv2d(xt - zp_a, wt, stride=16).permute(0, 2, 3, 1).numpy()
    pad = zp_a if pad_code is None else pad_code
    xp = F.pad(xt, (1, 1, 1, 1), value=float(pad))
    return F.conv2d(xp - zp_a, wt).permute(0, 2, 3, 1).numpy()


def im2col(x, mode: int, pad_code: int):
    """The explicit A matrix of the implicit GEMM: mode 1 rows (b, gy, gx) x (c, kh, kw) of NCHW x;
    mode 2 rows x (ky, kx, c) of the map padded with ``pad_code`` (x NCHW here too)."""
    b, cin, side, _ = x.shape
    if mode == 1:
        g = side // 16
        t = x.reshape(b, cin, g, 16, g, 16).transpose(0, 2, 4, 1, 3, 5)
        return np.ascontiguousarray(t.reshape(b * g * g, cin * 256))
    g = side
    xp = np.full((b, g + 2, g + 2, cin), pad_code, np.int8)
    xp[:, 1:-1, 1:-1] = x.transpose(0, 2, 3, 1)
    cols = [xp[:, ky:ky + g, kx:kx + g, :] for ky in range(3) for kx in range(3)]
    return np.ascontiguousarray(np.concatenate(cols, axis=-1).reshape(b * g * g, 9 * cin))
