"""Seeded inputs and float64 / integer numpy restatements for the Power-of-Two Factor tests (test_ptf.py,
golden/make_golden_ptf.py).

A PTF quantiser is ``(s0, zp, exp[C])``: channel c has the scale ``s0 * 2^exp[c]``, exp in 0..3, and the
layer's one zero point (fq_vit observer/ptf.py).  The GEMM problems here are exact: small-integer
weights, power-of-two scales, biases on the same grid, so that every fp32 step of the kernel's
epilogue is exact and the codes are fixed bit for bit, exact .5 ties included.
"""
from __future__ import annotations

import numpy as np
import torch

F32 = np.float32

# ----------------------------------------------------------------------------- observer cases
# name -> (shape, permute, seed); three calibration tensors each
OBSERVER_CASES = {
    "act3d": ((3, 50, 128), True, 101),
    "nhwc": ((1, 6, 5, 64), False, 202),
    "nchw": ((2, 64, 4, 4), True, 303),
}
BIT_TYPES = {"int8": (-128, 127), "uint8": (0, 255)}
MIN_GAP = 1e-6     # the bound test_observers_calib.py uses for omse


# the calibrated model of the fixture: weights from oracle.synth (fp16-rounded), seeded images
MODEL = dict(name="vit_b", depth=2, global_attn_indexes=(1,), img_size=256, seed=3, calib_seeds=(11, 12, 13),
             test_seed=14)


def model_state(synth):
    cfg = synth.encoder_config(MODEL["name"], depth=MODEL["depth"], global_attn_indexes=MODEL["global_attn_indexes"],
                               img_size=MODEL["img_size"])
    return {k: torch.from_numpy(v.astype(np.float16).astype(np.float32))
            for k, v in synth.make_encoder_state(cfg, seed=MODEL["seed"]).items()}


def observer_inputs(case: str):
    """Three f32 tensors of the case's shape: Gaussians whose spread varies by channel over 2^0..2^-4 (so
    that all four factors are picked), a channel-dependent offset, a few outliers."""
    shape, permute, seed = OBSERVER_CASES[case]
    g = torch.Generator().manual_seed(seed)
    cdim = 1 if (len(shape) == 4 and permute) else len(shape) - 1
    c = shape[cdim]
    view = [1] * len(shape)
    view[cdim] = c
    spread = (2.0 ** -(torch.arange(c) % 5).float()).reshape(view)
    offset = (0.3 * torch.randn(c, generator=g)).reshape(view)
    out = []
    for _ in range(3):
        x = torch.randn(shape, generator=g) * spread + offset * spread
        flat = x.reshape(-1)
        flat[torch.randint(0, flat.numel(), (4,), generator=g)] *= 2.5
        out.append(x.contiguous())
    return out


def channel_last(x: torch.Tensor, permute: bool) -> torch.Tensor:
    if x.dim() == 4 and permute:
        x = x.permute(0, 2, 3, 1)
    return x.reshape(-1, x.shape[-1]).contiguous()


def scores64(x2d, s1, zp, qmin, qmax):
    """[C, 4] float64 sums over the rows of the f32 terms (x - fq_k(x))^2, scales s1 * 2^k: each f32 step
    rounded separately (numpy), the sum in float64."""
    x = np.asarray(x2d).astype(F32)
    out = np.empty((x.shape[1], 4), np.float64)
    for k in range(4):
        s = F32(s1) * F32(2.0 ** k)
        q = np.clip(np.rint(x / s + F32(zp)), F32(qmin), F32(qmax)).astype(F32)
        xq = (q - F32(zp)) * s
        d = x - xq
        out[:, k] = (d * d).astype(np.float64).sum(0)
    return out


# ----------------------------------------------------------------------------- quantiser / LayerNorm
def quant_cols(x, s, zp, exp=None):
    """clamp(rint(x / (s * 2^exp[n]) + zp), -128, 127) in float64, exp per column (None = 0)."""
    sc = np.float64(s) * (1.0 if exp is None else 2.0 ** np.asarray(exp, np.float64)[None, :])
    return np.clip(np.rint(np.asarray(x, np.float64) / sc + zp), -128, 127).astype(np.int64)


def ln64_ptf(codes, zp_in, in_scale, exp, gamma, beta, eps):
    """LayerNorm in float64 of the rows ((code - zp_in) << exp[c]) * in_scale."""
    x = (codes.double() - zp_in) * (2.0 ** exp.double())[None, :] * float(in_scale)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma.double(), beta.double(), eps).numpy()


def exp_pattern(n: int, kind: str, seed: int = 0):
    """uint8 [n] exponents: 'mixed' all four values inside every 16-column group, 'zero', 'e<k>' one value."""
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind.startswith("e"):
        return np.full(n, int(kind[1:]), np.uint8)
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    e = rng.integers(0, 4, n).astype(np.uint8)
    for g0 in range(0, n, 16):
        e[g0:g0 + 4] = rng.permutation(4)
    return e


# ----------------------------------------------------------------------------- GEMM epilogues
A_SCALE, W_SCALE = 2.0 ** -4, 2.0 ** -4          # csc = 2^-8 on every column
OUT_SCALE, MID_SCALE, RES_SCALE = 2.0 ** -5, 2.0 ** -6, 2.0 ** -6
ZP_A, ZP_MID, ZP_RES, ZP_OUT = -47, -21, 11, 37  # odd: exact ties round differently under them
RMOD = 13


class EpiProblem:
    """a int8 [m, k] full range; w [n, k] with eight non-zero small integers per row (row 3 all positive on
    its support); bias an integer multiple of csc.  y = (acc + col_offset) * csc + bias is exact in fp32."""

    def __init__(self, m, n, k, seed=0):
        rng = np.random.Generator(np.random.PCG64([m, n, k, seed, 77]))
        self.m, self.n, self.k = m, n, k
        self.a = rng.integers(-128, 128, (m, k), dtype=np.int8)
        w = np.zeros((n, k), np.int8)
        for r in range(n):
            idx = rng.choice(k, 8, replace=False)
            w[r, idx] = rng.choice([-3, -2, -1, 1, 2, 3], 8)
        w[3] = np.abs(w[3])
        self.w = w
        self.csc = A_SCALE * W_SCALE
        self.wscale = np.full(n, W_SCALE, F32)
        self.b_int = 4 * rng.integers(-40, 41, n)
        self.bias = (self.b_int * self.csc).astype(F32)
        self.acc = self.a.astype(np.int64) @ w.astype(np.int64).T
        self.col_offset = (-ZP_A * w.astype(np.int64).sum(1)).astype(np.int32)
        self.res = rng.integers(-128, 128, (max(m, RMOD), n), dtype=np.int8)

    def y(self):
        tot = self.acc + self.col_offset.astype(np.int64)[None, :] + self.b_int[None, :]
        assert np.abs(tot).max() < 2 ** 24
        return tot.astype(np.float64) * self.csc

    def q8(self, out_exp=None):
        return quant_cols(self.y(), OUT_SCALE, ZP_OUT, out_exp)

    def q8_res(self, mid, rmod, out_exp=None, res_exp=None):
        x = self.y()
        if mid:
            x = (quant_cols(x, MID_SCALE, ZP_MID) - ZP_MID) * MID_SCALE
        r = self.res[np.arange(self.m) % rmod] if rmod else self.res[:self.m]
        re = 1.0 if res_exp is None else 2.0 ** np.asarray(res_exp, np.float64)[None, :]
        rv = (r.astype(np.float64) - ZP_RES) * re * RES_SCALE
        tot = rv + x
        assert np.array_equal(tot.astype(F32).astype(np.float64), tot)   # exact in fp32 as well
        return quant_cols(tot, OUT_SCALE, ZP_OUT, out_exp)


def gelu64(y):
    import math
    v = np.vectorize(math.erf)(np.asarray(y, np.float64) / math.sqrt(2.0))
    return 0.5 * y * (1.0 + v)


# ----------------------------------------------------------------------------- replay GEMM
def replay_problem(m, n, ka, levels, z_a, seed=0):
    """Worst-case magnitudes: codes in {-128, -127, 127} and full range, weights +-127 with row 3 all +127,
    every channel but one on the largest exponent.  Returns a, w, exp[ka] and the int64 sums
    sum_k (a_k - z_a) 2^exp[k] w[n, k]."""
    rng = np.random.Generator(np.random.PCG64([m, n, ka, len(levels), z_a + 128, seed]))
    a = rng.integers(-128, 128, (m, ka), dtype=np.int8)
    a[0] = -128 if z_a > 0 else 127                  # |a - z_a| = 255 on a whole row
    if m > 1:
        a[1] = rng.choice(np.array([-128, -127, 127], np.int8), ka)
    w = rng.choice(np.array([-127, 127], np.int8), (n, ka))
    w[3] = 127
    w[5] = -127
    e = np.full(ka, max(levels), np.uint8)
    e[7] = 0
    for i, lv in enumerate(sorted(levels)):
        e[11 + 5 * i::17][:3] = lv
    assert set(np.unique(e).tolist()) == set(levels) | {0}
    tot = (a.astype(np.int64) - z_a) * (2 ** e.astype(np.int64))[None, :] @ w.astype(np.int64).T
    assert np.abs(tot).max() < 2 ** 31
    return a, w, e, tot
