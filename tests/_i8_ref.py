"""Exact inputs and a float64 numpy reference for the int8 GEMM tests (test_i8_gemm.py).

The kernels compute ``y = float(acc) * (a_scale * wscale[n]) + bias[n]`` in fp32 and feed it to an
epilogue.  ``problem()`` draws inputs on which every fp32 operation of that chain is EXACT, so a
correct kernel reproduces the float64 reference bit for bit:

* ``a_scale * wscale[n]`` (``csc``) is a power of two, the exponent varies from column to column;
  grouped W4 scales are per-group powers of two;
* ``bias[n]`` (and the fp32 residual of RESADD_F32) is an integer multiple of ``csc[n]`` and
  ``|acc + bias / csc + residual / csc| < 2^24``;
* ``out_scale``, ``mid_scale`` and ``res_scale`` are ``odd * 2^e`` (3, 5, 7): ``code * scale`` and the
  residual sum are exact and the quantiser's division is a true division, not a shift;
* most rows of A and most columns of W are drawn from a coarse grid (multiples of 16; W4: ``q - zp``
  a multiple of 4), which puts a large share of the quotients ``y / out_scale`` exactly on
  ``k + 0.5``; every 7th row and every 8th column is full range (-128 and 127 included), two rows
  are all 127 and two all -128;
* W4 zero-point nibbles cover 0..15 (column 7: nibble 0 under all-positive weights, column 15:
  nibble 15), weight nibbles 0 and 15 occur throughout.

Each problem carries two sets of output scales: "fine" (most quotients inside the code range) and
"sat" (a small out_scale: most quotients far beyond +-130).
"""
from __future__ import annotations

import functools
import math

import numpy as np

MAXM, MAXN = 1025, 1152
A_SCALE = np.float32(2.0 ** -6)
GELU_E = 2 * 7.1e-7          # twice the error csrc/common.h documents for gelu_r16_2

# per weight format: exponent of the largest wscale, coarse step of acc (16 * 16 / 16 * 4), and
# log2 of the "fine" scales relative to W8 (int4 weights are 8x smaller than int8 ones)
_FMT = {
    "w8": dict(e_w=-9, unit=256, shift=0),
    "w4": dict(e_w=-7, unit=64, shift=-1),
    "w4g": dict(e_w=-7, unit=64, shift=0),
}


def _p2(e):
    return np.float64(2.0) ** e


def pack_qweight(q: np.ndarray) -> np.ndarray:
    """uint8 nibbles (K, N) -> GPTQ qweight int32 (K/8, N): feature k in bits 4*(k%8) of word k//8."""
    q = q.astype(np.uint32)
    out = np.zeros((q.shape[0] // 8, q.shape[1]), np.uint32)
    for j in range(8):
        out |= q[j::8] << np.uint32(4 * j)
    return out.view(np.int32)


def pack_qzeros(nib: np.ndarray) -> np.ndarray:
    """zero-point nibbles (G, N) (zp = nibble + 1) -> GPTQ qzeros int32 (G, N/8)."""
    nib = nib.astype(np.uint32)
    out = np.zeros((nib.shape[0], nib.shape[1] // 8), np.uint32)
    for j in range(8):
        out |= nib[:, j::8] << np.uint32(4 * j)
    return out.view(np.int32)


def quant(x, s, lo=-128, half_even=True):
    """fq_vit's quantiser in float64: clamp(round_half_even(x / s), -128, 127)."""
    r = np.asarray(x, np.float64) / np.float64(s)
    r = np.rint(r) if half_even else np.sign(r) * np.floor(np.abs(r) + 0.5)
    return np.clip(r, lo, 127).astype(np.int8)


def quant32(x, s):
    """The same quantiser evaluated in fp32 (correctly rounded fp32 division)."""
    r = np.asarray(x, np.float32) / np.float32(s)
    return np.clip(np.rint(r), -128, 127).astype(np.int8)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(y):
    y = np.asarray(y, np.float64)
    return 0.5 * y * (1.0 + _erf(y / math.sqrt(2.0)))


def q8_res(y, r, mid, res, out, signed=True):
    """Q8_RES in float64: q(R * res_scale + fq(y, mid_scale), out_scale); mid <= 0: no mid quantiser."""
    x = np.asarray(y, np.float64)
    if mid > 0:
        x = quant(x, mid).astype(np.float64) * np.float64(mid)
    r = r.astype(np.float64) if signed else r.view(np.uint8).astype(np.float64)
    return quant(r * np.float64(res) + x, out)


class Problem:
    """One (format, K[, groupsize]) input set at MAXM x MAXN; tests slice rows [:M] and columns [:N]."""

    def __init__(self, fmt: str, k: int, group: int = 0):
        assert fmt in _FMT and k % 128 == 0 and (fmt == "w4g") == (group > 0)
        f = _FMT[fmt]
        self.fmt, self.k, self.group = fmt, k, group
        rng = np.random.Generator(np.random.PCG64([k, group, sorted(_FMT).index(fmt)]))
        rows, cols = np.arange(MAXM), np.arange(MAXN)
        self.row_full = rows % 7 == 3
        self.col_full = cols % 8 == 5
        a = (rng.integers(-8, 8, (MAXM, k)) * 16).astype(np.int8)
        a[self.row_full] = rng.integers(-128, 128, (int(self.row_full.sum()), k), dtype=np.int8)
        a[5:7] = 127
        a[8:10] = -128
        self.a = a
        self.a_scale = A_SCALE
        e_col = f["e_w"] - rng.integers(0, 3, MAXN)                 # wscale[n] = 2^e_col[n]
        nfull = int(self.col_full.sum())
        if fmt == "w8":
            w = (rng.integers(-8, 8, (MAXN, k)) * 16).astype(np.int8)
            w[self.col_full] = rng.integers(-128, 128, (nfull, k), dtype=np.int8)
            self.w = w                                              # [N, K], the nn.Linear layout
            self.wscale = _p2(e_col).astype(np.float32)
            acc = a.astype(np.float64) @ w.astype(np.float64).T
        else:
            g = group or k
            ng = (k + g - 1) // g
            gidx = np.arange(k) // g
            nib = rng.integers(0, 16, (ng, MAXN))
            nib[:, 7], nib[:, 15] = 0, 15
            zp = nib + 1
            q = (zp[gidx] % 4) + 4 * rng.integers(0, 4, (k, MAXN))  # q - zp a multiple of 4
            q[:, self.col_full] = rng.integers(0, 16, (k, nfull))
            q[:, 7] = rng.integers(1, 16, k)                        # all-positive weights, nibble 0
            assert q.min() == 0 and q.max() == 15
            self.q, self.zp = q.astype(np.uint8), zp
            self.qweight, self.qzeros = pack_qweight(self.q), pack_qzeros(nib)
            d = rng.integers(0, 2, (ng, MAXN))
            d -= d.min(0, keepdims=True)                            # the finest group scale is 2^e_col
            if fmt == "w4":
                d[:] = 0
            self.wscale = _p2(e_col[None, :] + d).astype(np.float32)   # (G, N)
            acc = np.zeros((MAXM, MAXN))
            self.acc_groups, self.d = [], d
            for gi in range(ng):                                    # zero points subtracted in integers
                ks = slice(gi * g, min(k, (gi + 1) * g))
                wg = q[ks].astype(np.int64) - zp[gi][None, :]
                self.acc_groups.append(a[:, ks].astype(np.float64) @ wg.astype(np.float64))
                acc += self.acc_groups[-1] * _p2(d[gi])[None, :]
            if fmt == "w4":
                self.wscale = self.wscale.reshape(-1)
        b_int = np.where(self.col_full, rng.integers(-5000, 5001, MAXN), f["unit"] * rng.integers(-12, 13, MAXN))
        self.acc, self.b_int = acc, b_int
        csc = np.float64(A_SCALE) * _p2(e_col)                      # a_scale * (finest) wscale[n]
        self.csc = csc
        self.bias = (b_int * csc).astype(np.float32)
        r_int = rng.integers(-2 ** 20, 2 ** 20, (MAXM, MAXN))
        self.res_f32 = (r_int * csc[None, :]).astype(np.float32)    # RESADD_F32 residual on the exact grid
        assert np.abs(acc + b_int[None, :]).max() + 2 ** 20 < 2 ** 24
        self.y = (acc + b_int[None, :]) * csc[None, :]              # float64, exact
        self.y_resadd = (acc + b_int[None, :] + r_int) * csc[None, :]
        self.res_i8 = rng.integers(-128, 128, (MAXM, MAXN), dtype=np.int8)
        self.rowsum_a = a.astype(np.int64).sum(1).astype(np.int32)
        s = f["shift"]
        self.scales = {
            "fine": dict(out=np.float32(3 * 2.0 ** (-6 + s)), mid=np.float32(5 * 2.0 ** (-7 + s)),
                         res=np.float32(7 * 2.0 ** (-8 + s)), out_res=np.float32(3 * 2.0 ** (-6 + s)),
                         out_gelu=np.float32(3 * 2.0 ** (-7 + s))),
            "sat": dict(out=np.float32(3 * 2.0 ** (-13 + s)), mid=np.float32(5 * 2.0 ** (-12 + s)),
                        res=np.float32(7 * 2.0 ** (-8 + s)), out_res=np.float32(3 * 2.0 ** (-12 + s)),
                        out_gelu=np.float32(3 * 2.0 ** (-13 + s))),
        }

    # ---- fp32 re-computations (what the kernel's arithmetic gives when every step is exact)
    def y32(self):
        csc = self.csc.astype(np.float32)[None, :]
        if self.fmt != "w4g":
            return self.acc.astype(np.float32) * csc + self.bias[None, :]
        facc = np.zeros((MAXM, MAXN), np.float32)       # the grouped kernel: f32 group accumulators
        for gi, ag in enumerate(self.acc_groups):
            facc = ag.astype(np.float32) * self.wscale[gi][None, :] + facc
        return facc * self.a_scale + self.bias[None, :]

    @functools.cached_property
    def gelu_y(self):
        return gelu(self.y)

    @functools.lru_cache(maxsize=None)
    def ref(self, what: str, variant: str = "fine"):
        """Full-size reference of one epilogue run: 'f32', 'resadd', 'f16', 'q8', 'q8_res',
        'q8_res_nomid' (mid_scale = 0), 'gelu' (float64 GELU(y), compared with a tolerance)."""
        sc = self.scales[variant]
        if what == "f32":
            return self.y.astype(np.float32)
        if what == "resadd":
            return self.y_resadd.astype(np.float32)
        if what == "f16":
            return self.y.astype(np.float16)
        if what == "q8":
            return quant(self.y, sc["out"])
        if what == "q8_res":
            return q8_res(self.y, self.res_i8, sc["mid"], sc["res"], sc["out_res"])
        if what == "q8_res_nomid":
            return q8_res(self.y, self.res_i8, 0.0, sc["res"], sc["out_res"])
        if what == "gelu":
            return self.gelu_y
        raise KeyError(what)


@functools.lru_cache(maxsize=None)
def problem(fmt: str, k: int, group: int = 0) -> Problem:
    return Problem(fmt, k, group)


def check_gelu_f16(got: np.ndarray, g: np.ndarray):
    """BIAS_GELU: fp16 outputs against float64 GELU(y).  An output may differ from float16(g) only by
    one fp16 step and only where g lies within GELU_E of the rounding boundary between the two.
    Returns (share differing, largest boundary distance among them, number of violations)."""
    ref = g.astype(np.float16)
    diff = got != ref
    if not diff.any():
        return 0.0, 0.0, 0
    go, rf, gd = got[diff], ref[diff], g[diff]
    one_step = go == np.nextafter(rf, go)
    dist = np.abs(gd - (go.astype(np.float64) + rf.astype(np.float64)) / 2)
    bad = ~one_step | (dist > GELU_E)
    return float(diff.mean()), float(dist[one_step].max()) if one_step.any() else float("inf"), int(bad.sum())


def check_gelu_q8(got: np.ndarray, g: np.ndarray, out_scale):
    """Q8_GELU: codes against float64 GELU(y).  A code may differ from the reference by one step and
    only where the reference quotient lies within GELU_E / out_scale plus two fp32 ulps of the
    quotient of the midpoint between the two codes.  Returns (share, largest distance in units of
    out_scale, violations)."""
    qt = g / np.float64(out_scale)
    ref = np.clip(np.rint(qt), -128, 127).astype(np.int64)
    gi = got.astype(np.int64)
    diff = gi != ref
    if not diff.any():
        return 0.0, 0.0, 0
    go, rf, qd = gi[diff], ref[diff], qt[diff]
    one_step = np.abs(go - rf) == 1
    dist = np.abs(qd - (go + rf) / 2.0)
    tol = GELU_E / np.float64(out_scale) + 2 * np.spacing(np.abs(qd).astype(np.float32)).astype(np.float64)
    bad = ~one_step | (dist > tol)
    return float(diff.mean()), float(dist[one_step].max()) if one_step.any() else float("inf"), int(bad.sum())
