"""Exact inputs and a float64 numpy reference for the W4A16 GEMM tests (test_w4a16_gemm.py).

The kernels multiply fp16 A by the exact integers ``q - zp`` and accumulate in fp32.  Per channel
the epilogue is ``fma(acc, s[n], b[n])`` in fp32; grouped, the weight is ``fp16((q - zp) * s[g, n])``
and the epilogue scale is 1.  Then one conversion to f16, or a store / add in f32.  ``problem()``
draws inputs on which every one of those operations is EXACT in any summation order, so a correct
kernel reproduces the float64 reference bit for bit:

* A holds fp16 integer multiples of 2^-3, ``|A| <= amax * 2^-3`` (amax = 64; 32 for K > 640): most
  rows from a coarse grid (multiples of 2^0), every 7th row full range, rows 5, 6 all ``+amax`` and
  rows 8, 9 all ``-amax``; no value is an fp16 subnormal;
* weight nibbles: most columns coarse (``q - zp`` a multiple of 4), every 8th column full range;
  zero-point nibbles cover 0..15; columns 7 + 64 j hold nibble 0 (zp = 1) under all-positive
  weights, columns 15 + 64 j nibble 15 (zp = 16); nibbles 0 and 15 occur throughout;
* ``scales`` are fp16 powers of two, 2^-9 .. 2^-11 per column (the column's finest scale
  ``2^e_col[n]``), grouped 2^0 .. 2^2 times that per group: ``16 * s`` and ``s`` itself are normal;
* the column quantum is ``qn[n] = 2^-3 * 2^e_col[n] >= 2^-14``: every partial sum, ``bias[n]``
  (``m * 2^p`` quanta, ``|m| <= 2047``: 11 significant bits, exact in fp16), the fp32 residual and
  every output is an integer multiple of it, ``|acc + bias + residual| < 2^21`` quanta (far below
  2^24) and ``|y| < 512``; a non-zero output is never an fp16 subnormal.
"""
from __future__ import annotations

import functools

import numpy as np

from _i8_ref import gelu, pack_qweight, pack_qzeros   # noqa: F401  (re-exported)

MAXM, MAXN = 1025, 1152
GELU_E = 2 * 3.3e-7          # twice the error csrc/common.h documents for gelu_fast
E_S = -9                     # exponent of the largest per-column (finest group) scale


def _p2(e):
    return np.float64(2.0) ** e


class Problem:
    """One (K, groupsize) input set at m x n; tests slice rows [:M] and columns [:N].
    ``group`` 0 = per channel; otherwise ``ceil(K / group)`` scale / zero rows (ragged last group)."""

    def __init__(self, k: int, group: int = 0, m: int = MAXM, n: int = MAXN):
        assert k % 64 == 0 and group % 64 == 0 and n % 64 == 0
        self.k, self.group, self.m, self.n = k, group, m, n
        rng = np.random.Generator(np.random.PCG64([k, group, m, n]))
        self.amax = amax = 64 if k <= 640 else 32
        cols = np.arange(n)
        self.row_full = np.arange(m) % 7 == 3
        self.col_full = cols % 8 == 5
        a = rng.integers(-amax // 8, amax // 8 + 1, (m, k)) * 8
        a[self.row_full] = rng.integers(-amax, amax + 1, (int(self.row_full.sum()), k))
        a[5:7] = amax
        a[8:10] = -amax
        self.a_int = a
        self.a = (a * 0.125).astype(np.float16)
        g = group or k
        self.ng = ng = (k + g - 1) // g
        self.gidx = gidx = np.arange(k) // g
        nib = rng.integers(0, 16, (ng, n))
        nib[:, 7::64], nib[:, 15::64] = 0, 15
        self.nib, self.zp = nib, nib + 1
        q = (self.zp[gidx] % 4) + 4 * rng.integers(0, 4, (k, n))      # q - zp a multiple of 4
        nfull = int(self.col_full.sum())
        q[:, self.col_full] = rng.integers(0, 16, (k, nfull))
        q[:, 7::64] = rng.integers(1, 16, (k, len(cols[7::64])))       # all-positive weights, nibble 0
        assert q.min() == 0 and q.max() == 15
        self.q = q.astype(np.uint8)
        self.qweight, self.qzeros = pack_qweight(self.q), pack_qzeros(nib)
        self.e_col = E_S - rng.integers(0, 3, n)
        d = rng.integers(0, 3, (ng, n))
        d -= d.min(0, keepdims=True)                                   # the finest group scale is 2^e_col
        self.d = d
        sc = _p2(self.e_col[None, :] + d).astype(np.float16)           # (G, N)
        self.scales = sc if group else sc.reshape(-1)
        self.qn = _p2(self.e_col - 3)                                  # the column quantum, float64
        self.b_int = rng.integers(-2047, 2048, n) * 2 ** rng.integers(0, 6, n)
        self.bias = (self.b_int * self.qn).astype(np.float16)
        assert np.array_equal(self.bias.astype(np.float64), self.b_int * self.qn)
        self.acc = self.acc_of(self.a_int, self.q, self.zp, d)        # quanta, exact integers in float64
        self.y = (self.acc + self.b_int[None, :]) * self.qn[None, :]

    # ---- the reference sum in quanta for (possibly mutated) operands
    def w_int(self, q, zp, d, gidx=None):
        gidx = self.gidx if gidx is None else gidx
        return (q.astype(np.int64) - zp[gidx]) * 2 ** d[gidx]

    def acc_of(self, a_int, q, zp, d, gidx=None):
        return a_int.astype(np.float64) @ self.w_int(q, zp, d, gidx).astype(np.float64)

    @functools.cached_property
    def r_int(self):
        rng = np.random.Generator(np.random.PCG64([self.k, self.group, 99]))
        return rng.integers(-2 ** 18, 2 ** 18, (self.m, self.n))

    @functools.cached_property
    def res_f32(self):
        """RESADD_F32 residual: an fp32 multiple of the column quantum."""
        return (self.r_int * self.qn[None, :]).astype(np.float32)

    @functools.cached_property
    def y_resadd(self):
        return (self.acc + self.b_int[None, :] + self.r_int) * self.qn[None, :]

    @functools.cached_property
    def gelu_y(self):
        return gelu(self.y)

    @functools.lru_cache(maxsize=None)
    def ref(self, what: str):
        """'f32', 'resadd' (fp32), 'f16' (= float16(y)), 'gelu' (float64 GELU(y), compared with a tolerance)."""
        if what == "f32":
            return self.y.astype(np.float32)
        if what == "resadd":
            return self.y_resadd.astype(np.float32)
        if what == "f16":
            return self.y.astype(np.float16)
        if what == "gelu":
            return self.gelu_y
        raise KeyError(what)

    # ---- fp32 re-computations (what the kernels' arithmetic gives when every step is exact)
    def w_mfma(self, ks: slice):
        """The B operand the MFMA sees for K rows ks (all of one group), as fp32: per channel the
        integers q - zp, grouped fp16((q - zp) * s[g, n]) computed in fp16."""
        gi = int(self.gidx[ks.start])
        assert gi == int(self.gidx[ks.stop - 1])
        w16 = self.q[ks].astype(np.float16) - self.zp[gi].astype(np.float16)[None, :]
        if self.group:
            w16 = w16 * self.scales[gi][None, :]
        return w16.astype(np.float32)

    def acc32(self, order: str):
        """The fp32 accumulator: one fp32 matrix product per 64-deep K tile, added in 'forward' or
        'reverse' tile order, or ('group') one product per group."""
        a32 = self.a.astype(np.float32)
        step = (self.group or self.k) if order == "group" else 64
        parts = [slice(k0, min(self.k, k0 + step)) for k0 in range(0, self.k, step)]
        acc = np.zeros((self.m, self.n), np.float32)
        for ks in (reversed(parts) if order == "reverse" else parts):
            acc = a32[:, ks] @ self.w_mfma(ks) + acc
        return acc

    def y32(self, acc32, fused: bool):
        """The fp32 epilogue on an fp32 accumulator: fma(acc, s[n], b[n]) (one rounding) or mul + add
        (two); grouped weights carry their scale already, the epilogue scale is 1."""
        s = np.ones(self.n, np.float32) if self.group else self.scales.astype(np.float32)
        b = self.bias.astype(np.float32)
        if fused:
            return (acc32.astype(np.float64) * s.astype(np.float64)[None, :] + b.astype(np.float64)[None, :]).astype(np.float32)
        return acc32 * s[None, :] + b[None, :]


@functools.lru_cache(maxsize=None)
def problem(k: int, group: int = 0) -> Problem:
    return Problem(k, group)


@functools.lru_cache(maxsize=2)
def tall_problem(k: int, group: int, m: int, n: int) -> Problem:
    """A problem taller / wider than MAXM x MAXN (the persistent and automatic-pick launches)."""
    return Problem(k, group, m, n)


def check_gelu_f16(got: np.ndarray, g: np.ndarray):
    """BIAS_GELU: fp16 outputs against float64 GELU(y): an output passes iff
    float16(g - E) <= got <= float16(g + E).  Returns (share differing from float16(g), largest
    |got - g| among them, largest distance of g from the fp16 rounding boundary on got's side --
    the E such an output needs -- and the number of violations).  |got - g| includes the fp16
    rounding itself: the exact inputs put many y on fp16 ties, where GELU(y) = y - 1e-15 rounds
    the other way than y."""
    lo, hi = (g - GELU_E).astype(np.float16), (g + GELU_E).astype(np.float16)
    bad = ~((got >= lo) & (got <= hi))
    ref = g.astype(np.float16)
    diff = (got != ref) & np.isfinite(got)
    if not diff.any():
        return 0.0, 0.0, 0.0, int(bad.sum())
    go, gd = got[diff], g[diff]
    err = float(np.abs(go.astype(np.float64) - gd).max())
    edge = (go.astype(np.float64) + np.nextafter(go, ref[diff]).astype(np.float64)) / 2
    return float(diff.mean()), err, float(np.abs(edge - gd).max()), int(bad.sum())


def _nibbles(qweight: np.ndarray) -> np.ndarray:
    """GPTQ qweight int32 (K/8, N) -> nibbles (K, N)."""
    w = qweight.view(np.uint32)
    q = np.empty((w.shape[0] * 8, w.shape[1]), np.uint32)
    for j in range(8):
        q[j::8] = (w >> np.uint32(4 * j)) & np.uint32(15)
    return q


def repack_ref(qweight: np.ndarray, layout: int) -> np.ndarray:
    """The packed layouts 1 and 3 as the comments at the top of csrc/gemm_w4a16.hip document them,
    written as a gather over the output word index."""
    q = _nibbles(qweight)
    k, n = q.shape
    idx = np.arange(k * n // 8, dtype=np.int64)
    out = np.zeros(idx.shape, np.uint32)
    if layout == 1:
        # word ((nt * (K/64) + kb) * 64 + lane) * 4 + s: column nt*32 + (lane&31),
        # k = kb*64 + 16 s + 8 (lane>>5) + {0..7}, nibble order [k0,k2,k4,k6 | k1,k3,k5,k7]
        s, lane, blk = idx & 3, (idx >> 2) & 63, idx >> 8
        kb, nt = blk % (k // 64), blk // (k // 64)
        col = nt * 32 + (lane & 31)
        k0 = kb * 64 + 16 * s + 8 * (lane >> 5)
        order = (0, 2, 4, 6, 1, 3, 5, 7)
    elif layout == 3:
        # 2-KiB blocks (nt, kb) over 128-deep K tiles, two 1-KiB pieces p; word w of lane l in piece p:
        # column nt*32 + (l&31), k = kb*128 + 32 (2p + (w>>1)) + 16 (l>>5) + 8 (w&1) + {0..7},
        # nibble order [k0,k4,k1,k5,k2,k6,k3,k7]
        w, lane, p, blk = idx & 3, (idx >> 2) & 63, (idx >> 8) & 1, idx >> 9
        kb, nt = blk % (k // 128), blk // (k // 128)
        col = nt * 32 + (lane & 31)
        k0 = kb * 128 + 32 * (2 * p + (w >> 1)) + 16 * (lane >> 5) + 8 * (w & 1)
        order = (0, 4, 1, 5, 2, 6, 3, 7)
    else:
        raise ValueError(layout)
    for pos, j in enumerate(order):
        out |= q[k0 + j, col] << np.uint32(4 * pos)
    return out.view(np.int32)

