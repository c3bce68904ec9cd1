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



# ------------------------------------------------------------------ LayerNorm fold and gated MLP
# (test_w4a16_lnf_gated.py)
U24 = 2.0 ** -24             # half an fp32 ulp, relative: the error of one fp32 rounding
LNF_EPS = float(np.float32(1e-6))
LNF_MS = (1, 31, 33, 255, 256, 257, 2 * 256 + 13)
RSQRT_U = 2                  # rsqrtf: 1 ulp in the HIP math API's accuracy table = 2 * 2^-24 relative


def check_interval_f16(got: np.ndarray, y: np.ndarray, e: np.ndarray):
    """fp16 outputs against a float64 reference y with a per-element bound e: an output passes iff
    float16(y - e) <= got <= float16(y + e) (check_gelu_f16 with any bound; a NaN never passes).
    Returns (violations, the largest need / e over the finite outputs that differ from float16(y),
    need = the distance of y from the fp16 rounding boundary on got's side: the bound that output
    would have needed)."""
    e = np.broadcast_to(np.asarray(e, np.float64), y.shape)
    lo, hi = (y - e).astype(np.float16), (y + e).astype(np.float16)
    bad = ~((got >= lo) & (got <= hi))
    ref = y.astype(np.float16)
    diff = (got != ref) & np.isfinite(got)
    if not diff.any():
        return int(bad.sum()), 0.0
    go = got[diff]
    edge = (go.astype(np.float64) + np.nextafter(go, ref[diff]).astype(np.float64)) / 2
    return int(bad.sum()), float((np.abs(edge - y[diff]) / e[diff]).max())


class LnfProducer:
    """RESADD_LNF operands and float64 expectations on the first n columns of a problem:
    x_new = y_resadd (exact in fp32), mu_p a multiple of 2^-12 within about 0.5 of the row mean and
    different in every row, gamma from {1, 2, 4}.  x_new is a multiple of 2^-14 below 512 and so is
    d = x_new - mu_p (below 1024: 24 bits), hence d and d * gamma are exact in fp32 and aout is ONE
    rounding of the float64 d * gamma; d != 0 is at least 2^-14, no fp16 subnormal."""

    def __init__(self, p: Problem, n: int):
        rng = np.random.Generator(np.random.PCG64([p.k, p.group, n, 7]))
        x = p.y_resadd[:, :n]
        off = (rng.permutation(p.m) + 0.5) / p.m - 0.5               # distinct, inside (-0.5, 0.5)
        t, seen = np.round((x.mean(1) + off) * 4096).astype(np.int64), set()
        for r in range(p.m):                                         # a value taken by an earlier row: one step up
            while int(t[r]) in seen:
                t[r] += 1
            seen.add(int(t[r]))
        mu = t / 4096.0
        self.n, self.x = n, x
        self.mu = mu.astype(np.float32)
        self.gamma = (2.0 ** rng.integers(0, 3, n)).astype(np.float32)
        self.d = x - mu[:, None]
        self.aout64 = self.d * self.gamma.astype(np.float64)[None, :]
        self.aout = self.aout64.astype(np.float16)
        blk = self.d.reshape(p.m, n // 64, 64)
        self.s1, self.s2, self.sa = blk.sum(2), (blk * blk).sum(2), np.abs(blk).sum(2)

    def stats_bounds(self):
        """lnf_res4 + sum16_dpp: a lane adds its 4 columns as (d0 + d1) + (d2 + d3) (two levels),
        four DPP levels follow: 6 roundings on any path to the total, |s1 - S1| <= 6 u sum|d|;
        the squares add one rounding each and the terms are positive: |s2 - S2| <= 8 u S2 (the 7
        first-order roundings rounded up)."""
        return 6 * U24 * self.sa, 8 * U24 * self.s2

    def stats_violations(self, got: np.ndarray, m: int) -> int:
        """got (m, n / 64, 2): the number of block sums outside their bound."""
        b1, b2 = self.stats_bounds()
        g = got.astype(np.float64)
        return int((~(np.abs(g[..., 0] - self.s1[:m]) <= b1[:m])).sum() +
                   (~(np.abs(g[..., 1] - self.s2[:m]) <= b2[:m])).sum())


@functools.lru_cache(maxsize=None)
def lnf_producer(k: int, group: int, n: int) -> LnfProducer:
    return LnfProducer(problem(k, group), n)


def _zigzag(nblk: int) -> np.ndarray:
    """nblk values evenly spaced over [0.5, 1.5], ordered low, high, low, ...: neighbours lie half
    the range apart."""
    v = np.linspace(0.5, 1.5, nblk) if nblk > 1 else np.ones(1)
    lo, hi = v[:(nblk + 1) // 2], v[(nblk + 1) // 2:]
    out = np.empty(nblk)
    out[0::2], out[1::2] = lo, hi
    return out


class LnfStats:
    """Synthetic consumer ``stats`` (rows x K / 64 x 2, fp32), independent of any producer: row r has
    its own variance, about 0.25 * 64^u in [0.25, 16] (even rows u in [0, 0.4], odd rows [0.6, 1]:
    neighbouring rows lie a factor 2.3 or more apart) and its own delta, 0.3 .. 1 times sqrt(var) / 2
    of either sign.  The row totals S1 = K delta and S2 = K (var + delta^2) are dealt over the
    blocks by two different zigzag weight vectors (neighbouring blocks differ by half the mean
    block and more; every s1 of a row has one sign, every s2 is positive, so the sums lose no
    bits to cancellation).  delta, var and rstd are recomputed in float64 from the fp32 pairs."""

    def __init__(self, k: int, m: int = MAXM):
        self.k, self.nblk = k, k // 64
        nb = self.nblk
        rng = np.random.Generator(np.random.PCG64([k, m, 11]))
        rows = np.arange(m)
        u = 0.6 * (rows % 2) + 0.4 * (rng.permutation(m) + 0.5) / m
        var = 0.25 * 64.0 ** u
        delta = rng.choice([-1.0, 1.0], m) * np.sqrt(var) / 2 * rng.uniform(0.3, 1.0, m)
        w1 = _zigzag(nb)[None, :] * rng.uniform(1.0, 1.05, (m, nb))
        w2 = _zigzag(nb)[::-1][None, :] * rng.uniform(1.0, 1.05, (m, nb))
        st = np.empty((m, nb, 2), np.float32)
        st[..., 0] = (k * delta)[:, None] * w1 / w1.sum(1, keepdims=True)
        st[..., 1] = (k * (var + delta * delta))[:, None] * w2 / w2.sum(1, keepdims=True)
        self.stats = st
        self.delta, self.var, self.rstd = self.rowinfo(st)
        self.mu0 = (rng.choice([-1.0, 1.0], m) * rng.uniform(8.0, 16.0, m)).astype(np.float32)

    def rowinfo(self, st):
        s = st.astype(np.float64).sum(1)
        delta = s[:, 0] / self.k
        var = s[:, 1] / self.k - delta * delta
        with np.errstate(invalid="ignore"):
            return delta, var, 1.0 / np.sqrt(var + LNF_EPS)


@functools.lru_cache(maxsize=None)
def lnf_stats(k: int) -> LnfStats:
    return LnfStats(k)


def lnf_consts(k: int, n: int):
    """The consumer's gw, bw: small fp32 vectors, |gw| <= 2, |bw| <= 1."""
    rng = np.random.Generator(np.random.PCG64([k, n, 13]))
    return rng.uniform(-2, 2, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)


def lnf_c(nblk: int) -> int:
    """The count of fp32 roundings between the staged pairs and the fp32 value the consumer converts
    to fp16 (lnf_rowinfo_wg, lnf_out8 in csrc/gemm_w4a16.hip), each at most 2^-24 relative:

    * nblk - 1   the adds of a row's nblk pairs (the first add, to 0, is exact);
    * 3          inv_k = 1 / K and its two products s1 * inv_k, s2 * inv_k;
    * 1          the variance subtraction s2 * inv_k - delta^2 (|delta|^2 <= var / 4 on the test's
                 inputs, so it amplifies what it subtracts by at most 1.5);
    * RSQRT_U    rsqrtf: 1 ulp = 2 * 2^-24 in the HIP math API's accuracy table;
    * 2          the two fmas of lnf_out8, fma(rstd, fma(-delta, gw, v), bw + bias).

    c = nblk + 5 + RSQRT_U, applied to the magnitude of the terms that carry the roundings,
    E = c 2^-24 (|rstd| (|acc s| + |delta gw|) + |bw + bias|).  The count treats the roundings as
    one chain; the fp32 sum bw + bias, the + eps and the second use of delta^2 are covered by the
    terms that the chain counts against the whole magnitude although they touch only part of it
    (the delta path's nblk + 1 roundings reach |delta gw| alone, the rstd path halves what the
    variance collected)."""
    return nblk + 5 + RSQRT_U


def lnf_consumer_ref(p: Problem, rowinfo, m: int, n: int, gw, bw, bias, act: bool, mat=None, c=None):
    """float64 y = rstd (acc s - delta gw) + bw + bias (-> GELU) for rows [:m], columns [:n] and its
    bound E (GELU: 1.13 E + GELU_E, 1.13 bounding |GELU'|).  mat: acc s if not the problem's."""
    delta, _, rstd = (x[:m, None] for x in rowinfo)
    mat = p.acc[:m, :n] * p.qn[None, :n] if mat is None else mat
    gw, bb = gw.astype(np.float64)[None, :], bw.astype(np.float64)[None, :]
    if bias is not None:
        bb = bb + bias.astype(np.float64)[None, :n]
    y = rstd * (mat - delta * gw) + bb
    c = lnf_c(p.k // 64) if c is None else c
    e = c * U24 * (np.abs(rstd) * (np.abs(mat) + np.abs(delta * gw)) + np.abs(bb))
    if act:
        with np.errstate(invalid="ignore"):
            return gelu(y), 1.13 * e + GELU_E
    return y, e


# ---- gated MLP: gate = columns [0, n), up = columns [n, 2n) of a problem, bias dropped
GATED_ROWS = (5, 8)          # the all +amax and all -amax rows


def gated_scale(k: int) -> int:
    """A rows GATED_ROWS times 4 at K = 64 (gates past +-20 there too); exact in fp16 and fp32."""
    return 4 if k == 64 else 1


def gated_a(p: Problem) -> np.ndarray:
    a = p.a.copy()
    a[list(GATED_ROWS)] *= np.float16(gated_scale(p.k))
    return a


def gated_ref(p: Problem, n: int):
    """float64 gate g, up u and silu(g) * u = g / (1 + exp(-g)) * u of the scaled A."""
    acc = p.acc[:, :2 * n].copy()
    acc[list(GATED_ROWS)] *= gated_scale(p.k)
    g, u = acc[:, :n] * p.qn[None, :n], acc[:, n:2 * n] * p.qn[None, n:2 * n]
    with np.errstate(over="ignore"):
        return g, u, g / (1.0 + np.exp(-g)) * u, acc


def interleave32_ref(gate_words, up_words, gate_sc, up_sc, gate_qz, up_qz, k: int):
    """samq_w4a16_gated_mlp's operand layout from the comment of ops.w4_interleave32, as a gather
    over the output index: 32-column block B of the 2N columns is block B // 2 of the gate (B even)
    or of the up projection (B odd).  A block is (K / 64) * 256 consecutive words of a layout-1
    matrix, 32 scales of a group row and 4 qzeros words (8 columns each) of a group row."""
    def gather(gate, up, per_block):
        i = np.arange(2 * gate.shape[-1])
        b, inner = i // per_block, i % per_block
        src = (b // 2) * per_block + inner
        return np.where(b % 2 == 0, gate[..., src], up[..., src])
    return (gather(gate_words, up_words, k // 64 * 256), gather(gate_sc, up_sc, 32), gather(gate_qz, up_qz, 4))
