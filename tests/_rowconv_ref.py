"""Float64 / exact-integer references and small tools for test_row_kernels.py and
test_conv_kernels.py: sentinel frames, the LayerNorm tolerances, the quantiser's adversarial operand
set with numpy stand-ins of the wrong quantisers, and integer convolution inputs on which every
summation order gives the same bits.  Nothing here is derived from a kernel's output.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np
import torch

SENTINEL = 0x5A
F32_EPS = 2.0 ** -24            # half an ulp of 1.0f: the unit roundoff of fp32


# ----------------------------------------------------------------------------- frames
class Frame:
    """A contiguous tensor that is a window of a larger byte buffer filled with 0x5A: at least
    ``guard`` bytes (rounded up to 16) on both sides, the window itself 16-byte aligned."""

    def __init__(self, shape, dtype, dev, guard=0):
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape)) * item
        row = (shape[-1] if shape else 1) * item
        self.pad = (max(int(guard), row, 16) + 15) // 16 * 16
        self.buf = torch.full((2 * self.pad + self.nbytes,), SENTINEL, dtype=torch.uint8, device=dev)
        self.t = self.buf[self.pad:self.pad + self.nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def untouched(self) -> bool:
        lo, hi = self.buf[:self.pad], self.buf[self.pad + self.nbytes:]
        return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())

    def pristine(self) -> bool:
        """Nothing at all was written: borders and window still hold the sentinel."""
        return bool((self.buf == SENTINEL).all())


def ulp_f16(v):
    """The spacing of fp16 at |v| (float64 in, float64 out); subnormal spacing below 2^-14."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, -14.0), -14.0)
    return 2.0 ** (e - 10.0)


# ----------------------------------------------------------------------------- LayerNorm
LN_WIDTHS = (4, 252, 260, 516, 772, 1024, 1028, 1280, 1284, 2560, 4092, 4096)
ADD_LN_WIDTHS = (4, 260, 768, 772, 1024, 1028, 1280)
LN_ROWS = (1, 13, 37)
LN_RPW = (0, 1, 2, 4)
LN_IN_SCALE = 3 * 2.0 ** -5     # int8-code input: code * 3/32 is exact in fp32, code 16 is 1.5
EDGE_ZERO, EDGE_CONST, EDGE_OFFSET = 3, 4, (5, 6)


@functools.lru_cache(maxsize=None)
def ln_problem(c: int, src: str):
    """37 rows of width c as the kernel sees them (``x``: torch f32 / f16 / int8), their float64
    values ``x64`` and gamma / beta.  Rows 3..6 are the edge rows: all zero, constant 1.5, and two
    rows 10 + 0.1 N(0,1); a launch of the first 13 or 37 rows contains them, a launch of 1 does not."""
    g = torch.Generator().manual_seed(1000 + c)
    x = torch.randn(37, c, generator=g) * 3 + 1.5
    x[EDGE_ZERO] = 0.0
    x[EDGE_CONST] = 1.5
    for r in EDGE_OFFSET:
        x[r] = 10.0 + 0.1 * torch.randn(c, generator=g)
    gamma = 1 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    if src == "f16":
        x = x.half()
        x64 = x.double()
    elif src == "i8":
        x = torch.clamp(torch.round(x / LN_IN_SCALE), -128, 127).to(torch.int8)
        x64 = (x.float() * np.float32(LN_IN_SCALE)).double()      # fl32(code * in_scale), widened
    else:
        x64 = x.double()
    return x, x64, gamma, beta


def ln64(x64, gamma, beta, eps):
    return torch.nn.functional.layer_norm(x64, (x64.shape[-1],), gamma.double(), beta.double(), eps).numpy()


def ln_tol(x64: torch.Tensor, y64: np.ndarray, gamma) -> np.ndarray:
    """Per-row fp32 bound (rows, 1): 2e-5 max(1, max|y64|), plus 32 * 2^-24 * (|mean| / std) * max|gamma|
    on the rows with a large common offset (the cancellation in x - mean costs |mean| / std ulps)."""
    base = 2e-5 * max(1.0, float(np.abs(y64).max()))
    tol = np.full((x64.shape[0], 1), base)
    for r in EDGE_OFFSET:
        if r < x64.shape[0]:
            row = x64[r].numpy()
            tol[r] += 32 * F32_EPS * abs(row.mean()) / row.std() * float(gamma.abs().max())
    return tol


def plain_rows(rows: int) -> np.ndarray:
    """Mask of the rows that are neither constant nor offset rows."""
    m = np.ones(rows, bool)
    for r in (EDGE_ZERO, EDGE_CONST) + EDGE_OFFSET:
        if r < rows:
            m[r] = False
    return m


def const_rows(rows: int):
    return [r for r in (EDGE_ZERO, EDGE_CONST) if r < rows]


def check_codes(got: np.ndarray, y64: np.ndarray, out_scale, tol: np.ndarray, share_rows: np.ndarray):
    """int8 codes against float64: with tau = 2 tol / out_scale, every element whose quotient
    y64 / out_scale lies farther than tau from the nearest k + 0.5 equals clamp(rint(q)) exactly, the
    others differ by at most 1.  Returns (excluded share over ``share_rows``, exact mismatches among
    the decided elements, largest difference among the excluded ones)."""
    q = y64 / np.float64(out_scale)
    ref = np.clip(np.rint(q), -128, 127).astype(np.int64)
    tau = 2.0 * tol / np.float64(out_scale)
    near = np.abs(q - np.floor(q) - 0.5) <= tau
    near &= (q > -128.5 - tau) & (q < 127.5 + tau)        # beyond the clamp no tie can matter
    d = np.abs(got.astype(np.int64) - ref)
    wrong = int((d[~near] != 0).sum())
    loose = int(d[near].max()) if near.any() else 0
    return float(near[share_rows].mean()), wrong, loose


# ----------------------------------------------------------------------------- quantiser operands
def _steps(v: np.ndarray, d: int) -> np.ndarray:
    out = v.copy()
    for _ in range(abs(d)):
        out = np.nextafter(out, out.dtype.type(np.inf if d > 0 else -np.inf))
    return out


def quant_scales():
    s = [np.float32(0.037), np.float32(3 * 2.0 ** -7), np.float32((2 - 2.0 ** -23) * 2.0 ** -6),
         np.float32((1 + 2.0 ** -23) * 2.0 ** -5)]
    for seed in range(4):
        s.append(np.float32(np.exp(np.random.default_rng(seed).uniform(-12, 3))))
    # 7 * 2^-8: every tie (k + 0.5) s is an fp16 number and fl(1 / s) is 2^-24.5 too large, enough to
    # push v * fl(1 / s) off a tie -- the one scale at which fp16 operands can see a reciprocal multiply
    s.append(np.float32(7 * 2.0 ** -8))
    return s


F16_TIE_SCALE = 8     # index of 7 * 2^-8 in quant_scales()


def tie_operands(s, dtype=np.float32) -> np.ndarray:
    """fl((k + 0.5) s) for k in [-131, 130] and its neighbours at -2..+2 ulps of ``dtype``."""
    k = np.arange(-131, 131, dtype=np.float64)
    v = ((k + 0.5) * np.float64(s)).astype(dtype)
    return np.concatenate([_steps(v, d) for d in (-2, -1, 0, 1, 2)])


def quant_operands(s, seed=0) -> np.ndarray:
    """The fp32 operand vector of one scale: ties and near-ties, +-0, +-inf, +-FLT_MAX, the clamp
    edges +-127.5 s and +-128.5 s, +-1e30 and 4096 Gaussian values spanning the code range."""
    s64 = np.float64(s)
    fmax = np.finfo(np.float32).max
    special = np.array([0.0, -0.0, np.inf, -np.inf, fmax, -fmax, 127.5 * s64, -127.5 * s64, 128.5 * s64,
                        -128.5 * s64, 1e30, -1e30], np.float64).astype(np.float32)
    rng = np.random.default_rng(100 + seed)
    gauss = (rng.standard_normal(4096) * 60.0 * s64).astype(np.float32)
    return np.concatenate([tie_operands(s), special, gauss])


def quant_operands_f16(s, seed=0) -> np.ndarray:
    """The same in fp16: ties rebuilt on the fp16 grid (exact ties survive where (k + 0.5) s is an
    fp16 number, as for 3 * 2^-7), fp16 specials, Gaussians rounded to fp16."""
    s64 = np.float64(s)
    with np.errstate(over="ignore"):
        special = np.array([0.0, -0.0, np.inf, -np.inf, 65504.0, -65504.0, 127.5 * s64, -127.5 * s64,
                            128.5 * s64, -128.5 * s64, 6e4, -6e4], np.float64).astype(np.float16)
        rng = np.random.default_rng(200 + seed)
        gauss = (rng.standard_normal(4096) * 60.0 * s64).astype(np.float16)
        return np.concatenate([tie_operands(s, np.float16), special, gauss])


def quant_ref(v, s) -> np.ndarray:
    """The documented contract: clamp(rint(fl32(v / s)), -128, 127) with a true fp32 division."""
    with np.errstate(over="ignore"):
        q = np.asarray(v).astype(np.float32) / np.float32(s)
    return np.clip(np.rint(q), -128, 127).astype(np.int8)


def _codes(q) -> np.ndarray:
    return np.clip(np.rint(q), -128, 127).astype(np.int8)


def quant_recip(v, s) -> np.ndarray:
    """Stand-in of a wrong quantiser: rint(v * fl(1 / s)), one reciprocal multiply."""
    with np.errstate(over="ignore"):
        y = np.float32(1.0) / np.float32(s)
        return _codes(np.asarray(v, np.float32) * y)


def quant_one_step(v, s) -> np.ndarray:
    """Stand-in of the one-step quantiser: one Markstein correction fma(fma(-q0, s, v), y, q0) with
    y = fl(1 / s), each fma rounded once (exact rational arithmetic; finite, normal operands)."""
    v = np.asarray(v, np.float32)
    assert np.isfinite(v).all()
    s = np.float32(s)
    y = np.float32(1.0) / s
    q0 = (v * y).astype(np.float32)
    fs, fy = Fraction(float(s)), Fraction(float(y))
    q1 = [_rn32(Fraction(float(q)) + _rn32(Fraction(float(x)) - Fraction(float(q)) * fs) * fy) for x, q in zip(v, q0)]
    return _codes(np.array([float(q) for q in q1], np.float32))


def _rn32(fr: Fraction) -> Fraction:
    """An exact rational rounded once to fp32 (round half to even, normal range)."""
    if fr == 0:
        return fr
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    r = round(a / ulp) * ulp          # Python rounds halves to even
    return r if fr > 0 else -r


def silu_mul64(g, u) -> np.ndarray:
    g = np.asarray(g, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * np.asarray(u, np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- convolutions
def ints(gen, lo, hi, shape) -> torch.Tensor:
    """Integers in [lo, hi] as float64."""
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def patch_ref(x64, w64, bias64, pos64, patch) -> torch.Tensor:
    """Conv2d(k = stride = patch) + bias + pos in float64: x (B, Cin, S, S), w (N, Cin p p),
    pos (G, G, N) -> (B, G, G, N)."""
    n, cin = w64.shape[0], x64.shape[1]
    y = torch.nn.functional.conv2d(x64, w64.view(n, cin, patch, patch), bias64, stride=patch).permute(0, 2, 3, 1)
    return y + pos64 if pos64 is not None else y


def patch_abs_ref(x64, w64, bias64, pos64, patch) -> torch.Tensor:
    """sum_k |a_k w_k| + |bias| + |pos|: the magnitude the fp32 summation bound scales with."""
    return patch_ref(x64.abs(), w64.abs(), None if bias64 is None else bias64.abs(),
                     None if pos64 is None else pos64.abs(), patch)


def normalise_u8(img: torch.Tensor, mean, std, size: int, f32: bool) -> torch.Tensor:
    """Sam.preprocess in float64 (or on fp32 values): (pixel - mean) / std, zero-padded to size."""
    b, c, h, w = img.shape
    x = torch.zeros(b, c, size, size, dtype=torch.float64)
    m, s = mean.view(1, c, 1, 1), std.view(1, c, 1, 1)
    v = ((img.float() - m.float()) / s.float()).double() if f32 else (img.double() - m.double()) / s.double()
    x[:, :, :h, :w] = v
    return x


def conv3x3_ref(x64, w64_tap_major) -> torch.Tensor:
    """x (B, G, G, Cin), w (N, 3, 3, Cin), zero padding 1, float64 -> (B, G, G, N)."""
    y = torch.nn.functional.conv2d(x64.permute(0, 3, 1, 2), w64_tap_major.permute(0, 3, 1, 2), padding=1)
    return y.permute(0, 2, 3, 1)


def i8_conv_problem(mode: int, b: int, cin: int, g: int, n: int, seed: int):
    """Inputs of the int8 implicit-GEMM conv by the rules of tests/_i8_ref.py: a_scale * wscale[n] a
    power of two that varies by column, bias an integer multiple of it, codes mostly multiples of
    16 (a few tokens and every 8th column full range, -128 and 127 included), so that y = (acc + b_int) * csc is exact in
    fp32 and many quotients y / (3 * 2^e) are ties.  Returns a dict with the codes, the tap-major
    weight matrix (N, K), wscale, bias, the int64 sums ``acc`` (M, N) and y in float64."""
    rng = np.random.Generator(np.random.PCG64([seed, mode, cin, g, n]))
    if mode == 1:
        side = 16 * g
        k = cin * 256
        cols = (rng.integers(-8, 8, (b * g * g, k)) * 16).astype(np.int8)
        full = np.arange(b * g * g) % 7 == 3                      # full-range tokens (patches)
        cols[full] = rng.integers(-128, 128, (int(full.sum()), k), dtype=np.int8)
        cols[full, :2] = (-128, 127)
        x = np.ascontiguousarray(cols.reshape(b, g, g, cin, 16, 16).transpose(0, 3, 1, 4, 2, 5)).reshape(b, cin, side, side)
    else:
        x = (rng.integers(-8, 8, (b, g, g, cin)) * 16).astype(np.int8)
        x[1:, g - 1, 0] = rng.integers(-128, 128, (b - 1, cin), dtype=np.int8)   # one full-range token per later image
        x[1:, g - 1, 0, :2] = (-128, 127)
        k = 9 * cin
        pad = np.zeros((b, g + 2, g + 2, cin), np.int8)
        pad[:, 1:-1, 1:-1] = x
        cols = np.stack([pad[:, ky:ky + g, kx:kx + g] for ky in range(3) for kx in range(3)], 3).reshape(b * g * g, k)
    w = (rng.integers(-8, 8, (n, k)) * 16).astype(np.int8)
    w[5::8] = rng.integers(-128, 128, w[5::8].shape, dtype=np.int8)
    acc = cols.astype(np.int64) @ w.astype(np.int64).T
    e_col = -9 - rng.integers(0, 3, n)
    a_scale = np.float32(2.0 ** -6)
    wscale = (2.0 ** e_col).astype(np.float32)
    csc = np.float64(a_scale) * 2.0 ** e_col
    b_int = 256 * rng.integers(-12, 13, n)
    b_int[5::8] = rng.integers(-5000, 5001, b_int[5::8].shape)
    assert np.abs(acc + b_int[None, :]).max() < 2 ** 24
    return dict(x=x, w=w, k=k, a_scale=a_scale, wscale=wscale, bias=(b_int * csc).astype(np.float32),
                acc=acc, y=(acc + b_int[None, :]) * csc[None, :], y_nobias=acc * csc[None, :],
                res=rng.integers(-128, 128, (b * g * g, n), dtype=np.int8))
