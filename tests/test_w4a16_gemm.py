"""The W4A16 GEMM (csrc/gemm_w4a16.hip) against an independent float64 reference, bit for bit.

Inputs come from ``_w4a16_ref.problem``: every fp32 operation of the kernels -- the MFMA sums in
any order, the fp16 group scaling, the ``fma(acc, s, b)`` epilogue, the residual add and the final
fp16 conversion -- is exact on them, so a kernel may differ from the reference only if it is wrong
(a wrong ring slot, group row, zero point, scale or bias column, a dropped or repeated K tile).
A is a column window of a wider buffer filled with NaN (``lda = K + 48``, 16 bytes in): one stray
read poisons an output.  Every output is a window of a taller, wider buffer filled with a sentinel
(``ldc > N``, the window 16 bytes in), and every element outside the M x N window must stay
untouched.  BIAS_GELU goes through an approximate GELU and is compared with the float64 erf form
within ``_w4a16_ref.GELU_E``.
"""
import math

import numpy as np
import pytest
import torch

import _w4a16_ref as R

# BM, BN of launch_epi (csrc/gemm_w4a16.hip); every ping-pong config is 256 x 256
V1_CFGS = (1, 2, 3, 4, 5, 6, 7, 9)
V3_CFGS = (21, 22, 23, 24, 25, 26, 29, 30, 31)
PP_CFGS = (55, 56, 57, 58, 62, 64, 65, 100, 101, 104, 107, 108, 109, 110, 111, 112, 113, 114)
TILES = {1: (256, 256), 7: (256, 256), 21: (256, 256), 2: (256, 128), 24: (256, 128), 3: (128, 128), 23: (128, 128),
         4: (64, 64), 26: (64, 64), 5: (64, 32), 6: (128, 256), 9: (128, 256), 22: (128, 256), 25: (128, 256),
         29: (128, 320), 31: (128, 320), 30: (256, 320), **{c: (256, 256) for c in PP_CFGS}}
K_PER_CHANNEL = (64, 128, 192, 256, 320, 576)        # 1, 2, 3, 4, 5 and 9 K tiles
LONG_K, LONG_K_CFGS = 2560, (22, 57, 64, 107, 112)
GROUPED_CFGS = V1_CFGS + V3_CFGS + (57, 64, 112, 113, 114)
GROUPED_KG = ((128, 64), (320, 64), (384, 128), (576, 192), (512, 256), (640, 256))   # (640, 256): ragged last group
F16_ONLY_CFGS = (104,)                               # NotImplementedError for F32 / RESADD_F32

CASES = ([(c, k, 0) for c in sorted(TILES) for k in K_PER_CHANNEL] + [(c, LONG_K, 0) for c in LONG_K_CFGS] +
         [(c, k, g) for c in GROUPED_CFGS for k, g in GROUPED_KG])
_CASE_IDS = [f"cfg{c}-k{k}" + (f"-g{g}" if g else "") for c, k, g in CASES]
PROBLEMS = sorted({(k, g) for _, k, g in CASES})

_SENTINEL = {torch.float16: 60000.0, torch.float32: -7777.25}   # |y| < 512


def _is_smallest_k(k, group):
    return (k, group) in ((K_PER_CHANNEL[0], 0), GROUPED_KG[0])


def _shapes(cfg, k, group):
    """(2 BM + 13, 3 BN) and (4 BM + 1, 3 BN); 4 BN where 3 BN is no multiple of 64 (cfg 5); at the
    smallest K also M = 1 and M = BM."""
    bm, bn = TILES[cfg]
    n = 3 * bn if (3 * bn) % 64 == 0 else 4 * bn
    ms = [2 * bm + 13, 4 * bm + 1] + ([1, bm] if _is_smallest_k(k, group) else [])
    return [(m, n) for m in ms]


def _smallest_slice(k, group):
    """The smallest (M, N) any GPU test takes of problem (k, group): cfg 5 runs N = 128 and M = 1 (at
    the smallest K) or 2 * 64 + 13; the long-K problem is run by 128 x 256 tiles and larger only."""
    if k == LONG_K:
        return 2 * 128 + 13, 768
    return (1 if _is_smallest_k(k, group) else 141), 128


def test_tile_table_covers_every_product_config():
    """A config added to ops.W4A16_CFGS cannot ship without a row in TILES (and so in CASES)."""
    from samq import ops
    assert set(TILES) == set(ops.W4A16_CFGS)
    assert set(V1_CFGS) | set(V3_CFGS) | set(PP_CFGS) == set(TILES)
    assert {c for c, _, _ in CASES} == set(TILES)


def _y64(a_int, q, zpk, sk, bias):
    """float64 y for per-K-row zero points zpk and scales sk (both (K, N))."""
    return (a_int * 0.125) @ ((q.astype(np.float64) - zpk) * sk) + bias[None, :]


@pytest.mark.parametrize("k,group", PROBLEMS)
def test_exact_w4a16_inputs_pin_the_kernels(k, group):
    """CPU: what the GPU tests below rely on, for every (K, group) in use.

    On the full 1025 x 1152 problem (and so on every slice of it; the smallest slice in use is
    compared once more explicitly): the fp32 accumulator summed per 64-deep K tile in forward and in
    reverse order and per group -- grouped with the weights fp16((q - zp) * s[g, n]) -- followed by
    the fp32 epilogue as one fma or as mul + add, equals the float64 y exactly; so do the fp32
    residual sum and the fp16 conversion.  No input and no non-zero output is an fp16 subnormal,
    |acc + bias + residual| < 2^24 quanta and |y| < 512.

    On the smallest slice in use each of the listed faults changes at least one element of the
    reference (the share that changes is printed).  The row fault needs two rows: where the
    smallest slice has M = 1 it is checked on the next M in use, 64."""
    p = R.problem(k, group)
    ms, ns = _smallest_slice(k, group)
    tiny = np.float64(2.0 ** -14)
    # ---- exactness
    for order in ("forward", "reverse", "group"):
        acc = p.acc32(order)
        y_fma, y_ma = p.y32(acc, True), p.y32(acc, False)
        assert np.array_equal(y_fma, y_ma), order
        assert np.array_equal(y_fma.astype(np.float64), p.y), order
        assert np.array_equal(y_fma[:ms, :ns].astype(np.float64), p.y[:ms, :ns]), order
    y32 = p.ref("f32")
    assert np.array_equal(y32.astype(np.float64), p.y)
    assert np.array_equal((y32 + p.res_f32).astype(np.float64), p.y_resadd)
    assert np.array_equal(p.ref("resadd").astype(np.float64), p.y_resadd)
    assert np.array_equal(p.res_f32.astype(np.float64), p.r_int * p.qn[None, :])
    # ---- no subnormals: A, scales, 16 * s, bias, every (q - zp) * s, every non-zero output
    for x in (p.a.astype(np.float64), p.bias.astype(np.float64), p.y, p.ref("f16").astype(np.float64)):
        nz = np.abs(x[x != 0])
        assert nz.min() >= tiny
    sc = p.scales.astype(np.float64)
    assert sc.min() >= tiny and np.all(np.log2(sc) % 1 == 0) and 16 * sc.max() < 1
    # ---- bounds
    quanta = np.abs(p.acc + p.b_int[None, :]) + np.abs(p.r_int)
    assert quanta.max() < 2 ** 24
    assert np.abs(p.acc).max() < 2 ** 24
    assert np.abs(p.y).max() < 512 and np.abs(p.y_resadd).max() < 512
    # ---- inputs cover what the docstring promises
    assert set(np.unique(p.nib)) == set(range(16)) or p.ng * p.n < 64
    assert (p.nib[:, 7] == 0).all() and (p.q[:, 7] >= 1).all() and (p.nib[:, 15] == 15).all()
    assert (p.a_int[5:7] == p.amax).all() and (p.a_int[8:10] == -p.amax).all()
    if group:
        assert p.scales.shape == (math.ceil(k / group), p.n) and p.qzeros.shape == (math.ceil(k / group), p.n // 8)
        assert p.ng == 1 or int(p.d.max()) == 2

    # ---- sharpness on the smallest slice
    mr = max(ms, 64) if ms < 2 else ms                     # rows for the row fault
    a, q = p.a_int[:mr], p.q[:, :ns + 1]
    zpk = p.zp[p.gidx][:, :ns + 1].astype(np.float64)
    sk = p.scales.astype(np.float64).reshape(p.ng, p.n)[p.gidx][:, :ns + 1]
    bias = p.bias.astype(np.float64)[:ns + 1]
    base = _y64(a, q[:, :ns], zpk[:, :ns], sk[:, :ns], bias[:ns])
    assert np.array_equal(base, p.y[:mr, :ns])
    shares = {}

    def fault(name, y, rows=ms, cols=np.s_[:]):
        ch = (y[:rows] != base[:rows])
        shares[name] = float(ch.mean())
        assert ch[:, cols].any(), f"{name}: the reference on the smallest slice does not change"

    fault("bias of column n + 1", _y64(a, q[:, :ns], zpk[:, :ns], sk[:, :ns], bias[1:]))
    fault("scale of column n + 1", _y64(a, q[:, :ns], zpk[:, :ns], sk[:, 1:], bias[:ns]))
    for col in (7, 15):
        z2 = zpk[:, :ns].copy()
        z2[:, col] -= 1
        fault(f"zero point - 1 on column {col}", _y64(a, q[:, :ns], z2, sk[:, :ns], bias[:ns]), cols=col)
    if p.ng > 1:
        g = group
        last = np.arange(k) >= (p.ng - 1) * g
        z2, s2 = zpk[:, :ns].copy(), sk[:, :ns].copy()
        z2[last], s2[last] = p.zp[p.ng - 2][None, :ns], sk[(p.ng - 2) * g, :ns][None, :]
        fault("group row g - 1 for the last group", _y64(a, q[:, :ns], z2, s2, bias[:ns]))
    nt = k // 64
    w = (q[:, :ns].astype(np.float64) - zpk[:, :ns]) * sk[:, :ns]
    contrib = [(a[:, 64 * t:64 * t + 64] * 0.125) @ w[64 * t:64 * t + 64] for t in range(nt)]
    for t in range(nt):
        fault(f"K tile {t} dropped", base - contrib[t])
        fault(f"K tile {t} used twice", base + contrib[t])
        if nt > 1:
            fault(f"K tile {(t + 1) % nt} in place of tile {t}", base - contrib[t] + contrib[(t + 1) % nt])
    swap = np.arange(k) ^ 1                                 # repacked word: even-k half <-> odd-k half
    fault("nibble halves of a packed word swapped", _y64(a, q[swap][:, :ns], zpk[:, :ns], sk[:, :ns], bias[:ns]))
    prev = np.maximum(np.arange(mr) - 1, 0)
    fault("A row m - 1 in place of row m", _y64(a[prev], q[:, :ns], zpk[:, :ns], sk[:, :ns], bias[:ns]), rows=mr)
    tile_shares = [v for n_, v in shares.items() if n_.startswith("K tile")]
    print(f"\n[w4a16 inputs K={k} g={group}] slice {ms} x {ns}: share of the reference each fault changes")
    for name, v in shares.items():
        if not name.startswith("K tile"):
            print(f"    {name}: {v:.3f}")
    print(f"    one K tile dropped / used twice / replaced by its neighbour ({nt} tiles): "
          f"{min(tile_shares):.3f} .. {max(tile_shares):.3f}")


# ------------------------------------------------------------------------------------------ GPU
def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


class _Dev:
    """Device copies of one problem's weights for the first n columns."""

    def __init__(self, p, n, dev):
        from samq import ops
        self.w = ops.w4_repack(_t(p.qweight[:, :n], dev))
        self.sc = _t(p.scales[..., :n], dev)
        self.qz = _t(p.qzeros[:, :n // 8], dev)
        self.bias = _t(p.bias[:n], dev)


_DEV = {}


def _dev(p, n, dev):
    key = (p.k, p.group, p.m, p.n, n)
    if key not in _DEV:
        _DEV[key] = _Dev(p, n, dev)
    return _DEV[key]


def _a_window(p, m, dev):
    """A[:m] as a column window of a wider buffer (lda = K + 48, 16 bytes in) filled with NaN."""
    big = torch.full((m, p.k + 48), float("nan"), dtype=torch.float16, device=dev)
    a = big[:, 8:8 + p.k]
    a.copy_(torch.from_numpy(p.a[:m]))
    return a


def _launch(p, dv, a, n, epi, out, cfg):
    from samq import ops
    return ops.w4a16_gemm(a, dv.w, dv.sc, dv.qz, dv.bias, n, p.group or -1, epi, out=out, cfg=cfg)


def _frame(dtype, m, n, dev):
    """An M x N window of a sentinel-filled buffer 3 rows taller and 8 columns wider on both sides:
    the window starts a multiple of 16 bytes in and ldc = N + 16 is a multiple of 8 elements."""
    big = torch.full((m + 6, n + 16), _SENTINEL[dtype], dtype=dtype, device=dev)
    return big, big[3:3 + m, 8:8 + n]


def _frame_untouched(big, win, what):
    _window_untouched(big, 3, 8, win.shape[0], win.shape[1], _SENTINEL[big.dtype], what)


def _window_untouched(big, r0, c0, m, n, sentinel, what):
    """A window anywhere in ``big``: everything outside it still holds the sentinel."""
    chk = big.clone()
    chk[r0:r0 + m, c0:c0 + n] = sentinel
    bad = int((chk != sentinel).sum())
    assert bad == 0, f"{what}: {bad} elements outside the M x N window were written"


_GELU_STATS = [0.0, 0.0, 0.0, 0]    # largest share, largest |got - g|, largest E needed, outputs checked


class _Case:
    """One (problem, cfg, M, N): launches epilogues into sentinel frames and compares."""

    def __init__(self, p, cfg, m, n, dev):
        self.p, self.cfg, self.m, self.n, self.dev = p, cfg, m, n, dev
        self.dv = _dev(p, n, dev)
        self.a = _a_window(p, m, dev)
        self.tag = f"cfg {cfg} {m}x{n}x{p.k}" + (f" g{p.group}" if p.group else "")

    def run(self, epi, dtype, prefill=None):
        big, win = _frame(dtype, self.m, self.n, self.dev)
        if prefill is not None:
            win.copy_(prefill)
        _launch(self.p, self.dv, self.a, self.n, epi, win, self.cfg)
        return big, win

    def exact(self, what, epi, dtype, ref, prefill=None):
        ref_t = _t(ref[:self.m, :self.n], self.dev)
        pre = None if prefill is None else _t(prefill[:self.m, :self.n], self.dev)
        big, win = self.run(epi, dtype, pre)
        nbad = int((win != ref_t).sum())
        assert nbad == 0, f"{self.tag} {what}: {nbad} of {win.numel()} outputs differ"
        _frame_untouched(big, win, f"{self.tag} {what}")

    def unsupported(self, what, epi, dtype):
        big, win = _frame(dtype, self.m, self.n, self.dev)
        with pytest.raises(NotImplementedError):
            _launch(self.p, self.dv, self.a, self.n, epi, win, self.cfg)
        torch.cuda.synchronize()
        assert bool((big == _SENTINEL[dtype]).all()), f"{self.tag} {what}: the refused call wrote to its output"

    def gelu(self):
        big, win = self.run(_epi("BIAS_GELU"), torch.float16)
        _frame_untouched(big, win, f"{self.tag} BIAS_GELU")
        got = win.cpu().numpy()
        share, err, need, bad = R.check_gelu_f16(got, self.p.ref("gelu")[:self.m, :self.n])
        st = _GELU_STATS
        st[0], st[1], st[2], st[3] = max(st[0], share), max(st[1], err), max(st[2], need), st[3] + got.size
        print(f"  [gelu] {self.tag}: {share:.3e} differ from float16(g), largest |got - g| among them {err:.3e}, "
              f"E needed {need:.3e}, violations {bad}; run maxima {st[0]:.3e} / {st[1]:.3e} / {st[2]:.3e} "
              f"over {st[3]} outputs")
        assert bad == 0, f"{self.tag} BIAS_GELU: {bad} outputs outside [f16(g - E), f16(g + E)] (share differing {share:.2e})"

    def all_epilogues(self):
        p = self.p
        if self.cfg in F16_ONLY_CFGS:
            self.unsupported("F32", _epi("F32"), torch.float32)
            self.unsupported("RESADD_F32", _epi("RESADD_F32"), torch.float32)
        else:
            self.exact("F32", _epi("F32"), torch.float32, p.ref("f32"))
            self.exact("RESADD_F32", _epi("RESADD_F32"), torch.float32, p.ref("resadd"), prefill=p.res_f32)
        self.exact("BIAS", _epi("BIAS"), torch.float16, p.ref("f16"))
        self.gelu()


def _epi(name):
    from samq import ops
    return getattr(ops, "EPI_" + name)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,k,group", CASES, ids=_CASE_IDS)
def test_w4a16_gemm_tile_configs(cuda, cfg, k, group):
    """Every product tile config, per channel at K = 64 .. 576 (1, 2, 3, 4, 5 and 9 K tiles: fewer
    than every lookahead, equal to the 3- and 4-slot rings, one more, two ring wraps), K = 2560 on
    configs 22, 57, 64, 107 and 112, and grouped on every config that takes groups ((640, 256): a
    ragged last group), at the shapes of _shapes(): F32, RESADD_F32 (in place on a prefilled window)
    and BIAS equal the float64 reference exactly; BIAS_GELU lies within [f16(g - E), f16(g + E)] of
    the float64 erf GELU g, E = 6.6e-7; nothing outside the M x N window is written.  Config 104 has
    f16 epilogues only and refuses the two f32 ones without writing.

    Measured on gfx950 over all 347 cases (3.1e8 GELU outputs, no violation): at most 3.3e-2 of a
    case's outputs differ from float16(g), the largest |got - g| among them 3.9e-3 -- half an fp16
    step at 8 <= |y| < 16: the exact inputs put many y on fp16 ties, which y and GELU(y) = y - 1e-15
    round in opposite directions -- and the farthest g lies 2.95e-7 (0.45 E) from the rounding
    boundary on the output's side."""
    p = R.problem(k, group)
    print()
    for m, n in _shapes(cfg, k, group):
        _Case(p, cfg, m, n, cuda).all_epilogues()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [64, 192, 320])
def test_w4a16_gemm_persistent_more_tiles_than_cus(cuda, k):
    """The persistent configs 107 / 108 with more tiles than workgroups: N = 2048 (8 column tiles),
    M = 256 t - 7 with 8 t just above the CU count, so some workgroups run two tiles and hand the
    ring over with 1, 3 and 5 K tiles (fewer than, equal to and more than the lookahead); F32 and
    BIAS exactly, in frames."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    t = cus // 8 + 1
    m, n = 256 * t - 7, 2048
    p = R.tall_problem(k, 0, m, n)
    for cfg in (107, 108):
        c = _Case(p, cfg, m, n, cuda)
        c.exact("F32", _epi("F32"), torch.float32, p.ref("f32"))
        c.exact("BIAS", _epi("BIAS"), torch.float16, p.ref("f16"))


# automatic pick (cfg = 0): one shape per branch of pick_cfg -- 64, 57, grouped 57, 22, 23, 26, 5
PICK_SHAPES = [(8197, 256, 0), (8197, 2048, 0), (1030, 512, 0), (520, 384, 0), (141, 192, 0), (141, 96, 0),
               (8197, 2048, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,group", PICK_SHAPES)
def test_w4a16_gemm_auto_pick_exact(cuda, m, n, group):
    """cfg = 0 on a shape for each branch of pick_cfg, K = 192: F32 and BIAS exactly, in frames."""
    p = R.tall_problem(192, group, 8197, 2048)
    c = _Case(p, 0, m, n, cuda)
    c.exact("F32", _epi("F32"), torch.float32, p.ref("f32"))
    c.exact("BIAS", _epi("BIAS"), torch.float16, p.ref("f16"))


def _odd_windows(dtype, m, n, dev):
    """Windows the 16-byte row-vector stores cannot take: (a) one element past a 16-byte boundary
    (ldc still a multiple of 8), (b) 16-byte aligned but ldc % 8 == 4.  Yields (what, big, r0, c0,
    window)."""
    s = _SENTINEL[dtype]
    big = torch.full((m + 6, n + 16), s, dtype=dtype, device=dev)
    win = big[3:3 + m, 9:9 + n]
    assert big.stride(0) % 8 == 0 and win.data_ptr() % 16 != 0
    yield "window one element in", big, 3, 9, win
    big = torch.full((m + 7, n + 20), s, dtype=dtype, device=dev)
    win = big[4:4 + m, 8:8 + n]
    assert big.stride(0) % 8 == 4 and win.data_ptr() % 16 == 0
    yield "ldc % 8 == 4", big, 4, 8, win


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(520, 384), (141, 192), (141, 96)])
def test_w4a16_gemm_unaligned_c_falls_back(cuda, m, n):
    """cfg = 0 with a C the vector epilogues cannot take (not 16-byte aligned, or ldc % 8 != 0):
    samq_w4a16_gemm_cfg falls back to the scalar-store configs 3 / 4 / 5 (N = 384 / 192 / 96); the
    result is exact and the frame untouched.  f32 (F32, RESADD_F32) and f16 (BIAS)."""
    p = R.problem(192)
    dv, a = _dev(p, n, cuda), _a_window(p, m, cuda)
    for epi, dtype, ref, pre in (("F32", torch.float32, p.ref("f32"), None),
                                 ("RESADD_F32", torch.float32, p.ref("resadd"), p.res_f32),
                                 ("BIAS", torch.float16, p.ref("f16"), None)):
        for what, big, r0, c0, win in _odd_windows(dtype, m, n, cuda):
            if pre is not None:
                win.copy_(_t(pre[:m, :n], cuda))
            _launch(p, dv, a, n, _epi(epi), win, 0)
            nbad = int((win != _t(ref[:m, :n], cuda)).sum())
            assert nbad == 0, f"{m}x{n} {epi}, {what}: {nbad} outputs differ"
            _window_untouched(big, r0, c0, m, n, _SENTINEL[dtype], f"{m}x{n} {epi}, {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [22, 29, 57, 111])
def test_w4a16_gemm_unaligned_c_refused(cuda, cfg):
    """An explicit v3 / ping-pong config refuses such a C with AssertionError and writes nothing."""
    p = R.problem(192)
    m, n = 141, 3 * TILES[cfg][1]
    dv, a = _dev(p, n, cuda), _a_window(p, m, cuda)
    for epi, dtype in (("F32", torch.float32), ("BIAS", torch.float16)):
        for what, big, r0, c0, win in _odd_windows(dtype, m, n, cuda):
            with pytest.raises(AssertionError):
                _launch(p, dv, a, n, _epi(epi), win, cfg)
            torch.cuda.synchronize()
            assert bool((big == _SENTINEL[dtype]).all()), f"cfg {cfg} {epi}, {what}: the refused call wrote"


@pytest.mark.gpu
def test_w4a16_gemm_refusals_before_any_write(cuda):
    """Grouped weights on a per-channel-only ping-pong config and N that is no multiple of the
    config's BN are refused, and the sentinel output is untouched."""
    m = 141
    pg, pc = R.problem(128, 64), R.problem(192)
    cases = [(pg, c, 768) for c in (55, 56, 58, 62, 65, 100, 101, 104, 107, 108, 109, 110, 111)]
    cases += [(pc, 29, 768), (pc, 30, 768), (pc, 31, 768), (pc, 22, 384), (pc, 57, 384), (pc, 3, 192), (pc, 26, 96)]
    for p, cfg, n in cases:
        dv, a = _dev(p, n, cuda), _a_window(p, m, cuda)
        for epi, dtype in (("F32", torch.float32), ("BIAS", torch.float16)):
            big, win = _frame(dtype, m, n, cuda)
            with pytest.raises((AssertionError, NotImplementedError)):
                _launch(p, dv, a, n, _epi(epi), win, cfg)
            torch.cuda.synchronize()
            assert bool((big == _SENTINEL[dtype]).all()), f"cfg {cfg} N {n} g {p.group} {epi}: the refused call wrote"


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,layouts", [(192, 96, (1,)), (256, 320, (1, 3)), (4096, 4608, (1,))])
def test_w4_repack_layouts(cuda, k, n, layouts):
    """ops.w4_repack against a numpy gather written from the index comments at the top of
    gemm_w4a16.hip, random full-range words, bit for bit: layouts 1 and 3 (3: K % 128 == 0, so not
    at K = 192); (4096, 4608) is more than 8192 x 256 words, so the kernel's grid-stride loop runs."""
    from samq import ops
    rng = np.random.Generator(np.random.PCG64([k, n]))
    qw = rng.integers(0, 2 ** 32, (k // 8, n), dtype=np.uint64).astype(np.uint32).view(np.int32)
    if k * n // 8 > 8192 * 256:
        assert layouts == (1,)
    if k % 128:
        with pytest.raises(AssertionError):      # layout 3 packs 128-deep K tiles
            ops.w4_repack(_t(qw, cuda), layout=3)
    for layout in layouts:
        got = ops.w4_repack(_t(qw, cuda), layout=layout).cpu().numpy()
        ref = R.repack_ref(qw, layout)
        nbad = int((got != ref).sum())
        assert nbad == 0, f"layout {layout} ({k}, {n}): {nbad} of {ref.size} words differ"
    if 1 in layouts:
        assert torch.equal(ops.w4_repack(_t(qw, cuda)), ops.w4_repack(_t(qw, cuda), layout=1))

