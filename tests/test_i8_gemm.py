"""The int8 GEMMs (csrc/gemm_i8.hip) against an independent float64 reference, bit for bit.

Inputs come from ``_i8_ref.problem``: every fp32 operation of the kernels' dequantisation,
quantisers and residual sums is exact on them, a large share of the quantiser arguments are exact
``k + 0.5`` ties, and both clamp ends are hit, so a kernel may differ from the reference only if it
is wrong (rounding mode, clamp end, a skipped tile or slice, a wrong zero point or scale column).
Every output is written into a column window of a wider, taller buffer filled with a sentinel
(``ldc > N``), A is a column window too (``lda > K``), and every byte outside the M x N window must
stay untouched.  int8 outputs can take any value, so those runs are made twice with two sentinels.
"""
import numpy as np
import pytest
import torch

import _i8_ref as R

# BM, BN of with_i8_cfg (csrc/gemm_i8.hip)
TILES = {81: (256, 256), 82: (128, 256), 83: (128, 128), 84: (64, 64), 85: (256, 256), 86: (256, 256),
         87: (128, 64), 88: (64, 128), 89: (64, 64), 90: (64, 128), 91: (32, 64), 92: (64, 32),
         180: (128, 128), 181: (128, 64), 182: (128, 128)}
W8_CFGS = [0, 81, 82, 83, 84, 87, 88, 89, 90, 91, 92, 180, 181, 182]
W4_CFGS = W8_CFGS + [85, 86]
GROUPED_CFGS = [0, 83, 84, 87, 88]
GROUPED_KG = [(384, 128), (640, 256), (640, 128)]      # (640, 256): a ragged last group
# cfg 0: shapes on which i8_pick_cfg (M <= 1024) takes each config it can reach -- W8: 89 (any N),
# 90 (N % 128 == 0, N > 1024); W4: 83 (N % 128 == 0, M >= 256), 84 (otherwise); grouped W4: 84, and
# 83 from M = 1024 with N % 128 == 0
PICK_SHAPES = {"w8": [(141, 192), (141, 1152)], "w4": [(269, 384), (141, 192)], "w4g": [(141, 192), (1024, 384)]}

CASES = ([("w8", c, k, 0) for c in W8_CFGS for k in (128, 256, 384, 640)] +
         [("w4", c, k, 0) for c in W4_CFGS for k in (128, 256, 384, 640)] +
         [("w4g", c, k, g) for c in GROUPED_CFGS for k, g in GROUPED_KG])

_CASE_IDS = [f"{f}-cfg{c}-k{k}" + (f"-g{g}" if g else "") for f, c, k, g in CASES]

_SENTINELS = {torch.int8: (77, -78), torch.float16: (60000.0,), torch.float32: (-7777.25,)}   # |y| < 512
_ALIGN = {torch.int8: 16, torch.float16: 8, torch.float32: 4}                                # 16-byte rows


def _shapes(fmt, cfg):
    """Shape A: M = 2 BM + 13 (a last row tile shorter than one 32-row slice), N = 3 BN: 9 workgroups;
    shape B: M = 4 BM + 1: 15 workgroups (both leave xcd_remap a remainder).  BN = 32 (cfg 92) takes
    N = 4 BN, the API needs N % 64 == 0: 12 and 20 workgroups."""
    if cfg == 0:
        return PICK_SHAPES[fmt]
    bm, bn = TILES[cfg]
    n = 3 * bn if (3 * bn) % 64 == 0 else 4 * bn
    return [(2 * bm + 13, n), (4 * bm + 1, n)]


class _Dev:
    """Device copies of one problem's weights for the first n columns."""

    def __init__(self, p, n, dev):
        from samq import ops
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        self.bias = t(p.bias[:n])
        self.qz = None
        if p.fmt == "w8":
            self.w = ops.w8_repack(t(p.w[:n]))
            self.ws = t(p.wscale[:n])
        else:
            self.w = ops.w4_repack(t(p.qweight[:, :n]), layout=3)
            self.qz = t(p.qzeros[:, :n // 8])
            self.ws = t(p.wscale[..., :n]).reshape(-1)


_DEV = {}


def _dev(p, n, dev):
    key = (p.fmt, p.k, p.group, n)
    if key not in _DEV:
        _DEV[key] = _Dev(p, n, dev)
    return _DEV[key]


def _a_window(p, m, dev):
    """A[:m] as a column window of a wider buffer (lda = K + 48, 16 bytes in) filled with 99."""
    big = torch.full((m, p.k + 48), 99, dtype=torch.int8, device=dev)
    a = big[:, 16:16 + p.k]
    a.copy_(torch.from_numpy(p.a[:m]))
    return a


def _frame(dtype, m, n, sentinel, dev, extra=3):
    al = _ALIGN[dtype]
    big = torch.full((m + 3, n + extra * al), sentinel, dtype=dtype, device=dev)
    return big, big[:m, al:al + n]


def _frame_untouched(big, win, sentinel, what):
    al, (m, n) = _ALIGN[big.dtype], win.shape
    chk = big.clone()
    chk[:m, al:al + n] = sentinel
    bad = int((chk != sentinel).sum())
    assert bad == 0, f"{what}: {bad} elements outside the M x N window were written"


def _launch(p, dv, a, n, epi, out, cfg, out_scale=0.0, mid=0.0, res_scale=0.0, res=None, **rs):
    from samq import ops
    if p.fmt == "w8":
        return ops.w8a8_gemm(a, dv.w, dv.ws, n, dv.bias, epi, float(p.a_scale), float(out_scale), float(mid),
                             float(res_scale), res, out, cfg)
    return ops.w4a8_gemm(a, dv.w, dv.ws, dv.qz, n, dv.bias, epi, float(p.a_scale), float(out_scale), out=out,
                         groupsize=p.group or -1, cfg=cfg, **rs)


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


_GELU_STATS = {}


def _note_gelu(kind, share, dist, n_out):
    s = _GELU_STATS.setdefault(kind, [0.0, 0.0, 0])
    s[0], s[1], s[2] = max(s[0], share), max(s[1], dist), s[2] + n_out


class _Case:
    """One (problem, cfg, M, N): launches epilogues into sentinel frames and compares."""

    def __init__(self, p, cfg, m, n, dev):
        self.p, self.cfg, self.m, self.n, self.dev = p, cfg, m, n, dev
        self.dv = _dev(p, n, dev)
        self.a = _a_window(p, m, dev)
        self.tag = f"{p.fmt} cfg {cfg} {m}x{n}x{p.k}" + (f" g{p.group}" if p.group else "")
        self.rowsum_in = _t(p.rowsum_a[:m], dev) if (p.fmt == "w4" and cfg == 86) else None

    def _rs_variants(self):
        """Per launch: no row sums; on cfg 86 also with the producer's exact sums of A."""
        return [{}] + ([dict(rowsum=self.rowsum_in)] if self.rowsum_in is not None else [])

    def run(self, epi, dtype, sentinel, prefill=None, res=None, extra=3, **kw):
        big, win = _frame(dtype, self.m, self.n, sentinel, self.dev, extra)
        if prefill is not None:
            win.copy_(prefill)
        if isinstance(res, str):   # "alias": R is the output window itself (in place, ldr == ldc)
            res = win
        kws = dict(kw)
        if res is not None:
            kws["res"] = res
        _launch(self.p, self.dv, self.a, self.n, epi, win, self.cfg, **kws)
        return big, win

    def exact(self, what, epi, dtype, ref, prefill=None, res=None, extra=3, **kw):
        ref_t = _t(ref[:self.m, :self.n], self.dev)
        pre = None if prefill is None else _t(prefill[:self.m, :self.n], self.dev)
        for sentinel in _SENTINELS[dtype]:
            for rs in self._rs_variants():
                big, win = self.run(epi, dtype, sentinel, pre, res, extra, **kw, **rs)
                nbad = int((win != ref_t).sum())
                assert nbad == 0, f"{self.tag} {what}{' +rowsum' if rs else ''}: {nbad} outputs differ"
                _frame_untouched(big, win, sentinel, f"{self.tag} {what}")

    def gelu(self, what, epi, dtype, variant):
        sc = self.p.scales[variant]
        g = self.p.ref("gelu")[:self.m, :self.n]
        kw = dict(out_scale=sc["out_gelu"]) if dtype == torch.int8 else {}
        outs = []
        for sentinel in _SENTINELS[dtype]:
            for rs in self._rs_variants():
                big, win = self.run(epi, dtype, sentinel, **kw, **rs)
                _frame_untouched(big, win, sentinel, f"{self.tag} {what}")
                outs.append(win.clone())
        assert all(torch.equal(o, outs[0]) for o in outs[1:]), f"{self.tag} {what}: runs differ"
        got = outs[0].cpu().numpy()
        if dtype == torch.int8:
            share, dist, bad = R.check_gelu_q8(got, g, sc["out_gelu"])
        else:
            share, dist, bad = R.check_gelu_f16(got, g)
        _note_gelu(what, share, dist, got.size)
        print(f"  [{self.tag}] {what}: {share:.2e} differ, largest boundary distance {dist:.3e}, violations {bad}")
        assert bad == 0, f"{self.tag} {what}: {bad} outputs differ beyond the GELU allowance (share {share:.2e})"
        return outs[0]

    def rowsum_out(self, what, epi, codes, out_scale):
        """rowsum_out prefilled with 5 accumulates exactly the row sums of the codes written."""
        acc = torch.full((self.m,), 5, dtype=torch.int32, device=self.dev)
        big, win = self.run(epi, torch.int8, 77, out_scale=out_scale, rowsum_out=acc)
        assert torch.equal(win, codes), f"{self.tag} {what} with rowsum_out: codes differ"
        want = codes.to(torch.int32).sum(1, dtype=torch.int32) + 5
        assert torch.equal(acc, want), f"{self.tag} {what}: rowsum_out is not prefill + row sums"


@pytest.mark.parametrize("fmt,k,group", [("w8", k, 0) for k in (128, 256, 384, 640)] +
                         [("w4", k, 0) for k in (128, 256, 384, 640)] + [("w4g", k, g) for k, g in GROUPED_KG])
def test_exact_i8_inputs_pin_the_epilogues(fmt, k, group):
    """CPU: what the GPU tests below rely on, for every problem and both variants, on the full
    1025 x 1152 problem and on its smallest slice in use (M = 1 .. 77, N = 64 .. 192).

    float64 and fp32 evaluations of y, of the mid fake quantiser and of the residual sum agree
    exactly, and so do the codes of a correctly rounded fp32 division.  "fine": at least 5 % of
    the quotients y / out_scale are exact ties, and round-half-away, truncation (>= 1e-3 of the
    codes) and a low clamp at -127 (>= 1e-4) all change the Q8 reference; dropping the mid
    quantiser or reading the residual bytes as unsigned changes >= 1e-3 of the Q8_RES reference.
    The clamp-edge quotients -128.5 and 127.5 both occur in the K = 640 problem of every format.  A plain
    reciprocal multiply is NOT detectable on these inputs: the product rounds back onto the tie."""
    p = R.problem(fmt, k, group)
    assert np.array_equal(p.y32().astype(np.float64), p.y)
    assert np.array_equal(p.ref("f32").astype(np.float64), p.y)
    assert np.array_equal(p.ref("resadd").astype(np.float64), p.y_resadd)
    assert np.abs(p.y).max() < 512 and np.abs(p.y_resadd).max() < 512
    for variant in ("fine", "sat"):
        sc = p.scales[variant]
        for win in (np.s_[:, :], np.s_[:77, :192]):
            y, r = p.y[win], p.res_i8[win]
            c = R.quant(y, sc["out"])
            assert np.array_equal(R.quant32(y.astype(np.float32), sc["out"]), c)
            # Q8_RES: mid fake quant, residual sum and final codes, fp32 against float64
            for mid in (sc["mid"], 0.0):
                x64 = y if mid <= 0 else R.quant(y, mid).astype(np.float64) * np.float64(mid)
                x32 = y.astype(np.float32) if mid <= 0 else R.quant32(y.astype(np.float32), mid).astype(np.float32) * mid
                assert np.array_equal(x32.astype(np.float64), x64)
                s64 = r.astype(np.float64) * np.float64(sc["res"]) + x64
                s32 = r.astype(np.float32) * sc["res"] + x32
                assert np.array_equal(s32.astype(np.float64), s64)
                assert np.array_equal(R.quant32(s32, sc["out_res"]), R.quant(s64, sc["out_res"]))
            cr = R.q8_res(y, r, sc["mid"], sc["res"], sc["out_res"])
            qt = y / np.float64(sc["out"])
            inside = float((np.abs(qt) < 128).mean())
            if variant == "sat":
                assert inside < 0.1 and float((np.abs(qt) > 130).mean()) > 0.8
                assert (c == 127).any() and (c == -128).any()
                continue
            assert inside > 0.8
            ties = float((qt - np.floor(qt) == 0.5).mean())
            assert ties >= 0.05, ties
            if k == 640 and y.size == p.y.size:
                assert (qt == -128.5).any() and (qt == 127.5).any()
            frac = lambda wrong, ref: float((wrong != ref).mean())
            assert frac(R.quant(y, sc["out"], half_even=False), c) >= 1e-3
            assert frac(np.clip(np.trunc(qt), -128, 127).astype(np.int8), c) >= 1e-3
            assert frac(R.quant(y, sc["out"], lo=-127), c) >= 1e-4
            assert frac(R.q8_res(y, r, 0.0, sc["res"], sc["out_res"]), cr) >= 1e-3
            assert frac(R.q8_res(y, r, sc["mid"], sc["res"], sc["out_res"], signed=False), cr) >= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,cfg,k,group", CASES, ids=_CASE_IDS)
def test_i8_gemm_tile_configs(cuda, fmt, cfg, k, group):
    """Every tile config of with_i8_cfg (per channel and grouped) on both weight formats, K = 128 (one K
    tile, shorter than any ring), 256, 384 and 640 (five tiles: wraps the 2- and the 3-slot ring),
    every epilogue but BIAS_GELU (below), at shapes A and B of _shapes().  F32, RESADD_F32, BIAS (= float16(y)), Q8 and
    Q8_RES (in place; separate R with ldr != ldc; mid_scale = 0) equal the float64 reference
    exactly, in the "fine" and the saturating variant.  W4 per channel: rowsum_out = prefill + the
    row sums of the written codes on every config; cfg 86 gives the same bits with the producer's
    row sums of A.

    Q8_GELU goes through the approximate GELU (gelu_r16_2, documented |error| 7.1e-7, fp32
    emulation): a code may differ from the float64 erf reference by one step, and only where the
    reference quotient lies within E / out_scale + 2 fp32 ulps of the midpoint, E = 1.42e-6
    (_i8_ref.check_gelu_q8).  Measured on gfx950 over 139 cases (these and a since-removed W4
    config), every difference one step: "fine"
    (out_scale 3 * 2^-7 / 2^-8) at most 5.5e-5 of a case's codes differ, the farthest 2.6e-5 of a
    code = 3.0e-7 from its midpoint; saturating (3 * 2^-13 / 2^-14) at most 3.4e-4 differ, the
    farthest 2.4e-3 of a code = 4.3e-7 from its midpoint (0.3 E).  The fp16 GELU epilogue is
    test_i8_gemm_bias_gelu_f16."""
    from samq import ops
    p = R.problem(fmt, k, group)
    w8 = fmt == "w8"
    print()
    for m, n in _shapes(fmt, cfg):
        c = _Case(p, cfg, m, n, cuda)
        fine, sat = p.scales["fine"], p.scales["sat"]
        c.exact("F32", ops.EPI_F32, torch.float32, p.ref("f32"))
        c.exact("BIAS", ops.EPI_BIAS, torch.float16, p.ref("f16"))
        c.exact("RESADD_F32", ops.EPI_RESADD_F32, torch.float32, p.ref("resadd"), prefill=p.res_f32)
        for v, sc in (("fine", fine), ("sat", sat)):
            c.exact(f"Q8 {v}", ops.EPI_Q8, torch.int8, p.ref("q8", v), out_scale=sc["out"])
        if w8:
            c.exact("Q8_RES in place", ops.EPI_Q8_RES, torch.int8, p.ref("q8_res", "fine"), prefill=p.res_i8,
                    res="alias", out_scale=fine["out_res"], mid=fine["mid"], res_scale=fine["res"])
            rbig, rwin = _frame(torch.int8, m, n, 0, cuda, extra=5)      # ldr = N + 80 != ldc = N + 48
            rwin.copy_(_t(p.res_i8[:m, :n], cuda))
            c.exact("Q8_RES separate R, sat", ops.EPI_Q8_RES, torch.int8, p.ref("q8_res", "sat"), res=rwin,
                    out_scale=sat["out_res"], mid=sat["mid"], res_scale=sat["res"])
            c.exact("Q8_RES mid_scale 0", ops.EPI_Q8_RES, torch.int8, p.ref("q8_res_nomid", "fine"), res=rwin,
                    out_scale=fine["out_res"], mid=0.0, res_scale=fine["res"])
        codes = {v: c.gelu(f"Q8_GELU {v}", ops.EPI_Q8_GELU, torch.int8, v) for v in ("fine", "sat")}
        if fmt == "w4":
            c.rowsum_out("Q8", ops.EPI_Q8, _t(p.ref("q8", "fine")[:m, :n], cuda), fine["out"])
            c.rowsum_out("Q8_GELU", ops.EPI_Q8_GELU, codes["fine"], fine["out_gelu"])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,cfg,k,group", CASES, ids=_CASE_IDS)
def test_i8_gemm_bias_gelu_f16(cuda, fmt, cfg, k, group):
    """BIAS_GELU (fp16 GELU(y)) on the cases and shapes of test_i8_gemm_tile_configs, against the
    float64 erf reference: an output may differ from float16(GELU(y)) only by ONE fp16 step and only
    where the reference lies within E = 1.42e-6 (twice the 7.1e-7 csrc/common.h documents for
    gelu_r16_2) of the rounding boundary between the two; nothing outside the window is written.

    This test caught the fp16 epilogue on gelu_r16_2: its absolute error was inside the documented
    bound (|out - GELU(y)| minus half an fp16 step <= 4.94e-7, one-step differences within 4.3e-7
    of the boundary), but 1.0e-2 .. 2.4e-2 of the outputs were 2 .. 8 fp16 steps off, all of them
    with |GELU(y)| <= 4.9e-4 (y in [-5.03, -3.64]) where one fp16 step is 6.0e-8 .. 2.4e-7, finer
    than an absolute error of 5e-7.  The epilogue now takes gelu_erfc2 (library erfc: relative
    accuracy down the negative tail).  Measured on gfx950 with it, over 139 cases (these and a
    since-removed W4 config): at most
    6.0e-4 of a case's outputs differ, every one by one step, the farthest 2.4e-7 from the
    boundary (0.17 E)."""
    from samq import ops
    p = R.problem(fmt, k, group)
    print()
    for m, n in _shapes(fmt, cfg):
        _Case(p, cfg, m, n, cuda).gelu("BIAS_GELU", ops.EPI_BIAS_GELU, torch.float16, "fine")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,cfg", [("w8", 91), ("w8", 84), ("w8", 92), ("w8", 83), ("w4", 81), ("w4", 86)])
def test_i8_gemm_row_count_edges(cuda, fmt, cfg):
    """M = 1, 31, 32, 33, BM - 1, BM, BM + 1 at N = 2 BN, K = 256: fewer rows than one tile, than one
    32-row epilogue slice, and a single row; Q8, BIAS and F32 exactly, nothing written outside."""
    from samq import ops
    p = R.problem(fmt, 256)
    bm, bn = TILES[cfg]
    n = 2 * bn
    for m in sorted({1, 31, 32, 33, bm - 1, bm, bm + 1}):
        c = _Case(p, cfg, m, n, cuda)
        sc = p.scales["fine"]
        c.exact("Q8", ops.EPI_Q8, torch.int8, p.ref("q8", "fine"), out_scale=sc["out"])
        c.exact("BIAS", ops.EPI_BIAS, torch.float16, p.ref("f16"))
        c.exact("F32", ops.EPI_F32, torch.float32, p.ref("f32"))
        if cfg == 86:
            c.rowsum_out("Q8", ops.EPI_Q8, _t(p.ref("q8", "fine")[:m, :n], cuda), sc["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", W8_CFGS)
def test_w8a8_gemm_v16_copy(cuda, cfg):
    """samq_w8a8_gemm_v16 on every W8 tile config, N = 768, M = 2 BM + 13, v_col0 = 64, 512, 704: the
    codes equal the plain Q8 run (and the reference), v16 holds the codes of columns >= v_col0 as
    fp16 and nothing else of the wider, taller v16 buffer is written.  Contract: v_col0 % 64 == 0
    (a wave's columns -- WN <= 64, static_assert in i8_epilogue_slice -- never straddle it)."""
    from samq import ops
    p = R.problem("w8", 256)
    n = 768
    m = 2 * (TILES[cfg][0] if cfg else 64) + 13
    dv, a = _dev(p, n, cuda), _a_window(p, m, cuda)
    sc = p.scales["fine"]
    ref = _t(p.ref("q8", "fine")[:m, :n], cuda)
    plain = ops.w8a8_gemm(a, dv.w, dv.ws, n, dv.bias, ops.EPI_Q8, float(p.a_scale), float(sc["out"]), cfg=cfg)
    assert torch.equal(plain, ref)
    for v0 in (64, 512, 704):
        ldv = n - v0 + 24
        vbig = torch.full((m + 2, ldv), 60000.0, dtype=torch.float16, device=cuda)
        big, win = _frame(torch.int8, m, n, 77, cuda)
        ops.w8a8_gemm_v16(a, dv.w, dv.ws, n, dv.bias, float(p.a_scale), float(sc["out"]), vbig[:m], v0, out=win,
                          cfg=cfg)
        assert torch.equal(win, ref), f"cfg {cfg} v_col0 {v0}: codes differ from the plain Q8 run"
        _frame_untouched(big, win, 77, f"v16 cfg {cfg} v_col0 {v0}")
        assert torch.equal(vbig[:m, :n - v0], ref[:, v0:].to(torch.float16)), f"cfg {cfg} v_col0 {v0}: v16"
        vbig[:m, :n - v0] = 60000.0
        assert bool((vbig == 60000.0).all()), f"cfg {cfg} v_col0 {v0}: v16 written outside its window"
    for v0 in (32, 96):   # the documented contract: multiples of 64 only
        with pytest.raises(AssertionError):
            ops.w8a8_gemm_v16(a, dv.w, dv.ws, n, dv.bias, float(p.a_scale), float(sc["out"]),
                              torch.zeros((m, n), dtype=torch.float16, device=cuda), v0, cfg=cfg)


@pytest.mark.gpu
def test_i8_gemm_refusals(cuda):
    """Every documented refusal raises and leaves the sentinel output untouched."""
    from samq import ops
    from samq import _lib
    p8, p4, pg = R.problem("w8", 128), R.problem("w4", 128), R.problem("w4g", 384, 128)
    m, n = 77, 256
    d8, d4, dg = _dev(p8, n, cuda), _dev(p4, n, cuda), _dev(pg, n, cuda)
    a = _a_window(p8, m, cuda)
    ag = _a_window(pg, m, cuda)
    a_s = float(p8.a_scale)
    DT = {ops.EPI_BIAS: torch.float16, ops.EPI_BIAS_GELU: torch.float16, ops.EPI_F32: torch.float32,
          ops.EPI_RESADD_F32: torch.float32}
    res = _t(p8.res_i8[:m, :n], cuda)

    def refused(what, fn, epi=ops.EPI_Q8, cols=n, exc=(AssertionError, NotImplementedError), win=None):
        dtype = DT.get(epi, torch.int8)
        big, w = _frame(dtype, m, cols, _SENTINELS[dtype][0], cuda)
        if win is not None:
            w = win(big)
        with pytest.raises(exc):
            fn(w)
        torch.cuda.synchronize()
        assert bool((big == _SENTINELS[dtype][0]).all()), f"{what}: the refused call wrote to its output"

    w8 = lambda out, aa=a, epi=ops.EPI_Q8, cfg=0, nn=n, **kw: ops.w8a8_gemm(
        aa, d8.w, d8.ws, nn, d8.bias, epi, a_s, kw.pop("out_scale", 0.05), out=out, cfg=cfg, **kw)
    refused("K % 128", lambda o: w8(o, aa=torch.zeros((m, 192), dtype=torch.int8, device=cuda)))
    refused("N % 64", lambda o: w8(o, nn=96), cols=96)
    refused("N % BN", lambda o: w8(o, cfg=81, nn=192), cols=192)
    refused("unknown cfg", lambda o: w8(o, cfg=7))
    for cfg in (85, 86, 93):   # 85 / 86: the W4 ping-pong kernel; 93: the id of a removed kernel, unknown
        refused(f"cfg {cfg} on W8", lambda o: w8(o, cfg=cfg))
    wide = torch.zeros((m, 128 + 24), dtype=torch.int8, device=cuda)
    refused("lda % 16", lambda o: w8(o, aa=wide[:, :128]))                       # lda = 152
    wide = torch.zeros((m, 128 + 16), dtype=torch.int8, device=cuda)
    refused("A + 8 bytes", lambda o: w8(o, aa=wide[:, 8:136]))
    refused("C + 8 bytes (int8)", w8, win=lambda big: big[:m, 8:8 + n])
    refused("C + 8 bytes (f16)", lambda o: w8(o, epi=ops.EPI_BIAS), epi=ops.EPI_BIAS, win=lambda big: big[:m, 4:4 + n])
    refused("C + 8 bytes (f32)", lambda o: w8(o, epi=ops.EPI_F32), epi=ops.EPI_F32, win=lambda big: big[:m, 2:2 + n])
    for epi, dtype, pad in ((ops.EPI_Q8, torch.int8, 8), (ops.EPI_BIAS, torch.float16, 4), (ops.EPI_F32, torch.float32, 2)):
        odd = torch.full((m, n + pad), _SENTINELS[dtype][0], dtype=dtype, device=cuda)   # ldc breaks 16-byte rows
        with pytest.raises(AssertionError):
            w8(odd[:, :n], epi=epi)
        torch.cuda.synchronize()
        assert bool((odd == _SENTINELS[dtype][0]).all())
    for epi in (ops.EPI_Q8, ops.EPI_Q8_GELU):
        refused("out_scale 0", lambda o: w8(o, epi=epi, out_scale=0.0))
    refused("out_scale 0 (Q8_RES)", lambda o: w8(o, epi=ops.EPI_Q8_RES, out_scale=0.0, mid_scale=0.04, res_scale=0.03,
                                                 res=res))
    refused("Q8_RES without R", lambda o: w8(o, epi=ops.EPI_Q8_RES, mid_scale=0.04, res_scale=0.03))
    refused("W4 without qzeros", lambda o: ops.i8_gemm(a, _lib.BF_W4, d4.w, d4.ws, n, d4.bias, None, ops.EPI_Q8, a_s,
                                                       0.05, out=o))
    refused("Q8_RES on W4", lambda o: ops.w4a8_gemm(a, d4.w, d4.ws, d4.qz, n, d4.bias, ops.EPI_Q8_RES, a_s, 0.05, out=o))
    grouped = lambda o, **kw: ops.w4a8_gemm(ag, dg.w, dg.ws, dg.qz, n, dg.bias, ops.EPI_Q8, a_s, 0.05, out=o,
                                            **{"groupsize": 128, **kw})
    refused("grouped cfg 81", lambda o: grouped(o, cfg=81))
    refused("grouped cfg 86", lambda o: grouped(o, cfg=86))
    refused("groupsize 64", lambda o: grouped(o, groupsize=64))
    rs = torch.full((m,), 5, dtype=torch.int32, device=cuda)
    for epi in (ops.EPI_BIAS, ops.EPI_F32):
        refused("rowsum_out, non-code epilogue",
                lambda o: ops.w4a8_gemm(a, d4.w, d4.ws, d4.qz, n, d4.bias, epi, a_s, out=o, rowsum_out=rs), epi=epi)
    # silently dropped arguments: grouped weights have no row-sum path
    refused("grouped rowsum", lambda o: grouped(o, rowsum=rs))
    refused("grouped rowsum_out", lambda o: grouped(o, rowsum_out=rs))
    assert bool((rs == 5).all())
    # ... and layernorm_q zeroes zero_rows only on its row-sum path
    x = torch.randn((m, 128), dtype=torch.float32, device=cuda)
    g1, b1 = torch.ones(128, device=cuda), torch.zeros(128, device=cuda)
    with pytest.raises(AssertionError):
        ops.layernorm_q(x, g1, b1, 1e-6, out_scale=0.05, zero_rows=rs)
    assert bool((rs == 5).all())


def _conv_case(rng, mode, b, cin, side, n):
    """Exact conv inputs: coarse codes (multiples of 16) with full-range channels, power-of-two
    a_scale * wscale[n], bias an integer multiple of it.  Returns NCHW float64 codes for conv2d."""
    g = side // 16 if mode == 1 else side
    x = (rng.integers(-8, 8, (b, cin, side, side)) * 16).astype(np.int8)
    x[:, ::3, ::5] = rng.integers(-128, 128, x[:, ::3, ::5].shape, dtype=np.int8)
    kk = 16 if mode == 1 else 3
    w = (rng.integers(-8, 8, (n, cin, kk, kk)) * 16).astype(np.int8)
    w[5::8] = rng.integers(-128, 128, w[5::8].shape, dtype=np.int8)
    e_col = -9 - rng.integers(0, 3, n)
    csc = np.float64(R.A_SCALE) * np.float64(2.0) ** e_col
    b_int = 256 * rng.integers(-12, 13, n)
    pos = rng.integers(-128, 128, (g * g, n), dtype=np.int8)
    return x, w, (np.float64(2.0) ** e_col).astype(np.float32), b_int, csc, pos, g


_CONV = ([(1, 2, 3, 32), (1, 2, 3, 128)] +
         [(2, b, cin, g) for cin in (128, 256) for g in (1, 2, 3, 12) for b in (1, 2)])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,b,cin,side", _CONV)
def test_w8a8_conv_gemm_vs_conv2d(cuda, mode, b, cin, side):
    """The implicit-GEMM convolutions against torch.nn.functional.conv2d in float64 on the integer
    codes followed by the numpy quantiser, exactly: the 16x16 / stride-16 PatchEmbed (NCHW, Cin = 3,
    sides 32 and 128) and the 3x3 / pad-1 neck conv (NHWC) on 1x1, 2x2, 3x3 and 12x12 grids, B = 1
    and 2 -- every tap of the zero-padding gather is hit, M runs from 1 to 288.  Q8 everywhere;
    Q8_RES with the per-image residual rows (rmod) in patch mode and on the 12x12 grid."""
    import torch.nn.functional as F
    from samq import ops
    n = 192
    rng = np.random.Generator(np.random.PCG64([mode, b, cin, side]))
    x, w, ws, b_int, csc, pos, g = _conv_case(rng, mode, b, cin, side, n)
    xt, wt = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    acc = (F.conv2d(xt, wt, stride=16) if mode == 1 else F.conv2d(xt, wt, padding=1)).permute(0, 2, 3, 1).numpy()
    assert np.abs(acc + b_int).max() < 2 ** 24
    y = (acc + b_int) * csc                                          # (B, G, G, N) float64, exact
    std = float(y.std()) or 1.0
    e = int(np.floor(np.log2(std / 48)))
    s_out, s_mid, s_res = np.float32(3 * 2.0 ** e), np.float32(5 * 2.0 ** (e - 1)), np.float32(7 * 2.0 ** (e - 2))
    if mode == 1:
        xk, wk = x, w.reshape(n, -1)
    else:
        xk, wk = np.ascontiguousarray(x.transpose(0, 2, 3, 1)), np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(n, -1)
    dx, dw = _t(xk, cuda), ops.w8_repack(_t(wk, cuda))
    dws, db = _t(ws, cuda), _t((b_int * csc).astype(np.float32), cuda)
    a_s = float(R.A_SCALE)
    out = ops.w8a8_conv_gemm(dx, mode, dw, dws, n, db, ops.EPI_Q8, a_s, float(s_out))
    assert out.shape == (b, g, g, n)
    ref = R.quant(y, s_out)
    assert np.array_equal(out.cpu().numpy(), ref), "Q8"
    if mode == 1 or g == 12:
        r = np.broadcast_to(pos.reshape(1, g, g, n), y.shape)
        ref = R.q8_res(y, np.ascontiguousarray(r), s_mid, s_res, s_out)
        out = ops.w8a8_conv_gemm(dx, mode, dw, dws, n, db, ops.EPI_Q8_RES, a_s, float(s_out), mid_scale=float(s_mid),
                                 res_scale=float(s_res), res=_t(pos, cuda), rmod=g * g)
        assert np.array_equal(out.cpu().numpy(), ref), "Q8_RES with rmod"
