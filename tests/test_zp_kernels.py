"""The kernels that take activation zero points -- samq_quantize_zp, samq_layernorm_q_zp,
samq_i8_gemm_zp, samq_w8a8_conv_gemm_zp -- against CPU references (tests/_zp_ref.py), and CPU-only
checks that the chosen inputs can see the mistakes such kernels make: the zero point added after
the rounding, col_offset dropped on a column, the residual's zero point ignored, a zero pad code.
"""
import numpy as np
import pytest
import torch

import _i8_ref as R
import _zp_ref as Z

# BM, BN of the W8 tile configs (with_i8_cfg, csrc/gemm_i8.hip)
TILES = {81: (256, 256), 82: (128, 256), 83: (128, 128), 84: (64, 64), 87: (128, 64), 88: (64, 128), 89: (64, 64),
         90: (64, 128), 91: (32, 64), 92: (64, 32), 180: (128, 128), 181: (128, 64), 182: (128, 128)}
W8_CFGS = [0] + sorted(TILES)
LN_WIDTHS = (4, 252, 260, 516, 772, 1024, 1028, 1280, 1284, 2560, 4092, 4096)   # every VPT branch
LN_MAX_SHARE = 1e-3      # test_quantize_and_layernorm_q's bound


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


# ============================================================================= CPU: what the inputs can see
def test_quantiser_inputs_pin_the_zero_point_order():
    """rint(q + zp) against the wrong rint(q) + zp: equal for even zero points, different on the
    exact ties for odd ones; fp32 and float64 evaluations of the contract agree on these operands."""
    for dtype in (np.float32, np.float16):
        v = Z.quant_operands(dtype)
        fin = np.isfinite(v.astype(np.float64))
        for zp in Z.QUANT_ZPS:
            ref = Z.quant32(v, Z.TIE_SCALE, zp)
            assert np.array_equal(ref[fin], Z.quant64(v.astype(np.float64)[fin], Z.TIE_SCALE, zp))
            wrong = Z.quant32(v, Z.TIE_SCALE, zp, after=True)
            assert ref.min() == -128 and ref.max() == 127
            if zp % 2:
                assert (wrong != ref).sum() >= 50, zp      # the ties inside the code range
            else:
                assert np.array_equal(wrong, ref)


@pytest.mark.parametrize("k", (128, 384))
def test_gemm_inputs_pin_the_zero_points(k):
    """On the GEMM problem: fp32 and float64 agree; zero point after the rounding, col_offset dropped
    on one column, the residual zero point ignored and the mid zero point ignored each change the
    reference; the all-positive weight row makes col_offset large against its sums."""
    p = Z.gemm_problem(k)
    sc = p.scales
    y = p.y()
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    q = y / np.float64(sc["out"])
    assert float((q - np.floor(q) == 0.5).mean()) >= 0.02
    ref = Z.quant32(y, sc["out"], Z.ZP_OUT)
    assert np.array_equal(ref, Z.quant64(y, sc["out"], Z.ZP_OUT))
    frac = lambda wrong, good: float((wrong != good).mean())
    assert frac(Z.quant32(y, sc["out"], Z.ZP_OUT, after=True), ref) >= 1e-3
    coff = p.col_offset.copy()
    coff[Z.POS_ROW] = 0
    y_drop = p.y(coff)
    assert np.array_equal(y_drop[:, :Z.POS_ROW], y[:, :Z.POS_ROW])
    assert frac(Z.quant32(y_drop, sc["out"], Z.ZP_OUT)[:, Z.POS_ROW], ref[:, Z.POS_ROW]) >= 0.5
    for rmod in (0, Z.RMOD):
        r = p.residual(rmod)
        args = (sc["mid"], sc["res"], sc["out_res"])
        good = Z.q8_res(y, r, *args, Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT)
        assert frac(Z.q8_res(y, r, *args, Z.ZP_MID, 0, Z.ZP_OUT), good) >= 0.5          # residual zp ignored
        assert frac(Z.q8_res(y, r, *args, 0, Z.ZP_RES, Z.ZP_OUT), good) >= 1e-3          # mid zp ignored
        assert frac(Z.q8_res(y, r, *args, Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT, after=True), good) >= 1e-3
        assert frac(Z.q8_res(y, r, 0.0, *args[1:], Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT), good) >= 1e-3   # no mid quantiser
    assert frac(Z.q8_res(y, p.residual(0), *args, Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT),
                Z.q8_res(y, p.residual(Z.RMOD), *args, Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT)) >= 0.5


@pytest.mark.parametrize("side", (2, 3))
def test_conv_inputs_pin_the_pad_code(side):
    """3x3 conv: padding with the code 0 instead of the zero-point code changes every border pixel's
    sums (all of side 2, all but the centre of side 3); im2col + col_offset equals the convolution of
    x - zp."""
    x, w, ws, b_int, csc, pos, g = Z.conv_problem(2, 1, 128, side, 64)
    good = Z.conv_acc(x, w, 2, Z.ZP_A)
    wk = w.transpose(0, 2, 3, 1).reshape(64, -1).astype(np.float64)
    coff = -Z.ZP_A * wk.sum(1)
    a = Z.im2col(x, 2, Z.ZP_A).astype(np.float64)
    assert np.array_equal((a @ wk.T + coff).reshape(good.shape), good)
    bad = Z.conv_acc(x, w, 2, Z.ZP_A, pad_code=0)
    differs = (bad != good).any(-1)[0]
    border = np.ones((side, side), bool)
    border[1:-1, 1:-1] = False
    assert differs[border].all() and not differs[~border].any()


# ============================================================================= quantiser
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", (np.float32, np.float16), ids=("f32", "f16"))
def test_quantize_zp(cuda, dtype):
    """samq_quantize_zp, n = 4099 (vector part and a 3-element tail), codes and fake output, bit for
    bit against the fp32 formula on every exact tie, both saturated ends and a non-dyadic scale;
    zp = 0 equals samq_quantize."""
    from samq import ops
    v = Z.quant_operands(dtype)
    x = _t(v, cuda)
    for s in (Z.TIE_SCALE, np.float32(0.037)):
        for zp in Z.QUANT_ZPS:
            ref = Z.quant32(v, s, zp)
            codes = ops.quantize_zp(x, float(s), zp)
            assert codes.dtype == torch.int8
            assert np.array_equal(codes.cpu().numpy(), ref), (dtype, s, zp)
            fq = ops.quantize_zp(x, float(s), zp, fake=True).cpu().numpy()
            assert np.array_equal(fq, Z.fake32(ref, s, zp)), (dtype, s, zp)
        assert torch.equal(ops.quantize_zp(x, float(s), 0), ops.quantize(x, float(s)))
        assert torch.equal(ops.quantize_zp(x, float(s), 0, fake=True), ops.quantize(x, float(s), fake=True))
    for zp in (-129, 128):
        with pytest.raises(AssertionError):
            ops.quantize_zp(x, 0.05, zp)
    with pytest.raises(AssertionError):
        ops.quantize_zp(x, 0.0, 3)


# ============================================================================= LayerNorm
@pytest.mark.gpu
@pytest.mark.parametrize("c", LN_WIDTHS)
def test_layernorm_q_zp(cuda, c):
    """samq_layernorm_q_zp on 37 rows of full-range int8 codes, every (zp_in, zp_out) of
    {-128, -3, 0, 90}^2 and every rows-per-wave: codes within +-1 of the float64 reference, the
    off-by-one share over the case at most 1e-3; the f32 fake output is (code - zp_out) * out_scale
    exactly; zero points 0 equal samq_layernorm_q bit for bit."""
    from samq import ops
    codes, gamma, beta = Z.ln_problem(c)
    xd, gd, bd = codes.to(cuda), gamma.to(cuda), beta.to(cuda)
    s_in = float(Z.LN_IN_SCALE)
    off = tot = 0
    for eps in (1e-6, 1e-5):
        for zi in Z.LN_ZPS:
            y64 = Z.ln64(codes, zi, gamma, beta, eps)
            s_out = np.float32(np.abs(y64).max() / 100.0)
            for zo in Z.LN_ZPS:
                ref = np.clip(np.rint(y64 / np.float64(s_out) + zo), -128, 127).astype(np.int64)
                outs = [ops.layernorm_q_zp(xd, gd, bd, eps, s_in, float(s_out), zi, zo, rows_per_wave=r)
                        for r in (0, 1, 2, 4)]
                for o in outs[1:]:
                    assert torch.equal(o, outs[0]), (c, zi, zo)
                got = outs[0].cpu().numpy().astype(np.int64)
                d = np.abs(got - ref)
                assert d.max() <= 1, f"c {c} zp {zi} -> {zo}: code off by {d.max()}"
                off += int((d > 0).sum())
                tot += d.size
                fq = ops.layernorm_q_zp(xd, gd, bd, eps, s_in, float(s_out), zi, zo, out_dtype=torch.float32)
                assert np.array_equal(fq.cpu().numpy(), Z.fake32(got, s_out, zo)), (c, zi, zo)
        s_out = 0.03
        for r in (0, 1, 2, 4):
            assert torch.equal(ops.layernorm_q_zp(xd, gd, bd, eps, s_in, s_out, 0, 0, rows_per_wave=r),
                               ops.layernorm_q(xd, gd, bd, eps, in_scale=s_in, out_scale=s_out, rows_per_wave=r))
        assert torch.equal(ops.layernorm_q_zp(xd, gd, bd, eps, s_in, s_out, 0, 0, out_dtype=torch.float32),
                           ops.layernorm_q(xd, gd, bd, eps, in_scale=s_in, out_scale=s_out, out_dtype=torch.float32))
    print(f"\n  layernorm_q_zp c {c}: {off} of {tot} codes off by one ({off / tot:.2e})")
    assert off / tot <= LN_MAX_SHARE
    with pytest.raises(AssertionError):
        ops.layernorm_q_zp(xd, gd, bd, 1e-6, s_in, 0.03, 128, 0)


# ============================================================================= GEMM
class _GemmDev:
    def __init__(self, p, n, dev):
        from samq import ops
        self.w = ops.w8_repack(_t(p.w[:n], dev))
        self.ws = _t(p.p.wscale[:n], dev)
        self.bias = _t(p.p.bias[:n], dev)
        self.coff = _t(p.col_offset[:n], dev)
        assert torch.equal(ops.w8a8_col_offset(_t(p.w[:n], dev), Z.ZP_A), self.coff)


def _frame(m, n, sentinel, dev):
    big = torch.full((m + 3, n + 48), sentinel, dtype=torch.int8, device=dev)
    return big, big[:m, 16:16 + n]


def _outside_untouched(big, win, sentinel):
    chk = big.clone()
    chk[:win.shape[0], 16:16 + win.shape[1]] = sentinel
    return bool((chk == sentinel).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", W8_CFGS)
def test_i8_gemm_zp(cuda, cfg):
    """samq_i8_gemm_zp on every W8 tile config and the automatic pick (N = 192 -> 89, 1152 -> 90):
    M = 77 (a partial row tile), K = 128 and 384, N = one and two tile widths, input codes with -128
    and 127, an all-positive weight row, four distinct non-zero zero points (mid and out odd, exact-tie
    quotients).  Q8 and Q8_RES (mid quantiser on / off, rmod on / off, in place and with a separate R)
    equal the fp32 reference bit for bit and write nothing outside the M x N window; Q8_GELU by the
    rule of _zp_ref.check_gelu_q8_zp; zero points 0 with a null col_offset equal samq_i8_gemm_cfg."""
    from samq import ops
    m = Z.GEMM_M
    bn = TILES[cfg][1] if cfg else 0
    widths = (192, 1152) if cfg == 0 else (bn, 2 * bn) if bn % 64 == 0 else (2 * bn, 4 * bn)   # N % 64 == 0
    for k in (128, 384):
        p = Z.gemm_problem(k)
        sc = p.scales
        a_big = torch.full((m, k + 48), 99, dtype=torch.int8, device=cuda)
        a = a_big[:, 16:16 + k]
        a.copy_(_t(p.a, cuda))
        y = p.y()
        for n in widths:
            dv = _GemmDev(p, n, cuda)
            yn = y[:, :n]
            kw = dict(bias=dv.bias, a_scale=float(p.p.a_scale), cfg=cfg, col_offset=dv.coff)

            def run(epi, sentinel=77, prefill=None, **kws):
                big, win = _frame(m, n, sentinel, cuda)
                if prefill is not None:
                    win.copy_(prefill)
                if isinstance(kws.get("res"), str):   # "alias": R is the output window itself
                    kws["res"] = win
                ops.i8_gemm_zp(a, dv.w, dv.ws, n, epilogue=epi, out=win, **kw, **kws)
                assert _outside_untouched(big, win, sentinel), f"cfg {cfg} {m}x{n}x{k}: wrote outside the window"
                return win.cpu().numpy()

            tag = f"cfg {cfg} {m}x{n}x{k}"
            ref = Z.quant32(yn, sc["out"], Z.ZP_OUT)
            for sentinel in (77, -78):
                assert np.array_equal(run(ops.EPI_Q8, sentinel, out_scale=float(sc["out"]), out_zp=Z.ZP_OUT), ref), \
                    f"{tag} Q8"
            for rmod in (0, Z.RMOD):
                r = p.residual(rmod)[:, :n]
                rdev = _t(p.res_i8[:rmod or m, :n], cuda)
                for mid in (sc["mid"], 0.0):
                    ref = Z.q8_res(yn, r, mid, sc["res"], sc["out_res"], Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT)
                    got = run(ops.EPI_Q8_RES, res=rdev, rmod=rmod, out_scale=float(sc["out_res"]), mid_scale=float(mid),
                              res_scale=float(sc["res"]), mid_zp=Z.ZP_MID, res_zp=Z.ZP_RES, out_zp=Z.ZP_OUT)
                    assert np.array_equal(got, ref), f"{tag} Q8_RES rmod {rmod} mid {mid}"
            ref = Z.q8_res(yn, p.res_i8[:, :n], sc["mid"], sc["res"], sc["out_res"], Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT)
            got = run(ops.EPI_Q8_RES, prefill=_t(p.res_i8[:, :n], cuda), res="alias", out_scale=float(sc["out_res"]),
                      mid_scale=float(sc["mid"]), res_scale=float(sc["res"]), mid_zp=Z.ZP_MID, res_zp=Z.ZP_RES,
                      out_zp=Z.ZP_OUT)
            assert np.array_equal(got, ref), f"{tag} Q8_RES in place"
            got = run(ops.EPI_Q8_GELU, out_scale=float(sc["out_gelu"]), out_zp=Z.ZP_OUT)
            share, bad = Z.check_gelu_q8_zp(got, R.gelu(yn), sc["out_gelu"], Z.ZP_OUT)
            print(f"  [{tag}] Q8_GELU: {share:.2e} differ, violations {bad}")
            assert bad == 0, f"{tag} Q8_GELU: {bad} codes differ beyond the GELU allowance"
            # zero points 0, no col_offset: the symmetric kernel's bits
            kw0 = dict(kw, col_offset=None)
            rdev = _t(p.res_i8[:, :n], cuda)
            for epi, args in ((ops.EPI_Q8, dict(out_scale=float(sc["out"]))),
                              (ops.EPI_Q8_GELU, dict(out_scale=float(sc["out_gelu"]))),
                              (ops.EPI_Q8_RES, dict(out_scale=float(sc["out_res"]), mid_scale=float(sc["mid"]),
                                                    res_scale=float(sc["res"]), res=rdev))):
                z = ops.i8_gemm_zp(a, dv.w, dv.ws, n, epilogue=epi, **kw0, **args)
                sym = ops.w8a8_gemm(a, dv.w, dv.ws, n, dv.bias, epi, float(p.p.a_scale), cfg=cfg, **args)
                assert torch.equal(z, sym), f"{tag} epilogue {epi}: zero zero points differ from samq_i8_gemm_cfg"


@pytest.mark.gpu
def test_i8_gemm_zp_refusals(cuda):
    """Unsupported epilogues, W4-only tile configs, zero points outside [-128, 127], a misplaced
    residual: each raises and leaves the output untouched."""
    from samq import ops
    p = Z.gemm_problem(128)
    m, n = Z.GEMM_M, 256
    dv = _GemmDev(p, n, cuda)
    a = _t(p.a, cuda)
    base = dict(bias=dv.bias, a_scale=0.02, out_scale=0.05, col_offset=dv.coff)

    def refused(exc, dtype=torch.int8, **kws):
        out = torch.full((m, n), 77, dtype=dtype, device=cuda)
        with pytest.raises(exc):
            ops.i8_gemm_zp(a, dv.w, dv.ws, n, out=out, **{**base, **kws})
        torch.cuda.synchronize()
        assert bool((out == 77).all())

    refused(NotImplementedError, dtype=torch.float16, epilogue=ops.EPI_BIAS)
    refused(NotImplementedError, dtype=torch.float16, epilogue=ops.EPI_BIAS_GELU)
    refused(NotImplementedError, dtype=torch.float32, epilogue=ops.EPI_F32)
    refused(NotImplementedError, dtype=torch.float32, epilogue=ops.EPI_RESADD_F32)
    for cfg in (85, 86, 7):
        refused(AssertionError, cfg=cfg)
    for name in ("mid_zp", "res_zp", "out_zp"):
        for z in (-129, 128):
            refused(AssertionError, **{name: z})
    refused(AssertionError, out_scale=0.0)
    refused(AssertionError, epilogue=ops.EPI_Q8_RES, res_scale=0.03)                       # no residual
    refused(AssertionError, col_offset=dv.coff[:n - 1])


# ============================================================================= convolutions
def _conv_run(cuda, mode, b, cin, side, n, epi):
    """One conv problem through samq_w8a8_conv_gemm_zp, through im2col + samq_i8_gemm_zp and on the CPU."""
    from samq import ops
    x, w, ws, b_int, csc, pos, g = Z.conv_problem(mode, b, cin, side, n)
    acc = Z.conv_acc(x, w, mode, Z.ZP_A)
    assert np.abs(acc + b_int).max() < 2 ** 24
    y = (acc + b_int) * csc
    std = float(y.std()) or 1.0
    e = int(np.floor(np.log2(std / 48)))
    s_out, s_mid, s_res = np.float32(3 * 2.0 ** e), np.float32(5 * 2.0 ** (e - 1)), np.float32(7 * 2.0 ** (e - 2))
    if mode == 1:
        xk, wk = x, w.reshape(n, -1)
    else:
        xk = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
        wk = np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(n, -1)
    dwk = _t(wk, cuda)
    dw, dws, db = ops.w8_repack(dwk), _t(ws, cuda), _t((b_int * csc).astype(np.float32), cuda)
    coff = ops.w8a8_col_offset(dwk, Z.ZP_A)
    pad16 = torch.full((16,), Z.ZP_A, dtype=torch.int8, device=cuda)
    a_s = float(R.A_SCALE)
    kw = dict(bias=db, epilogue=epi, a_scale=a_s, out_scale=float(s_out), col_offset=coff, out_zp=Z.ZP_OUT)
    if epi == ops.EPI_Q8_RES:
        kw.update(mid_scale=float(s_mid), res_scale=float(s_res), res=_t(pos, cuda), rmod=g * g, mid_zp=Z.ZP_MID,
                  res_zp=Z.ZP_RES)
        r = np.broadcast_to(pos.reshape(1, g, g, n), y.shape)
        ref = Z.q8_res(y, r, s_mid, s_res, s_out, Z.ZP_MID, Z.ZP_RES, Z.ZP_OUT)
    else:
        ref = Z.quant32(y, s_out, Z.ZP_OUT)
    out = ops.w8a8_conv_gemm_zp(_t(xk, cuda), mode, dw, dws, n, pad16=pad16 if mode == 2 else None, **kw)
    assert out.shape == (b, g, g, n)
    explicit = ops.i8_gemm_zp(_t(Z.im2col(x, mode, Z.ZP_A), cuda), dw, dws, n, **kw)
    assert torch.equal(out.reshape(-1, n), explicit), "implicit GEMM differs from im2col + samq_i8_gemm_zp"
    assert np.array_equal(out.cpu().numpy(), ref), "differs from the CPU reference"
    return out


@pytest.mark.gpu
def test_conv_gemm_zp_patch(cuda):
    """Mode 1 (PatchEmbed) at side 32: 2x2 patches, two images, Q8 and Q8_RES with the pos_embed
    codes shared by the images (rmod = 4)."""
    from samq import ops
    for epi in (ops.EPI_Q8, ops.EPI_Q8_RES):
        _conv_run(cuda, 1, 2, 3, 32, 64, epi)


@pytest.mark.gpu
@pytest.mark.parametrize("side", (2, 3))
def test_conv_gemm_zp_3x3(cuda, side):
    """Mode 2 (neck 3x3, padding 1) at side 2 (every pixel on the border) and 3 (one interior pixel),
    Cin 128, N 64: the gather pads with the zero-point code from pad16."""
    from samq import ops
    for epi in (ops.EPI_Q8, ops.EPI_Q8_RES):
        _conv_run(cuda, 2, 1, 128, side, 64, epi)
    x = torch.zeros((1, side, side, 128), dtype=torch.int8, device=cuda)
    w = ops.w8_repack(torch.zeros((64, 9 * 128), dtype=torch.int8, device=cuda))
    ws = torch.ones(64, device=cuda)
    with pytest.raises(AssertionError):      # 3x3 mode without pad16
        ops.w8a8_conv_gemm_zp(x, 2, w, ws, 64, out_scale=0.05)
    with pytest.raises(NotImplementedError):
        ops.w8a8_conv_gemm_zp(x, 2, w, ws, 64, epilogue=ops.EPI_Q8_GELU, out_scale=0.05,
                              pad16=torch.zeros(16, dtype=torch.int8, device=cuda))
