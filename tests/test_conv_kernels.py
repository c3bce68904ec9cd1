"""Implicit-GEMM convolutions (csrc/conv_gemm.hip, samq_w8a8_conv_gemm in csrc/gemm_i8.hip) on
ragged shapes: B = 3 images of a 5 x 5 grid (M = 75: one 128-row tile that straddles three images and
ends ragged), 7 x 7 (two tiles), single K steps, 1 x 1 to 3 x 3 grids where the padding dominates,
bias / pos present or NULL, u8 images cut inside an 8-pixel chunk.

Two kinds of case.  Exact: small integers (or k / 64 for the u8 paths with mean 128, std 64), so every
partial sum is representable and any summation order, MFMA's included, must reproduce the float64
reference bit for bit -- one wrong pixel, tap, channel, pad or pos row changes the result.  Random:
one case per kernel against float64 with the bounds of the existing tests (the per-element fp32
summation bound for the fp32-MFMA kernel).  Every output is a window of a 0x5A-filled buffer.

Kernel -> tests:

* ``conv_gemm_kernel<CG_PATCH>``: test_patch_embed_exact[*-f16], test_patch_embed_random
* ``conv_gemm_kernel<CG_PATCH_U8>``: test_patch_embed_u8_exact[p16-f16, p8-f16]
* ``conv_gemm_kernel<CG_1X1_F32>`` / ``<CG_3X3>``: test_conv1x1_exact, test_conv3x3_exact, test_neck_convs_random
* ``patch_embed_x3_kernel<false>`` / ``<true>``: test_patch_embed_exact[*-f32split], test_patch_embed_random /
  test_patch_embed_u8_exact[p16-f32split], test_patch_embed_u8_random_f32_weights[16]
* ``patch_embed_f32_kernel<false>`` / ``<true>``: test_patch_embed_f32_mfma_exact, test_patch_embed_random /
  test_patch_embed_u8_exact[p4-f32mfma, p12-f32mfma], test_patch_embed_u8_random_f32_weights[4, 12]
* int8 ``AG_PATCH`` / ``AG_3X3`` x ``EPI_Q8`` (bias, no bias) / ``EPI_Q8_RES`` (rmod = G * G, rmod = 0; with and
  without mid_scale): test_w8a8_conv_gemm_exact[*-patch-g5] / [*-3x3-g1, g2, g5]
"""
import numpy as np
import pytest
import torch

import _i8_ref as I8
import _rowconv_ref as R

pytestmark = pytest.mark.gpu
B = 3
BIAS_POS = [(True, True), (True, False), (False, True), (False, False)]
F16_SHAPES = [(16, 3, 5), (8, 3, 5), (8, 1, 5), (8, 4, 5), (16, 3, 7), (8, 3, 7), (8, 1, 7), (8, 4, 7)]
F32_MFMA_SHAPES = [(4, 3, 5), (4, 4, 5), (12, 3, 5)]


def _gen(*seed):
    return torch.Generator().manual_seed(int(np.random.SeedSequence(list(seed)).generate_state(1)[0]))


def _opt(t, cuda, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(cuda).contiguous()


def _equal(fr, ref64, dtype, what):
    assert fr.untouched(), what + ": wrote outside its window"
    want = ref64.to(dtype)
    assert torch.equal(want.double(), ref64), what + ": the reference is not exact in the output type"
    got = fr.t.cpu()
    bad = (got != want.view(got.shape))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}"


def _close(fr, ref64, rel, what):
    assert fr.untouched(), what + ": wrote outside its window"
    err = (fr.t.cpu().double() - ref64.view(fr.t.shape)).abs().max().item()
    bound = rel * max(1.0, ref64.abs().max().item())
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def _patch_inputs(patch, cin, grid, n, lim, seed):
    g = _gen(seed, patch, cin, grid, n)
    s = patch * grid
    x = R.ints(g, -lim, lim, (B, cin, s, s))
    w = R.ints(g, -lim, lim, (n, cin * patch * patch))
    bias = R.ints(g, -50, 50, (n,))
    pos = R.ints(g, -50, 50, (grid, grid, n))
    return x, w, bias, pos


# ----------------------------------------------------------------------------- patch embedding
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32split"])
@pytest.mark.parametrize("patch,cin,grid", F16_SHAPES)
def test_patch_embed_exact(cuda, patch, cin, grid, dtype):
    """conv_gemm_kernel<CG_PATCH> (f16) and patch_embed_x3_kernel<false> (f32, split fp16)."""
    from samq import ops
    for n in (128, 256):
        x, w, bias, pos = _patch_inputs(patch, cin, grid, n, 4, 1)
        xd, wd = _opt(x, cuda, dtype), _opt(w, cuda, dtype)
        for has_b, has_p in BIAS_POS:
            b, p = (bias if has_b else None), (pos if has_p else None)
            fr = R.Frame((B, grid, grid, n), torch.float32, cuda)
            ops.patch_embed(xd, wd, _opt(b, cuda), _opt(p, cuda), patch, out=fr.t)
            torch.cuda.synchronize()
            _equal(fr, R.patch_ref(x, w, b, p, patch), torch.float32,
                   f"patch={patch} Cin={cin} grid={grid} N={n} bias={has_b} pos={has_p} {dtype}")


@pytest.mark.parametrize("patch,cin,grid", F32_MFMA_SHAPES)
def test_patch_embed_f32_mfma_exact(cuda, patch, cin, grid):
    """patch_embed_f32_kernel<false>: patch % 8 != 0 (K = 48, 64, 432; 16-wide K steps)."""
    from samq import ops
    for n in (128, 256):
        x, w, bias, pos = _patch_inputs(patch, cin, grid, n, 4, 2)
        xd, wd = _opt(x, cuda), _opt(w, cuda)
        for has_b, has_p in BIAS_POS:
            b, p = (bias if has_b else None), (pos if has_p else None)
            fr = R.Frame((B, grid, grid, n), torch.float32, cuda)
            ops.patch_embed(xd, wd, _opt(b, cuda), _opt(p, cuda), patch, out=fr.t)
            torch.cuda.synchronize()
            _equal(fr, R.patch_ref(x, w, b, p, patch), torch.float32,
                   f"patch={patch} Cin={cin} N={n} bias={has_b} pos={has_p}")


def _rand_patch(patch, cin, grid, n, seed):
    g = _gen(seed, patch, cin, grid)
    s = patch * grid
    return (torch.randn(B, cin, s, s, generator=g), torch.randn(n, cin * patch * patch, generator=g) * 0.02,
            torch.randn(n, generator=g) * 0.02, torch.randn(grid, grid, n, generator=g) * 0.1)


def _f32_sum_bound(fr, x64, w64, bias, pos, patch, what):
    """True fp32 MFMA: |out - ref| <= (K + 4) 2^-24 (sum_k |a_k w_k| + |bias| + |pos|) per element."""
    assert fr.untouched(), what + ": wrote outside its window"
    ref = R.patch_ref(x64, w64, bias.double(), pos.double(), patch)
    mag = R.patch_abs_ref(x64, w64, bias.double(), pos.double(), patch)
    bound = (w64.shape[1] + 4) * R.F32_EPS * mag
    err = (fr.t.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), f"{what}: worst {float((err / bound).max()):.3f} of the bound"


def test_patch_embed_random(cuda):
    """One random-value case per kernel against float64: f16 2e-5, split fp16 2e-6 (its hi / lo'
    split is invisible to exact inputs), fp32 MFMA the summation bound."""
    from samq import ops
    n, grid = 256, 5
    x, w, bias, pos = _rand_patch(16, 3, grid, n, 3)
    fr = R.Frame((B, grid, grid, n), torch.float32, cuda)
    ops.patch_embed(_opt(x, cuda, torch.float16), _opt(w, cuda, torch.float16), _opt(bias, cuda), _opt(pos, cuda), 16, out=fr.t)
    _close(fr, R.patch_ref(x.half().double(), w.half().double(), bias.double(), pos.double(), 16), 2e-5, "f16")
    for patch, cin in ((16, 3), (8, 3)):
        x, w, bias, pos = _rand_patch(patch, cin, grid, n, 4)
        fr = R.Frame((B, grid, grid, n), torch.float32, cuda)
        ops.patch_embed(_opt(x, cuda), _opt(w, cuda), _opt(bias, cuda), _opt(pos, cuda), patch, out=fr.t)
        _close(fr, R.patch_ref(x.double(), w.double(), bias.double(), pos.double(), patch), 2e-6, f"split p={patch}")
    for patch, cin in ((4, 3), (12, 3)):
        x, w, bias, pos = _rand_patch(patch, cin, grid, n, 5)
        fr = R.Frame((B, grid, grid, n), torch.float32, cuda)
        ops.patch_embed(_opt(x, cuda), _opt(w, cuda), _opt(bias, cuda), _opt(pos, cuda), patch, out=fr.t)
        torch.cuda.synchronize()
        _f32_sum_bound(fr, x.double(), w.double(), bias, pos, patch, f"fp32 MFMA p={patch}")


# ----------------------------------------------------------------------------- u8 patch embedding
def _u8_sizes(size):
    return [(size, size), (size - 3, size - 13), (1, 1)]


@pytest.mark.parametrize("patch,wdtype", [(16, torch.float16), (8, torch.float16), (16, torch.float32),
                                          (4, torch.float32), (12, torch.float32)],
                         ids=["p16-f16", "p8-f16", "p16-f32split", "p4-f32mfma", "p12-f32mfma"])
def test_patch_embed_u8_exact(cuda, patch, wdtype):
    """conv_gemm_kernel<CG_PATCH_U8>, patch_embed_x3_kernel<true>, patch_embed_f32_kernel<true>:
    mean 128, std 64 make every normalised pixel k / 64, weights in [-2, 2]: all sums exact.  The
    image is img_size, 3 rows / 13 columns short (the width cuts an 8-pixel chunk and a patch), or
    a single pixel; everything beyond it is zero padding."""
    from samq import ops
    grid, cin = 5, 3
    size = grid * patch
    mean, std = torch.full((cin,), 128.0), torch.full((cin,), 64.0)
    for n in (128, 256):
        g = _gen(6, patch, n)
        w = R.ints(g, -2, 2, (n, cin * patch * patch))
        bias, pos = R.ints(g, -50, 50, (n,)), R.ints(g, -50, 50, (grid, grid, n))
        wd = _opt(w, cuda, wdtype)
        for h, wid in _u8_sizes(size):
            img = torch.randint(0, 256, (B, cin, h, wid), generator=g, dtype=torch.uint8)
            x64 = R.normalise_u8(img, mean, std, size, f32=False)
            for has_b, has_p in (BIAS_POS if (h, wid) == (size - 3, size - 13) else BIAS_POS[:1]):
                b, p = (bias if has_b else None), (pos if has_p else None)
                fr = R.Frame((B, grid, grid, n), torch.float32, cuda)
                ops.patch_embed_u8(img.to(cuda), mean.to(cuda), std.to(cuda), wd, _opt(b, cuda), _opt(p, cuda), patch,
                                   size, out=fr.t)
                torch.cuda.synchronize()
                _equal(fr, R.patch_ref(x64, w, b, p, patch), torch.float32,
                       f"u8 patch={patch} {wdtype} N={n} image {h}x{wid} bias={has_b} pos={has_p}")


@pytest.mark.parametrize("patch", [16, 4, 12])
def test_patch_embed_u8_random_f32_weights(cuda, patch):
    """SAM's own pixel mean / std, fp32 weights, a cut image, against float64 on the fp32-normalised
    pixels: 2e-6 for the split form (patch 16), the fp32 summation bound for the fp32-MFMA form."""
    from samq import ops
    grid, cin, n = 5, 3, 256
    size = grid * patch
    h, wid = size - 3, size - 13
    g = _gen(7, patch)
    img = torch.randint(0, 256, (B, cin, h, wid), generator=g, dtype=torch.uint8)
    mean = torch.tensor([123.675, 116.28, 103.53])
    std = torch.tensor([58.395, 57.12, 57.375])
    w = torch.randn(n, cin * patch * patch, generator=g) * 0.02
    bias, pos = torch.randn(n, generator=g) * 0.02, torch.randn(grid, grid, n, generator=g) * 0.1
    x64 = R.normalise_u8(img, mean, std, size, f32=True)
    fr = R.Frame((B, grid, grid, n), torch.float32, cuda)
    ops.patch_embed_u8(img.to(cuda), mean.to(cuda), std.to(cuda), _opt(w, cuda), _opt(bias, cuda), _opt(pos, cuda), patch,
                       size, out=fr.t)
    torch.cuda.synchronize()
    if patch == 16:
        _close(fr, R.patch_ref(x64, w.double(), bias.double(), pos.double(), patch), 2e-6, "u8 split")
    else:
        _f32_sum_bound(fr, x64, w.double(), bias, pos, patch, f"u8 fp32 MFMA p={patch}")


# ----------------------------------------------------------------------------- neck convs
@pytest.mark.parametrize("k", [32, 96, 1280])
@pytest.mark.parametrize("m", [1, 75, 129])
def test_conv1x1_exact(cuda, m, k):
    """conv_gemm_kernel<CG_1X1_F32>: values in {-1, 0, 1}, |sum| <= 1280 < 2048 is exact in fp16."""
    from samq import ops
    for n in (128, 256):
        g = _gen(8, m, k, n)
        x, w = R.ints(g, -1, 1, (m, k)), R.ints(g, -1, 1, (n, k))
        fr = R.Frame((m, n), torch.float16, cuda)
        ops.conv1x1_f32(_opt(x, cuda), _opt(w, cuda, torch.float16), out=fr.t)
        torch.cuda.synchronize()
        _equal(fr, x @ w.T, torch.float16, f"1x1 M={m} K={k} N={n}")


@pytest.mark.parametrize("grid,cin,n", [(1, 32, 128), (2, 32, 128), (3, 32, 128), (5, 32, 128), (1, 96, 128),
                                        (2, 96, 128), (3, 96, 128), (5, 96, 128), (5, 256, 256)])
def test_conv3x3_exact(cuda, grid, cin, n):
    """conv_gemm_kernel<CG_3X3>: grids of 1 to 3 are mostly padding; values in {-1, 0, 1}: the fp32
    partial sums are exact and the results (checked: below 2048) are fp16 numbers."""
    from samq import ops
    g = _gen(9, grid, cin, n)
    x = R.ints(g, -1, 1, (B, grid, grid, cin))
    w = R.ints(g, -1, 1, (n, 3, 3, cin))
    ref = R.conv3x3_ref(x, w)
    assert ref.abs().max().item() < 2048
    fr = R.Frame((B, grid, grid, n), torch.float16, cuda)
    ops.conv3x3_nhwc(_opt(x, cuda, torch.float16), _opt(w, cuda, torch.float16), out=fr.t)
    torch.cuda.synchronize()
    _equal(fr, ref, torch.float16, f"3x3 G={grid} Cin={cin} N={n}")


def test_neck_convs_random(cuda):
    """Random values against float64 on the values the kernels see: the f32 -> f16 conversion of the
    1 x 1 conv's A operand, fp16 outputs (2e-3)."""
    from samq import ops
    g = _gen(10)
    m, k, n = 75, 1280, 256
    x, w = torch.randn(m, k, generator=g), (torch.randn(n, k, generator=g) * 0.03).half()
    fr = R.Frame((m, n), torch.float16, cuda)
    ops.conv1x1_f32(_opt(x, cuda), w.to(cuda), out=fr.t)
    _close(fr, x.half().double() @ w.double().T, 2e-3, "1x1")
    grid, cin = 5, 256
    x = torch.randn(B, grid, grid, cin, generator=g).half()
    w = (torch.randn(n, 3, 3, cin, generator=g) * 0.03).half()
    fr = R.Frame((B, grid, grid, n), torch.float16, cuda)
    ops.conv3x3_nhwc(x.to(cuda), w.to(cuda), out=fr.t)
    _close(fr, R.conv3x3_ref(x.double(), w.double()), 2e-3, "3x3")


# ----------------------------------------------------------------------------- int8 implicit GEMM
_I8_CASES = [(1, 3, 5), (2, 128, 1), (2, 128, 2), (2, 128, 5)]
_I8_SCALES = dict(out=np.float32(3 * 2.0 ** -6), mid=np.float32(5 * 2.0 ** -7), res=np.float32(7 * 2.0 ** -8),
                  out_sat=np.float32(3 * 2.0 ** -13))


@pytest.mark.parametrize("mode,cin,grid", _I8_CASES, ids=["patch-g5", "3x3-g1", "3x3-g2", "3x3-g5"])
@pytest.mark.parametrize("n", [64, 192])
def test_w8a8_conv_gemm_exact(cuda, mode, cin, grid, n):
    """samq_w8a8_conv_gemm (AG_PATCH at side 80, AG_3X3) x EPI_Q8 (bias / none) and EPI_Q8_RES (pos
    codes shared by the images, rmod = G * G, and a full residual, rmod = 0): bit-equal to the
    int64 im2col sum followed by the documented chain in float64, on the exact scales of _i8_ref."""
    from samq import ops
    p = R.i8_conv_problem(mode, B, cin, grid, n, 11)
    gg, m = grid * grid, B * grid * grid
    xd = torch.from_numpy(p["x"]).to(cuda)
    wp = ops.w8_repack(torch.from_numpy(p["w"]).to(cuda))
    ws, bias = torch.from_numpy(p["wscale"]).to(cuda), torch.from_numpy(p["bias"]).to(cuda)
    sc = _I8_SCALES

    def run(what, ref, **kw):
        fr = R.Frame((B, grid, grid, n), torch.int8, cuda)
        ops.w8a8_conv_gemm(xd, mode, wp, ws, n, a_scale=float(p["a_scale"]), out=fr.t, **kw)
        torch.cuda.synchronize()
        assert fr.untouched(), what + ": wrote outside its window"
        got = fr.t.cpu().numpy().reshape(m, n)
        bad = got != ref
        assert not bad.any(), f"mode {mode} G={grid} N={n} {what}: {int(bad.sum())} of {bad.size} codes differ"

    for tag, s_out in (("fine", sc["out"]), ("sat", sc["out_sat"])):
        run(f"Q8 bias {tag}", I8.quant(p["y"], s_out), bias=bias, epilogue=ops.EPI_Q8, out_scale=float(s_out))
        run(f"Q8 no bias {tag}", I8.quant(p["y_nobias"], s_out), bias=None, epilogue=ops.EPI_Q8, out_scale=float(s_out))
    ties = np.abs(p["y"] / np.float64(sc["out"]) % 1) == 0.5
    assert ties.mean() > 0.01, "the exact inputs put too few quotients on a tie"
    res = p["res"]
    for mid in (sc["mid"], np.float32(0.0)):
        ref = I8.q8_res(p["y"], res, float(mid), sc["res"], sc["out"])
        run(f"Q8_RES full residual mid={float(mid)}", ref, bias=bias, epilogue=ops.EPI_Q8_RES, out_scale=float(sc["out"]),
            mid_scale=float(mid), res_scale=float(sc["res"]), res=torch.from_numpy(res).to(cuda), rmod=0)
        shared = np.ascontiguousarray(res[:gg])
        ref = I8.q8_res(p["y"], np.tile(shared, (B, 1)), float(mid), sc["res"], sc["out"])
        run(f"Q8_RES rmod=G*G mid={float(mid)}", ref, bias=bias, epilogue=ops.EPI_Q8_RES, out_scale=float(sc["out"]),
            mid_scale=float(mid), res_scale=float(sc["res"]), res=torch.from_numpy(shared).to(cuda), rmod=gg)


# ----------------------------------------------------------------------------- refusals
def test_conv_refusals(cuda):
    from samq import ops

    def refused(exc, fn, shape, dtype):
        fr = R.Frame(shape, dtype, cuda)
        with pytest.raises(exc):
            fn(fr.t)
        torch.cuda.synchronize()
        assert fr.pristine(), "a refused call wrote to its output"

    z = lambda *s, dtype=torch.float16: torch.zeros(*s, dtype=dtype, device=cuda)  # noqa: E731
    refused(NotImplementedError, lambda o: ops.patch_embed(z(1, 3, 60, 60), z(128, 432), None, None, 12, out=o),
            (1, 5, 5, 128), torch.float32)
    refused(NotImplementedError, lambda o: ops.patch_embed(z(1, 3, 80, 80), z(192, 768), None, None, 16, out=o),
            (1, 5, 5, 192), torch.float32)
    f32 = torch.float32
    refused(NotImplementedError, lambda o: ops.patch_embed(z(1, 3, 80, 80, dtype=f32), z(192, 768, dtype=f32), None, None,
                                                           16, out=o), (1, 5, 5, 192), torch.float32)
    refused(NotImplementedError, lambda o: ops.conv1x1_f32(z(8, 64, dtype=f32), z(192, 64), out=o), (8, 192), torch.float16)
    refused(NotImplementedError, lambda o: ops.conv3x3_nhwc(z(1, 2, 2, 32), z(192, 3, 3, 32), out=o), (1, 2, 2, 192),
            torch.float16)
    mean, std = torch.full((3,), 128.0, device=cuda), torch.full((3,), 64.0, device=cuda)
    for wdt in (torch.float16, torch.float32):
        refused(AssertionError, lambda o: ops.patch_embed_u8(z(1, 3, 81, 40, dtype=torch.uint8), mean, std,
                                                             z(128, 768, dtype=wdt), None, None, 16, 80, out=o),
                (1, 5, 5, 128), torch.float32)
        refused(NotImplementedError, lambda o: ops.patch_embed_u8(z(1, 3, 80, 80, dtype=torch.uint8), mean, std,
                                                                  z(192, 768, dtype=wdt), None, None, 16, 80, out=o),
                (1, 5, 5, 192), torch.float32)
    i8 = torch.int8
    ws = torch.ones(64, device=cuda)
    w64 = ops.w8_repack(z(64, 9 * 128, dtype=i8))
    refused(NotImplementedError, lambda o: ops.w8a8_conv_gemm(z(1, 2, 2, 64, dtype=i8), 2, w64, ws, 64, out_scale=0.05, out=o),
            (1, 2, 2, 64), i8)
    refused(NotImplementedError, lambda o: ops.w8a8_conv_gemm(z(1, 2, 2, 128, dtype=i8), 2, w64, ws, 64, epilogue=ops.EPI_BIAS,
                                                              out_scale=0.05, out=o), (1, 2, 2, 64), i8)
