"""Power-of-Two Factor activations (``Config(ptf=True)``): the ``PtfObserver`` mirror against the
reference's fixture (golden/fq_ptf.npz), the HIP kernels ``samq_ptf_scores``, ``samq_layernorm_q_ptf``,
``samq_i8_gemm_ptf`` (epilogue exponents and the masked-pass replay), ``samq_w8a8_conv_gemm_ptf`` against
the float64 / integer restatements of tests/_ptf_ref.py, and the zero-point engine on a PTF encoder.
"""
import copy
import functools
import json

import numpy as np
import pytest
import torch

import _ptf_ref as P
import _zp_ref as Z

# (BM, BN) of the tile configs built for PTF activations (I8Ring::PTF, csrc/gemm_i8.hip); 0 = the automatic pick
PTF_TILES = {0: (64, 64), 82: (128, 256), 83: (128, 128), 84: (64, 64), 88: (64, 128), 89: (64, 64), 90: (64, 128)}
CASES = [(c, b) for c in P.OBSERVER_CASES for b in P.BIT_TYPES]


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@functools.lru_cache(maxsize=None)
def _fixture(golden_dir):
    g = np.load(golden_dir / "fq_ptf.npz", allow_pickle=False)
    return g, json.loads(str(g["meta"]))


def _observer(case, bt):
    from samq import fq_vit
    return fq_vit.build_observer("ptf", "activation", fq_vit.BIT_TYPE_DICT[bt], "channel_wise",
                                 permute=P.OBSERVER_CASES[case][1])


# ============================================================================= CPU
@pytest.mark.parametrize("case,bt", CASES)
def test_ptf_observer_matches_reference(golden_dir, case, bt):
    """Running min / max after each update, the per-channel scale, the zero point and the picks equal the
    reference's bit for bit."""
    from samq import fq_vit
    g, meta = _fixture(golden_dir)
    assert meta["min_gap"] > P.MIN_GAP
    obs = _observer(case, bt)
    assert type(obs) is fq_vit.PtfObserver
    xs = P.observer_inputs(case)
    for i, x in enumerate(xs):
        obs.update(x)
        assert np.array_equal(obs.max_val.numpy(), g[f"{case}:{bt}:max{i}"])
        assert np.array_equal(obs.min_val.numpy(), g[f"{case}:{bt}:min{i}"])
    scale, zp = obs.get_quantization_params(xs[-1])
    assert scale.dtype == torch.float32 and scale.dim() == 1 and zp.dim() == 0
    assert np.array_equal(scale.numpy(), g[f"{case}:{bt}:scale"])
    assert float(zp) == float(g[f"{case}:{bt}:zp"])
    picks = np.log2(scale.numpy().astype(np.float64) / float(g[f"{case}:{bt}:scale1"]))
    assert np.array_equal(picks, g[f"{case}:{bt}:picks"].astype(np.float64))
    assert len(set(g[f"{case}:{bt}:picks"].tolist())) >= 3      # the inputs exercise several factors


def test_ptf_placement(golden_dir):
    """``Config(True, True, ...)``: PtfObserver on exactly the reference's QActs (those that feed a LayerNorm),
    the activation order unchanged; ``Config(False, False, ...)``: none."""
    from samq import fq_vit
    g, _ = _fixture(golden_dir)
    enc = fq_vit.build_fq_image_encoder("vit_b", img_size=64, depth=2, cfg=fq_vit.Config(True, True, "minmax"),
                                        global_attn_indexes=(1,))
    qa = fq_vit.act_quantizers(enc)
    assert list(qa) == [str(n) for n in g["act_names"]]
    ptf = [n for n, m in qa.items() if type(m.quantizer.observer) is fq_vit.PtfObserver]
    assert ptf == [str(n) for n in g["ptf_names"]]
    assert ptf == ["qact1", "blocks.0.qact2", "blocks.0.qact4", "blocks.1.qact2", "blocks.1.qact4", "qacts.0", "qacts.2"]
    for n in ptf:
        assert qa[n].calibration_mode == "channel_wise" and qa[n].quantizer.permute == n.startswith("qacts.")
    off = fq_vit.build_fq_image_encoder("vit_b", img_size=64, depth=2, cfg=fq_vit.Config(False, False, "minmax"),
                                        global_attn_indexes=(1,))
    assert not [n for n, m in fq_vit.act_quantizers(off).items() if type(m.quantizer.observer) is fq_vit.PtfObserver]


def _model(golden_dir, device, calibrated: bool):
    """The fixture's model (vit_b, depth 2, img 256, default uint8 ``Config()``) on ``device``; ``calibrated``:
    the reference's scales and zero points installed and quant mode on, else ready for calibration."""
    from oracle import synth
    from samq import fq_vit
    g, meta = _fixture(golden_dir)
    enc = fq_vit.build_fq_image_encoder(P.MODEL["name"], img_size=P.MODEL["img_size"], depth=P.MODEL["depth"],
                                        cfg=fq_vit.Config(), global_attn_indexes=P.MODEL["global_attn_indexes"])
    missing, unexpected = enc.load_state_dict(P.model_state(synth), strict=False)
    assert not unexpected and all("quantizer" in k for k in missing)
    enc = enc.to(device).eval()
    if calibrated:
        names = [str(n) for n in g["act_names"]]
        fq_vit.calibrate_weights(enc)
        fq_vit.set_act_scales(enc, {n: g[f"model:scale:{n}"] for n in names}, {n: g[f"model:zp:{n}"] for n in names})
        enc.model_quant()
    return enc


def test_ptf_module_calibration_matches_reference(golden_dir):
    """The fixture's model calibrated on the reference's three images with the default ``Config()``: every
    activation scale (the PTF vectors included) and zero point, and the quant-mode ``module_forward`` output
    codes on the test image, equal the reference's bit for bit."""
    from oracle import synth
    from samq import fq_vit
    g, meta = _fixture(golden_dir)
    assert meta["min_gap"] > P.MIN_GAP and meta["config"] == "Config()"
    enc = _model(golden_dir, "cpu", calibrated=False)
    assert enc.cfg.INT_NORM and enc.cfg.INT_SOFTMAX and enc.cfg.BIT_TYPE_A.name == "uint8"
    size = P.MODEL["img_size"]
    enc.calibrate_with([torch.from_numpy(synth.make_images(1, size, seed=s)) for s in P.MODEL["calib_seeds"]])
    qa = fq_vit.act_quantizers(enc)
    assert list(qa) == [str(n) for n in g["act_names"]]
    vectors = 0
    for n, m in qa.items():
        sc, zp = m.quantizer.scale, m.quantizer.zero_point
        assert sc.shape == g[f"model:scale:{n}"].shape and zp.dim() == 0, n
        assert np.array_equal(sc.numpy(), g[f"model:scale:{n}"]), n
        assert float(zp) == float(g[f"model:zp:{n}"]), n
        vectors += sc.dim() == 1
    assert vectors == len(g["ptf_names"]) == 7
    with torch.no_grad():
        y = enc.module_forward(torch.from_numpy(synth.make_images(1, size, seed=P.MODEL["test_seed"])))
    q3 = qa["qacts.3"].quantizer
    codes = torch.round(y / q3.scale + q3.zero_point).numpy()
    assert np.array_equal(codes, g["model:codes"].astype(np.float32))
    # the reference's state loads into a fresh encoder through set_act_scales as well
    ref = _model(golden_dir, "cpu", calibrated=True)
    assert torch.equal(fq_vit.act_quantizers(ref)["blocks.1.qact4"].quantizer.scale, qa["blocks.1.qact4"].quantizer.scale)


def test_ptf_exports_and_refusals():
    from samq import _lib, fq_sam, fq_vit
    assert {"samq_ptf_scores", "samq_ptf_scores_workspace", "samq_layernorm_q_ptf", "samq_i8_gemm_ptf",
            "samq_w8a8_conv_gemm_ptf"} <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.samq_ptf_scores_workspace(0, 8) == 0 and lib.samq_ptf_scores_workspace(8, 0) == 0
    small, big = lib.samq_ptf_scores_workspace(1, 4), lib.samq_ptf_scores_workspace(1 << 20, 768)
    assert small == 4 * 4 * 8 and big % (768 * 4 * 8) == 0 and small < big <= 256 * 768 * 4 * 8
    with pytest.raises(NotImplementedError):
        fq_vit.build_observer("ptf", "activation", fq_vit.BIT_TYPE_DICT["uint8"], "layer_wise")
    cfg = fq_vit.Config(True, True, "minmax")
    with pytest.raises(NotImplementedError, match="ptf"):
        fq_sam.PromptEncoder(256, (4, 4), (64, 64), 16, cfg=cfg)
    with pytest.raises(NotImplementedError, match="ptf"):
        fq_sam.TwoWayTransformer(2, 256, 8, 2048, cfg=cfg)
    with pytest.raises(NotImplementedError, match="ptf"):
        fq_sam.MaskDecoder(transformer_dim=256, transformer=torch.nn.Identity(), cfg=cfg)


def test_ptf_state_dict_and_szp():
    """A calibrated PTF state dict (scale [C], 0-dim zero point) loads; ``_szp`` splits a PTF scale into
    (s0, zp, exp) and refuses other per-channel scales and per-channel zero points."""
    from samq import fq_vit, synthetic
    enc = synthetic.random_fq_encoder("vit_b", device="cpu", img_size=64, depth=1, calib_images=2, act_bit_type="uint8",
                                      ptf=True, lis=True)
    assert enc.cfg.INT_NORM and enc.cfg.INT_SOFTMAX and enc._needs_zero_points()
    q = fq_vit.act_quantizers(enc)["qact1"].quantizer
    assert q.scale.shape == (768,) and q.zero_point.dim() == 0
    fresh = fq_vit.build_fq_image_encoder("vit_b", img_size=64, depth=1, cfg=fq_vit.Config(True, True, "minmax"))
    fresh.load_state_dict(enc.state_dict())
    assert torch.equal(fq_vit.act_quantizers(fresh)["qact1"].quantizer.scale, q.scale)
    s0, z, exp = fq_vit._szp(fq_vit.act_quantizers(enc)["qact1"])
    assert s0 == float(q.scale.min()) and z == int(q.zero_point) - 128
    assert torch.equal(torch.tensor(s0) * 2.0 ** exp.float(), q.scale)
    bad = copy.deepcopy(fq_vit.act_quantizers(enc)["qact1"])
    bad.quantizer.scale[5] *= 3
    with pytest.raises(NotImplementedError, match="Power-of-Two"):
        fq_vit._szp(bad)
    bad = copy.deepcopy(fq_vit.act_quantizers(enc)["qact1"])
    bad.quantizer._buffers["zero_point"] = torch.full((768,), 100.0)
    with pytest.raises(NotImplementedError, match="zero point"):
        fq_vit._szp(bad)


# ============================================================================= GPU: observer
@pytest.mark.gpu
@pytest.mark.parametrize("rows,c", [(1, 4), (37, 5), (300, 130), (4099, 768)])
def test_ptf_scores(cuda, rows, c):
    """samq_ptf_scores against the float64 restatement: rtol 2 * rows * 2^-53 (the bound for samq_omse_scores)."""
    from samq import ops
    rng = np.random.Generator(np.random.PCG64([rows, c]))
    x = (rng.standard_normal((rows, c)) * 2.0 ** -(np.arange(c) % 5)[None, :]).astype(np.float32)
    for dt in (np.float32, np.float16):
        xd = x.astype(dt)
        for zp, (qmin, qmax) in ((0, (-128, 127)), (129, (0, 255)), (129, (-128, 127)), (0, (0, 255))):
            s1 = np.float32(np.abs(x).max() * 2 / 255 / 8)
            ref = P.scores64(xd.astype(np.float32), s1, zp, qmin, qmax)
            got = ops.ptf_scores(_t(xd, cuda), float(s1), zp, qmin, qmax).cpu().numpy()
            assert got.shape == (c, 4)
            np.testing.assert_allclose(got, ref, rtol=2 * rows * 2.0 ** -53, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("case,bt", CASES)
def test_ptf_observer_gpu_equals_cpu(cuda, golden_dir, case, bt):
    """PtfObserver on GPU tensors: min / max bit for bit, identical picks, scales and zero point (the
    fixture's recorded gap > 1e-6 makes the float64 pick the reference's)."""
    g, _ = _fixture(golden_dir)
    cpu, gpu = _observer(case, bt), _observer(case, bt)
    xs = P.observer_inputs(case)
    for x in xs:
        cpu.update(x)
        gpu.update(x.to(cuda))
        assert gpu.max_val.is_cuda and torch.equal(gpu.max_val.cpu(), cpu.max_val)
        assert torch.equal(gpu.min_val.cpu(), cpu.min_val)
    sc, zc = cpu.get_quantization_params(xs[-1])
    sg, zg = gpu.get_quantization_params(xs[-1].to(cuda))
    assert sg.is_cuda and zg.is_cuda and zg.dim() == 0
    assert torch.equal(sg.cpu(), sc) and torch.equal(zg.cpu(), zc)
    assert np.array_equal(sg.cpu().numpy(), g[f"{case}:{bt}:scale"])


# ============================================================================= GPU: LayerNorm
@pytest.mark.gpu
@pytest.mark.parametrize("c", (4, 132, 768, 1280))
def test_layernorm_q_ptf(cuda, c):
    """samq_layernorm_q_ptf against the float64 LayerNorm of ((code - z) << e) * s: codes within +-1, the
    off-by-one share at most 1e-3 (test_zp_kernels.py's rule); all exponents 0 equals samq_layernorm_q_zp."""
    from samq import ops
    g = torch.Generator().manual_seed(8100 + c)
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    gd, bd = gamma.to(cuda), beta.to(cuda)
    s_in = float(Z.LN_IN_SCALE)
    off = tot = 0
    for rows in (1, 5, 9):
        codes = torch.randint(-128, 128, (rows, c), generator=g).to(torch.int8)
        xd = codes.to(cuda)
        for kind in ("mixed", "e3", "e1"):
            exp = torch.from_numpy(P.exp_pattern(c, kind, c))
            if kind == "mixed":
                assert set(exp.tolist()) == {0, 1, 2, 3}
            ed = exp.to(cuda)
            for zi in (-128, 1, 127):
                y64 = P.ln64_ptf(codes, zi, s_in, exp, gamma, beta, 1e-6)
                s_out, zo = np.float32(np.abs(y64).max() / 100.0), 37
                ref = np.clip(np.rint(y64 / np.float64(s_out) + zo), -128, 127).astype(np.int64)
                outs = [ops.layernorm_q_ptf(xd, gd, bd, 1e-6, s_in, float(s_out), zi, zo, ed, rows_per_wave=r)
                        for r in (0, 1, 2, 4)]
                for o in outs[1:]:
                    assert torch.equal(o, outs[0])
                got = outs[0].cpu().numpy().astype(np.int64)
                d = np.abs(got - ref)
                assert d.max() <= 1, f"c {c} rows {rows} {kind} zp {zi}: code off by {d.max()}"
                off += int((d > 0).sum())
                tot += d.size
                fq = ops.layernorm_q_ptf(xd, gd, bd, 1e-6, s_in, float(s_out), zi, zo, ed, out_dtype=torch.float32)
                assert np.array_equal(fq.cpu().numpy(), Z.fake32(got, s_out, zo))
        zero = torch.zeros(c, dtype=torch.uint8, device=cuda)
        for r in (0, 1, 2, 4):
            assert torch.equal(ops.layernorm_q_ptf(xd, gd, bd, 1e-6, s_in, 0.03, -3, 90, zero, rows_per_wave=r),
                               ops.layernorm_q_zp(xd, gd, bd, 1e-6, s_in, 0.03, -3, 90, rows_per_wave=r))
    print(f"\n  layernorm_q_ptf c {c}: {off} of {tot} codes off by one ({off / tot:.2e})")
    assert off / tot <= 1e-3
    with pytest.raises(AssertionError):
        ops.layernorm_q_ptf(xd, gd, bd, 1e-6, s_in, 0.03, 0, 0, None)


# ============================================================================= GPU: GEMM epilogue exponents
def _gemm_ns(cfg):
    bn = PTF_TILES[cfg][1]
    return [n for n in (64, 128) if n % bn == 0] or [bn]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", sorted(PTF_TILES))
def test_i8_gemm_ptf_epilogues(cuda, cfg):
    """Per-column output / residual exponents on exact inputs, Q8, Q8_GELU, Q8_RES (mid quantiser and rmod on
    and off): codes equal the integer restatement bit for bit (GELU: the near-tie rule); exponents zero or
    absent equal samq_i8_gemm_zp bit for bit."""
    from samq import ops
    for n in _gemm_ns(cfg):
        for k in (128, 256):
            for m in (1, 33, 69):
                p = P.EpiProblem(m, n, k)
                y = p.y()
                ties = (y / P.OUT_SCALE) % 1 == 0.5
                assert m == 1 or ties.mean() > 0.02
                a, w = _t(p.a, cuda), ops.w8_repack(_t(p.w, cuda))
                ws, bias, coff = _t(p.wscale, cuda), _t(p.bias, cuda), _t(p.col_offset, cuda)
                res = _t(p.res, cuda)
                mixed, zero = P.exp_pattern(n, "mixed", n + k), P.exp_pattern(n, "zero")
                assert all(set(mixed[g0:g0 + 16].tolist()) == {0, 1, 2, 3} for g0 in range(0, n, 16))
                kw = dict(a_scale=P.A_SCALE, out_scale=P.OUT_SCALE, cfg=cfg, col_offset=coff, out_zp=P.ZP_OUT)
                for oe in (mixed, None, zero):
                    oed = None if oe is None else _t(oe, cuda)
                    got = ops.i8_gemm_ptf(a, w, ws, n, bias, ops.EPI_Q8, out_exp=oed, **kw)
                    assert np.array_equal(got.cpu().numpy(), p.q8(oe)), (cfg, m, n, k, "Q8")
                    if oe is not mixed:
                        assert torch.equal(got, ops.i8_gemm_zp(a, w, ws, n, bias, ops.EPI_Q8, **kw))
                    gg = ops.i8_gemm_ptf(a, w, ws, n, bias, ops.EPI_Q8_GELU, out_exp=oed, **kw)
                    if oe is mixed:
                        g64 = P.gelu64(y)
                        for e in range(4):
                            cols = mixed == e
                            _, bad = Z.check_gelu_q8_zp(gg.cpu().numpy()[:, cols], g64[:, cols], P.OUT_SCALE * 2.0 ** e,
                                                        P.ZP_OUT)
                            assert bad == 0, (cfg, m, n, k, "Q8_GELU", e)
                    else:
                        assert torch.equal(gg, ops.i8_gemm_zp(a, w, ws, n, bias, ops.EPI_Q8_GELU, **kw))
                    for re in (P.exp_pattern(n, "mixed", 7 * n + k), None, zero):
                        red = None if re is None else _t(re, cuda)
                        for mid, rmod in ((True, 0), (False, P.RMOD), (True, P.RMOD)):
                            rk = dict(mid_scale=P.MID_SCALE if mid else 0.0, res_scale=P.RES_SCALE, res=res,
                                      mid_zp=P.ZP_MID, res_zp=P.ZP_RES, rmod=rmod, **kw)
                            got = ops.i8_gemm_ptf(a, w, ws, n, bias, ops.EPI_Q8_RES, out_exp=oed, res_exp=red, **rk)
                            assert np.array_equal(got.cpu().numpy(), p.q8_res(mid, rmod, oe, re)), (cfg, m, n, k, mid, rmod)
                            if oe is not mixed and (re is None or re is zero):
                                assert torch.equal(got, ops.i8_gemm_zp(a, w, ws, n, bias, ops.EPI_Q8_RES, **rk))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,side", [(1, 32), (2, 2), (2, 5)])
def test_w8a8_conv_gemm_ptf(cuda, mode, side):
    """The conv entry with out_exp: patch mode at side 32, 3x3 mode at 2x2 and 5x5 maps (Cin = 128), against
    the float64 restatement of _zp_ref on the same exact inputs; out_exp absent equals the _zp entry."""
    from samq import ops
    import _i8_ref as R
    cin, n, b = (3, 64, 2) if mode == 1 else (128, 64, 1)
    x, w, wscale, b_int, csc, pos, g = Z.conv_problem(mode, b, cin, side, n)
    acc = Z.conv_acc(x, w, mode, Z.ZP_A)
    assert np.abs(acc + b_int).max() < 2 ** 24
    y = (acc + b_int) * csc
    s_out = np.float32(3 * 2.0 ** int(np.floor(np.log2((float(y.std()) or 1.0) / 48))))
    xk = x if mode == 1 else np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    wk = (w if mode == 1 else np.ascontiguousarray(w.transpose(0, 2, 3, 1))).reshape(n, -1)
    dwk = _t(wk, cuda)
    dw, dws, db = ops.w8_repack(dwk), _t(wscale, cuda), _t((b_int * csc).astype(np.float32), cuda)
    kw = dict(bias=db, epilogue=ops.EPI_Q8, a_scale=float(R.A_SCALE), out_scale=float(s_out),
              col_offset=ops.w8a8_col_offset(dwk, Z.ZP_A), out_zp=Z.ZP_OUT,
              pad16=torch.full((16,), Z.ZP_A, dtype=torch.int8, device=cuda))
    oe = P.exp_pattern(n, "mixed", side)
    got = ops.w8a8_conv_gemm_ptf(_t(xk, cuda), mode, dw, dws, n, out_exp=_t(oe, cuda), **kw)
    assert got.shape == (b, g, g, n)
    ref = Z.quant32(y * 2.0 ** -oe.astype(np.float64), s_out, Z.ZP_OUT)       # x * 2^-e is exact
    assert np.array_equal(got.cpu().numpy(), ref)
    assert (ref != Z.quant32(y, s_out, Z.ZP_OUT)).mean() > 0.2                 # the exponents matter
    plain = ops.w8a8_conv_gemm_ptf(_t(xk, cuda), mode, dw, dws, n, **kw)
    assert torch.equal(plain, ops.w8a8_conv_gemm_zp(_t(xk, cuda), mode, dw, dws, n, **kw))


# ============================================================================= GPU: replay GEMM
@pytest.mark.gpu
@pytest.mark.parametrize("ka", (128, 256, 1280))
@pytest.mark.parametrize("levels", [(0, 1, 2, 3), (0, 3), (0, 1), (0,)])
def test_i8_gemm_ptf_replay(cuda, ka, levels):
    """An input with per-k exponents by masked-pass replay: the int32 sums sum_k (a_k - z_a) 2^e_k W[n, k] at
    worst-case magnitudes, read through the quantised output at a power-of-two scale that keeps them inside
    the code range (and through a scale at which the extreme rows saturate), equal the int64 restatement."""
    from samq import ops
    for z_a in (127, -128):
        for n in (64, 256):
            for m in (1, 33, 69):
                a, w, e, tot = P.replay_problem(m, n, ka, set(levels), z_a)
                stacked, shifts, coff = ops.ptf_stack_weight(_t(w, cuda), _t(e, cuda), z_a)
                passes = stacked.shape[1] // ka
                assert passes == len(levels) and sum(shifts) == max(levels)
                assert np.array_equal(coff.cpu().numpy().astype(np.int64),
                                      -z_a * (w.astype(np.int64) * 2 ** e.astype(np.int64)[None, :]).sum(1))
                wp = ops.w8_repack(stacked)
                ws = torch.ones(n, dtype=torch.float32, device=cuda)
                top = int(np.abs(tot).max())
                for sh in (max(0, top.bit_length() - 7), max(0, top.bit_length() - 10)):   # inside / saturating
                    s_out = float(2.0 ** sh)
                    got = ops.i8_gemm_ptf(_t(a, cuda), wp, ws, n, None, ops.EPI_Q8, a_scale=1.0, out_scale=s_out,
                                          col_offset=coff, out_zp=-3, passes=passes, k_shift=shifts)
                    # float(acc) rounds the int32 sum to fp32 first (the kernel's and the contract's conversion)
                    ref = P.quant_cols(tot.astype(np.float32).astype(np.float64), s_out, -3)
                    assert np.array_equal(got.cpu().numpy(), ref), (ka, levels, z_a, n, m, sh)
                if passes == 1:
                    assert torch.equal(got, ops.i8_gemm_zp(_t(a, cuda), wp, ws, n, None, ops.EPI_Q8, a_scale=1.0,
                                                           out_scale=s_out, col_offset=coff, out_zp=-3))


@pytest.mark.gpu
def test_ptf_kernel_refusals(cuda):
    from samq import ops
    p = P.EpiProblem(5, 64, 128)
    a, w = _t(p.a, cuda), ops.w8_repack(_t(p.w, cuda))
    ws = _t(p.wscale, cuda)
    oe = _t(P.exp_pattern(64, "mixed"), cuda)
    for cfg in (91, 92, 181):    # tiles that are not built for PTF: an error, no fallback
        with pytest.raises(NotImplementedError, match="PTF"):
            ops.i8_gemm_ptf(a, w, ws, 64, None, ops.EPI_Q8, a_scale=1.0, out_scale=1.0, cfg=cfg, out_exp=oe)
    with pytest.raises(AssertionError):      # a shift outside 1..3
        ops.i8_gemm_ptf(a, ops.w8_repack(_t(np.concatenate([p.w, p.w], 1), cuda)), ws, 64, None, ops.EPI_Q8, a_scale=1.0,
                        out_scale=1.0, passes=2, k_shift=(4, 0, 0))
    with pytest.raises(NotImplementedError):  # replay with another epilogue
        ops.i8_gemm_ptf(a, ops.w8_repack(_t(np.concatenate([p.w, p.w], 1), cuda)), ws, 64, None, ops.EPI_Q8_GELU,
                        a_scale=1.0, out_scale=1.0, passes=2, k_shift=(1, 0, 0))
    with pytest.raises(AssertionError):      # misaligned exponent array
        big = torch.zeros(80, dtype=torch.uint8, device=cuda)
        ops.i8_gemm_ptf(a, w, ws, 64, None, ops.EPI_Q8, a_scale=1.0, out_scale=1.0, out_exp=big[1:65])


# ============================================================================= GPU: engine
def _module_taps(enc_cpu, img_t):
    from samq import fq_vit
    taps = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: taps.__setitem__(n, out.detach()))
             for n, m in fq_vit.act_quantizers(enc_cpu).items()]
    with torch.no_grad():
        enc_cpu.module_forward(img_t)
    for h in hooks:
        h.remove()
    return taps


def _close(out, ref, what, max_frac=1e-4):
    d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
    frac = float((d > 0).mean())
    print(f"  [{what}] codes differing {frac:.2e}, max |dcode| {d.max()}")
    assert d.max() <= 1, f"{what}: code off by {d.max()}"
    assert frac <= max_frac, f"{what}: {frac:.2e} of codes off by one"


@pytest.mark.gpu
@pytest.mark.parametrize("img_size", (64, 256))
def test_ptf_engine_stage_local(cuda, img_size):
    """``random_fq_encoder(..., act_bit_type='uint8', ptf=True, lis=True)`` calibrated on the GPU: ``enc(img)``
    picks the zero-point engine; every PTF stage fed the CPU module graph's own codes reproduces its output
    codes (all within +-1, at most 1e-4 off by one); a captured graph replayed twice equals the eager forward."""
    from oracle import sam_ref
    from samq import fq_vit, ops, synthetic
    enc = synthetic.random_fq_encoder("vit_b", device=cuda, img_size=img_size, depth=2, global_attn_indexes=(1,),
                                      act_bit_type="uint8", ptf=True, lis=True, calib_images=2, seed=5)
    qa = fq_vit.act_quantizers(enc)
    assert all(qa[n].quantizer.scale.numel() == (256 if n.startswith("qacts") else 768) and
               qa[n].quantizer.zero_point.dim() == 0 for n in ("qact1", "blocks.0.qact2", "blocks.1.qact4", "qacts.0",
                                                               "qacts.2"))
    img = torch.randn((1, 3, img_size, img_size), generator=torch.Generator().manual_seed(77))
    ref = _module_taps(copy.deepcopy(enc).cpu(), img)      # (before the engine exists: it is not copyable)
    out = enc(img.to(cuda))
    assert enc._pick_zp and enc._engine_zp is not None and enc._engine is None
    eng = enc.engine(zero_points=True)
    assert eng.e_x0 is not None and eng.neck0["passes"] >= 2
    quant = {n: fq_vit._szp(m) for n, m in qa.items()}
    c, gsz = eng.embed_dim, img_size // 16

    def to_codes(n, nchw=False):       # the module graph's codes of QAct n, channel-last rows
        s, z, e = quant[n]
        t = ref[n].permute(0, 2, 3, 1) if nchw else ref[n]
        t = t.reshape(-1, t.shape[-1])
        sc = s if e is None else s * 2.0 ** e.cpu().float()[None, :]
        r = torch.round(t / sc + z)
        assert r.min() >= -128 and r.max() <= 127
        return r.to(torch.int8)

    def dev(n, nchw=False):
        return to_codes(n, nchw).to(cuda).contiguous()

    def check(what, got, n, nchw=False):
        _close(got.cpu().numpy().reshape(-1), to_codes(n, nchw).numpy().reshape(-1), what)

    # patch embed -> qact1
    pw = eng.patch_w
    icodes = ops.quantize_zp(img.to(cuda).contiguous(), *eng.q_in)
    x0 = ops.w8a8_conv_gemm_ptf(icodes, 1, pw["packed"], pw["scale"], pw["n"], pw["bias"], ops.EPI_Q8_RES, eng.q_in[0],
                                eng.q_x0[0], mid_scale=eng.q_pe[0], res_scale=eng.q_pos[0], res=eng.pos_codes,
                                rmod=gsz * gsz, col_offset=pw["col_offset"], mid_zp=eng.q_pe[1], res_zp=eng.q_pos[1],
                                out_zp=eng.q_x0[1], out_exp=eng.e_x0)
    check("patch embed -> qact1", x0, "qact1")
    check("image quantiser", icodes, "qact_input")      # (both NCHW: same element order)
    xin_n, q_in, e_in = "qact1", eng.q_x0, eng.e_x0
    for i, bl in enumerate(eng.blocks):
        pre, q, e = f"blocks.{i}.", bl["q"], bl["e"]
        assert e["x1"] is not None and e["x2"] is not None
        check(pre + "LN1", eng._ln_zp(dev(xin_n), bl["n1"], q_in, q["ln1"], e_in), pre + "qact1")
        # the layer-wise stages between the PTF quantisers, on the module graph's codes as well
        win = bl["window"]
        qkv_ref, ao_ref = ref[pre + "attn.qact1"], ref[pre + "attn.qact2"]
        if win:
            hp = -(-gsz // win) * win
            qkv_ref = sam_ref.window_unpartition(qkv_ref.reshape(-1, win, win, 3 * c), win, (hp, hp), (gsz, gsz))
            ao_ref = sam_ref.window_unpartition(ao_ref, win, (hp, hp), (gsz, gsz))
        else:
            qkv_ref = qkv_ref.reshape(1, gsz, gsz, 3 * c)
        qkv_codes = torch.round(qkv_ref / q["qkv"][0] + q["qkv"][1])
        ao_codes = torch.round(ao_ref / q["ao"][0] + q["ao"][1])
        qkv = eng._gemm_zp(dev(pre + "qact1"), bl["qkv"], ops.EPI_Q8, q["ln1"], q["qkv"])
        _close(qkv.cpu().numpy().reshape(-1), qkv_codes.numpy().reshape(-1), pre + "qkv")
        ao = ops.rel_attention_q8_zp(qkv_codes.to(torch.int8).to(cuda).contiguous(), bl["qkv_bias"], bl["relh"],
                                     bl["relw"], bl["heads"], win, bl["scale"], q["qkv"][0], q["a1"][0], q["a2"][0],
                                     q["ao"][0], q["qkv"][1], q["a1"][1], q["a2"][1], q["ao"][1])
        _close(ao.cpu().numpy().reshape(-1), ao_codes.numpy().reshape(-1), pre + f"attention (window {win})")
        check(pre + "lin1+gelu", eng._gemm_zp(dev(pre + "qact3"), bl["lin1"], ops.EPI_Q8_GELU, q["ln2"], q["h"]),
              pre + "mlp.qact1")
        x1 = dev(xin_n)
        eng._gemm_zp(dev(pre + "attn.qact2") if not bl["window"] else _unwindow(ref, pre, q, bl, gsz, c, cuda),
                     bl["proj"], ops.EPI_Q8_RES, q["ao"], q["x1"], q_mid=q["proj"], res=x1, q_res=q_in, out=x1,
                     e_out=e["x1"], e_res=e_in)
        check(pre + "proj+res -> qact2", x1, pre + "qact2")
        check(pre + "LN2", eng._ln_zp(dev(pre + "qact2"), bl["n2"], q["x1"], q["ln2"], e["x1"]), pre + "qact3")
        x3 = dev(pre + "qact2")
        eng._gemm_zp(dev(pre + "mlp.qact1"), bl["lin2"], ops.EPI_Q8_RES, q["h"], q["x2"], q_mid=q["l2"], res=x3,
                     q_res=q["x1"], out=x3, e_out=e["x2"], e_res=e["x1"])
        check(pre + "lin2+res -> qact4", x3, pre + "qact4")
        xin_n, q_in, e_in = pre + "qact4", q["x2"], e["x2"]
    sq, en = eng.q_neck, eng.e_neck
    y0 = eng._gemm_zp(dev(xin_n), eng.neck0, ops.EPI_Q8, q_in, sq[0], e_out=en[0])
    check("neck[0] (replay) -> qacts.0", y0, "qacts.0", nchw=True)
    check("neck LN 1", eng._ln_zp(dev("qacts.0", True), eng.ln_n1, sq[0], sq[1], en[0]), "qacts.1", nchw=True)
    n2 = eng.neck2
    y2 = ops.w8a8_conv_gemm_ptf(dev("qacts.1", True).view(1, gsz, gsz, -1), 2, n2["packed"], n2["scale"], n2["n"],
                                n2["bias"], ops.EPI_Q8, sq[1][0], sq[2][0], col_offset=n2["col_offset"],
                                out_zp=sq[2][1], pad16=eng.pad16, out_exp=en[2])
    check("3x3 conv -> qacts.2", y2, "qacts.2", nchw=True)
    y3 = eng._ln_zp(dev("qacts.2", True), eng.ln_n3, sq[2], sq[3], en[2], out_dtype=torch.float32)
    got3 = torch.round(y3 / sq[3][0] + sq[3][1]).cpu().numpy().reshape(-1)
    _close(got3, to_codes("qacts.3", True).numpy().reshape(-1), "neck LN 2")
    # the whole engine: taps dequantise per channel; graph replay equals eager
    taps = {}
    out2 = eng.forward(img.to(cuda), taps=taps)
    assert torch.equal(out, out2) and taps["qact1"].shape == (1, gsz, gsz, c)
    # end to end against the module graph's output (errors of one code step compound through the blocks)
    s3, z3, _ = quant["qacts.3"]
    oc, rc = np.round(out.cpu().numpy() / s3), np.round(ref["qacts.3"].numpy() / s3)
    d = np.abs(oc - rc)
    cos = float((oc * rc).sum() / np.sqrt((oc * oc).sum() * (rc * rc).sum()))
    print(f"  [end to end] mean |dcode| {d.mean():.3f}, max {d.max():.0f}, cosine {cos:.5f}")
    assert cos >= 0.995 and d.max() <= 0.15 * np.abs(rc).max()
    static = img.to(cuda).clone()
    graph, gout = eng.capture(static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, out)


@pytest.mark.gpu
def test_ptf_engine_vs_reference_golden(cuda, golden_dir):
    """The reference-calibrated PTF state on the GPU: ``enc(img)`` runs the zero-point engine; its output codes
    against the reference's own by the criteria of test_zp_engine_encoder_vs_omse_golden: mean |dcode| <= 1.25 x
    the float64 module graph's distance to the same golden + 0.05, cosine >= 0.995, max-abs <= 0.15 x absmax."""
    from oracle import synth
    g, _ = _fixture(golden_dir)
    enc = _model(golden_dir, cuda, calibrated=True)
    img_np = synth.make_images(1, P.MODEL["img_size"], seed=P.MODEL["test_seed"])
    with pytest.raises(NotImplementedError):
        enc.engine()
    out = enc(torch.from_numpy(img_np).to(cuda)).float().cpu().numpy()
    assert enc._engine_zp is not None and enc._engine is None and enc._engine_zp.neck0["passes"] >= 2
    s_out, z_out = float(g["model:scale:qacts.3"]), float(g["model:zp:qacts.3"])
    codes = np.round(out / s_out)                      # code - zp
    np.testing.assert_allclose(codes * s_out, out, rtol=0, atol=1e-5 * max(1.0, np.abs(out).max()))
    ref = g["model:codes"].astype(np.float64) - z_out
    e64 = _model(golden_dir, "cpu", calibrated=True).double()
    with torch.no_grad():
        c64 = np.round(e64.module_forward(torch.from_numpy(img_np).double()).numpy() / s_out)

    def stats(a, b):
        d = np.abs(a - b)
        return (float((d == 0).mean()), float(d.mean()), float(d.max()),
                float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())))

    ours, self_ = stats(codes, ref), stats(c64, ref)
    print(f"\nW8A8 ptf vit_b d2 256: ours vs reference: {ours[0] * 100:.2f}% codes equal, mean |dcode| {ours[1]:.3f}, "
          f"max {ours[2]:.0f}, cos {ours[3]:.5f} | float64 module graph vs reference: {self_[0] * 100:.2f}% equal, "
          f"mean {self_[1]:.3f}, max {self_[2]:.0f}, cos {self_[3]:.5f}")
    assert ours[1] <= 1.25 * self_[1] + 0.05
    assert ours[3] >= 0.995
    assert ours[2] <= 0.15 * np.abs(ref).max()


def _unwindow(ref, pre, q, bl, gsz, c, cuda):
    """attn.qact2's codes of a windowed block back on the token grid, as the engine's proj GEMM reads them."""
    from oracle import sam_ref
    win = bl["window"]
    hp = -(-gsz // win) * win
    t = sam_ref.window_unpartition(ref[pre + "attn.qact2"], win, (hp, hp), (gsz, gsz))
    return torch.round(t / q["ao"][0] + q["ao"][1]).to(torch.int8).reshape(-1, c).to(cuda).contiguous()


@pytest.mark.gpu
def test_ptf_engine_refusals(cuda):
    from samq import fq_vit, synthetic
    enc = synthetic.random_fq_encoder("vit_b", device=cuda, img_size=64, depth=1, act_bit_type="uint8", ptf=True,
                                      lis=True, calib_images=1)
    with pytest.raises(NotImplementedError):
        enc.engine()        # the symmetric engine keeps refusing INT_NORM
    eng = enc.engine(zero_points=True)
    eng.row_lanes = 2
    with pytest.raises(NotImplementedError, match="row_lanes"):
        eng.forward(torch.zeros(1, 3, 64, 64, device=cuda))
    q = fq_vit.act_quantizers(enc)["blocks.0.qact2"].quantizer
    q.scale[3] *= 1.5
    enc._engine_zp = None
    with pytest.raises(NotImplementedError, match="Power-of-Two"):
        enc.engine(zero_points=True)
