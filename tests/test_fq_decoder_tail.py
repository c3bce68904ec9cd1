"""The fused int8 tail of the fq_vit W8A8 mask decoder (``csrc/decoder_tail.hip``,
``W8A8DecoderEngine.forward_masks``): the three kernels against the float64 restatements of
``_fq_tail_ref.py`` and against compositions of existing kernels, the reference's golden taps
(``golden/fq_decoder_tail.npz``), and the whole click in one graph.

Figures measured on an MI355X (stage-local parity against the golden, share of codes that differ, one
point / two points + box, the float64 restatement's own share in brackets): qacts[0..2] 0 (<= 3.1e-5),
qacts[3] and qacts[4] 7.6e-6 (0 / 7.6e-6), masks 6.1e-5 / 0 (0), no MLP code; DESIGN.md section 4,
"W8A8 mask decoder tail"."""
from __future__ import annotations

import copy
import ctypes
import zlib

import numpy as np
import pytest
import torch

import _fq_decoder_ref as R
import _fq_tail_ref as T
from test_fq_decoder import _CACHE as _DECODER_CACHE
from test_fq_decoder import (_calibrated_cpu, _cpu_taps, _golden, _golden_tap, _gpu_model, _iou, _prompt_inputs,
                             _raw_tokens)

MLP_QACTS = ("qacts1.0", "qacts2.0", "qacts1.1", "qacts2.1", "qact3")
_CACHE = {}


def _mlp_module_name(j):
    return f"output_hypernetworks_mlps.{j}" if j < 4 else "iou_prediction_head"


def _tail_golden(golden_dir):
    if "g" not in _CACHE:
        g = np.load(golden_dir / "fq_decoder_tail.npz")
        _CACHE["g"] = {k: g[k] for k in g.files}
    return _CACHE["g"]


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _params(golden_dir):
    """The tail as numpy: the seeded float convT weights and LayerNorm parameters, the MLP weight codes
    (the engine's rounding) and every scale as the golden records it (the reference's calibration; a
    calibration rerun on another machine may differ in the last bit)."""
    if "p" not in _CACHE:
        g, _ = _golden(golden_dir)
        md = _calibrated_cpu().mask_decoder
        scales = dict(zip(g["act_scale_names"], g["act_scales"]))
        s = lambda n: float(scales["mask_decoder." + n])
        up = md.output_upscaling
        p = dict(su=[s(f"qacts.{i}") for i in range(5)], s_q1=s("qact1"), s_keys=s("transformer.layers.1.qact14"),
                 s_q=s("transformer.qact4"), eps=up[1].eps,
                 w0=up[0].weight.detach().numpy(), b0=up[0].bias.detach().numpy(),
                 gamma=up[1].weight.detach().numpy(), beta=up[1].bias.detach().numpy(),
                 w1=up[3].weight.detach().numpy(), b1=up[3].bias.detach().numpy(), mlps=[])
        for j in range(5):
            name = _mlp_module_name(j)
            layers = []
            for i, lay in enumerate(md.get_submodule(name).layers):
                sw = torch.from_numpy(g[f"wscale:mask_decoder.{name}.layers.{i}"]).float().reshape(-1)
                assert sw.numel() == 1
                w = lay.weight.detach().float()
                codes = torch.clamp(torch.round((w.double() / sw.double()[:, None]).float()), -128, 127).numpy()
                layers.append((codes.astype(np.int8), float(sw[0]), lay.bias.detach().numpy()))
            p["mlps"].append(dict(layers=layers, s1=[s(name + ".qacts1.0"), s(name + ".qacts1.1")],
                                  s2=[s(name + ".qacts2.0"), s(name + ".qacts2.1")], s3=s(name + ".qact3")))
        p["s_hyper"] = np.array([m["s3"] for m in p["mlps"][:4]], np.float32)
        _CACHE["p"] = p
    return _CACHE["p"]


def _golden_stage_inputs(golden_dir, shape):
    g, _ = _golden(golden_dir)
    t = _tail_golden(golden_dir)
    keys = _golden_tap(g, shape, "layers.1.keys").reshape(1, R.GRID, R.GRID, 256)
    queries = _golden_tap(g, shape, "queries")
    return dict(keys=keys, queries=queries, x2=_nhwc(t[f"{shape}:upscaling.qacts.2"]), hyper=t[f"{shape}:hyper_in"])


def _golden_stage_refs(golden_dir, shape):
    """name -> golden codes, laid out as the kernels' outputs (NHWC maps)."""
    g, _ = _golden(golden_dir)
    t = _tail_golden(golden_dir)
    ref = {f"q{i}": _nhwc(t[f"{shape}:upscaling.qacts.{i}"]) for i in range(5)}
    ref["masks"] = _golden_tap(g, shape, "qact1")
    for j in range(5):
        for q, name in zip(MLP_QACTS, ("q1.0", "q2.0", "q1.1", "q2.1", "q3")):
            ref[f"mlp{j}.{name}"] = t[f"{shape}:mlp.{j}.{q}"]
    return ref


def _restatement_vs_golden(golden_dir, shape):
    """The float64 restatement of each fused stage on the golden's input codes against the golden's
    output codes: name -> (max |dcode|, differing share, near-tie share, differing outside near ties,
    the restatement's quotients)."""
    key = ("rest", shape)
    if key not in _CACHE:
        p, ins, ref = _params(golden_dir), _golden_stage_inputs(golden_dir, shape), _golden_stage_refs(golden_dir, shape)
        su = p["su"]
        out = {}
        c, q = T.upscale0_ref(ins["keys"], p["s_keys"], p["w0"], p["b0"], p["gamma"], p["beta"], p["eps"], *su[:3])
        for n in ("q0", "q1", "q2"):
            out[n] = T.compare(c[n], ref[n], q[n], n) + (q[n],)
        c, q = T.upscale1_masks_ref(ins["x2"], su[2], p["w1"], p["b1"], ins["hyper"], p["s_hyper"], su[3], su[4],
                                    p["s_q1"])
        for n in ("q3", "q4", "masks"):
            out[n] = T.compare(c[n], ref[n], q[n], n) + (q[n],)
        for j, m in enumerate(p["mlps"]):
            c, q = T.mlp_ref(ins["queries"][:, 1 + j if j < 4 else 0], p["s_q"], m["layers"], m["s1"], m["s2"], m["s3"])
            for n in c:
                out[f"mlp{j}.{n}"] = T.compare(c[n], ref[f"mlp{j}.{n}"], q[n], n) + (q[n],)
        _CACHE[key] = out
    return _CACHE[key]


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("shape", R.PROMPT_SHAPES)
def test_tail_module_graph_matches_reference(golden_dir, shape):
    """The module graph on the CPU reproduces the golden's tail taps code for code (the rule of
    test_fq_decoder_module_graph_matches_reference)."""
    t = _tail_golden(golden_dir)
    acts = _cpu_taps(shape)[3]
    md = _calibrated_cpu().mask_decoder
    s = lambda n: float(md.get_submodule(n).quantizer.scale.reshape(-1)[0])
    for i in range(5):
        ours = np.round(acts[f"qacts.{i}"].numpy() / s(f"qacts.{i}"))
        assert np.array_equal(ours, t[f"{shape}:upscaling.qacts.{i}"].astype(np.float64)), i
    for j in range(5):
        for q in MLP_QACTS:
            n = f"{_mlp_module_name(j)}.{q}"
            assert np.array_equal(np.round(acts[n].numpy() / s(n)), t[f"{shape}:mlp.{j}.{q}"].astype(np.float64)), n
    hyper = np.stack([t[f"{shape}:mlp.{j}.qact3"] for j in range(4)], axis=1)
    assert np.array_equal(hyper, t[f"{shape}:hyper_in"]) and hyper.shape == (1, 4, 32)


@pytest.mark.parametrize("shape", R.PROMPT_SHAPES)
def test_tail_restatement_vs_golden(golden_dir, shape):
    """The float64 restatement against the reference's fp32 run, per stage: every code within +-1; the
    differing shares are the yardstick of the stage-local GPU test (printed)."""
    res = _restatement_vs_golden(golden_dir, shape)
    for n, (mx, share, ties, outside, _) in res.items():
        print(f"[tail restatement {shape}] {n}: max |dcode| {mx:.0f}, {share:.3e} differ, {ties:.3e} near a tie, "
              f"{outside} differ outside")
        assert mx <= 1, n
    assert {"q0", "q1", "q2", "q3", "q4", "masks", "mlp0.q3", "mlp4.q3"} <= set(res)


# (B, h, w) of the random-input stage tests: one pixel, a grid that is no multiple of anything, more
# than one 64-pixel tile, a tile boundary inside a row (hw = 65), each with a batch boundary inside a tile
STAGE_CASES = [(1, 1, 1), (2, 1, 1), (1, 3, 5), (2, 3, 5), (1, 16, 16), (2, 16, 16), (1, 5, 13)]
UP0_SCALES = tuple(float(np.float32(v)) for v in (0.02, 0.028, 0.0276, 0.0281))     # s_in, s0, s1, s2
UP1_SCALES = tuple(float(np.float32(v)) for v in (0.0276, 0.02, 0.0203, 0.08))      # s_in, s3, s4, s_q1


def _rng(tag, case):
    return np.random.Generator(np.random.PCG64(2024 + zlib.crc32(repr((tag, case)).encode())))


def _up0_inputs(case, exact=False):
    b, h, w = case
    rng = _rng("up0", case)
    x = rng.integers(-128, 128, (b, h, w, 256), dtype=np.int8)
    if exact:   # small integers and power-of-two scales: every fp32 sum and quotient is exact, ties included
        wt = rng.integers(-2, 3, (256, 64, 2, 2)).astype(np.float32)
        bias = (rng.integers(-8, 9, 64) * 0.125).astype(np.float32)
        scales = (2.0 ** -6, 2.0 ** -1, 2.0 ** -5, 2.0 ** -5)
    else:
        wt = (rng.standard_normal((256, 64, 2, 2)) * 0.05).astype(np.float32)
        bias = (rng.standard_normal(64) * 0.05).astype(np.float32)
        scales = UP0_SCALES
    gamma = (1.0 + 0.1 * rng.standard_normal(64)).astype(np.float32)
    beta = (0.05 * rng.standard_normal(64)).astype(np.float32)
    return x, wt, bias, gamma, beta, scales


def _up1_inputs(case, exact=False):
    b, h, w = case
    rng = _rng("up1", case)
    x = rng.integers(-20, 128, (b, h, w, 64), dtype=np.int8)
    hyper = rng.integers(-128, 128, (b, 4, 32), dtype=np.int8)
    if exact:   # mask quotients dot / 8, / 4, / 16, / 8: exact, with .5 ties and clamps
        wt = rng.integers(-2, 3, (64, 32, 2, 2)).astype(np.float32)
        bias = (rng.integers(-8, 9, 32) * 0.125).astype(np.float32)
        hyper = (hyper.astype(np.int64) % 7 - 3).astype(np.int8)
        scales = (2.0 ** -5, 2.0 ** -1, 2.0 ** -1, 2.0 ** -5)
        s_hyper = np.array([2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -7], np.float32)
    else:
        wt = (rng.standard_normal((64, 32, 2, 2)) * 0.1).astype(np.float32)
        bias = (rng.standard_normal(32) * 0.05).astype(np.float32)
        scales = UP1_SCALES
        s_hyper = np.array([0.0101, 0.0123, 0.0087, 0.0095], np.float32)
    return x, wt, bias, hyper, s_hyper, scales


@pytest.mark.parametrize("case", STAGE_CASES, ids=str)
def test_tail_stage_inputs_near_tie_share(case):
    """The condition on the random stage inputs: under 1 % of a stage's codes lie within 1e-3 of a
    rounding midpoint in float64 (the set the GPU test leaves out), and the code range is used."""
    x, wt, bias, gamma, beta, sc = _up0_inputs(case)
    c, q = T.upscale0_ref(x, sc[0], wt, bias, gamma, beta, 1e-5, *sc[1:])
    x1, wt1, bias1, hyper, s_hyper, sc1 = _up1_inputs(case)
    c1, q1 = T.upscale1_masks_ref(x1, sc1[0], wt1, bias1, hyper, s_hyper, *sc1[1:])
    for n, qq in list(q.items()) + list(q1.items()):
        share = float(T.near_tie(qq).mean())
        print(f"[tail inputs {case}] {n}: {share:.3e} near a tie")
        assert share <= 0.01, n
    assert np.abs(c["q0"]).max() > 60 and np.abs(c["q1"]).max() > 60 and c["q2"].max() > 60
    assert np.abs(c1["q3"]).max() > 60 and c1["q4"].max() > 60 and np.abs(c1["masks"]).max() > 30


def test_tail_kernels_refuse_bad_shapes():
    """The documented error codes, before anything reaches the device (runs without a GPU)."""
    from samq import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    up0 = lambda x, cin, cout, s0=0.1, B=1: lib.samq_upscale0_q8(x, p, p, p, p, p, p, None, None, B, 4, 4, cin, cout,
                                                                1e-5, 0.1, s0, 0.1, 0.1, None)
    assert up0(p, 256, 32) == _lib.SAMQ_ERR_UNSUPPORTED and "64 output channels" in lib.samq_last_error().decode()
    assert up0(p, 250, 64) == _lib.SAMQ_ERR_UNSUPPORTED
    assert up0(None, 256, 64) == _lib.SAMQ_ERR_INVALID and "null pointer" in lib.samq_last_error().decode()
    assert up0(p, 256, 64, s0=0.0) == _lib.SAMQ_ERR_INVALID
    assert up0(ctypes.c_void_p(260), 256, 64) == _lib.SAMQ_ERR_INVALID      # alignment
    assert up0(None, 256, 64, B=0) == _lib.SAMQ_OK                           # empty batch: nothing to do
    assert up0(p, 256, 64, B=-1) == _lib.SAMQ_ERR_INVALID
    up1 = lambda x, cin, cout, nm=4, hyper=p: lib.samq_upscale1_masks_q8(x, p, p, p, hyper, p, p, None, None, 1, 8, 8,
                                                                         cin, cout, nm, 0.1, 0.1, 0.1, 0.1, None)
    assert up1(p, 64, 64) == _lib.SAMQ_ERR_UNSUPPORTED and "32 output channels" in lib.samq_last_error().decode()
    assert up1(p, 60, 32) == _lib.SAMQ_ERR_UNSUPPORTED
    assert up1(None, 64, 32) == _lib.SAMQ_ERR_INVALID
    assert up1(p, 64, 32, hyper=None) == _lib.SAMQ_ERR_INVALID
    assert up1(p, 64, 32, nm=65) == _lib.SAMQ_ERR_INVALID
    mlp = lambda q, nt, c, hd, nh=4, noh=32, B=1: lib.samq_decoder_mlps_q8(q, p, p, p, p, p, p, p, p, p, None, B, nt, c,
                                                                           hd, nh, noh, 4, 0.1, None)
    assert mlp(p, 7, 256, 512) == _lib.SAMQ_ERR_UNSUPPORTED                  # hidden width past one workgroup
    assert mlp(p, 7, 254, 256) == _lib.SAMQ_ERR_UNSUPPORTED
    assert mlp(p, 7, 256, 256, noh=300) == _lib.SAMQ_ERR_UNSUPPORTED
    assert mlp(p, 4, 256, 256) == _lib.SAMQ_ERR_INVALID                      # no token for the fourth MLP
    assert "token" in lib.samq_last_error().decode()
    assert mlp(None, 7, 256, 256) == _lib.SAMQ_ERR_INVALID
    assert mlp(None, 7, 256, 256, B=0) == _lib.SAMQ_OK


def test_tail_weight_layouts():
    """``ops.convt_split_weight`` / ``ops.mlp_pack_weight``: the documented fragment and dword orders,
    and hi + lo 2^-11 reproducing the fp32 weight to 2^-22 relative."""
    from samq import ops
    rng = np.random.Generator(np.random.PCG64(5))
    w = torch.from_numpy((rng.standard_normal((32, 8, 2, 2)) * 0.1).astype(np.float32))
    hi, lo = ops.convt_split_weight(w)
    n, k = 32, 32
    mat = w.permute(2, 3, 1, 0).reshape(n, k)                                # W[(2 kh + kw) Cout + co][ci]
    rec = (hi.float() + lo.float() / 2048.0).reshape(n // 32, k // 16, 2, 32, 8)
    for nt, ks, half, nn, j in [(0, 0, 0, 0, 0), (0, 1, 1, 31, 7), (0, 1, 0, 5, 3)]:
        want = mat[nt * 32 + nn, ks * 16 + 8 * half + j]
        assert abs(float(rec[nt, ks, half, nn, j] - want)) <= 2.0 ** -21 * abs(float(want))
    assert float((rec.permute(0, 3, 1, 2, 4).reshape(n, k) - mat).abs().max()) <= 2.0 ** -21 * float(mat.abs().max())
    codes = torch.from_numpy(rng.integers(-128, 128, (4, 16), dtype=np.int8))
    pk = ops.mlp_pack_weight(codes, 8)
    assert tuple(pk.shape) == (4, 8, 4) and torch.equal(pk[2, 3], codes[3, 8:12]) and not pk[:, 4:].any()


# ----------------------------------------------------------------------------- GPU: exact kernels on exact inputs
def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run_up0(cuda, x, wt, bias, gamma, beta, sc, eps=1e-5):
    from samq import ops
    b, h, w, _ = x.shape
    hi, lo = ops.convt_split_weight(_dev(cuda, wt))
    d0 = torch.empty((b, 2 * h, 2 * w, 64), dtype=torch.int8, device=cuda)
    d1 = torch.empty_like(d0)
    out = ops.upscale0_q8(_dev(cuda, x).view(-1, x.shape[-1]), hi, lo, _dev(cuda, bias), _dev(cuda, gamma),
                          _dev(cuda, beta), eps, b, h, w, *sc, dbg_q0=d0, dbg_q1=d1)
    plain = ops.upscale0_q8(_dev(cuda, x).view(-1, x.shape[-1]), hi, lo, _dev(cuda, bias), _dev(cuda, gamma),
                            _dev(cuda, beta), eps, b, h, w, *sc)
    assert torch.equal(plain, out)                                           # the debug outputs change nothing
    return d0.cpu().numpy(), d1.cpu().numpy(), out.cpu().numpy()


def _run_up1(cuda, x, wt, bias, hyper, s_hyper, sc):
    from samq import ops
    b, h, w, _ = x.shape
    hi, lo = ops.convt_split_weight(_dev(cuda, wt))
    d3 = torch.empty((b, 2 * h, 2 * w, 32), dtype=torch.int8, device=cuda)
    x4 = torch.empty_like(d3)
    args = (_dev(cuda, x), hi, lo, _dev(cuda, bias), _dev(cuda, hyper), _dev(cuda, s_hyper), *sc)
    masks = ops.upscale1_masks_q8(*args, dbg_q3=d3, x4=x4)
    assert torch.equal(ops.upscale1_masks_q8(*args), masks)
    return d3.cpu().numpy(), x4.cpu().numpy(), masks.cpu().numpy()


def _stage(what, out, ref, quot, exact=False):
    """Every code within +-1; no code differs outside the near-tie set, which holds at most 1 % of the stage."""
    mx, share, ties, outside = T.compare(out, ref, quot, what)
    print(f"[tail] {what}: max |dcode| {mx:.0f}, {share:.3e} differ, {ties:.3e} near a tie, {outside} differ outside")
    assert mx <= 1, what
    assert outside == 0, f"{what}: {outside} codes differ outside the near-tie set"
    if exact:
        assert share == 0.0, what
    else:
        assert ties <= 0.01, what


EXACT_CASES = [(1, 1, 1), (2, 1, 1), (1, 3, 5), (2, 3, 5), (1, 16, 16), (2, 16, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=str)
def test_upscale_kernels_exact_inputs(cuda, case):
    """Small-integer transposed-convolution weights and power-of-two scales: every fp32 sum and quotient
    is exact (exact .5 ties included), so the codes of qacts[0] / qacts[3] and the mask codes (an int32
    dot times a power of two) equal the numpy integer restatement bit for bit."""
    x, wt, bias, gamma, beta, sc = _up0_inputs(case, exact=True)
    d0, d1, out = _run_up0(cuda, x, wt, bias, gamma, beta, sc)
    c, q = T.upscale0_ref(x, sc[0], wt, bias, gamma, beta, 1e-5, *sc[1:])
    assert (np.abs(q["q0"] - np.floor(q["q0"])) == 0.5).mean() > 0.01      # exact ties are there
    assert np.array_equal(d0.astype(np.float64), c["q0"]), T.compare(d0, c["q0"], q["q0"])
    x1, wt1, bias1, hyper, s_hyper, sc1 = _up1_inputs(case, exact=True)
    d3, x4, masks = _run_up1(cuda, x1, wt1, bias1, hyper, s_hyper, sc1)
    c1, q1 = T.upscale1_masks_ref(x1, sc1[0], wt1, bias1, hyper, s_hyper, *sc1[1:], c4=x4)
    assert (np.abs(q1["q3"] - np.floor(q1["q3"])) == 0.5).mean() > 0.01
    assert np.array_equal(d3.astype(np.float64), c1["q3"]), T.compare(d3, c1["q3"], q1["q3"])
    _stage(f"exact {case} qacts[4]", x4, T.upscale1_masks_ref(x1, sc1[0], wt1, bias1, hyper, s_hyper, *sc1[1:],
                                                               c3=d3)[0]["q4"], q1["q4"])
    # the mask product from the kernel's own qacts[4] codes: integers times powers of two, ties and clamps
    assert (np.abs(q1["masks"] - np.floor(q1["masks"])) == 0.5).mean() > 0.01 and (np.abs(q1["masks"]) > 128).any()
    assert np.array_equal(masks.astype(np.float64), c1["masks"] * sc1[3]), T.compare(np.round(masks / sc1[3]), c1["masks"],
                                                                                      q1["masks"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", STAGE_CASES, ids=str)
def test_upscale_kernels_random_inputs_vs_float64(cuda, case):
    """Random float weights and scales, every quantiser stage against the float64 restatement of that
    stage on the kernel's own input codes: +-1, and equal outside the near-tie set (<= 1 % of the codes)."""
    x, wt, bias, gamma, beta, sc = _up0_inputs(case)
    d0, d1, out = _run_up0(cuda, x, wt, bias, gamma, beta, sc)
    c, q = T.upscale0_ref(x, sc[0], wt, bias, gamma, beta, 1e-5, *sc[1:])
    _stage(f"{case} convT + qacts[0]", d0, c["q0"], q["q0"])
    c, q = T.upscale0_ref(x, sc[0], wt, bias, gamma, beta, 1e-5, *sc[1:], c0=d0, c1=d1)
    _stage(f"{case} LayerNorm2D + qacts[1]", d1, c["q1"], q["q1"])
    _stage(f"{case} GELU + qacts[2]", out, c["q2"], q["q2"])
    x1, wt1, bias1, hyper, s_hyper, sc1 = _up1_inputs(case)
    d3, x4, masks = _run_up1(cuda, x1, wt1, bias1, hyper, s_hyper, sc1)
    c1, q1 = T.upscale1_masks_ref(x1, sc1[0], wt1, bias1, hyper, s_hyper, *sc1[1:])
    _stage(f"{case} convT + qacts[3]", d3, c1["q3"], q1["q3"])
    c1, q1 = T.upscale1_masks_ref(x1, sc1[0], wt1, bias1, hyper, s_hyper, *sc1[1:], c3=d3, c4=x4)
    _stage(f"{case} GELU + qacts[4]", x4, c1["q4"], q1["q4"])
    _stage(f"{case} masks", np.round(masks / np.float32(sc1[3])), c1["masks"], q1["masks"])
    assert np.array_equal(np.round(masks / np.float32(sc1[3])) * np.float32(sc1[3]), masks)   # code * s_q1 in f32


def _mlp_inputs(b, same):
    rng = _rng("mlp", (b, same))
    q = rng.integers(-128, 128, (b, 7, 256), dtype=np.int8)
    mlps = []
    for j in range(5):
        layers = []
        for n in (256, 256, 32 if j < 4 else 4):
            layers.append((rng.integers(-128, 128, (n, 256), dtype=np.int8), float(np.float32(rng.uniform(0.5, 1.5) * 1e-3)),
                           rng.standard_normal(n).astype(np.float32)))
        s1 = [float(np.float32(rng.uniform(0.015, 0.03))) for _ in range(2)]
        s2 = list(s1) if same else [float(np.float32(v * rng.uniform(0.6, 0.9))) for v in s1]
        mlps.append(dict(layers=layers, s1=s1, s2=s2, s3=float(np.float32(rng.uniform(0.02, 0.05)))))
    return q, mlps, float(np.float32(0.021))


def _run_mlps(cuda, q, mlps, s_in):
    from samq import ops
    pk = lambda i, pad=0: torch.stack([ops.mlp_pack_weight(torch.from_numpy(m["layers"][i][0]), pad) for m in mlps])
    bias = lambda i, n: torch.stack([torch.nn.functional.pad(torch.from_numpy(m["layers"][i][2]),
                                                             (0, n - m["layers"][i][2].size)) for m in mlps])
    scales = torch.tensor([[m["layers"][0][1], m["layers"][1][1], m["layers"][2][1], m["s1"][0], m["s2"][0],
                            m["s1"][1], m["s2"][1], m["s3"]] for m in mlps], dtype=torch.float32)
    b = q.shape[0]
    dbg = torch.empty((b, 5, 4, 256), dtype=torch.int8, device=cuda)
    args = (_dev(cuda, q), pk(0).to(cuda), pk(1).to(cuda), pk(2, 32).to(cuda), bias(0, 256).to(cuda),
            bias(1, 256).to(cuda), bias(2, 32).to(cuda), scales.to(cuda), 4, 32, 4, s_in)
    hyper, iou = ops.decoder_mlps_q8(*args, dbg=dbg)
    h2, i2 = ops.decoder_mlps_q8(*args)
    assert torch.equal(h2, hyper) and torch.equal(i2, iou)
    return hyper.cpu().numpy(), iou.cpu().numpy(), dbg.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("b,same", [(1, False), (3, False), (1, True), (3, True)])
def test_decoder_mlps_equal_composition_of_kernels(cuda, b, same):
    """The five MLPs in one launch against ``w8a8_gemm(EPI_Q8)`` -> ``relu_q8`` -> ``add_q8`` (the
    requantiser) per layer: bit-identical codes on random codes, scales and biases, with qacts1 and
    qacts2 at different and at equal scales.  The last layers' 32 / 4 rows are padded with zero rows
    to a width the GEMM takes."""
    from samq import ops
    q, mlps, s_in = _mlp_inputs(b, same)
    hyper, iou, dbg = _run_mlps(cuda, q, mlps, s_in)
    NP = 256
    for j, m in enumerate(mlps):
        x = _dev(cuda, q[:, 1 + j if j < 4 else 0])
        s = s_in
        for i, (w, sw, bias) in enumerate(m["layers"]):
            n = w.shape[0]
            wp = np.zeros((NP, 256), np.int8)
            wp[:n] = w
            bp = np.zeros(NP, np.float32)
            bp[:n] = bias
            ws = torch.full((NP,), sw, dtype=torch.float32, device=cuda)
            so = m["s1"][i] if i < 2 else m["s3"]
            y = ops.w8a8_gemm(x, ops.w8_repack(_dev(cuda, wp)), ws, NP, _dev(cuda, bp), ops.EPI_Q8, s, so)
            if i < 2:
                assert np.array_equal(dbg[:, j, 2 * i], y.cpu().numpy()), (j, i, "qacts1")
                y = ops.add_q8(ops.relu_q8(y), m["s1"][i], None, 0.0, m["s2"][i])
                assert np.array_equal(dbg[:, j, 2 * i + 1], y.cpu().numpy()), (j, i, "qacts2")
                assert (y > 0).any() and (y == 0).any()
                x, s = y, m["s2"][i]
            elif j < 4:
                assert np.array_equal(hyper[:, j], y[:, :n].cpu().numpy()), j
                assert np.abs(hyper[:, j]).max() > 40
            else:
                want = y[:, :n].cpu().float() * torch.tensor(m["s3"], dtype=torch.float32)
                assert np.array_equal(iou, want.numpy())


# ----------------------------------------------------------------------------- GPU: stage-local parity vs the reference
@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.PROMPT_SHAPES)
def test_tail_stage_local_parity(cuda, golden_dir, shape):
    """Each kernel on the golden's input codes (``layers.1.keys``; ``queries``; the golden's own
    ``qacts[2]`` and ``hyper_in``): every output code within +-1 of the golden's; stages of >= 1e4 codes
    differ in at most the float64 restatement's own share (test_tail_restatement_vs_golden) + 1e-4;
    the small stages (the MLPs' QActs, ``hyper_in``, ``iou_pred``) in no code outside the near-tie set.
    One derived exception, inside upscale1_masks only (below): qacts[4] and the masks behind a qacts[3]
    code that differs from the golden's are bounded by what that input difference implies."""
    p, ins, ref = _params(golden_dir), _golden_stage_inputs(golden_dir, shape), _golden_stage_refs(golden_dir, shape)
    rest = _restatement_vs_golden(golden_dir, shape)
    su = p["su"]
    got = {}
    got["q0"], got["q1"], got["q2"] = _run_up0(cuda, ins["keys"], p["w0"], p["b0"], p["gamma"], p["beta"],
                                               (p["s_keys"], su[0], su[1], su[2]), p["eps"])
    got["q3"], got["q4"], m = _run_up1(cuda, ins["x2"], p["w1"], p["b1"], ins["hyper"], p["s_hyper"],
                                       (su[2], su[3], su[4], p["s_q1"]))
    got["masks"] = np.round(m / np.float32(p["s_q1"]))
    hyper, iou, dbg = _run_mlps(cuda, ins["queries"], p["mlps"], p["s_q"])
    for j in range(5):
        for i, n in enumerate(("q1.0", "q2.0", "q1.1", "q2.1")):
            got[f"mlp{j}.{n}"] = dbg[:, j, i]
        got[f"mlp{j}.q3"] = hyper[:, j] if j < 4 else np.round(iou / np.float32(p["mlps"][4]["s3"]))
    # The issue's rules hold unmasked on every stage but two.  upscale1_masks chains qacts[3] -> GELU ->
    # qacts[4] -> mask product inside one launch and cannot be fed the golden's qacts[3]: where one of its
    # qacts[3] codes falls on the other side of a near tie (1 of 131072 here), the stages behind that
    # code no longer have the golden's input.  There, and only there, the bound is the one the input
    # difference implies (two quotients x apart round at most floor(x) + 1 apart):
    #  * qacts[4] behind a qacts[3] code d3 off: |GELU'| <= 1.13, so x <= 1.13 |d3| s3 / s4
    #    (s3 / s4 = 1.185: 2 codes; measured 2 and 1);
    #  * a mask behind a pixel whose qacts[4] codes are d4 off: the int32 dot moves by exactly
    #    hyper . d4, so x = |hyper . d4| s_hyper[m] s4 / s_q1.
    # The exempt positions are counted against the differing input codes.
    d3 = got["q3"].astype(np.float64) - ref["q3"]
    d4 = got["q4"].astype(np.float64) - ref["q4"]
    bound = {n: np.ones(ref[n].shape) for n in got}
    bound["q4"] = np.where(d3 != 0, np.floor(1.13 * np.abs(d3) * su[3] / su[4]) + 1, 1.0)
    dot = np.abs(np.einsum("bmc,byxc->bmyx", ins["hyper"].astype(np.float64), d4))
    x_m = dot * (p["s_hyper"].astype(np.float64)[None, :, None, None] * su[4] / p["s_q1"])
    px4 = np.transpose((d4 != 0).any(-1, keepdims=True), (0, 3, 1, 2))          # (B, 1, 2H, 2W)
    bound["masks"] = np.where(px4, np.floor(x_m) + 1, 1.0)
    exempt = {"q4": d3 != 0, "masks": np.broadcast_to(px4, ref["masks"].shape)}
    assert int(exempt["q4"].sum()) <= int((d3 != 0).sum())
    assert int(px4.sum()) <= int((d4 != 0).sum())
    fails = []
    for n, out in got.items():
        ex = exempt.get(n, np.zeros(ref[n].shape, bool))
        d = np.abs(out.astype(np.float64) - ref[n])
        over, share = int((d > bound[n]).sum()), float((d > 0).mean())
        outside = int(((d > 0) & ~ex & ~T.near_tie(rest[n][4])).sum())
        big = ref[n].size >= 10000
        print(f"[tail stage-local {shape}] {n}: {ref[n].size} codes, max |dcode| {d.max():.0f} (bound {bound[n].max():.0f} "
              f"at {int(ex.sum())} positions behind a differing input, 1 elsewhere), {share:.3e} differ (float64 "
              f"restatement {rest[n][1]:.3e}), {outside} outside the near-tie set")
        if over or (big and share > rest[n][1] + 1e-4) or (not big and outside):
            fails.append((n, float(d.max()), over, share, rest[n][1], outside))
    assert not fails, fails


# ----------------------------------------------------------------------------- GPU: end to end
def _predict(md, args, fused, taps=None):
    md.use_fused_tail = fused
    try:
        with torch.no_grad():
            masks, iou = md.predict_masks(*args, taps=taps)
        return masks.clone(), iou.clone()
    finally:
        md.use_fused_tail = True


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.PROMPT_SHAPES)
def test_fused_tail_end_to_end_vs_module_tail(cuda, golden_dir, shape):
    """``predict_masks`` with ``use_fused_tail`` True and False on the same engine: mask IoU with the
    golden >= the module-graph tail's - 0.01, ``iou_pred`` error <= its + 1e-3; the taps carry the new names
    and are the three kernels' outputs bit for bit."""
    g, _ = _golden(golden_dir)
    t = _tail_golden(golden_dir)
    sam = _gpu_model(cuda)
    md = sam.mask_decoder
    md.engine().drop_graphs()
    args = _prompt_inputs(sam, R.TEST_SEED, shape, cuda)
    taps = {}
    n0 = md.engine().forwards
    m_f, i_f = _predict(md, args, True, taps)
    m_m, i_m = _predict(md, args, False)
    assert md.engine().forwards == n0 + 2
    gold = _golden_tap(g, shape, "qact1").astype(np.float64)
    iou_f, iou_m = _iou(m_f.cpu().numpy(), gold), _iou(m_m.cpu().numpy(), gold)
    e_f = float(np.abs(i_f.cpu().numpy() - g[f"iou_pred:{shape}"]).max())
    e_m = float(np.abs(i_m.cpu().numpy() - g[f"iou_pred:{shape}"]).max())
    print(f"[tail e2e {shape}] mask IoU with the golden: fused {iou_f:.4f}, module tail {iou_m:.4f}; "
          f"iou_pred error: fused {e_f:.2e}, module tail {e_m:.2e}")
    assert m_f.shape == m_m.shape == (1, 4, 4 * R.GRID, 4 * R.GRID) and i_f.shape == i_m.shape == (1, 4)
    assert iou_f >= iou_m - 0.01
    assert e_f <= e_m + 1e-3
    names = [f"upscaling.qacts.{i}" for i in range(5)] + ["hyper_in", "qact1", "queries", "keys"]
    assert set(names) <= set(taps)
    assert torch.equal(taps["qact1"], m_f)
    # the taps are the kernels' own outputs: the three ops run here on the tapped queries / keys give
    # them back bit for bit, in the module graph's NCHW layout (parity with the golden: the stage-local test)
    from samq import ops
    eng = md.engine()
    tl, su = eng._tail, eng._tail["su"]
    s_k, s_q = eng.layers[-1]["s14"], eng.sf[4]
    kc = torch.round(taps["keys"] / s_k).to(torch.int8).view(-1, 256).contiguous()
    qc = torch.round(taps["queries"] / s_q).to(torch.int8).contiguous()
    assert torch.equal(kc.view(taps["keys"].shape).float() * s_k, taps["keys"])
    dbg = [torch.empty((1, 2 * R.GRID, 2 * R.GRID, 64), dtype=torch.int8, device=cuda) for _ in range(2)]
    dbg += [None] + [torch.empty((1, 4 * R.GRID, 4 * R.GRID, 32), dtype=torch.int8, device=cuda) for _ in range(2)]
    u0, u1 = tl["up0"], tl["up1"]
    dbg[2] = ops.upscale0_q8(kc, u0["hi"], u0["lo"], u0["bias"], tl["gamma"], tl["beta"], tl["eps"], 1, R.GRID, R.GRID,
                             s_k, su[0], su[1], su[2], dbg_q0=dbg[0], dbg_q1=dbg[1])
    hyper, iou = ops.decoder_mlps_q8(qc, tl["w1"], tl["w2"], tl["w3"], tl["b1"], tl["b2"], tl["b3"], tl["scales"],
                                     tl["n_hyper"], tl["no_h"], tl["no_i"], s_q)
    masks = ops.upscale1_masks_q8(dbg[2], u1["hi"], u1["lo"], u1["bias"], hyper, tl["s_hyper"], su[2], su[3], su[4],
                                  tl["s_q1"], dbg_q3=dbg[3], x4=dbg[4])
    for i in range(5):
        v = taps[f"upscaling.qacts.{i}"]
        assert tuple(v.shape) == t[f"{shape}:upscaling.qacts.{i}"].shape     # NCHW, as the module graph's
        assert torch.equal(v, dbg[i].permute(0, 3, 1, 2).float() * su[i]), i
    assert tuple(taps["hyper_in"].shape) == (1, 4, 32)
    assert torch.equal(taps["hyper_in"], hyper.float() * tl["s_hyper"][None, :, None])
    assert torch.equal(masks, m_f) and torch.equal(iou, i_f)


@pytest.mark.gpu
def test_fused_tail_replay_equals_eager(cuda):
    """The whole click from one graph: ``masks`` and ``iou_pred`` of the replay equal the eager run bit for
    bit, for two token counts and two images of the same grid (the fused tail is deterministic); the
    ``forward`` replay contract (``queries`` / ``keys``) holds beside it."""
    sam = _gpu_model(cuda)
    md = sam.mask_decoder
    eng = md.engine()
    eng.drop_graphs()
    with torch.no_grad():
        ins = {s: _prompt_inputs(sam, R.TEST_SEED, s, cuda) for s in R.PROMPT_SHAPES}
        emb2 = torch.from_numpy(R.image_embedding(R.CALIB_SEEDS[1])).to(cuda)
        embs = (ins["point"][0], emb2)
        eager = {(k, s): _predict(md, (e,) + ins[s][1:], True) for k, e in enumerate(embs) for s in ins}
        again = {(k, s): _predict(md, (e,) + ins[s][1:], True) for k, e in enumerate(embs) for s in ins}
        for key in eager:
            assert torch.equal(eager[key][0], again[key][0]) and torch.equal(eager[key][1], again[key][1]), key
        assert not torch.equal(eager[(0, "point")][0], eager[(1, "point")][0])
        md.predict_masks(*ins["point"])                                      # image 0 is the cached one again
        q_eager = [t.clone() for t in eng.forward(embs[0], ins["point"][3], ins["point"][1],
                                                  _raw_tokens(md, ins["point"][2]))]
        for s in ins:
            eng.capture(5 + ins[s][2].shape[1])
        assert len(eng._graphs) == 2 and all(g["graph_masks"] is not None for g in eng._graphs.values())
        n0 = eng.forwards
        for k, e in enumerate(embs):
            for s in ins:
                m, i = _predict(md, (e,) + ins[s][1:], True)
                assert torch.equal(m, eager[(k, s)][0]), (k, s)
                assert torch.equal(i, eager[(k, s)][1]), (k, s)
        assert eng.forwards == n0 + 4 and len(eng._graphs) == 2              # the new image kept the graphs
        md.predict_masks(*ins["point"])
        q_replay = eng.forward(embs[0], ins["point"][3], ins["point"][1], _raw_tokens(md, ins["point"][2]))
        assert torch.equal(q_replay[0], q_eager[0]) and torch.equal(q_replay[1], q_eager[1])
        eng.drop_graphs()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fused_tail_is_three_launches(cuda):
    """Profiler count: the tail behind the transformer's codes is exactly three kernel launches."""
    from torch.profiler import ProfilerActivity, profile
    sam = _gpu_model(cuda)
    md = sam.mask_decoder
    eng = md.engine()
    eng.drop_graphs()
    with torch.no_grad():
        args = _prompt_inputs(sam, R.TEST_SEED, "point", cuda)
        md.predict_masks(*args)
        img = eng._image
        qc = torch.zeros((1, 7, 256), dtype=torch.int8, device=cuda)
        K = torch.zeros((img["hw"], 256), dtype=torch.int8, device=cuda)
        run = lambda: eng._tail_run(qc, K, 0.05, 0.05, img, None)
        run()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
    ev = [(e.key, e.count) for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    print(f"[tail] launches: {ev}")
    assert sum(c for _, c in ev) == 3, ev
    assert sorted(k.split("(")[0].split("::")[-1] for k, _ in ev) == ["decoder_mlps_kernel", "upscale0_kernel",
                                                                      "upscale1_masks_kernel"]


@pytest.mark.gpu
def test_sam_predictor_through_fused_tail(cuda):
    """``SamPredictor.predict`` on ``build_fq_sam``: finite masks of the right shape through
    ``forward_masks`` (the engine's counter moves; ``heads_forward`` is not called)."""
    from samq.sam_decoder import SamPredictor
    sam = _gpu_model(cuda)
    enc = sam.image_encoder
    if "enc_ready" not in _DECODER_CACHE:   # shared with test_sam_predictor_on_fq_sam_uses_decoder_engine
        torch.manual_seed(3)
        with torch.no_grad():
            for prm in enc.parameters():
                if prm.dim() > 1:
                    prm.copy_(torch.randn_like(prm) * 0.05)
        img = torch.randn(1, 3, R.IMG, R.IMG, device=cuda)
        enc.model_dequant()          # Sam.model_quant switched the (uncalibrated) encoder too
        enc.calibrate_with([img, img * 0.5])
        _DECODER_CACHE["enc_ready"] = True
    md = sam.mask_decoder
    assert md.use_fused_tail and enc.is_quant() and md.is_quant()
    calls = []
    orig = md.heads_forward
    md.heads_forward = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        pred = SamPredictor(sam)
        rng = np.random.Generator(np.random.PCG64(1))
        pred.set_image(rng.integers(0, 256, (200, R.IMG, 3), dtype=np.uint8))
        n0 = md.engine().forwards
        masks, iou, low = pred.predict(point_coords=np.array([[100.0, 80.0]]), point_labels=np.array([1]))
    finally:
        del md.heads_forward
    assert md.engine().forwards == n0 + 1 and not calls
    assert masks.shape == (3, 200, R.IMG) and masks.dtype == bool
    assert iou.shape == (3,) and np.isfinite(iou).all()
    assert low.shape == (3, 4 * R.GRID, 4 * R.GRID) and np.isfinite(low).all()


# ----------------------------------------------------------------------------- GPU: refusals
@pytest.mark.gpu
def test_fused_tail_refusals(cuda):
    """``sigmoid_output=True``, a per-channel or non-zero-zero-point tail QAct: NotImplementedError when the
    engine is built; mismatched shapes at the wrappers: AssertionError before any launch."""
    from samq import ops
    base = _calibrated_cpu().mask_decoder

    def engine_of(edit):
        md = copy.deepcopy(base).to(cuda)
        edit(md)
        md.refresh()
        return md.engine()

    def sig(md):
        md.iou_prediction_head.sigmoid_output = True

    def per_channel(md):
        q = md.qacts[3].quantizer
        q.scale = q.scale.reshape(-1).repeat(32)
        q.zero_point = q.zero_point.reshape(-1).repeat(32)

    def zero_point(md):
        md.output_hypernetworks_mlps[1].qacts2[0].quantizer.zero_point += 3
    for edit in (sig, per_channel, zero_point):
        with pytest.raises(NotImplementedError):
            engine_of(edit)

    def off(md):   # the module-graph tail still runs such a model: the snapshot is skipped
        sig(md)
        md.use_fused_tail = False
    eng = engine_of(off)
    assert eng._tail is None
    x, wt, bias, hyper, s_hyper, sc = _up1_inputs((1, 3, 5))
    hi, lo = ops.convt_split_weight(_dev(cuda, wt))
    with pytest.raises(AssertionError):     # hyper rows for another batch size
        ops.upscale1_masks_q8(_dev(cuda, x), hi, lo, _dev(cuda, bias), _dev(cuda, np.concatenate([hyper, hyper])),
                              _dev(cuda, s_hyper), *sc)
    with pytest.raises(AssertionError):     # weight planes of another Cin
        ops.upscale1_masks_q8(_dev(cuda, x[..., :32]), hi, lo, _dev(cuda, bias), _dev(cuda, hyper), _dev(cuda, s_hyper),
                              *sc)
    with pytest.raises(NotImplementedError):   # 64 output channels into the 32-channel kernel (the C ABI's refusal)
        w64 = np.zeros((64, 64, 2, 2), np.float32)
        h64, l64 = ops.convt_split_weight(_dev(cuda, w64))
        ops.upscale1_masks_q8(_dev(cuda, x), h64, l64, _dev(cuda, np.zeros(64, np.float32)),
                              _dev(cuda, np.zeros((1, 4, 64), np.int8)), _dev(cuda, s_hyper), *sc)
