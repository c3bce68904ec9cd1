"""fq_vit W8A8 prompt encoder + mask decoder (``samq.fq_sam``): the module mirror against the
reference's golden (``golden/fq_decoder.npz``), the decoder's HIP kernels against the restatements of
``_fq_decoder_ref.py``, and the fused ``W8A8DecoderEngine``."""
from __future__ import annotations

import copy
import ctypes
import json

import numpy as np
import pytest
import torch

import _fq_decoder_ref as R
from samq import fq_sam  # noqa: F401  (every test here is about this module)


# ----------------------------------------------------------------------------- shared (built once)
_CACHE = {}


def _golden(golden_dir):
    if "g" not in _CACHE:
        g = np.load(golden_dir / "fq_decoder.npz")
        _CACHE["g"] = {k: g[k] for k in g.files}
        _CACHE["meta"] = json.loads(str(g["meta"]))
    return _CACHE["g"], _CACHE["meta"]


def _build(device="cpu"):
    """``build_fq_sam`` at the fixture's geometry with the seeded weights (encoder depth 1: unused)."""
    from samq import fq_sam
    sam = fq_sam.build_fq_sam("vit_b", img_size=R.IMG, depth=1)
    sub = {k: v for k, v in sam.state_dict().items() if k.startswith(("prompt_encoder.", "mask_decoder."))}
    state = R.decoder_state({k: tuple(v.shape) for k, v in sub.items()})
    missing, unexpected = sam.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(m.startswith("image_encoder.") for m in missing)
    return sam.to(device)


def _prompt_inputs(sam, seed, shape, device="cpu"):
    emb = torch.from_numpy(R.image_embedding(seed)).to(device)
    pt, lab, box = R.prompt_set(seed, shape)
    sparse, dense = sam.prompt_encoder(points=(torch.from_numpy(pt).to(device), torch.from_numpy(lab).to(device)),
                                       boxes=None if box is None else torch.from_numpy(box).to(device), masks=None)
    return emb, sam.prompt_encoder.get_dense_pe(), sparse, dense


def _calibrated_cpu():
    """The CPU model after the reference's calibration sequence on the fixture's three sets."""
    if "cpu" not in _CACHE:
        sam = _build()
        with torch.no_grad():
            sam.model_open_calibrate()
            for i, seed in enumerate(R.CALIB_SEEDS):
                if i == len(R.CALIB_SEEDS) - 1:
                    sam.model_open_last_calibrate()
                sam.mask_decoder.predict_masks(*_prompt_inputs(sam, seed, "point_box"))
            sam.model_close_calibrate()
            sam.model_quant()
        _CACHE["cpu"] = sam
    return _CACHE["cpu"]


def _cpu_taps(shape):
    """Module-graph quant forward on the held-out set: (taps, masks, iou_pred, every QAct's output)."""
    key = ("taps", shape)
    if key not in _CACHE:
        sam = _calibrated_cpu()
        from samq import fq_vit
        acts, hooks = {}, []
        for n, m in sam.mask_decoder.named_modules():
            if isinstance(m, fq_vit.QAct):
                hooks.append(m.register_forward_hook(lambda mod, i, o, n=n: acts.__setitem__(n, o.detach())))
        taps = {}
        with torch.no_grad():
            masks, iou = sam.mask_decoder.predict_masks(*_prompt_inputs(sam, R.TEST_SEED, shape), taps=taps)
        for h in hooks:
            h.remove()
        _CACHE[key] = (taps, masks, iou, acts)
    return _CACHE[key]


def _tap_scales(g):
    scales = dict(zip(g["act_scale_names"], g["act_scales"]))
    return {t: float(scales[n]) for t, n in zip(g["tap_scale_names"], g["tap_scale_of"])}


def _golden_tap(g, shape, name):
    return g["tap:" + name] if "tap:" + name in g else g[f"tap:{shape}:{name}"]


def _rows(x):
    """NCHW -> token rows (B, hw, C)."""
    return x.flatten(2).permute(0, 2, 1)


# ----------------------------------------------------------------------------- CPU: module mirror vs golden
def test_fq_decoder_state_dict_keys_match_reference(golden_dir):
    g, _ = _golden(golden_dir)
    sam = _build()
    sub = lambda m: sorted(k for k in m.state_dict() if k.startswith(("prompt_encoder.", "mask_decoder.")))
    assert sub(sam) == list(g["keys_built"])
    assert sub(_calibrated_cpu()) == list(g["keys_calibrated"])


def test_fq_decoder_calibration_matches_reference_scales(golden_dir):
    """open_calibrate -> three sets -> open_last_calibrate -> close_calibrate -> model_quant: every
    activation and weight scale equals the reference's bit for bit."""
    from samq import fq_vit
    g, _ = _golden(golden_dir)
    sam = _calibrated_cpu()
    named = {n: m for n, m in sam.named_modules() if n.startswith(("prompt_encoder.", "mask_decoder."))}
    ours = {n: m.quantizer.scale for n, m in named.items() if isinstance(m, fq_vit.QAct) and m.quantizer.scale is not None}
    assert sorted(ours) == sorted(g["act_scale_names"])
    for n, s in zip(g["act_scale_names"], g["act_scales"]):
        assert np.float32(ours[n].reshape(-1)[0].item()) == np.float32(s), n
    wnames = sorted(k[len("wscale:"):] for k in g if k.startswith("wscale:"))
    wours = {n: m.quantizer.scale for n, m in named.items()
             if isinstance(m, (fq_vit.QLinear, fq_vit.QConv2d)) and m.quantizer.scale is not None}
    assert sorted(wours) == wnames
    for n in wnames:
        assert np.array_equal(wours[n].reshape(-1).numpy(), g["wscale:" + n]), n
    # the transposed convolutions are outside the switches' type list: never calibrated, never quantised
    assert all(m.quantizer.scale is None and not m.quant for m in sam.mask_decoder.output_upscaling
               if hasattr(m, "quantizer"))


@pytest.mark.parametrize("shape", R.PROMPT_SHAPES)
def test_fq_decoder_module_graph_matches_reference(golden_dir, shape):
    """Quant-mode module graph on the held-out set: every tap's codes equal the golden's, iou_pred
    within 1e-5."""
    g, _ = _golden(golden_dir)
    taps, masks, iou, _ = _cpu_taps(shape)
    ts = _tap_scales(g)
    assert taps["qact_embed1"].shape[1] == (7 if shape == "point" else 9)
    for name, s in ts.items():
        ours = np.round(taps[name].numpy() / s)
        want = _golden_tap(g, shape, name).astype(np.float64)
        assert ours.shape == want.shape, name
        assert np.array_equal(ours, want), (name, float(np.abs(ours - want).max()))
    assert torch.equal(taps["keys"], taps["layers.1.keys"])
    if shape == R.STAGE_SHAPE:   # every transformer QAct on the token rows (the stage-local test's references)
        acts = _cpu_taps(shape)[3]
        names = [k[4:] for k in g if k.startswith("act:")]
        assert len(names) >= 50
        for n in names:
            s = float(dict(zip(g["act_scale_names"], g["act_scales"]))["mask_decoder." + n])
            assert np.array_equal(np.round(acts[n].numpy() / s), g["act:" + n].astype(np.float64)), n
    assert np.abs(iou.numpy() - g[f"iou_pred:{shape}"]).max() <= 1e-5


def test_fq_decoder_transformer_restatement_matches_module_graph(golden_dir):
    """The plain restatement (fp32) reproduces the module graph's transformer outputs (the same ops in
    another association: all codes within +-1, <= 1e-3 off by one)."""
    g, _ = _golden(golden_dir)
    ts = _tap_scales(g)
    sam = _calibrated_cpu()
    taps = _cpu_taps("point")[0]
    sd = sam.mask_decoder.state_dict()
    q, k = R.transformer_ref(sd, taps["qact_embed1"], _rows(taps["qact_embed2"]), _rows(taps["pos_src_qact"]))
    assert R.off_by_one(np.round(q.numpy() / ts["queries"]), np.round(taps["queries"].numpy() / ts["queries"]))[1] <= 1e-3
    assert R.off_by_one(np.round(k.numpy() / ts["layers.1.keys"]),
                        np.round(taps["keys"].numpy() / ts["layers.1.keys"]))[1] <= 1e-3


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=str)
def test_attention_inputs_fp32_vs_fp64(case):
    """The condition on the kernel-test inputs: the fp32 and fp64 restatements agree (all codes
    within +-1, <= 1e-4 off by one), so the GPU bound measures the kernel, not the reference."""
    q, k, v = R.attn_inputs(case)
    a = R.attention_ref(q, k, v, case[1], *R.attn_scales(case), dtype=torch.float32)
    b = R.attention_ref(q, k, v, case[1], *R.attn_scales(case), dtype=torch.float64)
    mx, frac = R.off_by_one(a, b)
    print(f"[attn inputs] {case}: fp32 vs fp64 max {mx:.0f}, {frac:.2e} off by one")
    assert mx <= 1 and frac <= 1e-4
    assert np.abs(b).max() > 60   # the output range is used


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=str)
def test_exact_attention_inputs_fp32_vs_fp64(case):
    q, k, v, scales = R.exact_attn_inputs(case)
    a = R.attention_ref(q, k, v, case[1], *scales, dtype=torch.float32)
    b = R.attention_ref(q, k, v, case[1], *scales, dtype=torch.float64)
    mx, frac = R.off_by_one(a, b)
    assert mx <= 1 and frac <= 1e-4


@pytest.mark.parametrize("case", R.EXACT_PEAKED_CASES, ids=str)
def test_exact_peaked_attention_inputs_fp32_vs_fp64(case):
    """The same condition at the sharp softmax scale (s_a1 = 2^-1): the codes are those of the plain
    set and so are the integer score codes."""
    q, k, v, scales = R.exact_attn_inputs(case, peaked=True)
    plain = R.exact_attn_inputs(case)
    assert all(np.array_equal(x, y) for x, y in zip((q, k, v), plain[:3]))
    assert scales[0] * scales[1] / scales[3] == plain[3][0] * plain[3][1] / plain[3][3]   # the same score codes
    a = R.attention_ref(q, k, v, case[1], *scales, dtype=torch.float32)
    b = R.attention_ref(q, k, v, case[1], *scales, dtype=torch.float64)
    mx, frac = R.off_by_one(a, b)
    print(f"[exact peaked inputs] {case}: fp32 vs fp64 max {mx:.0f}, {frac:.2e} off by one")
    assert mx <= 1 and frac <= 1e-4


def test_decoder_kernels_refuse_unsupported_shapes():
    """The documented error codes, before anything reaches the device (runs without a GPU)."""
    from samq import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    run = lambda q, B, nq, nk, heads, hd: lib.samq_attention_q8_plain(q, p, p, p, B, nq, nk, heads, hd, 0.1, 0.1, 0.1,
                                                                      0.1, 0.1, None)
    assert run(p, 1, 7, 7, 8, 24) == _lib.SAMQ_ERR_UNSUPPORTED          # D = 24
    assert "head_dim" in lib.samq_last_error().decode()
    assert run(p, 1, 7, 7, 16, 32) == _lib.SAMQ_ERR_UNSUPPORTED         # H * D = 512
    assert run(None, 1, 7, 7, 8, 16) == _lib.SAMQ_ERR_INVALID           # null pointer with Nq > 0
    assert "null pointer" in lib.samq_last_error().decode()
    assert run(None, 1, 0, 7, 8, 16) == _lib.SAMQ_OK                    # Nq = 0: nothing to do
    assert run(p, 1, 7, 0, 8, 16) == _lib.SAMQ_ERR_INVALID              # a softmax over no key
    assert lib.samq_add_q8(None, 0.1, None, 0.1, 0, None, 0, 0.1, 0, None) == _lib.SAMQ_OK
    assert lib.samq_add_q8(None, 0.1, None, 0.1, 0, p, 8, 0.1, 0, None) == _lib.SAMQ_ERR_INVALID
    assert lib.samq_add_q8(p, 0.1, p, 0.1, 16, p, 8, 0.1, 0, None) == _lib.SAMQ_ERR_INVALID   # period > n
    assert lib.samq_relu_q8(None, 0, None) == _lib.SAMQ_OK
    assert lib.samq_relu_q8(None, 4, None) == _lib.SAMQ_ERR_INVALID


def test_fq_decoder_cpu_quant_runs_module_graph():
    """On the CPU the quantised decoder is the module graph throughout (no engine is built)."""
    sam = _calibrated_cpu()
    assert sam.mask_decoder.is_quant() and sam.mask_decoder._engine is None
    with pytest.raises(RuntimeError):
        sam.mask_decoder.engine()


# ----------------------------------------------------------------------------- GPU: kernels
def _codes_close(out, ref, frac_max, what):
    mx, frac = R.off_by_one(out, ref)
    print(f"[fq decoder] {what}: max |dcode| {mx:.0f}, {frac:.3e} off by one")
    assert mx <= 1, f"{what}: code differs by {mx}"
    assert frac <= frac_max, f"{what}: {frac:.3e} of the codes off by one (> {frac_max})"
    return frac


def _attn_gpu(cuda, q, k, v, heads, scales):
    from samq import ops
    t = lambda a: torch.from_numpy(a).to(cuda)
    return ops.attention_q8_plain(t(q), t(k), t(v), heads, *(float(s) for s in scales)).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=str)
def test_attention_q8_plain_vs_restatement(cuda, case):
    """All codes within +-1 and <= 5e-3 off by one of the fp32 restatement, on every launch branch."""
    q, k, v = R.attn_inputs(case)
    ref = R.attention_ref(q, k, v, case[1], *R.attn_scales(case), dtype=torch.float32)
    _codes_close(_attn_gpu(cuda, q, k, v, case[1], R.attn_scales(case)), ref, 5e-3, f"attention {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.EXACT_CASES, ids=str)
def test_attention_q8_plain_exact_ties(cuda, case):
    """Exact-tie scores (round half to even in the score quantiser) and the uniform row against fp64."""
    q, k, v, scales = R.exact_attn_inputs(case)
    ref = R.attention_ref(q, k, v, case[1], *scales, dtype=torch.float64)
    out = _attn_gpu(cuda, q, k, v, case[1], scales)
    _codes_close(out, ref, 1e-4, f"exact attention {case}")
    # query 0 (all-zero codes): equal scores on every key, in every key chunk -> the mean of v
    mean_v = v.astype(np.float64).mean(axis=1) * scales[2] / scales[4]
    assert np.abs(out[:, 0].astype(np.float64) - np.clip(mean_v, -128, 127)).max() <= 0.5 + 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.EXACT_PEAKED_CASES, ids=str)
def test_attention_q8_plain_exact_ties_peaked(cuda, case):
    """test_attention_q8_plain_exact_ties at the sharp softmax scale (s_a1 = 2^-1): near one-hot rows,
    partial softmax states of lanes and waves whose integer maxima lie far apart."""
    q, k, v, scales = R.exact_attn_inputs(case, peaked=True)
    ref = R.attention_ref(q, k, v, case[1], *scales, dtype=torch.float64)
    out = _attn_gpu(cuda, q, k, v, case[1], scales)
    _codes_close(out, ref, 1e-4, f"exact peaked attention {case}")
    mean_v = v.astype(np.float64).mean(axis=1) * scales[2] / scales[4]
    assert np.abs(out[:, 0].astype(np.float64) - np.clip(mean_v, -128, 127)).max() <= 0.5 + 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.TIE_CASES, ids=str)
def test_attention_q8_plain_output_ties(cuda, case):
    """The output quantiser on exact quotients: uniform softmax rows whose p.v / s_out is exact in any
    precision, with exact .5 ties (round half to even) and clamps -- every code equal, on both branches."""
    q, k, v, want, quot = R.output_tie_inputs(case)
    ties = np.abs(np.abs(quot - np.floor(quot)) - 0.5) == 0
    assert ties.mean() > 0.01
    ref = R.attention_ref(q, k, v, case[1], *R.tie_scales(case), dtype=torch.float64)
    assert np.array_equal(ref, want)
    out = _attn_gpu(cuda, q, k, v, case[1], R.tie_scales(case))
    assert np.array_equal(out.astype(np.float64), want), R.off_by_one(out, want)


def _add_ref(a, s_a, b, s_b, s_out):
    """torch on f32: two fake-quant tensors added, then UniformQuantizer (CPU: correctly rounded division)."""
    x = a.float() * torch.tensor(s_a, dtype=torch.float32)
    if b is not None:
        x = x + b.float() * torch.tensor(s_b, dtype=torch.float32)
    return (x / torch.tensor(s_out, dtype=torch.float32)).round().clamp(-128, 127)


@pytest.mark.gpu
def test_add_q8_bit_identical_to_torch(cuda):
    from samq import ops
    rng = np.random.Generator(np.random.PCG64(77))
    s_a, s_b = float(np.float32(0.0371)), float(np.float32(0.0203))
    for rows, c, brows, s_out in [(37, 256, 37, 0.05), (3 * 50, 256, 50, 0.031), (7, 13, 7, 0.05), (6, 13, 3, 0.0123),
                                  (1, 3, 1, 0.04)]:
        s_out = float(np.float32(s_out))
        a = torch.from_numpy(rng.integers(-128, 128, (rows, c), dtype=np.int8))
        b = torch.from_numpy(rng.integers(-128, 128, (brows, c), dtype=np.int8))
        ref = _add_ref(a, s_a, b.repeat(rows // brows, 1), s_b, s_out)
        assert (ref == 127).any() and (ref == -128).any() or c < 16      # clamps at both ends
        out = ops.add_q8(a.to(cuda), s_a, b.to(cuda), s_b, s_out)
        assert torch.equal(out.cpu().float(), ref), (rows, c, brows)
        fq = ops.add_q8(a.to(cuda), s_a, b.to(cuda), s_b, s_out, fake=True)
        assert torch.equal(fq.cpu(), ref * torch.tensor(s_out, dtype=torch.float32))
        req = ops.add_q8(a.to(cuda), s_a, None, 0.0, s_out)             # requantisation
        assert torch.equal(req.cpu().float(), _add_ref(a, s_a, None, 0.0, s_out))
    # x * s requantised at s is the identity on the codes (qact8 on mlp.qact2's output)
    a = torch.arange(-128, 128, dtype=torch.int8).repeat(3)[:767]
    assert torch.equal(ops.add_q8(a.to(cuda), s_a, None, 0.0, s_a).cpu(), a)


@pytest.mark.gpu
def test_relu_q8_matches_q8_of_relu(cuda):
    """``max(q8(y), 0)`` on the EPI_Q8 output of a decoder-sized GEMM == q8(relu(y)) of the f32 output."""
    from samq import ops
    rng = np.random.Generator(np.random.PCG64(5))
    m, k, n = 7, 256, 2048
    a = torch.from_numpy(rng.integers(-128, 128, (m, k), dtype=np.int8)).to(cuda)
    w = torch.from_numpy(rng.integers(-128, 128, (n, k), dtype=np.int8)).to(cuda)
    ws = torch.from_numpy((rng.uniform(0.5, 1.5, n) * 1e-3).astype(np.float32)).to(cuda)
    bias = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(cuda)
    wp = ops.w8_repack(w)
    s_in, s_out = 0.02, float(np.float32(0.011))
    codes = ops.w8a8_gemm(a, wp, ws, n, bias, ops.EPI_Q8, s_in, s_out)
    want = torch.clamp(codes, min=0)
    y = ops.w8a8_gemm(a, wp, ws, n, bias, ops.EPI_F32, s_in)
    via_f32 = ops.quantize(torch.relu(y).contiguous(), s_out)
    out = ops.relu_q8(codes.clone())
    assert torch.equal(out, want) and (codes < 0).any() and (want > 0).any()
    assert torch.equal(out, via_f32)
    for nn_ in (1, 2, 3, 5, 1027):                                       # tails
        x = torch.from_numpy(rng.integers(-128, 128, nn_, dtype=np.int8)).to(cuda)
        assert torch.equal(ops.relu_q8(x.clone()), torch.clamp(x, min=0))


# ----------------------------------------------------------------------------- GPU: engine
def _gpu_model(cuda):
    """The calibrated model on the GPU (a copy of the CPU one: the same scales, bit for bit)."""
    if "gpu" not in _CACHE:
        _CACHE["gpu"] = copy.deepcopy(_calibrated_cpu()).to(cuda)
    return _CACHE["gpu"]


@pytest.mark.gpu
def test_fq_decoder_stage_local_parity(cuda, golden_dir):
    """Every fused stage of the engine, fed the int8 input codes of that stage, reproduces its output
    codes: all within +-1 and, per stage, <= 1e-4 off by one for the integer-exact stages (adds, GEMM
    epilogues, LayerNorm), <= 5e-3 for the attentions.

    Inputs and references on the token rows (2304 codes a stage: a single code is over the 1e-4) are
    the golden's own ``act:`` codes of the reference run; on the image rows (65536 codes a stage) they
    are the CPU module graph's of the machine that runs the test, which
    test_fq_decoder_module_graph_matches_reference pins to the golden.  The module graph's fp32
    matmuls round differently from machine to machine: recomputed on another CPU, one mid-quantiser
    quotient of the final out_proj (-49.49998 in fp64) fell on the other side of its midpoint, and
    the engine, which agrees with the golden and with fp64 there, was off by one against it."""
    from samq import ops
    g, _ = _golden(golden_dir)
    shape = R.STAGE_SHAPE
    taps, _, _, acts = _cpu_taps(shape)
    sam = _calibrated_cpu()
    md = sam.mask_decoder
    eng = _gpu_model(cuda).mask_decoder.engine()
    scale = {n: float(m.quantizer.scale) for n, m in md.named_modules() if n in acts}
    assert sum(k.startswith("act:") for k in g) >= 50

    def codes(n):
        if "act:" + n in g:
            t = torch.from_numpy(g["act:" + n])
        else:
            t = torch.round(acts[n] / scale[n]).to(torch.int8)
        if t.dim() == 4:
            t = _rows(t)
        return t.reshape(-1, t.shape[-1]).contiguous().to(cuda)

    def check(what, out, n, tol=1e-4):
        _codes_close(out.cpu().numpy().reshape(-1), codes(n).cpu().numpy().reshape(-1), tol, what)

    T, P = codes("qact_embed1"), codes("pos_src_qact")
    s_T, s_P = scale["qact_embed1"], scale["pos_src_qact"]
    b = 1

    def attention(pre, a, qin_n, kin_n, vin_n):
        for proj, inn, outn in (("q", qin_n, "qact1_1"), ("k", kin_n, "qact1_2"), ("v", vin_n, "qact1_3")):
            check(pre + proj + "_proj", eng._gemm(codes(inn), a[proj], ops.EPI_Q8, scale[inn], scale[pre + outn]),
                  pre + outn)
        q, k, v = (codes(pre + n).view(b, -1, a["q"]["n"]) for n in ("qact1_1", "qact1_2", "qact1_3"))
        o = ops.attention_q8_plain(q, k, v, a["heads"], a["s_q"], a["s_k"], a["s_v"], a["s_a1"], a["s_ao"])
        check(pre + "attention", o, pre + "qact2", 5e-3)

    def out_proj(pre, a, res_n, out_n):
        res = codes(res_n) if res_n else torch.zeros_like(codes(out_n))
        out = eng._gemm(codes(pre + "qact2"), a["o"], ops.EPI_Q8_RES, a["s_ao"], scale[out_n], mid=a["s_o"], res=res,
                        res_scale=scale[res_n] if res_n else 1.0)
        check(pre + "out_proj+res", out, out_n)

    def ln(norm, in_n, out_n):
        check(out_n + " (LayerNorm)", ops.layernorm_q(codes(in_n), *norm, in_scale=scale[in_n], out_scale=scale[out_n]),
              out_n)

    q_in, k_in = "qact_embed1", "qact_embed2"
    for i, L in enumerate(eng.layers):
        p = f"transformer.layers.{i}."
        if i == 0:
            attention(p + "self_attn.", L["self_attn"], q_in, q_in, q_in)
            out_proj(p + "self_attn.", L["self_attn"], None, p + "qact2")
        else:
            check(p + "qact_pos", ops.add_q8(T, s_T, None, 0.0, scale[p + "qact_pos"]), p + "qact_pos")
            check(p + "qact1", ops.add_q8(codes(q_in), scale[q_in], codes(p + "qact_pos"), scale[p + "qact_pos"],
                                          scale[p + "qact1"]), p + "qact1")
            attention(p + "self_attn.", L["self_attn"], p + "qact1", p + "qact1", q_in)
            out_proj(p + "self_attn.", L["self_attn"], q_in, p + "qact2")
        ln(L["norms"][0], p + "qact2", p + "qact3")
        check(p + "qact4", ops.add_q8(codes(p + "qact3"), scale[p + "qact3"], T, s_T, scale[p + "qact4"]), p + "qact4")
        check(p + "qact5", ops.add_q8(codes(k_in), scale[k_in], P, s_P, scale[p + "qact5"]), p + "qact5")
        attention(p + "cross_attn_token_to_image.", L["t2i"], p + "qact4", p + "qact5", k_in)
        out_proj(p + "cross_attn_token_to_image.", L["t2i"], p + "qact3", p + "qact6")
        ln(L["norms"][1], p + "qact6", p + "qact7")
        h = ops.relu_q8(eng._gemm(codes(p + "qact7"), L["lin1"], ops.EPI_Q8, scale[p + "qact7"], scale[p + "mlp.qact1"]))
        check(p + "lin1+relu", h, p + "mlp.qact1")
        assert scale[p + "qact8"] == scale[p + "mlp.qact2"]       # minmax on the same tensor
        check(p + "lin2+res", eng._gemm(codes(p + "mlp.qact1"), L["lin2"], ops.EPI_Q8_RES, scale[p + "mlp.qact1"],
                                        scale[p + "qact9"], mid=scale[p + "mlp.qact2"], res=codes(p + "qact7"),
                                        res_scale=scale[p + "qact7"]), p + "qact9")
        ln(L["norms"][2], p + "qact9", p + "qact10")
        check(p + "qact11", ops.add_q8(codes(p + "qact10"), scale[p + "qact10"], T, s_T, scale[p + "qact11"]),
              p + "qact11")
        check(p + "qact12", ops.add_q8(codes(k_in), scale[k_in], P, s_P, scale[p + "qact12"]), p + "qact12")
        attention(p + "cross_attn_image_to_token.", L["i2t"], p + "qact12", p + "qact11", p + "qact10")
        out_proj(p + "cross_attn_image_to_token.", L["i2t"], k_in, p + "qact13")
        ln(L["norms"][3], p + "qact13", p + "qact14")
        q_in, k_in = p + "qact10", p + "qact14"
    p = "transformer."
    check(p + "qact1", ops.add_q8(codes(q_in), scale[q_in], T, s_T, scale[p + "qact1"]), p + "qact1")
    check(p + "qact2", ops.add_q8(codes(k_in), scale[k_in], P, s_P, scale[p + "qact2"]), p + "qact2")
    attention(p + "final_attn_token_to_image.", eng.final, p + "qact1", p + "qact2", k_in)
    out_proj(p + "final_attn_token_to_image.", eng.final, q_in, p + "qact3")
    ln(eng.norm_final, p + "qact3", p + "qact4")


def _cos(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def _iou(a, b):
    a, b = np.asarray(a) > 0, np.asarray(b) > 0
    u = (a | b).sum()
    return 1.0 if u == 0 else float((a & b).sum() / u)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.PROMPT_SHAPES)
def test_fq_decoder_engine_vs_golden(cuda, golden_dir, shape):
    """End to end on the 16 x 16 grid: the engine's final queries / keys and the low-res mask codes
    against the golden -- mean |dcode| <= 1.25 x (the fp64 restatement's own distance to the golden,
    computed here) + 0.05 and cosine >= 0.995; thresholded masks' IoU with the golden's >= the
    restatement's - 0.01; iou_pred within the restatement's own error + 1e-3."""
    g, _ = _golden(golden_dir)
    ts = _tap_scales(g)
    gold = {n: _golden_tap(g, shape, n).astype(np.float64) for n in ("queries", "layers.1.keys", "qact1")}
    # fp64 restatement from the golden's input codes: the transformer restated, the heads as the module in fp64
    cpu = _calibrated_cpu()
    md64 = copy.deepcopy(cpu.mask_decoder).double()
    f64 = lambda n: torch.from_numpy(_golden_tap(g, shape, n).astype(np.float64)) * ts[n]
    with torch.no_grad():
        q64, k64 = R.transformer_ref(cpu.mask_decoder.state_dict(), f64("qact_embed1"), _rows(f64("qact_embed2")),
                                     _rows(f64("pos_src_qact")), dtype=torch.float64)
        m64, iou64 = md64.heads_forward(q64, k64, (1, 256, R.GRID, R.GRID))
    rest = {"queries": q64.numpy() / ts["queries"], "layers.1.keys": k64.numpy() / ts["layers.1.keys"],
            "qact1": m64.numpy() / ts["qact1"]}
    # the engine
    sam = _gpu_model(cuda)
    eng = sam.mask_decoder.engine()
    n0 = eng.forwards
    taps = {}
    with torch.no_grad():
        masks, iou = sam.mask_decoder.predict_masks(*_prompt_inputs(sam, R.TEST_SEED, shape, cuda), taps=taps)
    assert eng.forwards == n0 + 1
    ours = {"queries": taps["queries"].cpu().numpy() / ts["queries"],
            "layers.1.keys": taps["keys"].cpu().numpy() / ts["layers.1.keys"],
            "qact1": masks.cpu().numpy() / ts["qact1"]}
    for n in gold:
        d_ref = float(np.abs(np.round(rest[n]) - gold[n]).mean())
        d = float(np.abs(np.round(ours[n]) - gold[n]).mean())
        cos = _cos(ours[n], gold[n])
        print(f"[fq decoder e2e {shape}] {n}: mean |dcode| {d:.4f} (fp64 restatement {d_ref:.4f}), cosine {cos:.5f}")
        assert d <= 1.25 * d_ref + 0.05, (n, d, d_ref)
        assert cos >= 0.995, (n, cos)
    iou_m, iou_r = _iou(ours["qact1"], gold["qact1"]), _iou(rest["qact1"], gold["qact1"])
    e_iou = float(np.abs(iou.cpu().numpy() - g[f"iou_pred:{shape}"]).max())
    e_ref = float(np.abs(iou64.numpy() - g[f"iou_pred:{shape}"]).max())
    print(f"[fq decoder e2e {shape}] mask IoU {iou_m:.4f} (restatement {iou_r:.4f}); iou_pred err {e_iou:.2e} "
          f"(restatement {e_ref:.2e})")
    assert iou_m >= iou_r - 0.01
    assert e_iou <= e_ref + 1e-3


def _raw_tokens(md, sparse):
    """The transformer's token input before ``qact_embed1``, as ``predict_masks`` builds it."""
    out = torch.cat([md.iou_token.weight, md.mask_tokens.weight], dim=0)
    return torch.cat((out.unsqueeze(0).expand(sparse.size(0), -1, -1), sparse), dim=1)


@pytest.mark.gpu
def test_fq_decoder_engine_capture_and_image_cache(cuda):
    """The engine's graph replay equals its eager forward bit for bit (``queries`` and ``keys``) for both
    token counts; a second forward with other prompts on the same image reuses the cached src / pos
    codes; a new image of the same grid keeps the graphs.  The comparison is on the engine's own
    outputs: the module-graph tail behind it is torch's (its transposed convolutions are not promised
    to be run-to-run bit-identical) and not part of the graph."""
    sam = _gpu_model(cuda)
    md = sam.mask_decoder
    eng = md.engine()
    eng.drop_graphs()

    def run(emb, pe, sparse, dense):
        q, k = eng.forward(emb, dense, pe, _raw_tokens(md, sparse))
        return q.clone(), k.clone()
    with torch.no_grad():
        ins = {s: _prompt_inputs(sam, R.TEST_SEED, s, cuda) for s in R.PROMPT_SHAPES}
        other = _prompt_inputs(sam, R.CALIB_SEEDS[0], "point", cuda)
        emb = ins["point"][0]
        eager = {s: run(emb, pe, sparse, dense) for s, (_, pe, sparse, dense) in ins.items()}
        again = {s: run(emb, pe, sparse, dense) for s, (_, pe, sparse, dense) in ins.items()}
        for s in ins:   # the eager engine is deterministic
            assert torch.equal(eager[s][0], again[s][0]) and torch.equal(eager[s][1], again[s][1]), s
        nq = eng.image_quantisations
        # other prompts, same image tensors: no new image-side quantisation
        q2, _ = run(emb, other[1], other[2], other[3])
        assert eng.image_quantisations == nq
        assert not torch.equal(q2, eager["point"][0])
        m_eager = md.predict_masks(emb, *ins["point"][1:])[0].clone()
        for s, (_, pe, sparse, dense) in ins.items():
            eng.capture(5 + sparse.shape[1])
        assert len(eng._graphs) == 2
        n0 = eng.forwards
        for s, (_, pe, sparse, dense) in ins.items():
            q, k = run(emb, pe, sparse, dense)
            assert torch.equal(q, eager[s][0]), s
            assert torch.equal(k, eager[s][1]), s
        m_replay = md.predict_masks(emb, *ins["point"][1:])[0]
        print(f"[fq decoder] masks behind the replayed graph equal the eager ones bit for bit: "
              f"{torch.equal(m_replay, m_eager)}")
        assert _cos(m_replay.cpu().numpy(), m_eager.cpu().numpy()) >= 0.995
        assert eng.forwards == n0 + 3 and eng.image_quantisations == nq
        # a new image of the same geometry keeps the graphs and matches its own eager run
        emb2 = torch.from_numpy(R.image_embedding(R.CALIB_SEEDS[1])).to(cuda)
        _, pe, sparse, dense = ins["point"]
        q_graph, k_graph = run(emb2, pe, sparse, dense)
        assert eng.image_quantisations == nq + 1 and len(eng._graphs) == 2
        eng.drop_graphs()
        q_eager, k_eager = run(emb2, pe, sparse, dense)
        assert torch.equal(q_graph, q_eager) and torch.equal(k_graph, k_eager)
        assert not torch.equal(k_eager, eager["point"][1])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fq_decoder_engine_matches_module_graph_on_gpu(cuda):
    """``use_engine = False`` runs the module graph on the GPU (the engine's counter stands still): the
    same low-res masks by the end-to-end test's cosine criterion."""
    sam = _gpu_model(cuda)
    md = sam.mask_decoder
    with torch.no_grad():
        args = _prompt_inputs(sam, R.TEST_SEED, "point", cuda)
        m_eng, _ = md.predict_masks(*args)
        n0 = md.engine().forwards
        md.use_engine = False
        try:
            m_mod, _ = md.predict_masks(*args)
        finally:
            md.use_engine = True
        assert md.engine().forwards == n0
    s = float(md.qact1.quantizer.scale)
    d = (m_eng - m_mod).abs().cpu().numpy() / s
    print(f"[fq decoder] engine vs GPU module graph: mean |dcode| {d.mean():.4f}")
    assert _cos(m_eng.cpu().numpy(), m_mod.cpu().numpy()) >= 0.995


@pytest.mark.gpu
def test_sam_predictor_on_fq_sam_uses_decoder_engine(cuda):
    """``SamPredictor(build_fq_sam(...)).predict`` with one click: masks of the right shape, through the
    decoder engine (its forward counter moves)."""
    from samq import fq_vit
    from samq.sam_decoder import SamPredictor
    sam = _gpu_model(cuda)
    enc = sam.image_encoder
    if "enc_ready" not in _CACHE:
        torch.manual_seed(3)
        with torch.no_grad():
            for p in enc.parameters():
                if p.dim() > 1:
                    p.copy_(torch.randn_like(p) * 0.05)
        img = torch.randn(1, 3, R.IMG, R.IMG, device=cuda)
        enc.model_dequant()          # Sam.model_quant switched the (uncalibrated) encoder too
        enc.calibrate_with([img, img * 0.5])
        _CACHE["enc_ready"] = True
    assert enc.is_quant() and sam.mask_decoder.is_quant()
    pred = SamPredictor(sam)
    rng = np.random.Generator(np.random.PCG64(1))
    image = rng.integers(0, 256, (200, R.IMG, 3), dtype=np.uint8)
    pred.set_image(image)
    eng = sam.mask_decoder.engine()
    n0 = eng.forwards
    masks, iou, low = pred.predict(point_coords=np.array([[100.0, 80.0]]), point_labels=np.array([1]))
    assert eng.forwards == n0 + 1
    assert masks.shape == (3, 200, R.IMG) and masks.dtype == bool
    assert iou.shape == (3,) and low.shape == (3, 4 * R.GRID, 4 * R.GRID) and np.isfinite(low).all()
    masks2, _, _ = pred.predict(point_coords=np.array([[30.0, 150.0]]), point_labels=np.array([1]))
    assert eng.forwards == n0 + 2 and masks2.shape == masks.shape
