"""W8A8 (fq_vit) int8 attention at head dim 80 and the fused engine on SAM ViT-H.

Kernel tests mirror test_w8a8.py at d = 80 (same recipes, same bounds): random inputs against the
fp32 reference (all codes within +-1, <= 5e-3 off by one; the reference's own fp32-vs-fp64 distance
on these inputs is <= 1.6e-5), exact ties against the fp64 reference (+-1, <= 1e-4), the zero k-slots
of the tail MFMA, the refusals.  Engine tests run a depth-2 ViT-H (block 1 global) against the
reference's golden (fq_vith_d2_img256.npz, tests/golden/make_golden_fq_vith.py).
"""
import functools
import json

import numpy as np
import pytest
import torch

import _attn_q8_ref as A
from oracle import fq_ref, sam_ref, synth

D = 80
SM = D ** -0.5


def _codes_close(out, ref, max_frac, what):
    out = out.astype(np.int64)
    ref = ref.astype(np.int64)
    d = np.abs(out - ref)
    frac = float((d > 0).mean())
    assert d.max() <= 1, f"{what}: code off by {d.max()}"
    assert frac <= max_frac, f"{what}: {frac:.2e} of codes off by one (> {max_frac:.1e})"
    return frac


# ----------------------------------------------------------------------------- CPU: the helper
@pytest.mark.parametrize("b,hw,window", [(1, 20, 14), (1, 16, 0)])
def test_attn_ref_helper_equals_test_w8a8_at_d64(b, hw, window):
    """_attn_q8_ref.attn_ref with sm_scale = 64^-0.5 is test_w8a8._attn_ref bit for bit (output codes and
    second-quantiser codes), on the random and the exact-tie inputs."""
    import test_w8a8 as W
    heads = 2
    qkv, bias, relh, relw = W._q8_inputs(b, hw, hw, heads, window, hw + window)
    mine = A.q8_inputs(b, hw, hw, heads, window, hw + window, 64)
    assert all(np.array_equal(x, y) for x, y in zip(mine, (qkv, bias, relh, relw)))
    c_old, c_new = [], []
    old = W._attn_ref(qkv, bias, relh, relw, heads, window, *W._Q8_SCALES, codes2=c_old)
    new = A.attn_ref(qkv, bias, relh, relw, heads, window, 64 ** -0.5, *A.Q8_SCALES, codes2=c_new)
    np.testing.assert_array_equal(new, old)
    assert all(torch.equal(x, y) for x, y in zip(c_old, c_new))
    ex_old = W._exact_attn_inputs(b, hw, hw, heads, window, "fine", seed=3)
    ex_new = A.exact_attn_inputs(b, hw, hw, heads, window, "fine", seed=3, d=64)
    assert all(np.array_equal(x, y) for x, y in zip(ex_old[:4], ex_new[:4])) and ex_old[4] == ex_new[4]
    old = W._attn_ref(*ex_old[:4], heads, window, *ex_old[4], dtype=torch.float64)
    new = A.attn_ref(*ex_new[:4], heads, window, A.EXACT_SM_SCALE, *ex_new[4], dtype=torch.float64)
    np.testing.assert_array_equal(new, old)


# ----------------------------------------------------------------------------- CPU: ViT-H module mirror
GLOBAL = (1,)


def _golden_vith(golden_dir):
    g = np.load(golden_dir / "fq_vith_d2_img256.npz", allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    cfg = synth.encoder_config("vit_h", depth=meta["depth"], global_attn_indexes=meta["global_attn_indexes"],
                               img_size=meta["img_size"])
    st = {k: v.astype(np.float16).astype(np.float32) for k, v in synth.make_encoder_state(cfg, seed=meta["seed"]).items()}
    return g, meta, cfg, st


def _product_fq_vith(cfg, st, device="cpu"):
    from samq import fq_vit
    enc = fq_vit.build_fq_image_encoder("vit_h", img_size=cfg["img_size"], depth=cfg["depth"],
                                        global_attn_indexes=cfg["global_attn_indexes"])
    missing, unexpected = enc.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    assert not unexpected, unexpected
    assert all("quantizer" in k for k in missing), missing
    return enc.to(device).eval()


def test_fq_vith_module_calibration_matches_reference_scales(golden_dir):
    """build_fq_image_encoder("vit_h", depth=2, global_attn_indexes=(1,)) loads the synthetic ViT-H state
    (block 1's rel-pos tables are the global 2 * 16 - 1 rows) and, after CPU calibration, reproduces the
    reference's 30 activation scales, every per-channel weight scale and the output codes bit for bit."""
    g, meta, cfg, st = _golden_vith(golden_dir)
    assert (meta["depth"], tuple(meta["global_attn_indexes"]), meta["img_size"]) == (2, GLOBAL, 256)
    enc = _product_fq_vith(cfg, st)
    assert enc.global_attn_indexes == GLOBAL and enc.blocks[1].attn.rel_pos_h.shape == (31, D)
    enc.calibrate_with([torch.from_numpy(synth.make_images(1, 256, seed=s)) for s in meta["calib_seeds"]])
    names = list(g["act_scale_names"])
    assert len(names) == 30
    from samq import fq_vit
    qa = fq_vit.act_quantizers(enc)
    assert set(qa) == set(names)
    mine = np.array([float(qa[n].quantizer.scale) for n in names], np.float32)
    np.testing.assert_array_equal(mine, g["act_scales"])
    mods = dict(enc.named_modules())
    for k in g.files:
        if k.startswith("wscale:"):
            np.testing.assert_array_equal(mods[k[7:]].quantizer.scale.numpy(), g[k])
    out = enc.module_forward(torch.from_numpy(synth.make_images(1, 256, seed=meta["test_seed"]))).detach().numpy()
    np.testing.assert_array_equal(np.round(out / g["out_scale"]), g["codes"].astype(np.float64))


def test_fq_builder_default_global_indexes_unchanged():
    """global_attn_indexes=None keeps the named model's indexes (a depth-2 ViT-H has no global block)."""
    from samq import fq_vit
    enc = fq_vit.build_fq_image_encoder("vit_h", img_size=64, depth=2)
    assert enc.global_attn_indexes == (7, 15, 23, 31)
    assert all(b.attn.rel_pos_h.shape == (27, D) for b in enc.blocks)


# ----------------------------------------------------------------------------- CPU: exact inputs at d = 80
@pytest.mark.parametrize("variant", ["fine", "saturating", "peaked", "needle"])
@pytest.mark.parametrize("b,hw,window", [(1, 20, 14), (1, 16, 0), (1, 20, 0)])
def test_exact_attn_inputs_d80_pin_the_quantisers(b, hw, window, variant):
    """test_w8a8.test_exact_attn_inputs_pin_the_quantisers at d = 80 with sm_scale = 2^-3: fp32 and fp64
    evaluations of the reference give identical second-quantiser codes and output codes differing in at
    most 1e-4 of the positions, both clamp ends are hit, and a reference with round-half-away at
    either score quantiser or with the low clamp at -127 differs in > 1e-3 of the output codes
    (> 1e-4 for the known weak case: half-away at quantiser 1 on "saturating").  "peaked" / "needle": the
    fp32-vs-fp64 condition, the lazy offset moves after the first key row, the wrong-quantiser shares
    printed only (as in test_w8a8)."""
    import test_w8a8 as W
    heads = 2
    qkv, bias, relh, relw, scales = A.exact_attn_inputs(b, hw, hw, heads, window, variant, seed=2 * hw + window, d=D)
    ref = functools.partial(A.attn_ref, qkv, bias, relh, relw, heads, window, A.EXACT_SM_SCALE, *scales)
    c32, c64 = [], []
    ref32 = ref(codes2=c32)
    ref64 = ref(dtype=torch.float64, codes2=c64)
    assert all(torch.equal(a, b_) for a, b_ in zip(c32, c64))
    codes = torch.cat([t.reshape(-1) for t in c64])
    hi, lo = float((codes == 127).double().mean()), float((codes == -128).double().mean())
    own = float((ref32 != ref64).mean())
    print(f"\n[exact d80 {variant} {b}x{hw} win {window}] second-quantiser codes at 127: {hi:.3f}, at -128: {lo:.3f}; "
          f"output codes fp32 vs fp64 {own:.2e}")
    assert np.abs(ref32 - ref64).max() <= 1 and own <= 1e-4
    if variant not in A.PEAKED_VARIANTS:
        assert hi > 0 and lo > 0
    else:
        lazyc = A.lazy_codes(scales[2])
        moves = A.offset_moves_after_row0(c64, window or hw, lazyc)
        print(f"    lazyc {lazyc}, second-quantiser codes {int(codes.min())}..{int(codes.max())}, "
              f"offset moves after the first key row: {moves}")
        assert lazyc == A.PEAKED_LAZYC[variant] and moves > 0
    for what, kw in [("half-away at quantiser 1", dict(fq1=W._fq_half_away)),
                     ("half-away at quantiser 2", dict(fq2=W._fq_half_away)),
                     ("low clamp -127", dict(fq1=W._fq_low127, fq2=W._fq_low127))]:
        wrong = ref(dtype=torch.float64, **kw)
        frac = float((wrong != ref64).mean())
        print(f"    {what}: {frac:.2e} of the output codes change")
        weak = variant == "saturating" and what == "half-away at quantiser 1"
        if variant not in A.PEAKED_VARIANTS:
            assert frac > (1e-4 if weak else 1e-3), what


# ----------------------------------------------------------------------------- zero k-slots of the tail MFMA
def _tail_inputs(b, hw, heads, window, tail_on, seed):
    """q and k codes 127 on dims 64..79 and 0 on dims 0..63 (``tail_on``) or the reverse; V, tables and
    bias random.  Every in-image q.k is then one constant, 16 (or 64) * 127^2: s_a1 puts its code at
    64 (100), s_a2 = s_a1 shifts the second quantiser's argument up by that many codes, so that 6 %
    (19 %) of the scores clamp at 127 -- a tail that is dropped (shift 0) or counted twice (shift 127)
    changes which scores clamp, which softmax, invariant to a shift otherwise, does show."""
    qkv, bias, relh, relw = A.q8_inputs(b, hw, hw, heads, window, seed, D)
    qk = qkv.reshape(b, hw, hw, 3, heads, D)
    qk[..., :2, :, :64] = 0 if tail_on else 127
    qk[..., :2, :, 64:] = 127 if tail_on else 0
    s1 = np.float32(0.18 if tail_on else 0.46)
    return qkv, bias, relh, relw, (np.float32(0.02), s1, s1, np.float32(2.6 / 127.5))


@pytest.mark.parametrize("tail_on", [True, False])
def test_tail_inputs_show_a_dropped_or_doubled_tail(tail_on):
    """CPU: on _tail_inputs a reference whose dims 64..79 are dropped from q.k, or counted twice, differs
    from the correct one in more than 1e-2 of the output codes (the GPU test's bound is 5e-3)."""
    heads, hw, window = 2, 16, 0
    qkv, bias, relh, relw, scales = _tail_inputs(1, hw, heads, window, tail_on, 5)
    ref = A.attn_ref(qkv, bias, relh, relw, heads, window, SM, *scales)
    q2 = qkv.reshape(1, hw, hw, 3, heads, D).copy()
    if tail_on:
        # dropped: q.k = 0; doubled: q.k twice the constant (the first quantiser clamps it at 127)
        q2[..., 1, :, :] = 0
        wrongs = {"dropped": (q2, SM), "doubled": (qkv, 2 * SM)}
    else:
        # a tail that is not zero: the k-slots past dim 63 pick up some other 127s
        q2[..., :2, :, 64:] = 127
        wrongs = {"garbage": (q2, SM)}
    for what, (q2, sm) in wrongs.items():
        # only q.k is wrong: the rel-pos terms and V come from the true codes
        wrong = _ref_with_qk_from(q2.reshape(qkv.shape), qkv, bias, relh, relw, heads, window, sm, scales)
        frac = float((wrong != ref).mean())
        print(f"\n[tail {'on' if tail_on else 'off'}] {what}: {frac:.2e} of the output codes change")
        assert frac > 1e-2, what


def _ref_with_qk_from(qkv_qk, qkv, bias, relh, relw, heads, window, sm, scales):
    """attn_ref whose first score quantiser sees q.k of ``qkv_qk`` while everything else (rel-pos, V) comes
    from ``qkv``: fq1 is replaced by one that ignores its argument's values and recomputes them."""
    c = heads * D
    t = torch.from_numpy(qkv_qk.astype(np.float32)) * torch.tensor(float(scales[0]))
    b, h, w, _ = qkv.shape
    tt = t.reshape(b, h * w, 3, heads, D).permute(2, 0, 3, 1, 4).reshape(3, b * heads, h * w, D)
    sc_all = (tt[0] * sm) @ tt[1].transpose(-2, -1)
    assert window == 0 and sc_all.shape[0] <= max(1, (1 << 24) // (h * w) ** 2)   # one step of attn_ref's loop

    def fq1(sc, s):
        return fq_ref.fake_quant(sc_all.to(sc.dtype), s)

    return A.attn_ref(qkv, bias, relh, relw, heads, window, sm, *scales, fq1=fq1)


# ----------------------------------------------------------------------------- GPU: kernels at d = 80
_RANDOM_CASES = {
    # name: (b, h, w, heads, window, with_bias)
    "win14_padded": (1, 20, 20, 3, 14, True),        # rel_attention_q8_win_kernel<80, 14, 7>, windows padded on both sides
    "win14_nonsquare_nobias": (1, 20, 33, 3, 14, False),
    "win14_unpadded": (2, 14, 14, 3, 14, True),
    "resident13": (1, 20, 20, 3, 8, True),           # resident kernel, 13 waves
    "resident16": (1, 20, 20, 3, 16, True),          # resident kernel, 16 waves
    "stream10": (1, 10, 10, 3, 0, True),             # streaming kernel, ragged last chunk and query tile
    "stream17": (1, 17, 17, 3, 0, True),
    "stream32": (1, 32, 32, 3, 0, True),             # full chunks
    "row64": (1, 64, 64, 2, 0, True),                # row64 kernel, int8 V
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_RANDOM_CASES))
def test_rel_attention_q8_d80(cuda, case):
    """Random inputs (recipe and bound of test_rel_attention_q8, sm_scale = 80^-0.5) against the fp32
    reference, one case per launch branch.  Measured on gfx950: at most 1.7e-5 of the codes off by one
    (row64), 0 on five of the nine cases."""
    b, h, w, heads, window, with_bias = _RANDOM_CASES[case]
    qkv, bias, relh, relw = A.q8_inputs(b, h, w, heads, window, h + w + window, D)
    if not with_bias:
        bias = None
    ref = A.attn_ref(qkv, bias, relh, relw, heads, window, SM, *A.Q8_SCALES)
    out = A.q8_launch(cuda, qkv, bias, relh, relw, heads, window, SM, A.Q8_SCALES)
    frac = _codes_close(out.cpu().numpy(), ref, 5e-3, f"attention_q8 d80 {case}")
    print(f"\n[d80 {case}] codes off by one {frac:.2e}")


@pytest.mark.gpu
def test_rel_attention_q8_d80_row64_batch_v16_rows(cuda):
    """The 64 x 64 global kernel at d = 80, two images, one head: against the reference; V staged from an
    fp16 copy of its codes and the row ranges (0, 28) + (28, 36), both bit-identical to the full int8-V
    launch."""
    b, heads, hw = 2, 1, 64
    qkv, bias, relh, relw = A.q8_inputs(b, hw, hw, heads, 0, 64 + 10 * b + heads, D)
    ref = A.attn_ref(qkv, bias, relh, relw, heads, 0, SM, *A.Q8_SCALES)
    dq, dh, dw = (torch.from_numpy(a).to(cuda) for a in (qkv, relh, relw))
    full = A.q8_launch(cuda, dq, None, dh, dw, heads, 0, SM, A.Q8_SCALES)
    frac = _codes_close(full.cpu().numpy(), ref, 5e-3, "attention_q8 d80 row64 B 2")
    print(f"\n[d80 row64 B 2] codes off by one {frac:.2e}")
    v16 = dq[..., 2 * heads * D:].to(torch.float16).contiguous()
    o16 = A.q8_launch(cuda, dq, None, dh, dw, heads, 0, SM, A.Q8_SCALES, v16=v16)
    torch.cuda.synchronize()
    assert torch.equal(o16, full)
    out = torch.zeros_like(full)
    for r0, n in ((0, 28), (28, 36)):
        A.q8_launch(cuda, dq, None, dh, dw, heads, 0, SM, A.Q8_SCALES, out=out, rows=(r0, n))
    torch.cuda.synchronize()
    assert torch.equal(out, full)


_EXACT_GEOMETRIES = {
    "win14": (2, 20, 33, 2, 14),
    "win8": (1, 20, 20, 2, 8),
    "win16": (1, 20, 20, 2, 16),
    "glob20": (1, 20, 20, 2, 0),
    "glob32": (1, 32, 32, 2, 0),
    "glob64": (1, 64, 64, 2, 0),      # int8 V and fp16 V
}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fine", "saturating", "peaked", "needle"])
@pytest.mark.parametrize("geom", list(_EXACT_GEOMETRIES))
def test_rel_attention_q8_d80_exact_ties(cuda, geom, variant):
    """test_rel_attention_q8_exact_ties at d = 80: on the exact inputs every output code is within +-1 of
    the float64 reference and at most 1e-4 of them differ
    (test_exact_attn_inputs_d80_pin_the_quantisers: what that bound can see).
    Measured on gfx950 (share of differing codes, all within +-1): glob64 fine 1.83e-5 (int8 and fp16 V
    alike), glob20 fine 1.56e-5, glob32 fine 1.22e-5, glob64 saturating 1.5e-6, every other case 0.
    "peaked" / "needle" (lazyc = 11 / 2): peaked 0 to 6.1e-6, glob64 3.51e-5; needle 0 to 3.13e-5 (win16)."""
    b, h, w, heads, window = _EXACT_GEOMETRIES[geom]
    qkv, bias, relh, relw, scales = A.exact_attn_inputs(b, h, w, heads, window, variant, seed=h + w + window, d=D)
    ref = A.attn_ref(qkv, bias, relh, relw, heads, window, A.EXACT_SM_SCALE, *scales, dtype=torch.float64)
    dq = torch.from_numpy(qkv).to(cuda)
    launches = [("int8 V", {})]
    if geom == "glob64":
        launches.append(("fp16 V", dict(v16=dq[..., 2 * heads * D:].to(torch.float16).contiguous())))
    for what, kw in launches:
        out = A.q8_launch(cuda, dq, bias, relh, relw, heads, window, A.EXACT_SM_SCALE, scales, **kw).cpu().numpy()
        d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
        print(f"\n[exact ties d80 {geom} {variant} {what}] codes differing {float((d > 0).mean()):.2e}, max |dcode| {d.max()}")
        _codes_close(out, ref, 1e-4, f"attention_q8 d80 exact {geom} {variant} {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("tail_on", [True, False])
@pytest.mark.parametrize("kernel,b,hw,heads,window", [("win14", 1, 20, 3, 14), ("resident", 1, 20, 3, 8),
                                                     ("stream", 1, 17, 3, 0), ("row64", 1, 64, 1, 0)])
def test_rel_attention_q8_d80_tail_slots(cuda, kernel, b, hw, heads, window, tail_on):
    """Dims 64..79 enter q.k once, and the zero k-slots of their MFMA add nothing: q, k codes 127 on dims
    64..79 and 0 elsewhere, and the reverse (_tail_inputs), against the reference, bound of the random
    test.  For row64 also with fp16 V."""
    qkv, bias, relh, relw, scales = _tail_inputs(b, hw, heads, window, tail_on, hw + window)
    ref = A.attn_ref(qkv, bias, relh, relw, heads, window, SM, *scales)
    dq = torch.from_numpy(qkv).to(cuda)
    launches = [{}] + ([dict(v16=dq[..., 2 * heads * D:].to(torch.float16).contiguous())] if kernel == "row64" else [])
    for kw in launches:
        out = A.q8_launch(cuda, dq, bias, relh, relw, heads, window, SM, scales, **kw)
        frac = _codes_close(out.cpu().numpy(), ref, 5e-3, f"attention_q8 d80 tail {kernel} on={tail_on} {sorted(kw)}")
        print(f"\n[d80 tail {kernel} on={tail_on} {sorted(kw)}] codes off by one {frac:.2e}")


@pytest.mark.gpu
def test_rel_attention_q8_d80_refusals(cuda):
    """Head dims other than 64 and 80 are refused, and so is every geometry refused at 64."""
    from samq import ops

    def run(b, h, w, heads, d, window, **kw):
        c = heads * d
        side = window or h
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)
        qkv = torch.zeros((b, h, w, 3 * c), dtype=torch.int8, device=cuda)
        return ops.rel_attention_q8(qkv, z(3 * c), z(2 * side - 1, d), z(2 * side - 1, d), heads, window, d ** -0.5,
                                    0.02, 0.02, 0.05, 0.02, **kw)
    run(1, 32, 32, 1, D, 0)                          # the whole H = 32 grid is served at d = 80
    for args, kw in [((1, 16, 16, 2, 32, 0), {}),                    # head dim 32
                     ((1, 16, 16, 2, 72, 0), {}),                    # head dim 72
                     ((1, 16, 16, 2, 96, 0), {}),                    # head dim 96
                     ((1, 20, 20, 1, D, 17), {}),                    # window 17
                     ((1, 65, 65, 1, D, 0), {}),                     # H = 65
                     ((1, 32, 32, 1, D, 0), dict(rows=(0, 16)))]:    # partial global row range off the 64 x 64 grid
        with pytest.raises(NotImplementedError):
            run(*args, **kw)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- GPU: the engine on ViT-H
def _gpu_fq_vith(cfg, st, g, device):
    from samq import fq_vit
    enc = _product_fq_vith(cfg, st, device)
    fq_vit.calibrate_weights(enc)
    fq_vit.set_act_scales(enc, dict(zip(g["act_scale_names"], g["act_scales"])))
    enc.model_quant()
    return enc


@pytest.mark.gpu
def test_w8a8_vith_stage_local_parity(cuda, golden_dir):
    """test_w8a8_stage_local_parity on the depth-2 ViT-H: each fused stage, fed the CPU module graph's own
    int8 inputs, reproduces its output codes (all within +-1, <= 1e-4 off by one) -- LN-q at C = 1280,
    the W8 GEMMs at K = 1280 / 5120 and N = 1280 / 3840 / 5120, the 14-window attention (block 0) and
    the streaming global attention on the 16 x 16 grid (block 1) at head dim 80."""
    from samq import fq_vit, ops
    g, meta, cfg, st = _golden_vith(golden_dir)
    img_t = torch.from_numpy(synth.make_images(1, 256, seed=meta["test_seed"]))
    cpu = _gpu_fq_vith(cfg, st, g, "cpu")
    ref = {}
    for n, m in fq_vit.act_quantizers(cpu).items():
        m.register_forward_hook(lambda mod, inp, out, n=n: ref.__setitem__(n, out.detach()))
    cpu.module_forward(img_t)
    scales = dict(zip(g["act_scale_names"], g["act_scales"]))
    eng = _gpu_fq_vith(cfg, st, g, cuda).engine()
    c, gsz = cfg["embed_dim"], 256 // 16
    assert c == 1280

    def codes(n, shape=None):
        t = torch.round(ref[n] / float(scales[n])).to(torch.int8)
        return (t if shape is None else t.reshape(shape)).to(cuda).contiguous()

    def check(what, out, n, natural=None):
        r = ref[n] if natural is None else natural
        rc = np.round(r.numpy() / scales[n]).reshape(-1)
        frac = _codes_close(out.cpu().numpy().reshape(-1), rc, 1e-4, what)
        print(f"[vit_h stage] {what}: {frac:.2e} off by one")

    windows = []
    for i in range(cfg["depth"]):
        bl, pre = eng.blocks[i], f"blocks.{i}."
        xin_n = "qact1" if i == 0 else f"blocks.{i - 1}.qact4"
        s_in = float(scales[xin_n])
        check(pre + "LN1", ops.layernorm_q(codes(xin_n, (-1, c)), *bl["n1"], in_scale=s_in, out_scale=bl["s_ln1"]),
              pre + "qact1")
        win = bl["window"]
        windows.append(win)
        assert bl["heads"] == 16
        qkv_ref = ref[pre + "attn.qact1"]
        ao_ref = ref[pre + "attn.qact2"]
        if win:
            hp = -(-gsz // win) * win
            qkv_ref = sam_ref.window_unpartition(qkv_ref.reshape(-1, win, win, 3 * c), win, (hp, hp), (gsz, gsz))
            ao_ref = sam_ref.window_unpartition(ao_ref, win, (hp, hp), (gsz, gsz))
        else:
            qkv_ref = qkv_ref.reshape(1, gsz, gsz, 3 * c)
        qkv = eng._gemm(codes(pre + "qact1", (-1, c)), bl["qkv"], ops.EPI_Q8, bl["s_ln1"], bl["s_qkv"])
        check(pre + "qkv", qkv, pre + "attn.qact1", qkv_ref)
        qc = torch.round(qkv_ref / float(scales[pre + "attn.qact1"])).to(torch.int8).to(cuda).contiguous()
        ao = ops.rel_attention_q8(qc, bl["qkv_bias"], bl["relh"], bl["relw"], bl["heads"], win, bl["scale"],
                                  bl["s_qkv"], bl["s_a1"], bl["s_a2"], bl["s_ao"])
        check(pre + f"attention (window {win})", ao, pre + "attn.qact2", ao_ref)
        aoc = torch.round(ao_ref / float(scales[pre + "attn.qact2"])).to(torch.int8).to(cuda).reshape(-1, c)
        x1 = codes(xin_n, (-1, c))
        eng._gemm(aoc.contiguous(), bl["proj"], ops.EPI_Q8_RES, bl["s_ao"], bl["s_x1"], mid=bl["s_proj"], res=x1,
                  res_scale=s_in, out=x1)
        check(pre + "proj+res", x1, pre + "qact2")
        check(pre + "LN2", ops.layernorm_q(codes(pre + "qact2", (-1, c)), *bl["n2"], in_scale=bl["s_x1"],
                                           out_scale=bl["s_ln2"]), pre + "qact3")
        check(pre + "lin1+gelu", eng._gemm(codes(pre + "qact3", (-1, c)), bl["lin1"], ops.EPI_Q8_GELU, bl["s_ln2"],
                                           bl["s_h"]), pre + "mlp.qact1")
        x3 = codes(pre + "qact2", (-1, c))
        eng._gemm(codes(pre + "mlp.qact1", (-1, 4 * c)), bl["lin2"], ops.EPI_Q8_RES, bl["s_h"], bl["s_x2"],
                  mid=bl["s_l2"], res=x3, res_scale=bl["s_x1"], out=x3)
        check(pre + "lin2+res", x3, pre + "qact4")
    assert windows == [14, 0]


@pytest.mark.gpu
def test_w8a8_vith_encoder_vs_golden(cuda, golden_dir):
    """The fused engine on the depth-2 ViT-H at img 256 with the reference's calibrated scales against the
    reference's output codes; tolerance in the form of test_w8a8_encoder_vs_golden, measured on the
    reference: mean |dcode| <= 1.25 x (the fp64 oracle's own distance to the golden, computed here)
    + 0.05, cosine >= 0.995, max-abs <= 0.15 x absmax."""
    g, meta, cfg, st = _golden_vith(golden_dir)
    enc = _gpu_fq_vith(cfg, st, g, cuda)
    img_np = synth.make_images(1, 256, seed=meta["test_seed"])
    out = enc(torch.from_numpy(img_np).to(cuda)).float().cpu().numpy()
    s_out = float(g["out_scale"])
    codes = np.round(out / s_out)
    np.testing.assert_allclose(codes * s_out, out, rtol=0, atol=1e-5 * max(1.0, np.abs(out).max()))
    ref = g["codes"].astype(np.float64)
    o64 = fq_ref.FQEncoderOracle(cfg, st, dtype=torch.float64)
    o64.set_scales(dict(zip(g["act_scale_names"], g["act_scales"])))
    c64 = np.round(o64(img_np).numpy() / s_out)

    def stats(a, b):
        d = np.abs(a - b)
        cos = float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
        return float((d == 0).mean()), float(d.mean()), float(d.max()), cos

    ours, self_ = stats(codes, ref), stats(c64, ref)
    print(f"\nW8A8 vit_h depth 2, 256: ours vs reference: {ours[0] * 100:.2f}% codes equal, mean |dcode| {ours[1]:.3f}, "
          f"max {ours[2]:.0f}, cos {ours[3]:.5f} | reference fp64 vs fp32: {self_[0] * 100:.2f}% equal, "
          f"mean {self_[1]:.3f}, max {self_[2]:.0f}, cos {self_[3]:.5f} | ours vs fp64: mean {stats(codes, c64)[1]:.3f}")
    assert ours[1] <= 1.25 * self_[1] + 0.05
    assert ours[3] >= 0.995
    assert ours[2] * s_out <= 0.15 * np.abs(ref).max() * s_out


@pytest.mark.gpu
def test_w8a8_vith_engine_paths_bit_identical(cuda):
    """random_fq_encoder("vit_h", depth=2, global_attn_indexes=(1,)) at 1024^2 (14-window block, 64 x 64
    global block at head dim 80, C = 1280): the fp16-V path on / off, two row lanes vs one chain, and a
    captured graph replayed once vs eager all give the same codes bit for bit."""
    from samq.synthetic import random_fq_encoder
    enc = random_fq_encoder("vit_h", device=cuda, depth=2, global_attn_indexes=GLOBAL)
    eng = enc.engine()
    assert [b["window"] for b in eng.blocks] == [14, 0] and eng.blocks[1]["heads"] == 16
    img = torch.randn((1, 3, 1024, 1024), generator=torch.Generator(device=cuda).manual_seed(8), device=cuda)
    eng.row_lanes = 1
    eng.v16 = False
    ref = eng(img).clone()
    assert int(ref.float().abs().sum()) > 0
    eng.v16 = True
    assert torch.equal(eng(img), ref)
    eng.row_lanes = 2
    assert eng._row_split(64) == 28
    got = eng(img)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    eng.row_lanes = 1
    graph, gout = eng.capture(img)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout, ref)
