"""The zero-point mode of the fused W8A8 encoder engine (``W8A8Engine(enc, zero_points=True)``):
omse calibrations (non-zero zero points, the reference's goldens of ``golden/fq_observers.npz``) and
the default ``Config``'s uint8 activations on the HIP ``_zp`` kernels.
"""
import copy
import functools
import json

import numpy as np
import pytest
import torch

from oracle import sam_ref, synth

STAGE_MAX_SHARE = 1e-4       # test_w8a8_stage_local_parity's bound


def _codes_close(out, ref, max_frac, what):
    d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
    frac = float((d > 0).mean())
    print(f"  [{what}] codes differing {frac:.2e}, max |dcode| {d.max()}")
    assert d.max() <= 1, f"{what}: code off by {d.max()}"
    assert frac <= max_frac, f"{what}: {frac:.2e} of codes off by one (> {max_frac:.1e})"


@functools.lru_cache(maxsize=None)
def _golden(golden_dir):
    g = np.load(golden_dir / "fq_observers.npz", allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    names = [str(n) for n in np.load(golden_dir / "fq_vitb_img256.npz", allow_pickle=False)["act_scale_names"]]
    cfg = synth.encoder_config("vit_b", img_size=meta["img_size"])
    st = {k: v.astype(np.float16).astype(np.float32) for k, v in synth.make_encoder_state(cfg, seed=meta["seed"]).items()}
    return g, meta, names, cfg, st


def _omse_encoder(golden_dir, device):
    """The golden model with the reference's omse scales and zero points installed, in quant mode."""
    from samq import fq_vit
    g, meta, names, cfg, st = _golden(golden_dir)
    qcfg = fq_vit.Config(False, False, "omse")
    qcfg.BIT_TYPE_A = fq_vit.BIT_TYPE_DICT["int8"]
    enc = fq_vit.build_fq_image_encoder("vit_b", img_size=cfg["img_size"], cfg=qcfg)
    missing, unexpected = enc.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    assert not unexpected and all("quantizer" in k for k in missing)
    enc = enc.to(device).eval()
    fq_vit.calibrate_weights(enc)
    fq_vit.set_act_scales(enc, dict(zip(names, g["mod:omse:scales"])), dict(zip(names, g["mod:omse:zps"])))
    enc.model_quant()
    return enc


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


def _stage_local(enc_gpu, ref, cuda, max_share=STAGE_MAX_SHARE):
    """Every fused stage of the zero-point engine fed the CPU module graph's own codes (``ref``: QAct
    name -> fake-quant output) reproduces the module graph's output codes."""
    from samq import fq_vit, ops
    eng = enc_gpu.engine(zero_points=True)
    quant = {n: fq_vit._sz(m) for n, m in fq_vit.act_quantizers(enc_gpu).items()}   # stored (scale, zp)
    c = eng.embed_dim
    gsz = enc_gpu.img_size // 16

    def to_codes(t, n):
        s, z = quant[n]
        return torch.round(t / s + z)

    def codes(n, shape=None):
        t = to_codes(ref[n], n).to(torch.int8)
        return (t if shape is None else t.reshape(shape)).to(cuda).contiguous()

    def check(what, out, n, natural=None):
        rc = to_codes(ref[n] if natural is None else natural, n).numpy().reshape(-1)
        assert rc.min() >= -128 and rc.max() <= 127
        _codes_close(out.cpu().numpy().reshape(-1), rc, max_share, what)

    for i, bl in enumerate(eng.blocks):
        pre, q = f"blocks.{i}.", bl["q"]
        xin_n = "qact1" if i == 0 else f"blocks.{i - 1}.qact4"
        q_in = quant[xin_n]
        check(pre + "LN1", ops.layernorm_q_zp(codes(xin_n, (-1, c)), *bl["n1"], q_in[0], q["ln1"][0], q_in[1], q["ln1"][1]),
              pre + "qact1")
        win = bl["window"]
        qkv_ref, ao_ref = ref[pre + "attn.qact1"], ref[pre + "attn.qact2"]
        if win:
            hp = -(-gsz // win) * win
            qkv_ref = sam_ref.window_unpartition(qkv_ref.reshape(-1, win, win, 3 * c), win, (hp, hp), (gsz, gsz))
            ao_ref = sam_ref.window_unpartition(ao_ref, win, (hp, hp), (gsz, gsz))
        else:
            qkv_ref = qkv_ref.reshape(1, gsz, gsz, 3 * c)
        qkv = eng._gemm_zp(codes(pre + "qact1", (-1, c)), bl["qkv"], ops.EPI_Q8, q["ln1"], q["qkv"])
        check(pre + "qkv", qkv, pre + "attn.qact1", qkv_ref)
        qc = to_codes(qkv_ref, pre + "attn.qact1").to(torch.int8).to(cuda).contiguous()
        ao = ops.rel_attention_q8_zp(qc, bl["qkv_bias"], bl["relh"], bl["relw"], bl["heads"], win, bl["scale"],
                                     q["qkv"][0], q["a1"][0], q["a2"][0], q["ao"][0], q["qkv"][1], q["a1"][1],
                                     q["a2"][1], q["ao"][1])
        check(pre + f"attention (window {win})", ao, pre + "attn.qact2", ao_ref)
        aoc = to_codes(ao_ref, pre + "attn.qact2").to(torch.int8).to(cuda).reshape(-1, c).contiguous()
        x1 = codes(xin_n, (-1, c))
        eng._gemm_zp(aoc, bl["proj"], ops.EPI_Q8_RES, q["ao"], q["x1"], q_mid=q["proj"], res=x1, q_res=q_in, out=x1)
        check(pre + "proj+res", x1, pre + "qact2")
        check(pre + "LN2", ops.layernorm_q_zp(codes(pre + "qact2", (-1, c)), *bl["n2"], q["x1"][0], q["ln2"][0],
                                              q["x1"][1], q["ln2"][1]), pre + "qact3")
        check(pre + "lin1+gelu", eng._gemm_zp(codes(pre + "qact3", (-1, c)), bl["lin1"], ops.EPI_Q8_GELU, q["ln2"],
                                              q["h"]), pre + "mlp.qact1")
        x3 = codes(pre + "qact2", (-1, c))
        eng._gemm_zp(codes(pre + "mlp.qact1", (-1, 4 * c)), bl["lin2"], ops.EPI_Q8_RES, q["h"], q["x2"], q_mid=q["l2"],
                     res=x3, q_res=q["x1"], out=x3)
        check(pre + "lin2+res", x3, pre + "qact4")


# ============================================================================= CPU
def test_set_act_scales_zero_points_and_engine_cache():
    """set_act_scales installs the optional zero points (default zeros) and drops both engine caches;
    random_fq_encoder takes an activation bit type, int8 by default."""
    from samq import fq_vit, synthetic
    enc = synthetic.random_fq_encoder("vit_b", device="cpu", img_size=64, depth=1, calib_images=1)
    assert enc.cfg.BIT_TYPE_A.name == "int8" and not enc._needs_zero_points()
    qa = fq_vit.act_quantizers(enc)
    scales = {n: float(m.quantizer.scale) for n, m in qa.items()}
    enc._engine, enc._engine_zp, enc._pick_zp = "a", "b", True
    fq_vit.set_act_scales(enc, scales, {n: 3 for n in qa})
    assert enc._engine is None and enc._engine_zp is None and enc._pick_zp is None
    assert all(int(m.quantizer.zero_point) == 3 for m in qa.values()) and enc._needs_zero_points()
    assert fq_vit._sz(qa["qact1"]) == (scales["qact1"], 3)
    fq_vit.set_act_scales(enc, scales)
    assert all(int(m.quantizer.zero_point) == 0 for m in qa.values()) and not enc._needs_zero_points()
    u8 = synthetic.random_fq_encoder("vit_b", device="cpu", img_size=64, depth=1, calib_images=1, act_bit_type="uint8")
    assert u8.cfg.BIT_TYPE_A.name == "uint8" and u8._needs_zero_points()
    s, z = fq_vit._sz(fq_vit.act_quantizers(u8)["qact1"])
    assert -128 <= z <= 127 and z == int(fq_vit.act_quantizers(u8)["qact1"].quantizer.zero_point) - 128


# ============================================================================= GPU
@pytest.mark.gpu
def test_zp_engine_zero_zero_points_is_the_symmetric_engine(cuda, golden_dir):
    """The symmetric golden scales through engine(zero_points=True) give engine()'s output bit for bit."""
    from samq import fq_vit
    g = np.load(golden_dir / "fq_vitb_img256.npz", allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    _, _, _, cfg, _ = _golden(golden_dir)
    st = {k: v.astype(np.float16).astype(np.float32) for k, v in synth.make_encoder_state(cfg, seed=meta["seed"]).items()}
    enc = fq_vit.build_fq_image_encoder("vit_b", img_size=256)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    enc = enc.to(cuda).eval()
    fq_vit.calibrate_weights(enc)
    fq_vit.set_act_scales(enc, dict(zip(g["act_scale_names"], g["act_scales"])))
    enc.model_quant()
    img = torch.from_numpy(synth.make_images(1, 256, seed=meta["test_seed"])).to(cuda)
    sym = enc.engine()(img)
    zp = enc.engine(zero_points=True)(img)
    assert enc.engine() is not enc.engine(zero_points=True) and enc.engine(zero_points=True).zero_points
    assert torch.equal(zp, sym)
    t0, t1 = {}, {}
    enc.engine().forward(img, taps=t0)
    enc.engine(zero_points=True).forward(img, taps=t1)
    assert t0.keys() == t1.keys() and all(torch.equal(t0[k], t1[k]) for k in t0)


@pytest.mark.gpu
def test_zp_engine_stage_local_parity_omse(cuda, golden_dir):
    """Each fused stage of the zero-point engine, fed the CPU module graph's own codes under the
    reference's omse scales and zero points, reproduces the module graph's output codes: all within
    +-1, at most 1e-4 of them off by one."""
    _, meta, _, cfg, _ = _golden(golden_dir)
    img_t = torch.from_numpy(synth.make_images(1, cfg["img_size"], seed=meta["test_seed"]))
    ref = _module_taps(_omse_encoder(golden_dir, "cpu"), img_t)
    print()
    _stage_local(_omse_encoder(golden_dir, cuda), ref, cuda)


@pytest.mark.gpu
def test_zp_engine_encoder_vs_omse_golden(cuda, golden_dir):
    """enc(img) of an omse-calibrated encoder runs the zero-point engine; its output codes against the
    reference's own (mod:omse:codes) by the criteria of test_w8a8_encoder_vs_golden: mean |dcode| <=
    1.25 x the float64 module graph's distance to the same golden + 0.05, cosine >= 0.995, max-abs <=
    0.15 x absmax.  engine() without arguments still refuses the encoder."""
    g, meta, names, cfg, _ = _golden(golden_dir)
    enc = _omse_encoder(golden_dir, cuda)
    img_np = synth.make_images(1, cfg["img_size"], seed=meta["test_seed"])
    with pytest.raises(NotImplementedError, match="symmetric"):
        enc.engine()
    out = enc(torch.from_numpy(img_np).to(cuda)).float().cpu().numpy()
    assert enc._engine_zp is not None and enc._engine is None
    s_out = float(g["mod:omse:scales"][names.index("qacts.3")])
    z_out = float(g["mod:omse:zps"][names.index("qacts.3")])
    codes = np.round(out / s_out)                      # code - zp, as the golden stores it
    np.testing.assert_allclose(codes * s_out, out, rtol=0, atol=1e-5 * max(1.0, np.abs(out).max()))
    ref = g["mod:omse:codes"].astype(np.float64)
    e64 = _omse_encoder(golden_dir, "cpu").double()
    with torch.no_grad():
        c64 = np.round(e64.module_forward(torch.from_numpy(img_np).double()).numpy() / s_out)

    def stats(a, b):
        d = np.abs(a - b)
        return float((d == 0).mean()), float(d.mean()), float(d.max()), float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))

    ours, self_ = stats(codes, ref), stats(c64, ref)
    print(f"\nW8A8 omse vit_b 256 (zp_out {z_out:.0f}): ours vs reference: {ours[0] * 100:.2f}% codes equal, mean |dcode| "
          f"{ours[1]:.3f}, max {ours[2]:.0f}, cos {ours[3]:.5f} | float64 module graph vs reference: "
          f"{self_[0] * 100:.2f}% equal, mean {self_[1]:.3f}, max {self_[2]:.0f}, cos {self_[3]:.5f}")
    assert ours[1] <= 1.25 * self_[1] + 0.05
    assert ours[3] >= 0.995
    assert ours[2] <= 0.15 * np.abs(ref).max()


@pytest.mark.gpu
def test_zp_engine_uint8_default_config(cuda):
    """Config(False, False, "minmax") with its default uint8 activations on a small encoder (one window
    and one global block, img 64), calibrated on the GPU: enc(img) runs the zero-point engine, its
    stages match the CPU module graph by the stage-local criteria, and one captured HIP graph replayed
    equals the eager forward bit for bit."""
    from samq import synthetic
    enc = synthetic.random_fq_encoder("vit_b", device=cuda, img_size=64, depth=2, calib_images=2,
                                      global_attn_indexes=(1,), act_bit_type="uint8")
    assert enc.cfg.BIT_TYPE_A.name == "uint8"
    with pytest.raises(NotImplementedError):
        enc.engine()
    img = torch.randn((1, 3, 64, 64), generator=torch.Generator(device="cpu").manual_seed(9))
    ref = _module_taps(copy.deepcopy(enc).cpu(), img)
    print()
    _stage_local(enc, ref, cuda)
    eager = enc(img.to(cuda)).clone()
    assert enc._engine_zp is not None and eager.shape == (1, 256, 4, 4) and bool(torch.isfinite(eager).all())
    eng = enc.engine(zero_points=True)
    static = img.to(cuda)
    graph, gout = eng.capture(static)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout, eager)
    eng.row_lanes = 2
    with pytest.raises(NotImplementedError):
        eng(static)
    eng.row_lanes = 1
