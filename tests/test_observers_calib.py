"""fq_vit calibration observers: ema, percentile and omse (``observer/{ema,percentile,omse}.py``).

CPU: the observer classes and the calibrated module tree against what the reference computes
(``golden/fq_observers.npz``, written by ``golden/make_golden_observers.py``), bit for bit; the
host finish of the percentile observer against ``torch.quantile`` / ``np.percentile``.
GPU: ``samq_order_stats`` against ``torch.sort``, ``samq_omse_scores`` against the float64
restatement of ``_observer_ref.py``, the HIP observer paths against the same classes on the CPU,
and calibrated vit_b encoders end to end.
"""
import functools
import json

import numpy as np
import pytest
import torch

from oracle import fq_ref, synth
import _observer_ref as R

METHODS = ("ema", "percentile", "omse")
ALPHA = 0.99999
BIG_N = 2 ** 24 + 3


def _observer(method, module_type="activation", mode="layer_wise", permute=True):
    from samq import fq_vit
    return fq_vit.build_observer(method, module_type, fq_vit.BIT_TYPE_DICT["int8"], mode, permute=permute)


@functools.lru_cache(maxsize=None)
def _fixture(golden_dir):
    g = np.load(golden_dir / "fq_observers.npz", allow_pickle=False)
    return g, json.loads(str(g["meta"]))


@functools.lru_cache(maxsize=None)
def _model_state(golden_dir):
    _, meta = _fixture(golden_dir)
    cfg = synth.encoder_config("vit_b", img_size=meta["img_size"])
    st = {k: v.astype(np.float16).astype(np.float32) for k, v in synth.make_encoder_state(cfg, seed=meta["seed"]).items()}
    return cfg, st


def _encoder(golden_dir, method, device="cpu"):
    from samq import fq_vit
    cfg, st = _model_state(golden_dir)
    qcfg = fq_vit.Config(False, False, method)
    qcfg.BIT_TYPE_A = fq_vit.BIT_TYPE_DICT["int8"]
    enc = fq_vit.build_fq_image_encoder("vit_b", img_size=cfg["img_size"], cfg=qcfg)
    missing, unexpected = enc.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    assert not unexpected, unexpected
    assert all("quantizer" in k for k in missing), missing
    return enc.to(device).eval()


def _calib_images(golden_dir, device="cpu"):
    _, meta = _fixture(golden_dir)
    return [torch.from_numpy(synth.make_images(1, meta["img_size"], seed=s)).to(device) for s in meta["calib_seeds"]]


# ----------------------------------------------------------------------------- CPU
def test_build_observer_dispatch():
    from samq import fq_vit
    for m, cls in (("minmax", fq_vit.MinmaxObserver), ("ema", fq_vit.EmaObserver),
                   ("percentile", fq_vit.PercentileObserver), ("omse", fq_vit.OmseObserver)):
        assert type(_observer(m)) is cls
    e, p = _observer("ema"), _observer("percentile")
    assert e.ema_sigma == 0.01 and (p.percentile_sigma, p.percentile_alpha) == (0.01, ALPHA)
    assert e.symmetric and e.max_val is None and e.min_val is None and e.eps == torch.finfo(torch.float32).eps
    with pytest.raises(NotImplementedError):
        _observer("ptf")
    with pytest.raises(AssertionError):
        _observer("percentile", mode="channel_wise").update(torch.randn(4, 8))


@pytest.mark.parametrize("method,case", [(m, c) for m in METHODS for c in R.METHOD_CASES[m]])
def test_observer_matches_reference(golden_dir, method, case):
    """Running max_val / min_val after every update and the final scale / zero point equal the
    reference observer's, bit for bit (same seeded inputs as the fixture generator)."""
    g, _ = _fixture(golden_dir)
    module_type, mode, _, permute, _ = R.OBSERVER_CASES[case]
    obs = _observer(method, module_type, mode, permute)
    key = f"obs:{method}:{case}"
    xs = R.case_inputs(case)
    for k, x in enumerate(xs):
        obs.update(x)
        np.testing.assert_array_equal(obs.max_val.numpy(), g[key + ":max"][k])
        np.testing.assert_array_equal(obs.min_val.numpy(), g[key + ":min"][k])
    scale, zp = obs.get_quantization_params(xs[-1]) if method == "omse" else obs.get_quantization_params()
    np.testing.assert_array_equal(scale.numpy(), g[key + ":scale"])
    np.testing.assert_array_equal(zp.numpy(), g[key + ":zp"])
    if method == "omse":   # the winner's range replaces the statistics (omse.py:52-53)
        np.testing.assert_array_equal(obs.max_val.numpy(), g[key + ":best_max"])
        np.testing.assert_array_equal(obs.min_val.numpy(), g[key + ":best_min"])


def _quantile_vectors(n, seed):
    g = torch.Generator().manual_seed(1000 * seed + n % 997)
    yield torch.randn(n, generator=g) * 3 + 0.5
    yield torch.round(torch.randn(n, generator=g) * 2)     # long runs of equal values


@pytest.mark.parametrize("n", [1, 2, 255, 99_999, 1_000_003])
def test_quantile_from_order_stats_vs_torch(n):
    from samq.fq_vit import _quantile_ranks, quantile_from_order_stats
    for seed in range(3):
        for v in _quantile_vectors(n, seed):
            s = torch.sort(v).values
            for q in (ALPHA, 1.0 - ALPHA):
                lo, hi = _quantile_ranks(n, q)
                got = quantile_from_order_stats(n, q, s[lo], s[hi])
                np.testing.assert_array_equal(got.numpy(), torch.quantile(v, q).numpy())


def test_quantile_from_order_stats_vs_numpy():
    """Above 2**24 elements torch.quantile refuses the tensor and the reference falls back to
    np.percentile on the float32 data (percentile.py:31-39)."""
    from samq.fq_vit import _quantile_ranks, quantile_from_order_stats
    with pytest.raises(RuntimeError):
        torch.quantile(torch.zeros(BIG_N), 0.5)
    for seed in range(2):
        for v in _quantile_vectors(BIG_N, seed):
            s = torch.sort(v).values
            for q in (ALPHA, 1.0 - ALPHA):
                lo, hi = _quantile_ranks(BIG_N, q)
                got = quantile_from_order_stats(BIG_N, q, s[lo], s[hi])
                want = np.percentile(v.numpy(), q * 100)
                assert want.dtype == np.float32
                np.testing.assert_array_equal(got.numpy(), want)


@pytest.mark.slow
@pytest.mark.parametrize("method", METHODS)
def test_module_calibration_matches_reference(golden_dir, method):
    """``Config(False, False, method)`` with int8 activations, calibrate_with of three images on the
    CPU: the reference's 140 activation scales (omse: and zero points, and the quant-mode module
    forward's output codes), bit for bit."""
    from samq import fq_vit
    g, meta = _fixture(golden_dir)
    names = [str(n) for n in np.load(golden_dir / "fq_vitb_img256.npz", allow_pickle=False)["act_scale_names"]]
    enc = _encoder(golden_dir, method)
    enc.calibrate_with(_calib_images(golden_dir))
    qa = fq_vit.act_quantizers(enc)
    assert list(qa) == names and len(names) == 140
    scales = np.array([float(qa[n].quantizer.scale.reshape(-1)[0]) for n in names], np.float32)
    zps = np.array([float(qa[n].quantizer.zero_point.reshape(-1)[0]) for n in names], np.float32)
    np.testing.assert_array_equal(scales, g[f"mod:{method}:scales"])
    if method != "omse":
        assert not zps.any()
        return
    np.testing.assert_array_equal(zps, g["mod:omse:zps"])
    assert zps.any()
    img = torch.from_numpy(synth.make_images(1, meta["img_size"], seed=meta["test_seed"]))
    with torch.no_grad():
        out = enc.module_forward(img).numpy()
    s_out = float(scales[names.index("qacts.3")])
    np.testing.assert_array_equal(np.round(out / s_out), g["mod:omse:codes"].astype(np.float32))


@pytest.mark.parametrize("method", ("minmax",) + METHODS)
def test_random_fq_encoder_quant_method(method):
    """``samq.synthetic.random_fq_encoder(quant_method=...)`` builds ``Config(False, False, method)``
    with int8 activations; only omse leaves non-zero zero points."""
    from samq import fq_vit, synthetic
    enc = synthetic.random_fq_encoder("vit_b", device="cpu", img_size=64, depth=1, calib_images=2,
                                      quant_method=method)
    assert enc.cfg.OBSERVER_A == method and enc.cfg.BIT_TYPE_A.name == "int8" and enc.is_quant()
    qa = fq_vit.act_quantizers(enc)
    assert all(type(m.observer) is fq_vit.OBSERVERS[method] for m in qa.values())
    assert all(type(m.observer) is fq_vit.MinmaxObserver for m in enc.modules()
               if isinstance(m, (fq_vit.QLinear, fq_vit.QConv2d)))
    assert any(int(m.quantizer.zero_point) != 0 for m in qa.values()) == (method == "omse")


def test_observer_abi_exports():
    """The new entry points are part of the C ABI; the workspace queries run without a GPU."""
    from samq import _lib
    lib = _lib.load()
    assert lib.samq_order_stats_workspace(0, 4) == 0
    assert lib.samq_order_stats_workspace(10, 5) == 0
    ws = lib.samq_order_stats_workspace(1, 1)
    assert ws > 0 and lib.samq_order_stats_workspace(2 ** 31 + 5, 4) == ws    # histograms only: no n-sized buffer
    assert lib.samq_omse_scores_workspace(0, 90) == 0
    assert lib.samq_omse_scores_workspace(10, 97) == 0
    small, big = lib.samq_omse_scores_workspace(1, 90), lib.samq_omse_scores_workspace(2 ** 31 + 5, 90)
    assert 0 < small <= big <= 1 << 20
    assert {"samq_order_stats", "samq_omse_scores"} <= set(_lib.exported_symbols())


# ----------------------------------------------------------------------------- GPU: order statistics
def _os_input(kind, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        v = torch.randn(n, generator=g)
    elif kind == "levels16":      # ranks fall inside long runs of equal keys
        v = torch.randint(0, 16, (n,), generator=g).float() * 0.25 - 2.0
    elif kind == "equal":
        v = torch.full((n,), -1.375)
    elif kind == "special":       # mixed signs, +-0, denormals (of the dtype), +-inf
        tiny = torch.finfo(dtype).tiny
        pool = torch.tensor([0.0, -0.0, tiny / 4, -tiny / 4, tiny / 2, -tiny / 2, tiny, -tiny, float("inf"),
                             float("-inf"), 1.5, -1.5, 3e4, -3e4, 1e-3, -1e-3], dtype=torch.float64)
        v = pool[torch.randint(0, len(pool), (n,), generator=g)].float()
    elif kind == "nan":
        v = torch.randn(n, generator=g)
        v[n // 2] = float("nan")
    return v.to(dtype)


def _percentile_ranks(n):
    from samq.fq_vit import _quantile_ranks
    return list(_quantile_ranks(n, ALPHA) + _quantile_ranks(n, 1.0 - ALPHA))


def _check_order_stats(v, cuda):
    from samq import ops
    n = v.numel()
    want = torch.sort(v.float()).values
    dv = v.to(cuda)
    for ranks in ([0, n - 1], _percentile_ranks(n)):
        vals, flag = ops.order_stats(dv, ranks)
        assert vals.is_cuda and flag.is_cuda and vals.dtype == torch.float32
        has_nan = bool(torch.isnan(v).any())
        assert int(flag) == int(has_nan)
        if not has_nan:
            got = vals.cpu()
            assert not torch.isnan(got).any()
            assert bool((got == want[ranks]).all()), (ranks, got, want[ranks])    # ==, so +-0 pass


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 1_000_003])
@pytest.mark.parametrize("kind", ["normal", "levels16", "equal", "special", "nan"])
def test_order_stats_vs_sort(cuda, kind, n, dtype):
    _check_order_stats(_os_input(kind, n, dtype, seed=n % 1000 + len(kind)), cuda)


@pytest.mark.gpu
def test_order_stats_above_2_24(cuda):
    _check_order_stats(_os_input("normal", BIG_N, torch.float32, seed=7), cuda)


@pytest.mark.gpu
def test_order_stats_past_2_31(cuda):
    """Element indices past 2^31 (f16, 4 GiB): zeros with four planted values, so the order
    statistics are known without a sort; the zeros are one 2^31-long run of equal keys."""
    from samq import ops
    n = 2 ** 31 + 77
    x = torch.zeros(n, dtype=torch.float16, device=cuda)
    x[5] = -3.0
    x[2 ** 31 - 1] = -0.5
    x[2 ** 31 + 3] = 5.0
    x[n - 1] = 7.0
    vals, flag = ops.order_stats(x, [0, 1, n - 2, n - 1])
    assert int(flag) == 0 and vals.cpu().tolist() == [-3.0, -0.5, 5.0, 7.0]
    vals, _ = ops.order_stats(x, [2, 2 ** 31, n - 3])
    assert vals.cpu().tolist() == [0.0, 0.0, 0.0]


# ----------------------------------------------------------------------------- GPU: observers vs CPU
def _compare_observers(method, module_type, mode, permute, xs, cuda):
    ref, hip = _observer(method, module_type, mode, permute), _observer(method, module_type, mode, permute)
    for x in xs:
        ref.update(x.float())         # exact for f16 (torch.quantile takes no f16 on the CPU)
        hip.update(x.to(cuda))
        assert hip.max_val.is_cuda
        np.testing.assert_array_equal(hip.max_val.cpu().numpy(), ref.max_val.float().numpy())
        np.testing.assert_array_equal(hip.min_val.cpu().numpy(), ref.min_val.float().numpy())
    s_ref, z_ref = ref.get_quantization_params()
    s_hip, z_hip = hip.get_quantization_params()
    assert s_hip.is_cuda
    np.testing.assert_array_equal(s_hip.cpu().numpy(), s_ref.numpy())
    np.testing.assert_array_equal(z_hip.cpu().numpy(), z_ref.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.METHOD_CASES["ema"])
def test_ema_observer_gpu_matches_cpu(cuda, case):
    module_type, mode, _, permute, _ = R.OBSERVER_CASES[case]
    _compare_observers("ema", module_type, mode, permute, R.case_inputs(case), cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.METHOD_CASES["percentile"])
def test_percentile_observer_gpu_matches_cpu(cuda, case):
    module_type, mode, _, permute, _ = R.OBSERVER_CASES[case]
    xs = R.case_inputs(case)
    xs[1] = xs[1].half()      # f16 activations take the in_f16 path
    _compare_observers("percentile", module_type, mode, permute, xs, cuda)


@pytest.mark.gpu
def test_percentile_observer_gpu_numpy_branch(cuda):
    """One update above 2**24 elements: the CPU class falls back to np.percentile, the HIP path to
    its restatement in quantile_from_order_stats."""
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(40, 96, generator=g), torch.randn(BIG_N, 1, generator=g) * 2 + 0.25,
          torch.randn(40, 96, generator=g) * 3]
    assert xs[1].numel() == BIG_N
    _compare_observers("percentile", "activation", "layer_wise", True, xs, cuda)


@pytest.mark.gpu
def test_percentile_observer_gpu_nan(cuda):
    x = torch.randn(300, 70)
    x[17, 5] = float("nan")
    ref, hip = _observer("percentile"), _observer("percentile")
    ref.update(x)
    hip.update(x.to(cuda))
    assert torch.isnan(ref.max_val) and torch.isnan(hip.max_val) and torch.isnan(hip.min_val)


# ----------------------------------------------------------------------------- GPU: omse
QMIN, QMAX = -128, 127


def _omse_input(kind):
    g = torch.Generator().manual_seed(11)
    if kind == "n1":
        return torch.tensor([0.7311])
    if kind == "n1m":
        return torch.randn(1_000_003, generator=g) * 1.7 + 0.4
    if kind == "f16":
        return (torch.randn(70_001, generator=g) * 2.5 - 0.3).half()
    if kind == "constant":      # max == min: the scale clamps to eps, the zero point clamps
        return torch.full((4099,), 0.625)
    if kind == "ties":
        # max 127.5, min -127.5: candidate 0 is scale 1.0, zero point 0, and every k + 0.5 is an exact tie
        x = torch.arange(-128, 128).float() + 0.5
        assert float(x.max()) == 127.5 and float(x.min()) == -127.5
        return torch.cat([x, x, torch.rand(301, generator=g) * 200 - 100])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["n1", "n1m", "f16", "constant", "ties"])
def test_omse_scores_vs_float64(cuda, kind):
    """The 90 sums against the per-element f32 torch terms summed in float64 on the CPU;
    rtol = 2 n 2^-53, the worst case between two float64 summation orders of non-negative terms."""
    from samq import ops
    x = _omse_input(kind)
    n = x.numel()
    xf = x.float()
    cands = R.omse_candidates(xf.max(), xf.min(), QMIN, QMAX)
    if kind == "ties":
        assert float(cands[0][2]) == 1.0 and float(cands[0][3]) == 0.0
    if kind == "constant":
        assert float(cands[0][2]) == torch.finfo(torch.float32).eps and float(cands[0][3]) == QMIN
    table = torch.tensor([[float(c[2]), float(c[3])] for c in cands], dtype=torch.float32)
    want = np.array([R.omse_sum_f64(x, c[2], c[3], QMIN, QMAX) for c in cands])
    got = ops.omse_scores(x.to(cuda), table.to(cuda), QMIN, QMAX)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (90,)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2 * n * 2.0 ** -53, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.METHOD_CASES["omse"])
def test_omse_observer_gpu_picks_float64_minimum(cuda, golden_dir, case):
    """OmseObserver on GPU tensors: the chosen candidate, scale and zero point are the first strict
    minimum of the float64 restatement (on these inputs also the reference's pick: the fixture
    generator asserts it and records the gap to the runner-up, far above the summation error)."""
    g, _ = _fixture(golden_dir)
    module_type, mode, _, permute, _ = R.OBSERVER_CASES[case]
    obs = _observer("omse", module_type, mode, permute)
    xs = R.case_inputs(case)
    for x in xs:
        obs.update(x.to(cuda))
    idx, cands, _, gap = R.omse_pick_f64(xs[-1], obs.max_val, obs.min_val, QMIN, QMAX)
    assert gap > 1e-6
    scale, zp = obs.get_quantization_params(xs[-1].to(cuda))
    assert scale.is_cuda and obs.max_val.is_cuda
    key = f"obs:omse:{case}"
    assert idx == int(g[key + ":idx"])
    np.testing.assert_array_equal(scale.cpu().numpy(), cands[idx][2].numpy())
    np.testing.assert_array_equal(zp.cpu().numpy(), cands[idx][3].numpy())
    np.testing.assert_array_equal(obs.max_val.cpu().numpy(), cands[idx][0].numpy())
    np.testing.assert_array_equal(scale.cpu().numpy(), g[key + ":scale"])
    np.testing.assert_array_equal(zp.cpu().numpy(), g[key + ":zp"])


@pytest.mark.gpu
def test_omse_encoder_runs_module_graph_and_engine_refuses(cuda, golden_dir):
    """An omse-calibrated encoder has non-zero activation zero points: the fused engine keeps its
    refusal, and QAct's quant forward takes the zero point into account (torch path)."""
    from samq import fq_vit
    enc = _encoder(golden_dir, "omse", cuda)
    enc.calibrate_with(_calib_images(golden_dir, cuda))
    qa = fq_vit.act_quantizers(enc)
    assert all(m.observer.max_val.is_cuda for m in qa.values())
    assert any(int(m.quantizer.zero_point) != 0 for m in qa.values())
    with pytest.raises(NotImplementedError, match="symmetric"):
        enc.engine()
    q = next(m for m in qa.values() if int(m.quantizer.zero_point) != 0)
    x = torch.randn(2, 16, 16, 768, device=cuda) * float(q.quantizer.scale) * 40
    np.testing.assert_array_equal(q(x).cpu().numpy(), q.quantizer(x).cpu().numpy())


# ----------------------------------------------------------------------------- GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("method", ["ema", "percentile"])
def test_calibrated_encoder_end_to_end(cuda, golden_dir, method):
    """vit_b at img 256 calibrated on the GPU with the HIP observers: every QAct's scale equals
    that of a CPU twin observer fed the identical tensors, and the engine's output meets the
    criteria of test_w8a8_encoder_vs_golden against the oracle with those scales."""
    from samq import fq_vit
    _, meta = _fixture(golden_dir)
    cfg, st = _model_state(golden_dir)
    enc = _encoder(golden_dir, method, cuda)
    qa = fq_vit.act_quantizers(enc)
    twins = {}
    for name, m in qa.items():
        twins[name] = _observer(method, "activation", m.calibration_mode, m.observer.permute)
        m.register_forward_pre_hook(
            lambda mod, inp, t=twins[name]: t.update(inp[0].detach().cpu()) if mod.calibrate else None)
    enc.calibrate_with(_calib_images(golden_dir, cuda))
    scales = {}
    for name, m in qa.items():
        assert m.observer.max_val.is_cuda and type(m.observer).__name__.lower().startswith(method)
        s_cpu, z_cpu = twins[name].get_quantization_params()
        np.testing.assert_array_equal(m.quantizer.scale.cpu().numpy(), s_cpu.numpy(), err_msg=name)
        assert int(z_cpu) == 0 and int(m.quantizer.zero_point) == 0
        scales[name] = float(s_cpu)
    assert len(scales) == 140
    img_np = synth.make_images(1, meta["img_size"], seed=meta["test_seed"])
    out = enc(torch.from_numpy(img_np).to(cuda)).float().cpu().numpy()
    s_out = scales["qacts.3"]
    codes = np.round(out / s_out)
    np.testing.assert_allclose(codes * s_out, out, rtol=0, atol=1e-5 * max(1.0, np.abs(out).max()))
    o32 = fq_ref.FQEncoderOracle(cfg, st)
    o32.set_scales(scales)
    ref = np.round(o32(img_np).numpy() / s_out).astype(np.float64)
    o64 = fq_ref.FQEncoderOracle(cfg, st, dtype=torch.float64)
    o64.set_scales(scales)
    c64 = np.round(o64(img_np).numpy() / s_out)

    def stats(a, b):
        d = np.abs(a - b)
        cos = float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
        return float((d == 0).mean()), float(d.mean()), float(d.max()), cos

    ours, self_ = stats(codes, ref), stats(c64, ref)
    print(f"\nW8A8 vit_b 256 ({method}): ours vs oracle fp32: {ours[0] * 100:.2f}% codes equal, mean |dcode| "
          f"{ours[1]:.3f}, max {ours[2]:.0f}, cos {ours[3]:.5f} | oracle fp64 vs fp32: mean {self_[1]:.3f}, "
          f"max {self_[2]:.0f}, cos {self_[3]:.5f}")
    assert ours[1] <= 1.25 * self_[1] + 0.05
    assert ours[3] >= 0.995
    assert ours[2] * s_out <= 0.15 * np.abs(ref).max() * s_out
