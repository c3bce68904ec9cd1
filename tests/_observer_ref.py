"""Shared inputs and the float64 restatement for the calibration-observer tests.

Used by ``tests/test_observers_calib.py`` and by ``tests/golden/make_golden_observers.py`` (which
feeds the same seeded tensors to the reference's observers), so the fixture stores no tensors.
"""
import torch

# observer-level cases: name -> (module_type, calibration_mode, shape, permute, seed)
OBSERVER_CASES = {
    "act_layer": ("activation", "layer_wise", (2, 64, 64, 96), False, 101),
    "act_nchw": ("activation", "layer_wise", (2, 96, 24, 20), True, 102),
    "act_channel": ("activation", "channel_wise", (3, 50, 128), True, 103),       # ema only
    "linear_weight": ("linear_weight", "channel_wise", (192, 80), True, 104),     # ema only
}
METHOD_CASES = {
    "ema": ("act_layer", "act_nchw", "act_channel", "linear_weight"),
    "percentile": ("act_layer", "act_nchw"),
    "omse": ("act_layer", "act_nchw"),
}
MODULE_CALIB_SEEDS = (21, 22, 23)   # fq_vitb_img256.npz: its two calibration seeds and its test seed
MODULE_TEST_SEED = 23


def case_inputs(name: str):
    """Three seeded updates of differing scale and offset."""
    shape, seed = OBSERVER_CASES[name][2], OBSERVER_CASES[name][4]
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) * (1.0 + 0.75 * k) + 0.3 * k - 0.1 for k in range(3)]


def omse_candidates(max_val: torch.Tensor, min_val: torch.Tensor, qmin: int, qmax: int, n: int = 90):
    """The omse candidate (max, min, scale, zero_point) 0-dim f32 CPU tensors: the range shrunk by
    i %, the asymmetric scale clamped to f32 eps, the zero point rounded and clamped."""
    eps = torch.finfo(torch.float32).eps
    out = []
    for i in range(n):
        new_max = max_val * (1.0 - (i * 0.01))
        new_min = min_val * (1.0 - (i * 0.01))
        scale = ((new_max - new_min) / float(qmax - qmin)).clamp_(eps)
        zero_point = (qmin - torch.round(new_min / scale)).clamp_(qmin, qmax)
        out.append((new_max, new_min, scale, zero_point))
    return out


def omse_sum_f64(x: torch.Tensor, scale, zero_point, qmin: int, qmax: int) -> float:
    """Sum over ``x`` of the f32 squared fake-quant error, each element computed with torch's
    separate f32 CPU ops, the terms then summed in float64."""
    x = x.detach().float().cpu().reshape(-1)
    s = torch.as_tensor(scale, dtype=torch.float32).reshape(())
    zp = torch.as_tensor(zero_point, dtype=torch.float32).reshape(())
    xq = ((x / s + zp).round().clamp(qmin, qmax) - zp) * s
    return float((x - xq).abs().pow(2.0).double().sum())


def omse_pick_f64(x: torch.Tensor, max_val, min_val, qmin: int, qmax: int):
    """``(index, candidates, scores, gap)``: the first strict minimum of the float64 mean scores in
    candidate order, and the relative gap between the best and the runner-up score."""
    cands = omse_candidates(max_val.detach().float().cpu(), min_val.detach().float().cpu(), qmin, qmax)
    n = x.numel()
    scores = [omse_sum_f64(x, c[2], c[3], qmin, qmax) / n for c in cands]
    best, idx = 1e10, None
    for i, s in enumerate(scores):
        if s < best:
            best, idx = s, i
    runner = min(s for i, s in enumerate(scores) if i != idx)
    return idx, cands, scores, (runner - best) / best
