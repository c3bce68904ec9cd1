"""samq_rel_attention_q8_zp (W8A8 attention on codes with zero points) against the CPU reference of
tests/_attn_zp_ref.py, on every kernel the launcher picks: the 14-window kernel, the resident kernel
on 13 and 16 waves, the streaming global kernel and the 64 x 64 kernel, at head dims 64 and 80.
"""
import numpy as np
import pytest
import torch

import _attn_zp_ref as A

# (b, hw, window, heads, with_bias)
GEOMS = {
    "win14": (1, 20, 14, 3, True),
    "win14-nobias": (1, 20, 14, 3, False),
    "win7": (1, 20, 7, 3, True),          # resident kernel, 13 waves
    "win16": (1, 20, 16, 3, True),        # resident kernel, 16 waves
    "glob16": (1, 16, 0, 3, True),        # streaming kernel
    "glob17": (1, 17, 0, 3, True),        # ... on a ragged grid
    "glob64": (1, 64, 0, 1, True),        # 64 x 64 kernel, int8 V
}
MAX_SHARE = 5e-3      # test_rel_attention_q8's bound for this kernel family


def _launch(cuda, qkv, bias, relh, relw, heads, window, scales, zps, sm_scale=None, **kw):
    from samq import ops
    dev = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(cuda)
    d = qkv.shape[-1] // 3 // heads
    return ops.rel_attention_q8_zp(dev(qkv), dev(bias), dev(relh), dev(relw), heads, window,
                                   d ** -0.5 if sm_scale is None else sm_scale, *(float(s) for s in scales), *zps, **kw)


def _close(out, ref, max_frac, what):
    d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
    frac = float((d > 0).mean())
    print(f"\n  [{what}] codes differing {frac:.2e}, max |dcode| {d.max()}")
    assert d.max() <= 1, f"{what}: code off by {d.max()}"
    assert frac <= max_frac, f"{what}: {frac:.2e} of codes off by one (> {max_frac:.1e})"


# ============================================================================= CPU: what the inputs can see
@pytest.mark.parametrize("geom", ["win14", "win14-nobias", "glob16"])
def test_attn_zp_inputs_pin_the_terms(geom):
    """On the GPU tests' inputs a reference without the key-sum or the query-sum term of
    sum (q - z)(k - z), or with zero pad codes, gives other output codes in far more than the GPU
    bound of 5e-3; 3 - 30 % of the first score quantiser's codes sit on a clamp end, so the clamp
    works on shifted arguments.  On the exact-tie inputs, fp32 and float64 references agree to 1e-4
    and zero points added after the rounding move more than 1e-3 of the codes."""
    b, hw, window, heads, with_bias = GEOMS[geom]
    zps = A.ZP_SETS[0]
    qkv, bias, relh, relw = A.inputs(b, hw, hw, heads, 64, window, zps[0], hw + window)
    bias = bias if with_bias else None
    sat = []
    ref = A.attn_ref_zp(qkv, bias, relh, relw, heads, window, A.Q8_SCALES, zps, codes1=sat)
    assert 0.03 <= np.mean(sat) <= 0.3, np.mean(sat)
    frac = lambda wrong: float((A.attn_ref_zp(qkv, bias, relh, relw, heads, window, A.Q8_SCALES, zps, wrong=wrong)
                                != ref).mean())
    assert frac("ksum") > 0.05 and frac("qsum") > 0.05
    if window:
        assert frac("pad0") > 0.02
    qkv, bias, relh, relw, scales = A.exact_inputs(b, hw, hw, 2, window, hw + window)
    bias = bias if with_bias else None
    r64 = A.attn_ref_zp(qkv, bias, relh, relw, 2, window, scales, A.EXACT_ZPS, torch.float64, sm_scale=0.125)
    r32 = A.attn_ref_zp(qkv, bias, relh, relw, 2, window, scales, A.EXACT_ZPS, sm_scale=0.125)
    assert float((r32 != r64).mean()) <= 1e-4
    late = A.attn_ref_zp(qkv, bias, relh, relw, 2, window, scales, A.EXACT_ZPS, torch.float64, "after", sm_scale=0.125)
    assert float((late != r64).mean()) > 1e-3


# ============================================================================= GPU
@pytest.mark.gpu
@pytest.mark.parametrize("zps", A.ZP_SETS, ids=("zpA", "zpB"))
@pytest.mark.parametrize("d", (64, 80))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_rel_attention_q8_zp(cuda, geom, d, zps):
    """Codes zp_qkv + U[-105, 104], the scales of test_rel_attention_q8, two sets of four non-zero
    zero points: every output code within +-1 of the fp32 reference, at most 5e-3 of them off by one."""
    b, hw, window, heads, with_bias = GEOMS[geom]
    qkv, bias, relh, relw = A.inputs(b, hw, hw, heads, d, window, zps[0], hw + window)
    bias = bias if with_bias else None
    ref = A.attn_ref_zp(qkv, bias, relh, relw, heads, window, A.Q8_SCALES, zps)
    out = _launch(cuda, qkv, bias, relh, relw, heads, window, A.Q8_SCALES, zps)
    _close(out.cpu().numpy(), ref, MAX_SHARE, f"attention_q8_zp {geom} d {d} zp {zps}")


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["win14", "win7", "win16", "glob16", "glob64"])
def test_rel_attention_q8_zp_exact_ties(cuda, geom):
    """One case per kernel on inputs whose score-side values are all exact, with odd zero points: the
    rounding of x / s + zp and the clamp ends.  Every code within +-1 of the float64 reference, at
    most 1e-4 of them differ (the bound of test_rel_attention_q8_exact_ties)."""
    b, hw, window, _, _ = GEOMS[geom]
    heads = 1 if hw == 64 else 2
    qkv, bias, relh, relw, scales = A.exact_inputs(b, hw, hw, heads, window, hw + window)
    ref = A.attn_ref_zp(qkv, bias, relh, relw, heads, window, scales, A.EXACT_ZPS, torch.float64, sm_scale=0.125)
    out = _launch(cuda, qkv, bias, relh, relw, heads, window, scales, A.EXACT_ZPS, sm_scale=0.125)
    _close(out.cpu().numpy(), ref, 1e-4, f"attention_q8_zp exact {geom}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", (64, 80))
@pytest.mark.parametrize("geom", ["win14", "win14-nobias", "win7", "win16", "glob17", "glob64"])
def test_rel_attention_q8_zp_zero_is_symmetric(cuda, geom, d):
    """All zero points 0: the codes of samq_rel_attention_q8_rows, bit for bit (full-range codes);
    zp_qkv = -128 (the constant MFMA operand runs twice) still matches the reference."""
    from samq import ops
    b, hw, window, heads, with_bias = GEOMS[geom]
    rng = np.random.Generator(np.random.PCG64([hw, window, d]))
    _, bias, relh, relw = A.inputs(b, hw, hw, heads, d, window, 0, hw + window)
    qkv = rng.integers(-128, 128, (b, hw, hw, 3 * heads * d), dtype=np.int8)
    bias = bias if with_bias else None
    dev = lambda a: None if a is None else torch.from_numpy(a).to(cuda)
    sym = ops.rel_attention_q8(dev(qkv), dev(bias), dev(relh), dev(relw), heads, window, d ** -0.5,
                               *(float(s) for s in A.Q8_SCALES))
    out = _launch(cuda, qkv, bias, relh, relw, heads, window, A.Q8_SCALES, (0, 0, 0, 0))
    assert torch.equal(out, sym)
    if geom in ("win14", "glob17"):
        zps = (-128, 5, -7, 9)
        q2 = (rng.integers(-128, 82, qkv.shape)).astype(np.int8)          # values (code + 128) s in [0, 209 s]
        ref = A.attn_ref_zp(q2, bias, relh, relw, heads, window, A.Q8_SCALES, zps)
        _close(_launch(cuda, q2, bias, relh, relw, heads, window, A.Q8_SCALES, zps).cpu().numpy(), ref, MAX_SHARE,
               f"attention_q8_zp {geom} d {d} zp_qkv -128")


@pytest.mark.gpu
def test_rel_attention_q8_zp_rows_and_refusals(cuda):
    """Row ranges on the 64 x 64 grid give the full launch's codes; an fp16 V copy, zero points outside
    [-128, 127] and the geometries samq_rel_attention_q8_rows refuses are refused."""
    heads, d, hw = 1, 64, 64
    zps = A.ZP_SETS[1]
    qkv, bias, relh, relw = A.inputs(1, hw, hw, heads, d, 0, zps[0], 7)
    dq, dh, dw = (torch.from_numpy(a).to(cuda) for a in (qkv, relh, relw))
    full = _launch(cuda, dq, None, dh, dw, heads, 0, A.Q8_SCALES, zps)
    out = torch.zeros_like(full)
    for r0, n in ((0, 28), (28, 36)):
        _launch(cuda, dq, None, dh, dw, heads, 0, A.Q8_SCALES, zps, out=out, rows=(r0, n))
    assert torch.equal(out, full)
    with pytest.raises(NotImplementedError):
        _launch(cuda, dq, None, dh, dw, heads, 0, A.Q8_SCALES, zps, v16=dq[..., 2 * d:].to(torch.float16).contiguous())
    for bad in ((-129, 0, 0, 0), (0, 128, 0, 0), (0, 0, 0, 200)):
        with pytest.raises(AssertionError):
            _launch(cuda, dq, None, dh, dw, heads, 0, A.Q8_SCALES, bad)
    small = torch.zeros((1, 32, 32, 3 * d), dtype=torch.int8, device=cuda)
    z = torch.zeros((63, d), device=cuda)
    with pytest.raises(NotImplementedError):
        _launch(cuda, small, None, z, z, heads, 0, A.Q8_SCALES, zps, rows=(0, 16))
    with pytest.raises(NotImplementedError):
        _launch(cuda, small, None, z[:33], z[:33], heads, 17, A.Q8_SCALES, zps)
