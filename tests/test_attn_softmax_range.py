"""fp16 attention kernels on peaked softmax rows: every branch of the lazily moved exp2 offset.

The kernels keep an online softmax whose offset m moves only when a key row's max leaves a band
above it (glob80: deferred move past m + 8, O rescaled and P recomputed past m + 15, the next row's
offset baked into its MFMA C input; general kernel: move past m + 8, O rescale skipped per wave when
no lane moved, the MFMA-held denominator rescaled with O).  ``test_rel_attention``'s scores are a
few units wide and all but never reach the recompute path (printed by
``test_plain_inputs_regime_counts``).  The inputs of ``_attn_peaked_ref`` carry a staircase of
row maxima; the CPU tests below prove on a float64 model of both rules that these inputs reach
every regime and that a machine with one broken step misses the GPU bound by far; the GPU tests
then hold the kernels to the float64 oracle.
"""
import numpy as np
import pytest
import torch

import _attn_peaked_ref as R

SEED = 20251

# (id, (b, h, w, heads, d, window), also run the int8 store)
REL_CASES = [
    ("glob80", (1, 64, 64, 8, 80, 0), True),
    ("stream32-3d", (1, 32, 32, 1, 64, 0), False),
    ("stream64-3d", (1, 64, 64, 1, 64, 0), False),
    ("stream32-xcd", (1, 32, 32, 8, 80, 0), False),
    ("resident16", (1, 16, 16, 2, 80, 0), False),
    ("resident12-masked", (2, 12, 12, 2, 64, 0), False),
    ("resident-win8", (1, 20, 33, 2, 64, 8), False),
    ("win14-d64", (1, 20, 33, 3, 64, 14), True),
    ("win14-d80", (1, 20, 33, 2, 80, 14), True),
]
# precomputed bias tensors through fused_attention.forward
PRE_CASES = [
    ("pre14", (1, 14, 14, 2, 80, 0)),      # the RS = 14 resident form
    ("pre32", (1, 32, 32, 2, 64, 0)),
    ("pre64", (1, 64, 64, 1, 80, 0)),      # the general kernel (glob80 takes no bias tensors)
]
GEOMETRIES = [(i, c) for i, c, _ in REL_CASES] + PRE_CASES

# fp16 P in the numerator and the denominator (2 * 2 * 2^-11 at |v| <= 2) + the fp16 output at
# |o| < 2 (2^-11) = 5 * 2^-11 = 2.44e-3: test_rel_attention's figure
KERNEL_BOUND = 2.5e-3


def _one_head(case):
    """The same construction at one image and one head (CPU cost of the 64 x 64 grids)."""
    b, h, w, heads, d, window = case
    return (1, h, w, 1, d, window)


def _ids(cases):
    return [c[0] for c in cases]


# ----------------------------------------------------------------------------- CPU: the model
@pytest.mark.parametrize("name,case", GEOMETRIES, ids=_ids(GEOMETRIES))
def test_streamed_model_reaches_every_regime(name, case):
    """With no fault the float64 state machine of either rule equals the oracle to 1e-9, keeps P
    inside the bound the kernels' comments state (2^15 glob80, 2^8 general kernel), and the inputs
    reach every regime, 32-query groups split by a branch included."""
    sc, v, ref = R.one_head_unit(_one_head(case), SEED)
    for rule, plim, keys in (("glob80", 2.0 ** 15, ("stay", "deferred", "recompute", "deferred_then_recompute",
                                                    "low14", "low24", "mixed_groups")),
                             ("rel", 2.0 ** 8, ("stay", "deferred", "low14", "low24", "mixed_groups"))):
        out, cnt, pmax = R.streamed_softmax_f64(sc, v, rule)
        err = float(np.abs(out - ref).max())
        print(f"\n[{name}] {rule}: model vs oracle {err:.2e}, log2 Pmax {np.log2(pmax):.3f}, {R.regime_line(cnt)}")
        assert err <= 1e-9
        assert pmax <= plim
        assert all(cnt[k] > 0 for k in keys), cnt
    assert float(np.abs(sc).max()) > 60.0   # scores tens of exp2 units wide, as on a real checkpoint


@pytest.mark.parametrize("name,case", GEOMETRIES, ids=_ids(GEOMETRIES))
def test_input_rounding_distance_is_small(name, case):
    """A condition on the inputs: the kernels' documented input roundings (fp16 scaled q, fp16
    rel-pos terms) move the float64 result by at most 1e-3, so the GPU bound stays tight."""
    dist = R.input_rounding_distance(_one_head(case), SEED)
    print(f"\n[{name}] input rounding distance {dist:.3e}")
    assert dist <= 1e-3


@pytest.mark.parametrize("name,case", GEOMETRIES, ids=_ids(GEOMETRIES))
def test_each_fault_misses_the_gpu_bound(name, case):
    """Each broken machine moves some output by more than 10x the GPU bound of this geometry."""
    one = _one_head(case)
    sc, v, ref = R.one_head_unit(one, SEED)
    bound = KERNEL_BOUND + R.input_rounding_distance(one, SEED)
    figs = []
    for rule, faults in (("glob80", R.FAULTS), ("rel", ("no_rescale_on_deferred", "denominator_not_rescaled"))):
        for fault in faults:
            out, _, _ = R.streamed_softmax_f64(sc, v, rule, fault)
            figs.append((rule, fault, float(np.abs(out - ref).max())))
    print(f"\n[{name}] bound {bound:.3e}; " + ", ".join(f"{r}/{f} {e:.3g}" for r, f, e in figs))
    for rule, fault, err in figs:
        assert err > 10 * bound, (rule, fault, err)


def test_plain_inputs_regime_counts():
    """The gap this file closes, stated on ``test_rel_attention``'s own 64 x 64, d = 80 input (one
    head): of its 258,048 steps after row 0 about a thousand take the deferred move, a handful at
    most the recompute path, none a deferred move followed by a recompute (printed, not asserted:
    the figures describe another test's inputs)."""
    from test_gpu_kernels import _attn_case
    b, h, w, heads, d = 2, 64, 64, 2, 80
    qkv16, _, rph, rpw, _ = _attn_case(b, h, w, heads, d, 0, seed=h * 100 + w + d)
    x = torch.from_numpy(qkv16[:1]).to(torch.float64).view(1, h, w, 3, heads, d)[:, :, :, :, 0].reshape(1, h, w, 3 * d)
    sc, v = R.scores_log2(x, rph, rpw)
    for rule in ("glob80", "rel"):
        _, cnt, pmax = R.streamed_softmax_f64(sc[0].numpy(), v[0].numpy(), rule)
        print(f"\n[test_rel_attention 64x64 d=80, head 0] {rule}: {R.regime_line(cnt)}, log2 Pmax {np.log2(pmax):.2f}")


# ----------------------------------------------------------------------------- GPU: the kernels
def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _rel_args(case, cuda):
    b, h, w, heads, d, window = case
    qkv, bias, rph, rpw = R.peaked_attn_inputs(case, SEED)
    return (_dev(qkv, cuda), _dev(bias, cuda), _dev(rph, cuda), _dev(rpw, cuda), heads, window, d ** -0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [(i, c) for i, c, _ in REL_CASES], ids=_ids(REL_CASES))
def test_rel_attention_peaked(cuda, name, case):
    """ops.rel_attention against the float64 oracle within 2.5e-3 + the case's input rounding
    distance; a second launch is bit-identical.
    Measured on gfx950 (max-abs / bound): glob80 7.5e-4 / 3.19e-3, the streaming cases 6.4e-4 to 7.5e-4 /
    2.96e-3 to 3.05e-3, resident 9.9e-4 to 1.30e-3 / 2.99e-3 to 3.31e-3, window kernel 6.6e-4, 6.8e-4 /
    3.09e-3, 3.01e-3."""
    from samq import ops
    args = _rel_args(case, cuda)
    ref = R.oracle_f64(case, SEED)
    dist = R.input_rounding_distance(case, SEED)
    out = ops.rel_attention(*args)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    print(f"\n[{name}] max-abs vs float64 oracle {err:.3e}, input rounding distance {dist:.3e}")
    assert np.isfinite(got).all()
    assert dist <= 1e-3
    assert err <= KERNEL_BOUND + dist
    assert torch.equal(ops.rel_attention(*args), out)


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [(i, c) for i, c, q in REL_CASES if q],
                         ids=[i for i, _, q in REL_CASES if q])
def test_rel_attention_peaked_q_out(cuda, name, case):
    """The int8 store (out_scale > 0) on the peaked inputs, with ``test_rel_attention_q_out``'s
    assertions: codes within one step of the quantised fp16 composition and of the oracle's codes,
    differing no more often than the composition does (+1e-4).  s = 0.016 keeps |o| <= 2 unclamped.
    Measured on gfx950 (share off by one, f32 store / via fp16): glob80 2.26e-3 / 3.33e-3, window kernel
    d = 64 2.8e-4 / 6.37e-3, d = 80 3.5e-4 / 5.85e-3."""
    from samq import ops
    args = _rel_args(case, cuda)
    ref = R.oracle_f64(case, SEED)
    s = 0.016
    o16 = ops.rel_attention(*args)
    via16 = ops.quantize(o16, s).cpu().numpy().astype(np.int32)
    got = ops.rel_attention(*args, out_scale=s)
    torch.cuda.synchronize()
    assert got.dtype == torch.int8
    assert torch.equal(ops.rel_attention(*args, out_scale=s), got)
    got = got.cpu().numpy().astype(np.int32)
    assert np.abs(got - via16).max() <= 1
    codes = np.clip(np.rint(ref / np.float64(np.float32(s))), -128, 127)
    f_got, f_16 = float((got != codes).mean()), float((via16 != codes).mean())
    print(f"\n[{name} q8] codes off by one vs oracle: f32 store {f_got:.2e}, via fp16 {f_16:.2e}")
    assert np.abs(got - codes).max() <= 1 and f_got <= f_16 + 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", PRE_CASES, ids=_ids(PRE_CASES))
def test_attention_relbias_peaked(cuda, name, case):
    """fused_attention.forward (precomputed fp16 bias tensors, the general kernel at every side)
    against the float64 oracle, same bound; a second launch is bit-identical.
    Measured on gfx950: 9.6e-4 (S = 14), 7.4e-4 (S = 32), 7.0e-4 (S = 64) against 2.9e-3 to 3.0e-3."""
    from samq import fused_attention
    b, h, w, heads, d, _ = case
    qkv = _dev(R.peaked_attn_inputs(case, SEED)[0], cuda)
    rel_h, rel_w = (t.to(cuda) for t in R.precomputed_bias(case, SEED))
    ref = R.oracle_f64(case, SEED)
    dist = R.input_rounding_distance(case, SEED)
    out = fused_attention.forward(qkv, rel_h, rel_w, heads, d, d ** -0.5)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64).reshape(ref.shape)
    err = float(np.abs(got - ref).max())
    print(f"\n[{name}] max-abs vs float64 oracle {err:.3e}, input rounding distance {dist:.3e}")
    assert np.isfinite(got).all()
    assert dist <= 1e-3
    assert err <= KERNEL_BOUND + dist
    assert torch.equal(fused_attention.forward(qkv, rel_h, rel_w, heads, d, d ** -0.5), out)


@pytest.mark.gpu
def test_attention_relbias_takes_strided_and_f32_bias(cuda):
    """fused_attention.forward converts bias tensors that are not contiguous fp16; the converted copies
    must outlive the launch.  (As temporaries, the rel_h copy's block was handed to the rel_w copy and
    the kernel read rel_w for both: found by these inputs with a permuted bias, max-abs 0.43 at
    S = 14, two heads.)  Head-major storage viewed as (B heads, S, S, S), and f32 values, give the
    bits of the contiguous fp16 launch."""
    from samq import fused_attention
    case = PRE_CASES[0][1]
    b, h, w, heads, d, _ = case
    qkv = _dev(R.peaked_attn_inputs(case, SEED)[0], cuda)
    rel_h, rel_w = (t.to(cuda) for t in R.precomputed_bias(case, SEED))
    want = fused_attention.forward(qkv, rel_h, rel_w, heads, d, d ** -0.5)
    strided = [t.transpose(0, 1).contiguous().transpose(0, 1) for t in (rel_h, rel_w)]
    assert not strided[0].is_contiguous() and torch.equal(strided[0], rel_h)
    assert torch.equal(fused_attention.forward(qkv, *strided, heads, d, d ** -0.5), want)
    assert torch.equal(fused_attention.forward(qkv, rel_h.float(), rel_w.float(), heads, d, d ** -0.5), want)
