"""The W4A16 LayerNorm-fold and gated-MLP epilogues (csrc/gemm_w4a16.hip: lnf_res4, lnf_stats16,
lnf_produce_slice, lnf_rowinfo_wg, lnf_out8 and the SILU_MUL branch of the 32x32 epilogue) against
float64 references on the exact inputs of ``_w4a16_ref.problem``.

``acc * s + b`` and the fp32 residual sum are exact on those inputs in any order, so the producer
(RESADD_LNF) must give the residual and the fp16 fold operand bit for bit and every block's partial
sums within the bound of its summation tree.  The consumers (BIAS_LNF, GELU_LNF) run on synthetic
per-row ``stats`` (``_w4a16_ref.LnfStats``) and must land within ``[f16(y - E), f16(y + E)]`` of
the float64 y, E counted from the fp32 roundings on the path (``_w4a16_ref.lnf_c``).  Every buffer
a launch writes is a row slice of a taller sentinel buffer whose other rows must stay untouched;
``stats`` sits in a NaN frame, so a pair read from outside a row's range poisons the output.
The launches are the four ``launch_lnf`` and the two ``launch_silu`` instantiations: configs 57 and
64, per channel and grouped, at 1, 3 and 5 K tiles (fewer than, equal to and more than the ring's
lookahead; K / 64 odd) and, for the consumers, 2 and 4 (K / 64 even).
"""
import numpy as np
import pytest
import torch

import _w4a16_ref as R

CFGS = (57, 64)
NS = (256, 768)                                       # 1 and 3 column tiles
MS = R.LNF_MS
ODD_KG = ((64, 0), (192, 0), (320, 0), (64, 64), (192, 64), (320, 64), (320, 128))   # (320, 128): ragged
EVEN_KG = ((128, 0), (256, 0), (128, 64), (256, 64))
CONS_KG = ODD_KG + EVEN_KG
GATED_NS = (128, 384)
SILU_E_REL = 2.0 ** -19        # the gated MLP's relative bound: 4 x the measured 2.95e-7, up to a power of two
F16_SENTINEL = 60000.0


def _kg_id(kg):
    return f"k{kg[0]}" + (f"-g{kg[1]}" if kg[1] else "")


def _f16_of(y):
    with np.errstate(over="ignore", invalid="ignore"):
        return y.astype(np.float16)


def _mutated_share(y, e, y_mut):
    """The share of outputs at which a kernel that computed y_mut exactly would fail the interval
    check against (y, e)."""
    lo, hi, got = _f16_of(y - e), _f16_of(y + e), _f16_of(y_mut)
    return float((~((got >= lo) & (got <= hi))).mean())


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("kg", ODD_KG, ids=_kg_id)
def test_lnf_producer_inputs_pin_the_kernel(kg):
    """CPU: on every (K, group, N) of the producer test, mu_p is a multiple of 2^-12 within 0.5 (+ one
    step) of the row mean and differs in every row; recomputed in fp32, d = x_new - mu_p and
    d * gamma equal the float64 values exactly (gamma from {1, 2, 4}), float16(d * gamma) is finite
    and no non-zero value is an fp16 subnormal.  Sensitivity: a block's sums written one block index
    off miss the bound of the GPU test at every (row, block)."""
    p = R.problem(*kg)
    for n in NS:
        pr = R.lnf_producer(*kg, n)
        mu = pr.mu.astype(np.float64)
        assert np.all((mu * 4096) % 1 == 0)
        assert np.abs(mu - pr.x.mean(1)).max() <= 0.5 + 2.0 ** -12
        assert len(np.unique(mu)) == p.m
        assert set(np.unique(pr.gamma)) == {1.0, 2.0, 4.0}
        x32 = p.ref("resadd")[:, :n]
        d32 = x32 - pr.mu[:, None]
        assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), pr.d)
        dg32 = d32 * pr.gamma[None, :]
        assert dg32.dtype == np.float32 and np.array_equal(dg32.astype(np.float64), pr.aout64)
        assert np.isfinite(pr.aout).all()
        nz = np.abs(pr.aout64[pr.aout64 != 0])
        assert nz.min() >= 2.0 ** -14
        b1, b2 = pr.stats_bounds()
        moved = (np.abs(np.roll(pr.s1, 1, 1) - pr.s1) > b1) | (np.abs(np.roll(pr.s2, 1, 1) - pr.s2) > b2)
        assert moved.all(), f"N={n}: {int((~moved).sum())} block sums equal their neighbour's within the bound"
        good = np.stack([pr.s1, pr.s2], 2).astype(np.float32)
        assert pr.stats_violations(good, p.m) == 0
        assert pr.stats_violations(np.roll(good, 1, 1), p.m) >= p.m * (n // 64)


@pytest.mark.parametrize("k", sorted({k for k, _ in CONS_KG}))
def test_lnf_consumer_inputs_pin_the_kernel(k):
    """CPU: the synthetic stats.  Every row has its own delta and variance, |delta|^2 <= var / 4, var
    spreads over [0.25, 16], a row's block pairs all differ.  Sensitivity on the float64 reference
    (N = 256, per channel, with bias, both consumers): the last row's last pair replaced by the pair
    before it -- at K / 64 = 1 the row before's, at M = 1 the NaN frame -- moves most of the last
    row's outputs past the bound, at every M of the test with M % 256 odd where K / 64 is odd; two
    rows' rowinfo swapped moves most of both rows; mu0 + 3 delta lies more than one ulp from
    float32(mu0 + delta) in every row."""
    st, p, n = R.lnf_stats(k), R.problem(k), 256
    nb, m_all = st.nblk, R.MAXM
    assert len(np.unique(st.delta)) == m_all and len(np.unique(st.var)) == m_all
    assert np.all(st.delta ** 2 <= st.var / 4)
    assert 0.24 <= st.var.min() < 0.3 and 13 < st.var.max() <= 16.1
    if nb > 1:
        for j in (0, 1):
            srt = np.sort(st.stats[..., j], 1)
            assert np.all(srt[:, 1:] != srt[:, :-1])
    ref32 = (st.mu0.astype(np.float64) + st.delta).astype(np.float32)
    three = st.mu0.astype(np.float64) + 3 * st.delta
    assert np.all(np.abs(three - ref32) > np.spacing(np.abs(ref32)))
    gw, bw = R.lnf_consts(k, n)
    print()
    for act in (False, True):
        y, e = R.lnf_consumer_ref(p, (st.delta, st.var, st.rstd), m_all, n, gw, bw, p.bias, act)
        assert np.isfinite(_f16_of(y)).all()
        sw = np.arange(m_all)
        sw[[0, 1]] = [1, 0]
        y_sw, _ = R.lnf_consumer_ref(p, tuple(x[sw] for x in (st.delta, st.var, st.rstd)), m_all, n, gw, bw, p.bias, act)
        share = _mutated_share(y[:2], e[:2], y_sw[:2])
        assert share > 0.5, f"rowinfo of rows 0, 1 swapped moves {share:.2f} of their outputs"
        if nb % 2 == 0:
            continue
        for m in (m for m in MS if m % 2):
            mut = np.full((m + 1, nb, 2), np.nan, np.float32)       # row 0: the frame before the stats
            mut[1:] = st.stats[:m]
            mut.reshape(-1, 2)[-1] = mut.reshape(-1, 2)[-2]
            y_mut, _ = R.lnf_consumer_ref(p, tuple(x[1:] for x in st.rowinfo(mut)), m, n, gw, bw, p.bias, act)
            share = _mutated_share(y[m - 1], e[m - 1], y_mut[m - 1])
            print(f"  [stale last pair] K={k} M={m} {'GELU' if act else 'BIAS'}_LNF: {share:.3f} of the last row moves")
            assert share > 0.5, f"K={k} M={m}: the stale last pair moves only {share:.2f} of the last row"


@pytest.mark.parametrize("kg", ODD_KG, ids=_kg_id)
def test_gated_inputs_pin_the_kernel(kg):
    """CPU: the gated-MLP inputs (A rows 5 and 8 times 4 at K = 64) hold gate values past +20 and
    past -20 and gates that are exactly 0, all within the first 525 rows; the scaled sums stay below
    2^24 quanta (exact in fp32), |g u| and silu(g) u stay finite in fp16."""
    p = R.problem(*kg)
    assert np.array_equal(R.gated_a(p).astype(np.float64)[list(R.GATED_ROWS)],
                          p.a.astype(np.float64)[list(R.GATED_ROWS)] * R.gated_scale(p.k))
    for n in GATED_NS:
        g, u, y, acc = R.gated_ref(p, n)
        m = MS[-1]
        assert g[:m].max() > 20 and g[:m].min() < -20 and (g[:m] == 0).any()
        assert np.abs(acc).max() < 2 ** 24
        assert np.abs(g * u).max() < 65504 and np.isfinite(y).all() and np.isfinite(_f16_of(y)).all()


# ------------------------------------------------------------------------------------------ GPU
def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


class _Dev:
    """Device copies of one problem's weights for columns [c0, c0 + n)."""

    def __init__(self, p, n, dev, c0=0):
        from samq import ops
        self.w = ops.w4_repack(_t(p.qweight[:, c0:c0 + n], dev))
        self.sc = _t(p.scales[..., c0:c0 + n], dev)
        self.qz = _t(p.qzeros[:, c0 // 8:(c0 + n) // 8], dev)
        self.bias = _t(p.bias[c0:c0 + n], dev)


_DEV = {}


def _dev(p, n, dev, c0=0):
    key = (p.k, p.group, n, c0)
    if key not in _DEV:
        _DEV[key] = _Dev(p, n, dev, c0)
    return _DEV[key]


def _a_window(a, dev):
    """a as a column window of a wider buffer (lda = K + 48, 16 bytes in) filled with NaN."""
    m, k = a.shape
    big = torch.full((m, k + 48), float("nan"), dtype=torch.float16, device=dev)
    win = big[:, 8:8 + k]
    win.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return win


def _rows(dtype, m, width, dev):
    """Rows [3, 3 + m) of a buffer 6 rows taller filled with a sentinel: NaN (fp32), 60000 (fp16)."""
    fill = F16_SENTINEL if dtype == torch.float16 else float("nan")
    big = torch.full((m + 6,) + tuple(width), fill, dtype=dtype, device=dev)
    return big, big[3:3 + m]


def _stats_frame(m, nb, dev):
    """The consumer's stats: rows [3, 3 + m) of an (m + 6) x nb x 2 NaN buffer -- NaN three rows deep
    on both sides -- that starts one pair into its allocation where 3 nb is odd, so that stats stays
    16-byte aligned as every allocation of its own is.  Returns (allocation, stats, the float range
    of the m rows in the allocation)."""
    pad = 2 * ((3 * nb) % 2)
    flat = torch.full((pad + (m + 6) * nb * 2,), float("nan"), dtype=torch.float32, device=dev)
    stats = flat[pad:].view(m + 6, nb, 2)[3:3 + m]
    assert stats.data_ptr() % 16 == 0
    return flat, stats, (pad + 3 * nb * 2, pad + (3 + m) * nb * 2)


def _stats_frame_untouched(flat, span, what):
    ok = torch.isnan(flat)
    ok[span[0]:span[1]] = True
    assert bool(ok.all()), f"{what}: the NaN frame of stats was written"


def _is_sentinel(x):
    return (x == F16_SENTINEL) if x.dtype == torch.float16 else torch.isnan(x)


def _rows_untouched(big, m, what, cols=None):
    """Everything outside rows [3, 3 + m) (and, cols = (c0, n): outside those columns) holds the sentinel."""
    ok = _is_sentinel(big)
    if cols is None:
        ok[3:3 + m] = True
    else:
        ok[3:3 + m, cols[0]:cols[0] + cols[1]] = True
    bad = int((~ok).sum())
    assert bad == 0, f"{what}: {bad} elements outside the M rows were written"


def _gs(p):
    return p.group or -1


def _check_producer(tag, p, pr, m, n, bigs, views):
    (big_c, big_a, big_s, big_m), (c, aout, stats, mu) = bigs, views
    dev = c.device
    nbad = int((c[:, :n] != _t(p.ref("resadd")[:m, :n], dev)).sum())
    assert nbad == 0, f"{tag}: {nbad} of {m * n} residual outputs differ"
    nbad = int((aout != _t(pr.aout[:m], dev)).sum())
    assert nbad == 0, f"{tag}: {nbad} of {m * n} fold operands differ from float16((x - mu) gamma)"
    nbad = pr.stats_violations(stats.cpu().numpy(), m)
    assert nbad == 0, f"{tag}: {nbad} of {2 * m * (n // 64)} block sums outside the summation bound"
    assert torch.equal(mu, _t(pr.mu[:m], dev)), f"{tag}: the producer changed mu"
    for big, what in ((big_a, "aout"), (big_s, "stats"), (big_m, "mu")):
        _rows_untouched(big, m, f"{tag} {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("kg", ODD_KG, ids=_kg_id)
@pytest.mark.parametrize("cfg", CFGS)
def test_lnf_producer(cuda, cfg, kg):
    """RESADD_LNF through ops.w4a16_gemm_lnf, N = 256 and 768, every M of LNF_MS: the residual equals
    the float64 sum bit for bit, aout equals float16((x_new - mu_p) gamma) (one rounding) bit for
    bit, EVERY block pair stats[r, b] lies within 6 * 2^-24 sum|d| (s1) and 8 * 2^-24 S2 (s2) of
    the float64 sums over its 64 columns, mu is unchanged, and the rows around the M rows of C,
    aout, stats and mu still hold their sentinel."""
    from samq import ops
    p = R.problem(*kg)
    for n in NS:
        pr, dv = R.lnf_producer(*kg, n), _dev(p, n, cuda)
        gamma = _t(pr.gamma, cuda)
        for m in MS:
            bigs, views = zip(_rows(torch.float32, m, (n,), cuda), _rows(torch.float16, m, (n,), cuda),
                              _rows(torch.float32, m, (n // 64, 2), cuda), _rows(torch.float32, m, (), cuda))
            c, aout, stats, mu = views
            c.copy_(_t(p.res_f32[:m, :n], cuda))
            mu.copy_(_t(pr.mu[:m], cuda))
            ops.w4a16_gemm_lnf(_t(p.a[:m], cuda), dv.w, dv.sc, dv.qz, dv.bias, n, _gs(p), ops.EPI_RESADD_LNF, c, stats,
                               mu, gamma=gamma, aout=aout, cfg=cfg)
            tag = f"cfg {cfg} RESADD_LNF {m}x{n}x{p.k} g{p.group}"
            _check_producer(tag, p, pr, m, n, bigs, views)
            _rows_untouched(bigs[0], m, f"{tag} C")


_NEED = {"lnf": 0.0, "silu": 0.0}      # run maxima: E needed / E, e_rel needed


def _check_consumer(tag, p, st, m, n, gw, bw, bias, act, out):
    """out (m, n) fp16 against the float64 reference; returns need / E."""
    y, e = R.lnf_consumer_ref(p, (st.delta, st.var, st.rstd), m, n, gw, bw, bias, act)
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), f"{tag}: {int(np.isnan(got).sum())} NaN outputs (a pair read outside the rows' stats)"
    bad, need = R.check_interval_f16(got, y, e)
    _NEED["lnf"] = max(_NEED["lnf"], need)
    rows = np.nonzero(~((got >= _f16_of(y - e)) & (got <= _f16_of(y + e))).all(1))[0]
    assert bad == 0, (f"{tag}: {bad} of {got.size} outputs outside [f16(y - E), f16(y + E)], rows {rows[:8].tolist()}; "
                      f"first: got {got[rows[0]][:4].tolist()} expected {_f16_of(y)[rows[0]][:4].tolist()}")
    return need


def _check_mu_once(tag, st, m, mu):
    ref = (st.mu0[:m].astype(np.float64) + st.delta[:m]).astype(np.float32)
    d = np.abs(mu.cpu().numpy().astype(np.float64) - ref)
    nbad = int((~(d <= np.spacing(np.abs(ref)))).sum())
    assert nbad == 0, f"{tag}: mu differs from float32(mu0 + delta) by more than one ulp in {nbad} of {m} rows"


@pytest.mark.gpu
@pytest.mark.parametrize("kg", CONS_KG, ids=_kg_id)
@pytest.mark.parametrize("cfg", CFGS)
def test_lnf_consumers(cuda, cfg, kg):
    """BIAS_LNF and GELU_LNF through ops.w4a16_gemm_lnf on the synthetic stats, A = problem.a[:M],
    N = 256 and 768, every M of LNF_MS (K / 64 and the rows left in the last row tile both odd at
    K = 64, 192, 320 with M = 1, 31, 33, 255, 257, 525: the rows' pairs end 8 bytes past a 16-byte
    boundary; K = 128, 256 are the controls), and once without bias.  Every output lies within
    [f16(y - E), f16(y + E)] of the float64 y = rstd (acc s - delta gw) + bw + bias,
    E = (K / 64 + 7) 2^-24 (|rstd| (|acc s| + |delta gw|) + |bw + bias|) (_w4a16_ref.lnf_c; GELU:
    1.13 E + 6.6e-7); no output is NaN although NaN surrounds the M rows of stats; mu[:M] is
    float32(mu0 + delta) to one ulp (column tile 0 alone adds delta: once, not three times at
    N = 768); out and mu rows >= M hold their sentinel; stats and A are unchanged.

    Measured on gfx950 over the 22 cases (6.4e7 outputs, no violation): the output that needed most
    needed 0.191 of the derived E.  Before lnf_rowinfo_wg read the last pair of an odd tail from
    global memory, every K = 64, 192, 320 case failed at its first odd M (M = 1: all 256 outputs NaN
    at K = 64, 253 of 256 off at K = 192) and K = 128, 256 passed."""
    from samq import ops
    p, st = R.problem(*kg), R.lnf_stats(kg[0])
    nb = st.nblk
    print()
    for n in NS:
        dv = _dev(p, n, cuda)
        gw, bw = R.lnf_consts(p.k, n)
        gw_d, bw_d = _t(gw, cuda), _t(bw, cuda)
        runs = [(epi, m, True) for epi in ("BIAS_LNF", "GELU_LNF") for m in MS]
        if n == NS[0]:
            runs.append(("BIAS_LNF", MS[-1], False))
        need = 0.0
        for epi, m, with_bias in runs:
            big_o, out = _rows(torch.float16, m, (n,), cuda)
            flat_s, stats, span = _stats_frame(m, nb, cuda)
            big_m, mu = _rows(torch.float32, m, (), cuda)
            stats.copy_(_t(st.stats[:m], cuda))
            mu.copy_(_t(st.mu0[:m], cuda))
            a = _t(p.a[:m], cuda)
            ops.w4a16_gemm_lnf(a, dv.w, dv.sc, dv.qz, dv.bias if with_bias else None, n, _gs(p), getattr(ops, "EPI_" + epi),
                               out, stats, mu, gw=gw_d, bw=bw_d, eps=R.LNF_EPS, cfg=cfg)
            tag = f"cfg {cfg} {epi} {m}x{n}x{p.k} g{p.group}" + ("" if with_bias else " no bias")
            need = max(need, _check_consumer(tag, p, st, m, n, gw, bw, p.bias if with_bias else None, epi == "GELU_LNF",
                                             out))
            _check_mu_once(tag, st, m, mu)
            for big, what in ((big_o, "out"), (big_m, "mu")):
                _rows_untouched(big, m, f"{tag} {what}")
            _stats_frame_untouched(flat_s, span, tag)
            assert torch.equal(stats, _t(st.stats[:m], cuda)), f"{tag}: stats changed"
            assert torch.equal(a, _t(p.a[:m], cuda)), f"{tag}: A changed"
        print(f"  [lnf E] cfg {cfg} K={p.k} g{p.group} N={n}: largest E needed {need:.3f} of the derived E "
              f"(c = {R.lnf_c(nb)}); run maximum {_NEED['lnf']:.3f}")


def _lnf_direct(a, lda, dv, bias, c, ldc, m, n, k, gs, epi, cfg, gamma, gw, bw, stats, mu, aout):
    from samq import _lib, ops
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    _lib.check(_lib.load().samq_w4a16_gemm_lnf(
        ptr(a), lda, ptr(dv.w), ptr(dv.sc), ptr(dv.qz), ptr(bias), ptr(c), ldc, m, n, k, gs, epi, cfg, ptr(gamma),
        ptr(gw), ptr(bw), ptr(stats), ptr(mu), ptr(aout), R.LNF_EPS, ops._stream()), "w4a16_gemm_lnf")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_lnf_strides(cuda, cfg):
    """samq_w4a16_gemm_lnf called directly with the strides the Python wrapper never passes: the
    producer with ldc = N + 8 (C a window 16 bytes into its rows), the consumer with lda = K + 48 (A
    a window of a NaN-filled buffer) and ldc = N + 8.  The checks of the two tests above, and the
    frame columns keep their sentinel.  K = 192, N = 768, M = 525 and 33."""
    from samq import ops
    k, n = 192, 768
    for group in (0, 64):
        p, st = R.problem(k, group), R.lnf_stats(k)
        pr, dv = R.lnf_producer(k, group, n), _dev(p, n, cuda)
        gw, bw = R.lnf_consts(k, n)
        for m in (525, 33):
            tag = f"cfg {cfg} {m}x{n}x{k} g{group} strided"
            bigs, views = zip(_rows(torch.float32, m, (n + 8,), cuda), _rows(torch.float16, m, (n,), cuda),
                              _rows(torch.float32, m, (n // 64, 2), cuda), _rows(torch.float32, m, (), cuda))
            c = views[0][:, 4:4 + n]
            c.copy_(_t(p.res_f32[:m, :n], cuda))
            views[3].copy_(_t(pr.mu[:m], cuda))
            _lnf_direct(_t(p.a[:m], cuda), k, dv, dv.bias, c, n + 8, m, n, k, _gs(p), ops.EPI_RESADD_LNF, cfg,
                        _t(pr.gamma, cuda), None, None, views[2], views[3], views[1])
            _check_producer(tag + " RESADD_LNF", p, pr, m, n, bigs, (c,) + views[1:])
            _rows_untouched(bigs[0], m, tag + " RESADD_LNF C", cols=(4, n))

            a = _a_window(p.a[:m], cuda)
            for epi in ("BIAS_LNF", "GELU_LNF"):
                big_o, rows_o = _rows(torch.float16, m, (n + 8,), cuda)
                out = rows_o[:, 8:8 + n]
                flat_s, stats, span = _stats_frame(m, st.nblk, cuda)
                big_m, mu = _rows(torch.float32, m, (), cuda)
                stats.copy_(_t(st.stats[:m], cuda))
                mu.copy_(_t(st.mu0[:m], cuda))
                _lnf_direct(a, k + 48, dv, dv.bias, out, n + 8, m, n, k, _gs(p), getattr(ops, "EPI_" + epi), cfg, None,
                            _t(gw, cuda), _t(bw, cuda), stats, mu, None)
                _check_consumer(f"{tag} {epi}", p, st, m, n, gw, bw, p.bias, epi == "GELU_LNF", out)
                _check_mu_once(f"{tag} {epi}", st, m, mu)
                _rows_untouched(big_o, m, f"{tag} {epi} out", cols=(8, n))
                _rows_untouched(big_m, m, f"{tag} {epi} mu")
                _stats_frame_untouched(flat_s, span, f"{tag} {epi}")
                assert torch.equal(stats, _t(st.stats[:m], cuda)) and torch.equal(a, _t(p.a[:m], cuda))


@pytest.mark.gpu
@pytest.mark.parametrize("group", [0, 64])
@pytest.mark.parametrize("c", [256, 768])
@pytest.mark.parametrize("cfg", CFGS)
def test_lnf_small_chain(cuda, cfg, c, group):
    """Producer (K = 192 -> N = C) then consumer (K = C -> N = 256) at M = 525 against the float64
    chain residual -> LayerNorm -> GEMM (-> GELU) built from the exact y_resadd: ties the producer's
    stats layout to the consumer's.  gamma is the producer's ({1, 2, 4}), beta a multiple of 2^-4, so
    gw = gamma . W and bw = beta . W are exact in fp32.  The interval check with E of the consumer
    test plus the fp16 rounding of aout, rstd 2^-11 sum_k |aout_k w_kn s_n|; afterwards mu equals the
    true row mean within 6 * 2^-24 sum|d| / K."""
    from samq import ops
    m, n2 = 525, 256
    p1, p2 = R.problem(192, group), R.problem(c, group)
    pr, dv1, dv2 = R.lnf_producer(192, group, c), _dev(p1, c, cuda), _dev(p2, n2, cuda)
    rng = np.random.Generator(np.random.PCG64([c, group, 17]))
    beta = rng.integers(-16, 17, c) / 16.0
    w = p2.w_int(p2.q, p2.zp, p2.d)[:, :n2] * 2.0 ** p2.e_col[None, :n2]          # the real weights, float64
    gamma = pr.gamma.astype(np.float64)
    gw, bw = (gamma @ w).astype(np.float32), (beta @ w).astype(np.float32)
    assert np.array_equal(gw.astype(np.float64), gamma @ w) and np.array_equal(bw.astype(np.float64), beta @ w)
    bias = p2.bias.astype(np.float64)[:n2]
    # float64 chain
    x = pr.x[:m]
    mean, var = x.mean(1), x.var(1)
    rstd = 1.0 / np.sqrt(var + R.LNF_EPS)
    ln = (x - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :]
    y_chain = ln @ w + bias[None, :]
    delta = mean - pr.mu[:m].astype(np.float64)
    mat = pr.aout64[:m] @ w
    e_a16 = rstd[:, None] * 2.0 ** -11 * (np.abs(pr.aout64[:m]) @ np.abs(w))

    c32, aout, stats, mu = (_rows(torch.float32, m, (c,), cuda), _rows(torch.float16, m, (c,), cuda),
                            _rows(torch.float32, m, (c // 64, 2), cuda), _rows(torch.float32, m, (), cuda))
    c32[1].copy_(_t(p1.res_f32[:m, :c], cuda))
    mu[1].copy_(_t(pr.mu[:m], cuda))
    ops.w4a16_gemm_lnf(_t(p1.a[:m], cuda), dv1.w, dv1.sc, dv1.qz, dv1.bias, c, _gs(p1), ops.EPI_RESADD_LNF, c32[1],
                       stats[1], mu[1], gamma=_t(pr.gamma, cuda), aout=aout[1], cfg=cfg)
    print()
    for epi in ("BIAS_LNF", "GELU_LNF"):
        tag = f"cfg {cfg} chain C={c} g{group} {epi}"
        big_o, out = _rows(torch.float16, m, (n2,), cuda)
        mu2 = mu[1].clone()
        ops.w4a16_gemm_lnf(aout[1], dv2.w, dv2.sc, dv2.qz, dv2.bias, n2, _gs(p2), getattr(ops, "EPI_" + epi), out,
                           stats[1], mu2, gw=_t(gw, cuda), bw=_t(bw, cuda), eps=R.LNF_EPS, cfg=cfg)
        y, e = R.lnf_consumer_ref(p2, (delta, var, rstd), m, n2, gw, bw, p2.bias, epi == "GELU_LNF", mat=mat)
        ref = R.gelu(y_chain) if epi == "GELU_LNF" else y_chain
        assert np.abs(y - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())    # the fold algebra, float64
        got = out.cpu().numpy()
        e = e + (1.13 if epi == "GELU_LNF" else 1.0) * e_a16
        bad, need = R.check_interval_f16(got, ref, e)
        print(f"  [chain] {tag}: largest bound needed {need:.3f} of E + the aout rounding term")
        assert bad == 0, f"{tag}: {bad} of {got.size} outputs outside the interval"
        d_mu = np.abs(mu2.cpu().numpy().astype(np.float64) - mean)
        lim = 6 * R.U24 * np.abs(pr.d[:m]).sum(1) / c
        assert np.all(d_mu <= lim), f"{tag}: mu off the row mean by up to {float((d_mu / lim).max()):.2f} of the bound"
        _rows_untouched(big_o, m, tag + " out")
    for big, what in ((c32[0], "C"), (aout[0], "aout"), (stats[0], "stats"), (mu[0], "mu")):
        _rows_untouched(big, m, f"cfg {cfg} chain C={c} g{group} {what}")


@pytest.mark.gpu
@pytest.mark.parametrize("kg", ODD_KG, ids=_kg_id)
def test_gated_mlp(cuda, kg):
    """ops.w4_interleave32 and ops.w4a16_gated_mlp, gate = columns [0, N), up = columns [N, 2N) of a
    problem, N = 128 and 384 (2N = 256, 768), every M of LNF_MS, A a column window (lda = K + 48) of
    a NaN-filled buffer, out rows [3, 3 + M) of a sentinel buffer.  The interleaved words, scales and
    qzeros equal a numpy gather written from the layout comment, bit for bit.  Every output lies
    within [f16(y - E), f16(y + E)] of the float64 y = g / (1 + exp(-g)) u, E = e_rel |y|; the largest
    e_rel any output needed is printed.  Rows >= M keep the sentinel.

    e_rel: __expf and the fp32 division are hardware approximations without a documented bound in
    csrc/common.h, so it is measured.  On gfx950, against e_rel = 2^-16, the output that needed most
    needed 2.95e-7 = 2^-21.7 (K = 320, group 128, N = 384; below the 2^-18 that would ask for an
    explanation); the bound is 4 times that, rounded up to a power of two: 2^-19.  A layout or row
    error is off by the size of the value itself."""
    from samq import ops
    p = R.problem(*kg)
    k, a_all = p.k, R.gated_a(p)
    print()
    for n in GATED_NS:
        gd, ud = _dev(p, n, cuda), _dev(p, n, cuda, c0=n)
        ng = p.ng if p.group else 1
        sc_g, sc_u = gd.sc.reshape(ng, n), ud.sc.reshape(ng, n)
        w2, s2, z2 = ops.w4_interleave32(gd.w, ud.w, sc_g, sc_u, gd.qz, ud.qz, n)
        wr, sr, zr = R.interleave32_ref(R.repack_ref(p.qweight[:, :n], 1), R.repack_ref(p.qweight[:, n:2 * n], 1),
                                        p.scales.reshape(ng, -1)[:, :n], p.scales.reshape(ng, -1)[:, n:2 * n],
                                        p.qzeros[:, :n // 8], p.qzeros[:, n // 8:n // 4], k)
        assert np.array_equal(w2.cpu().numpy(), wr), f"K={k} N={n}: interleaved words differ"
        assert np.array_equal(s2.cpu().numpy().view(np.uint16), np.ascontiguousarray(sr).view(np.uint16))
        assert np.array_equal(z2.cpu().numpy(), zr), f"K={k} N={n}: interleaved qzeros differ"
        _, _, y_all, _ = R.gated_ref(p, n)
        need_n = 0.0
        for m in MS:
            tag = f"gated MLP {m}x{n}x{k} g{p.group}"
            a = _a_window(a_all[:m], cuda)
            big, out = _rows(torch.float16, m, (n,), cuda)
            ops.w4a16_gated_mlp(a, w2, s2, z2, n, _gs(p), out=out)
            got, y = out.cpu().numpy(), y_all[:m]
            bad, need = R.check_interval_f16(got, y, np.maximum(SILU_E_REL * np.abs(y), 1e-300))
            need_n = max(need_n, need * SILU_E_REL)
            assert bad == 0, f"{tag}: {bad} of {got.size} outputs outside [f16(y - E), f16(y + E)], e_rel = {SILU_E_REL:.2e}"
            _rows_untouched(big, m, tag)
        _NEED["silu"] = max(_NEED["silu"], need_n)
        print(f"  [silu e_rel] K={k} g{p.group} N={n}: largest e_rel needed {need_n:.3e} (2^{np.log2(max(need_n, 1e-30)):.2f}); "
              f"run maximum {_NEED['silu']:.3e}")


@pytest.mark.gpu
def test_lnf_and_gated_refusals_before_any_write(cuda):
    """Each of these raises and writes nothing into its sentinel outputs: the plain GEMM entry with a
    fold epilogue or the internal SILU_MUL value; samq_w4a16_gemm_lnf with a non-fold epilogue, with
    cfg = 0 below M = 8192 (the automatic pick is no ping-pong config there) and with N % 256 != 0;
    samq_w4a16_gated_mlp with 2N % 256 != 0."""
    from samq import _lib, ops
    k, m = 192, 141
    p = R.problem(k)
    a = _a_window(p.a[:m], cuda)

    def bufs(n):
        out = {dt: _rows(dt, m, (n,), cuda) for dt in (torch.float16, torch.float32)}
        aout, stats, mu = _rows(torch.float16, m, (n,), cuda), _rows(torch.float32, m, (max(n, k) // 64, 2), cuda), \
            _rows(torch.float32, m, (), cuda)
        return out, aout, stats, mu

    def clean(what, *bigs):
        torch.cuda.synchronize()
        for big in bigs:
            assert bool(_is_sentinel(big).all()), f"{what}: the refused call wrote"

    n = 256
    dv = _dev(p, n, cuda)
    for epi in (ops.EPI_RESADD_LNF, ops.EPI_BIAS_LNF, ops.EPI_GELU_LNF, 10):       # 10: SAMQ_EPI_SILU_MUL
        for cfg in (0, 57, 64):
            out, *_ = bufs(n)
            for dt in out:
                with pytest.raises(AssertionError):
                    ops.w4a16_gemm(a, dv.w, dv.sc, dv.qz, dv.bias, n, -1, epi, out=out[dt][1], cfg=cfg)
                clean(f"w4a16_gemm epilogue {epi} cfg {cfg}", out[dt][0])
    gam, gw, bw = torch.ones(n, device=cuda), torch.ones(n, device=cuda), torch.zeros(n, device=cuda)
    ac = _t(p.a[:m], cuda)

    def lnf(n_, epi, cfg, dv_, out, aout, stats, mu):
        ops.w4a16_gemm_lnf(ac, dv_.w, dv_.sc, dv_.qz, dv_.bias, n_, -1, epi, out, stats, mu, gamma=gam[:n_], aout=aout,
                           gw=gw[:n_], bw=bw[:n_], cfg=cfg)

    for epi, dt in ((ops.EPI_BIAS, torch.float16), (ops.EPI_BIAS_GELU, torch.float16), (ops.EPI_F32, torch.float16),
                    (ops.EPI_RESADD_F32, torch.float16), (10, torch.float16)):
        out, aout, stats, mu = bufs(n)
        with pytest.raises(AssertionError):
            lnf(n, epi, 57, dv, out[dt][1], aout[1], stats[1], mu[1])
        clean(f"w4a16_gemm_lnf epilogue {epi}", out[dt][0], aout[0], stats[0], mu[0])
    for epi, dt in ((ops.EPI_RESADD_LNF, torch.float32), (ops.EPI_BIAS_LNF, torch.float16), (ops.EPI_GELU_LNF, torch.float16)):
        out, aout, stats, mu = bufs(n)
        with pytest.raises(NotImplementedError):
            lnf(n, epi, 0, dv, out[dt][1], aout[1], stats[1], mu[1])
        clean(f"w4a16_gemm_lnf epilogue {epi} cfg 0 at M = {m}", out[dt][0], aout[0], stats[0], mu[0])
        dv128 = _dev(p, 128, cuda)
        for cfg in CFGS:
            out, aout, stats, mu = bufs(128)
            with pytest.raises(AssertionError):
                lnf(128, epi, cfg, dv128, out[dt][1], aout[1], stats[1], mu[1])
            clean(f"w4a16_gemm_lnf epilogue {epi} N = 128", out[dt][0], aout[0], stats[0], mu[0])
    # gated MLP: N = 64 and N = 192 (2N = 128, 384)
    for n in (64, 192):
        gd, ud = _dev(p, n, cuda), _dev(p, n, cuda, c0=n)
        w2, s2, z2 = ops.w4_interleave32(gd.w, ud.w, gd.sc.reshape(1, n), ud.sc.reshape(1, n), gd.qz, ud.qz, n)
        big, out = _rows(torch.float16, m, (n,), cuda)
        with pytest.raises(AssertionError):
            ops.w4a16_gated_mlp(a, w2, s2, z2, n, -1, out=out)
        with pytest.raises(AssertionError):
            _lib.check(_lib.load().samq_w4a16_gated_mlp(a.data_ptr(), a.stride(0), w2.data_ptr(), s2.data_ptr(), z2.data_ptr(),
                                                        out.data_ptr(), n, m, 2 * n, k, -1, ops._stream()))
        clean(f"w4a16_gated_mlp N = {n}", big)
