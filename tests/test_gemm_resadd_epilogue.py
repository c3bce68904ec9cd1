"""The fp32 residual epilogue (SAMQ_EPI_RESADD_F32, ``C += y``) of the W4A16 and W4A8 GEMMs.

The kernels read the old residual of a whole batch of 16- or 32-row slices into registers before
the batch's first store, and the next batch's before this batch's stores (csrc/common.h
``res_load``).  What can go wrong there is an index: a prefetched chunk added to another chunk's
sums (wrong slice, wrong batch parity, wrong row when the tile is cut by M), a row at or past M
read or written, or a kernel that starts reading C where the epilogue is a plain store.

Inputs come from ``_w4a16_ref.problem`` / ``_i8_ref.problem``: every operation is exact in any
order (``|acc + bias + residual| < 2^21`` quanta for W4A16, so adding ``y`` twice still stays
below 2^24; the W4A8 bound is asserted below), hence a correct kernel equals the float64 reference
bit for bit and every comparison here is an equality of bit patterns.

Shapes: M in {1, 255, 277} -- 277 puts one full 16-row slice, one slice of 5 rows and slices wholly
past M into the second 256-row tile; 255 ends a tile one row short; N = 256 and 512 (320 and 640 on
the 320-column tiles of config 29): one and two column tiles; K = 64 and 192 (one K tile and three;
the W4A8 kernels take 128-deep K tiles, so K = 128 and 384 there).

C is a window (``ldc = N + 16``) of a larger buffer: three sentinel rows above, sentinel columns on
both sides, below the M rows NaN rows inside the window's columns down to the end of the last
256-row tile, then three sentinel rows.  After every launch the WHOLE buffer is compared bit for
bit with the expected one, which shows at once that the frame and the NaN rows are untouched and
that no NaN row was read into an output.
"""
import numpy as np
import pytest
import torch

import _i8_ref as RI
import _w4a16_ref as RW

SENTINEL = -7777.25            # |y| < 512
MS = (1, 255, 277)
# every W4A16 config family with its own RESADD_F32 code: 0 the automatic pick (64 x 64 v3 tiles at
# these M), 1 and 5 the direct scalar form, 22 / 29 the v3 epilogue (one-image lanes), 57 / 64 the
# product ping-pong pair (32x32x16 / 16x16x32 staging), 62 its 16-row slices of 128 columns, 107 /
# 108 the persistent forms and 110 the early scale / bias loads
W4A16_CFGS = (0, 1, 5, 22, 29, 57, 62, 64, 107, 108, 110)
W4A16_GROUPED = ((57, 192, 64), (64, 192, 64), (22, 192, 64))          # (cfg, K, groupsize)
# W4A8: 85 / 86 the ping-pong kernel (86 with and without the producer's row sums), 0 the automatic
# pick and 81 / 82 the 3-slot kernel with 256- and 128-row tiles; grouped: 0 and 83
W4A8_CFGS = (0, 81, 82, 85, 86)
W4A8_GROUPED = ((0, 384, 128), (83, 384, 128))


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _bits(x):
    return x.contiguous().view(torch.int32)


class _Frame:
    """The buffer around an M x N window of C (see the module docstring)."""

    def __init__(self, m, n, dev):
        self.m, self.n = m, n
        mp = -(-m // 256) * 256
        self.big = torch.full((3 + mp + 3, n + 16), SENTINEL, dtype=torch.float32, device=dev)
        self.big[3 + m:3 + mp, 8:8 + n] = float("nan")
        self.win = self.big[3:3 + m, 8:8 + n]
        assert self.win.data_ptr() % 16 == 0 and self.big.stride(0) % 4 == 0

    def check(self, want, what):
        """Bitwise: the window equals ``want`` and everything else is as it was."""
        exp = _Frame(self.m, self.n, self.big.device)
        exp.win.copy_(want)
        diff = _bits(self.big) != _bits(exp.big)
        inside = torch.zeros_like(diff)
        inside[3:3 + self.m, 8:8 + self.n] = True
        nan_rows = torch.isnan(exp.big)
        n_out = int((diff & inside).sum())
        n_nan_out = int(torch.isnan(self.win).sum())
        n_nan_rows = int((diff & nan_rows & ~inside).sum())
        n_frame = int((diff & ~inside & ~nan_rows).sum())
        assert n_nan_out == 0, f"{what}: {n_nan_out} NaN in rows below M (a row at or past M was read)"
        assert n_out == 0, f"{what}: {n_out} of {self.m * self.n} outputs differ"
        assert n_nan_rows == 0, f"{what}: {n_nan_rows} elements of the rows at or past M were written"
        assert n_frame == 0, f"{what}: {n_frame} elements of the frame were written"


def _check_resadd(launch, epi_resadd, epi_f32, y64, r64, m, n, dev, what):
    """launch(epi, window) runs the GEMM in place.  y64 / r64: the float64 y and residual, exact."""
    y, r = y64[:m, :n], r64[:m, :n]
    x0 = _t(r.astype(np.float32), dev)
    once, twice = (r + y).astype(np.float32), (r + 2 * y).astype(np.float32)
    assert np.array_equal(once.astype(np.float64), r + y) and np.array_equal(twice.astype(np.float64), r + 2 * y)
    f = _Frame(m, n, dev)
    f.win.copy_(x0)
    launch(epi_resadd, f.win)
    f.check(_t(once, dev), f"{what} RESADD_F32")
    launch(epi_resadd, f.win)                      # a second launch in place: x + 2 y
    f.check(_t(twice, dev), f"{what} RESADD_F32 twice")
    f = _Frame(m, n, dev)
    f.win.fill_(float("nan"))                      # a plain store never reads C
    launch(epi_f32, f.win)
    f.check(_t(y.astype(np.float32), dev), f"{what} F32 over NaN")


def _ns(cfg):
    return (320, 640) if cfg == 29 else (256, 512)


# ------------------------------------------------------------------------------------------ W4A16
def _w4a16_case(cuda, cfg, k, group, m, n):
    from samq import ops
    p = RW.problem(k, group)
    assert np.abs(p.acc[:m, :n] * 2 + p.b_int[None, :n] * 2 + p.r_int[:m, :n]).max() < 2 ** 24
    w = ops.w4_repack(_t(p.qweight[:, :n], cuda))
    sc, qz, bias = _t(p.scales[..., :n], cuda), _t(p.qzeros[:, :n // 8], cuda), _t(p.bias[:n], cuda)
    abig = torch.full((m, k + 48), float("nan"), dtype=torch.float16, device=cuda)   # one stray read poisons C
    a = abig[:, 8:8 + k]
    a.copy_(_t(p.a[:m], cuda))

    def launch(epi, out):
        ops.w4a16_gemm(a, w, sc, qz, bias, n, group or -1, epi, out=out, cfg=cfg)

    tag = f"w4a16 cfg {cfg} {m}x{n}x{k}" + (f" g{group}" if group else "")
    _check_resadd(launch, ops.EPI_RESADD_F32, ops.EPI_F32, p.y, p.r_int * p.qn[None, :], m, n, cuda, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (64, 192))
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("cfg", W4A16_CFGS)
def test_w4a16_resadd_batched(cuda, cfg, m, k):
    """Per-channel weights, every config of W4A16_CFGS at M x {N} x K of the module docstring: one
    RESADD_F32 launch gives x + y and a second one in place x + 2 y, bit for bit; the frame and the
    NaN rows at and past M are bitwise unchanged and no NaN reaches a row below M; F32 over a
    NaN-filled C gives y (the store path reads nothing)."""
    for n in _ns(cfg):
        _w4a16_case(cuda, cfg, k, 0, m, n)


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("cfg,k,group", W4A16_GROUPED)
def test_w4a16_resadd_batched_grouped(cuda, cfg, k, group, m):
    """The same on grouped weights (three groups of 64): the grouped ping-pong pair and cfg 22."""
    for n in _ns(cfg):
        _w4a16_case(cuda, cfg, k, group, m, n)


# ------------------------------------------------------------------------------------------ W4A8
def _w4a8_case(cuda, cfg, k, group, m, n, with_rowsum):
    from samq import ops
    p = RI.problem("w4g" if group else "w4", k, group)
    csc = p.csc[None, :n]
    y = p.y[:m, :n]
    r = p.res_f32[:m, :n].astype(np.float64)
    assert np.abs((2 * y + r) / csc).max() < 2 ** 24          # x + 2 y is still exact in fp32
    w = ops.w4_repack(_t(p.qweight[:, :n], cuda), layout=3)
    ws, qz, bias = _t(p.wscale[..., :n], cuda).reshape(-1), _t(p.qzeros[:, :n // 8], cuda), _t(p.bias[:n], cuda)
    abig = torch.full((m, k + 48), 99, dtype=torch.int8, device=cuda)
    a = abig[:, 16:16 + k]
    a.copy_(_t(p.a[:m], cuda))
    kw = dict(rowsum=_t(p.rowsum_a[:m], cuda)) if with_rowsum else {}

    def launch(epi, out):
        ops.w4a8_gemm(a, w, ws, qz, n, bias, epi, float(p.a_scale), 0.0, out=out, groupsize=group or -1, cfg=cfg, **kw)

    tag = f"w4a8 cfg {cfg} {m}x{n}x{k}" + (f" g{group}" if group else "") + (" +rowsum" if with_rowsum else "")
    _check_resadd(launch, ops.EPI_RESADD_F32, ops.EPI_F32, p.y, p.res_f32.astype(np.float64), m, n, cuda, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (128, 384))
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("cfg", W4A8_CFGS)
def test_w4a8_resadd_batched(cuda, cfg, m, k):
    """The W4A8 GEMM, per channel: the ping-pong kernel forced (85, 86; 86 also with the producer's
    row sums of A), the automatic pick and the 3-slot kernel (81, 82); K = 128 and 384 (one and three
    128-deep K tiles).  The same checks as for W4A16."""
    for n in (256, 512):
        for with_rowsum in ((False, True) if cfg == 86 else (False,)):
            _w4a8_case(cuda, cfg, k, 0, m, n, with_rowsum)


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("cfg,k,group", W4A8_GROUPED)
def test_w4a8_resadd_batched_grouped(cuda, cfg, k, group, m):
    """The W4A8 GEMM on grouped weights (three groups of 128; float accumulators): the automatic pick
    and cfg 83."""
    for n in (256, 512):
        _w4a8_case(cuda, cfg, k, group, m, n, False)
