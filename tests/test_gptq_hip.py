"""The GPTQ column loop as one HIP launch (``samq_gptq_quant`` / ``ops.gptq_quant``) against the torch loop
(``samq.gptq.column_loop``) run in float64 on the CPU: exact on inputs whose arithmetic is exact, row by
row on the real layer of tests/golden/gptq_layer.npz, and reached from ``GPTQ.fasterquant``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _grid_weight(rows, k, seed):
    """W on a 1/16 grid in [-1, 0.875]; every 32 columns hold -1.0 and 0.875, so every group of every size has
    scale 1.875 / maxq and (maxq 15) zero 8 exactly; about half of the entries are odd multiples of 1/16."""
    w = torch.from_numpy(np.random.default_rng(seed).integers(-16, 15, (rows, k)) / 16.0).float()
    w[:, 0::32] = -1.0
    w[:, 1::32] = 0.875
    return w


def _codes(q, s, z):
    rep = q.shape[1] // s.shape[1]
    return torch.round(q.double() / s.double().repeat_interleave(rep, 1)) + z.double().repeat_interleave(rep, 1)


@pytest.mark.parametrize("maxq", [15, 255])
@pytest.mark.parametrize("gs", [-1, 32, 128, 256])
def test_identity_u_is_rtn(cuda, gs, maxq):
    """U = I: no error moves, the loop is round-to-nearest per group -- bit-equal to ``rtn``, ties included,
    over one full and one ragged slab and (groups of 256) the group slice reaching into the next block."""
    from samq import ops
    from samq.gptq import rtn
    w = _grid_weight(20, 256, 1)
    fake, s, z = rtn(w, gs, 4 if maxq == 15 else 8)
    q, ks, kz, kc = ops.gptq_quant(w.to(cuda), torch.eye(256, device=cuda), gs, maxq)
    assert torch.equal(ks.cpu(), s) and torch.equal(kz.cpu(), z)
    assert torch.equal(q.cpu(), fake)
    assert torch.equal(kc.cpu().double(), _codes(fake, s, z))


def test_sparse_integer_u_exact(cuda):
    """Unit diagonal plus a few small integers: inside a block, across a block edge, two blocks ahead and
    into the last column.  Every product and sum is exact in fp32 and in float64, so both update phases and
    their indexing are pinned bit for bit."""
    from samq import ops
    from samq.gptq import Quantizer, column_loop
    k = 384
    w = _grid_weight(20, k, 2)
    u = torch.eye(k)
    for (r, c), v in {(3, 4): 2., (64, 65): -1., (130, 131): 1., (127, 128): -2., (5, 300): 1., (200, 383): 2.,
                      (382, 383): -1., (255, 256): 1., (0, 127): -1.}.items():
        u[r, c] = v
    rq, rs, rz = column_loop(w.double(), u.double(), Quantizer(4), 128, -1)
    q, s, z, codes = ops.gptq_quant(w.to(cuda), u.to(cuda), -1, 15)
    assert torch.equal(s.cpu().double(), rs) and torch.equal(z.cpu().double(), rz)
    assert torch.equal(q.cpu().double(), rq)
    assert torch.equal(codes.cpu().double(), _codes(rq, rs, rz))
    assert not torch.equal(rq.float(), ops.gptq_quant(w.to(cuda), torch.eye(k, device=cuda), -1, 15)[0].cpu())


def _gptq(golden_dir, device):
    from samq.gptq import GPTQ
    g = np.load(golden_dir / "gptq_layer.npz")
    w = torch.from_numpy(g["w"])
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False).to(device)
    lin.weight.data = w.to(device)
    q = GPTQ(lin)
    for i in range(4):
        q.add_batch(torch.from_numpy(g[f"x{i}"]).to(device))
    return lin, q


@pytest.mark.parametrize("gs,act", [(-1, False), (-1, True), (128, False), (128, True), (32, False), (64, True)])
def test_real_layer_rows_match_float64(cuda, golden_dir, gs, act):
    """Rows are independent, so a rounding flip spoils one row only: at least 94 of the 96 rows have every
    code equal to the float64 loop on the same W and U; those rows' zeros are equal and their scales within
    rtol 1e-5.  The first group's scale depends on the input alone: bit-equal to the fp32 formula."""
    from samq import ops
    from samq.gptq import Quantizer, column_loop
    _, g = _gptq(golden_dir, cuda)
    w, u, _, _, _, _ = g.prepare(0.01, act)
    q, s, z, codes = ops.gptq_quant(w, u, gs, 15)
    rq, rs, rz = column_loop(w.double().cpu(), u.double().cpu(), Quantizer(4), 128, gs)
    same = (codes.cpu().double() == _codes(rq, rs, rz)).all(1)
    print(f"\ngptq_quant vs float64 (g{gs}, act {act}): {int(same.sum())} / {same.numel()} rows identical")
    assert int(same.sum()) >= 94
    assert torch.equal(z.cpu().double()[same], rz[same])
    np.testing.assert_allclose(s.cpu().numpy()[same], rs.numpy()[same], rtol=1e-5)
    s0, _ = Quantizer(4).find_params(w.cpu()[:, :w.shape[1] if gs == -1 else gs])
    assert torch.equal(s.cpu()[:, 0], s0)
    rep = q.shape[1] // s.shape[1]
    sr, zr = s.cpu().repeat_interleave(rep, 1), z.cpu().repeat_interleave(rep, 1)
    assert torch.equal(q.cpu(), sr * (codes.cpu().float() - zr))


@pytest.mark.parametrize("gs,act", [(-1, False), (64, True)])
def test_fasterquant_reaches_the_kernel(cuda, golden_dir, monkeypatch, gs, act):
    """``fasterquant`` on the GPU returns exactly what ``ops.gptq_quant`` returns on the same W and U;
    ``backend="torch"`` never calls the kernel and stays within the torch loop's agreement with it."""
    from samq import ops
    _, g = _gptq(golden_dir, cuda)
    w, u, perm, _, _, _ = g.prepare(0.01, act)
    q, s, z, _ = ops.gptq_quant(w, u, gs, 15)
    if perm is not None:
        q = q[:, torch.argsort(perm)]
    lin, g = _gptq(golden_dir, cuda)
    fs, fz = g.fasterquant(groupsize=gs, actorder=act)
    assert torch.equal(lin.weight.data, q) and torch.equal(fs, s) and torch.equal(fz, z)

    def no_kernel(*a, **k):
        raise AssertionError("backend='torch' reached the kernel")
    monkeypatch.setattr(ops, "gptq_quant", no_kernel)
    lin_t, g = _gptq(golden_dir, cuda)
    ts, tz = g.fasterquant(groupsize=gs, actorder=act, backend="torch")
    assert ts.shape == s.shape and tz.shape == z.shape
    np.testing.assert_allclose(ts[:, 0].cpu().numpy(), s[:, 0].cpu().numpy(), rtol=1e-6)
    if not act:   # under act-order the groups run over permuted columns: codes are compared without it
        eq = _codes(lin_t.weight.data.cpu(), ts.cpu(), tz.cpu()) == _codes(q.cpu(), s.cpu(), z.cpu())
        assert eq.double().mean() >= 0.99


@pytest.mark.parametrize("k,gs", [(200, -1), (256, 48)])
def test_unsupported_shapes(cuda, monkeypatch, k, gs):
    """K % 128 != 0 and a group size outside the built set: ``ops.gptq_quant`` raises NotImplementedError,
    ``fasterquant`` quietly runs the torch loop."""
    from samq import ops
    from samq.gptq import GPTQ
    with pytest.raises(NotImplementedError):
        ops.gptq_quant(torch.zeros(8, k, device=cuda), torch.eye(k, device=cuda), gs, 15)
    monkeypatch.setattr(ops, "gptq_quant", None)
    torch.manual_seed(0)
    lin = torch.nn.Linear(k, 8, bias=False).to(cuda)
    g = GPTQ(lin)
    g.add_batch(torch.randn(2 * k, k, device=cuda))
    s, z = g.fasterquant(groupsize=gs)
    assert s.shape == z.shape == (8, 1 if gs == -1 else -(-k // gs))
    assert torch.isfinite(lin.weight.data).all()
