"""Torch-facing wrappers of the HIP kernels (device memory + current stream plumbing only).

Every op enqueues on ``torch.cuda.current_stream()`` and returns caller-owned tensors; no op
falls back to PyTorch or the CPU -- a non-CUDA tensor is an error.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

EPI_BIAS = _lib.EPI_BIAS
EPI_BIAS_GELU = _lib.EPI_BIAS_GELU
EPI_RESADD_F32 = _lib.EPI_RESADD_F32
EPI_F32 = _lib.EPI_F32
EPI_Q8 = _lib.EPI_Q8
EPI_Q8_GELU = _lib.EPI_Q8_GELU
EPI_Q8_RES = _lib.EPI_Q8_RES
EPI_RESADD_LNF = _lib.EPI_RESADD_LNF
EPI_BIAS_LNF = _lib.EPI_BIAS_LNF
EPI_GELU_LNF = _lib.EPI_GELU_LNF

# W4A16 tile configs of the product library (include/samq.h, samq_w4a16_gemm_cfg); 0 = automatic
W4A16_CFGS = frozenset((1, 2, 3, 4, 5, 6, 7, 9, 21, 22, 23, 24, 25, 26, 29, 30, 31, 55, 56, 57, 58, 62, 64, 65, 100, 101, 104, 107, 108, 109, 110, 111, 112, 113, 114))
# int8 GEMM tile configs of the product library (include/samq.h, samq_i8_gemm_cfg); 0 = automatic
I8_CFGS = frozenset((81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 180, 181, 182))
_Q8_EPIS = (EPI_Q8, EPI_Q8_GELU, EPI_Q8_RES)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("samq ops run on the GPU only (HIP); got a CPU tensor")


# ----------------------------------------------------------------------------- W4A16
def w4_repack(qweight: torch.Tensor, layout: int = 0) -> torch.Tensor:
    """Reference ``qweight`` int32 (K/8, N) -> kernel fragment layout (flat int32 K*N/8).
    ``layout`` 0 = the product layout expected by the default GEMM dispatch."""
    _need_cuda(qweight)
    assert qweight.dtype == torch.int32 and qweight.dim() == 2
    k, n = qweight.shape[0] * 8, qweight.shape[1]
    out = torch.empty(k * n // 8, dtype=torch.int32, device=qweight.device)
    lib = _lib.load()
    if layout:
        st = lib.samq_w4_repack_layout(_ptr(qweight.contiguous()), _ptr(out), k, n, layout, _stream())
    else:
        st = lib.samq_w4_repack(_ptr(qweight.contiguous()), _ptr(out), k, n, _stream())
    _lib.check(st, "w4_repack")
    return out


def w4a16_gemm(a: torch.Tensor, wpacked: torch.Tensor, scales: torch.Tensor, qzeros: torch.Tensor,
               bias: Optional[torch.Tensor], n: int, groupsize: int, epilogue: int = EPI_BIAS,
               out: Optional[torch.Tensor] = None, cfg: int = 0) -> torch.Tensor:
    """``epilogue(a @ W4 * s + bias)`` for a (..., K) fp16 (last dim contiguous)."""
    _need_cuda(a, wpacked, scales, qzeros, bias)
    assert a.dtype == torch.float16, "A must be float16"
    k = a.shape[-1]
    a2 = a.reshape(-1, k)
    if a2.stride(-1) != 1:
        a2 = a2.contiguous()
    m = a2.shape[0]
    if out is None:
        dt = torch.float32 if epilogue in (EPI_RESADD_F32, EPI_F32) else torch.float16
        out = torch.empty(a.shape[:-1] + (n,), dtype=dt, device=a.device)
        assert epilogue != EPI_RESADD_F32, "residual epilogue needs an out tensor"
    o2 = out.reshape(-1, n)
    assert o2.stride(-1) == 1 and o2.shape[0] == m
    if bias is not None:
        assert bias.dtype == torch.float16 and bias.numel() == n
    status = _lib.load().samq_w4a16_gemm_cfg(
        _ptr(a2), a2.stride(0), _ptr(wpacked), _ptr(scales), _ptr(qzeros), _ptr(bias), _ptr(o2), o2.stride(0),
        m, n, k, groupsize, epilogue, cfg, _stream())
    _lib.check(status, "w4a16_gemm")
    return out


def w4_interleave32(gate_packed: torch.Tensor, up_packed: torch.Tensor, gate_scales: torch.Tensor,
                    up_scales: torch.Tensor, gate_qzeros: torch.Tensor, up_qzeros: torch.Tensor, n: int):
    """The samq_w4a16_gated_mlp operand layout: two repacked (layout 1) int4 matrices of N columns
    -> one of 2N whose 32-column blocks alternate gate block j / up block j (each block is one
    contiguous run of K/64 KiB in the repacked layout), scales (G, N) / qzeros (G, N/8) the same."""
    _need_cuda(gate_packed, up_packed, gate_scales, up_scales, gate_qzeros, up_qzeros)
    assert n % 32 == 0 and gate_packed.numel() == up_packed.numel()
    nb = n // 32
    w = torch.stack([gate_packed.view(nb, -1), up_packed.view(nb, -1)], 1).reshape(-1).contiguous()
    g = gate_scales.shape[0]
    s = torch.stack([gate_scales.reshape(g, nb, 32), up_scales.reshape(g, nb, 32)], 2).reshape(g, 2 * n).contiguous()
    z = torch.stack([gate_qzeros.reshape(g, nb, 4), up_qzeros.reshape(g, nb, 4)], 2).reshape(g, n // 4).contiguous()
    return w, s, z


def w4a16_gated_mlp(a: torch.Tensor, wpacked2: torch.Tensor, scales2: torch.Tensor, qzeros2: torch.Tensor,
                    n: int, groupsize: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``silu(a . Wgate) * (a . Wup)`` f16 (..., N) in ONE launch (samq_w4a16_gated_mlp) from the
    ``w4_interleave32`` operands of the two projections."""
    _need_cuda(a, wpacked2, scales2, qzeros2)
    assert a.dtype == torch.float16 and a.stride(-1) == 1
    # the kernel's 256-column tiles over the interleaved 2N columns; the reference's
    # triton_llama_mlp_4 asserts N % 256 already (gptq_triton/fused_mlp.py:437)
    assert n % 128 == 0, "w4a16_gated_mlp: N must be a multiple of 128"
    k = a.shape[-1]
    x = a.reshape(-1, k)
    m = x.shape[0]
    if out is None:
        out = torch.empty(a.shape[:-1] + (n,), dtype=torch.float16, device=a.device)
    assert out.is_contiguous() and out.dtype == torch.float16 and out.numel() == m * n
    _lib.check(_lib.load().samq_w4a16_gated_mlp(_ptr(x), x.stride(0), _ptr(wpacked2), _ptr(scales2), _ptr(qzeros2),
                                                _ptr(out), n, m, 2 * n, k, groupsize, _stream()),
               "w4a16_gated_mlp")
    return out


def w4a16_gemm_lnf(a: torch.Tensor, wpacked: torch.Tensor, scales: torch.Tensor, qzeros: torch.Tensor,
                   bias: Optional[torch.Tensor], n: int, groupsize: int, epilogue: int, out: torch.Tensor,
                   stats: torch.Tensor, mu: torch.Tensor, gamma: Optional[torch.Tensor] = None,
                   aout: Optional[torch.Tensor] = None, gw: Optional[torch.Tensor] = None,
                   bw: Optional[torch.Tensor] = None, eps: float = 1e-6, cfg: int = 0) -> torch.Tensor:
    """The W4A16 GEMM with a LayerNorm folded into its epilogue (samq_w4a16_gemm_lnf,
    include/samq.h): ``EPI_RESADD_LNF`` -- out f32 residual += y, then aout = f16((x - mu) * gamma)
    and the per-row partial sums ``stats``; ``EPI_BIAS_LNF`` / ``EPI_GELU_LNF`` -- out f16 =
    LN(x) . W + bias (GELU) from a = that aout, ``stats`` and gw = gamma . W, bw = beta . W; mu += delta."""
    _need_cuda(a, wpacked, scales, qzeros, bias, out, stats, mu, gamma, aout, gw, bw)
    assert a.dtype == torch.float16 and a.is_contiguous() and out.is_contiguous()
    k = a.shape[-1]
    m = a.numel() // k
    assert out.numel() == m * n and stats.dtype == torch.float32 and mu.dtype == torch.float32 and mu.numel() >= m
    if epilogue == EPI_RESADD_LNF:
        assert out.dtype == torch.float32 and gamma is not None and aout is not None and aout.numel() == m * n
        assert stats.numel() >= m * (n // 64) * 2
    else:
        assert out.dtype == torch.float16 and gw is not None and bw is not None and stats.numel() >= m * (k // 64) * 2
    status = _lib.load().samq_w4a16_gemm_lnf(
        _ptr(a), k, _ptr(wpacked), _ptr(scales), _ptr(qzeros), _ptr(bias), _ptr(out), n, m, n, k, groupsize,
        epilogue, cfg, _ptr(gamma), _ptr(gw), _ptr(bw), _ptr(stats), _ptr(mu), _ptr(aout), float(eps), _stream())
    _lib.check(status, "w4a16_gemm_lnf")
    return out


# ----------------------------------------------------------------------------- LayerNorm
def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-6,
              out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float16,
              rows_per_wave: int = 0, mean_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row LayerNorm over the last dim; x f32 or f16 -> f16 (or f32); gamma/beta f32.
    ``rows_per_wave`` (1, 2, 4; 0 = library default) is a tuning knob (SAMQ_LN_RPW)."""
    _need_cuda(x, gamma, beta)
    c = x.shape[-1]
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.float16)
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    assert out.is_contiguous() and out.dtype in (torch.float16, torch.float32)
    flags = (_lib.LN_IN_F16 if x.dtype == torch.float16 else 0) | (_lib.LN_OUT_F32 if out.dtype == torch.float32 else 0)
    flags |= rows_per_wave << 16
    rows = x.numel() // c
    if mean_out is not None:
        assert mean_out.dtype == torch.float32 and mean_out.numel() >= rows and mean_out.is_cuda
        _lib.check(_lib.load().samq_layernorm_mean(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), rows, c, float(eps),
                                                   flags, _ptr(mean_out), _stream()), "layernorm_mean")
        return out
    _lib.check(_lib.load().samq_layernorm(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), rows, c, float(eps), flags,
                                          _stream()), "layernorm")
    return out


def add_layernorm(x: torch.Tensor, delta: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-6,
                  out: Optional[torch.Tensor] = None, out_scale: float = 0.0, rows_per_wave: int = 0) -> torch.Tensor:
    """x (f32, in place) += delta (f16 or f32, same shape); returns LayerNorm(x) as f16, or as int8
    codes q(LN(x), out_scale) when ``out`` is int8 (samq_add_layernorm: the residual add of the
    preceding GEMM moved out of its epilogue)."""
    _need_cuda(x, delta, gamma, beta)
    c = x.shape[-1]
    assert x.is_contiguous() and x.dtype == torch.float32 and delta.is_contiguous()
    assert delta.dtype in (torch.float16, torch.float32) and delta.numel() == x.numel()
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=torch.int8 if out_scale > 0 else torch.float16, device=x.device)
    assert out.is_contiguous() and out.dtype in (torch.float16, torch.int8) and out.numel() == x.numel()
    flags = (_lib.LN_DELTA_F16 if delta.dtype == torch.float16 else 0) | (_lib.LN_OUT_I8 if out.dtype == torch.int8
                                                                           else 0)
    flags |= rows_per_wave << 16
    _lib.check(_lib.load().samq_add_layernorm(_ptr(x), _ptr(delta), _ptr(out), _ptr(gamma), _ptr(beta), x.numel() // c,
                                              c, float(eps), flags, float(out_scale), _stream()), "add_layernorm")
    return out


# ----------------------------------------------------------------------------- patch embed / neck
def patch_embed(img: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], pos: Optional[torch.Tensor],
                patch: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img f16 (B, Cin, S, S) -> f32 (B, S/p, S/p, N) = Conv2d(k=p, stride=p)(img) + bias + pos;
    weight f16 (N, Cin*p*p), bias f32 (N,), pos f32 (S/p, S/p, N) or None.  With img and weight
    both f32 the whole GEMM runs in fp32 (``samq_patch_embed_f32``, the W4A8 embedding)."""
    _need_cuda(img, weight, bias, pos)
    b, cin, s, s2 = img.shape
    f32 = img.dtype == torch.float32
    dt = torch.float32 if f32 else torch.float16
    assert s == s2 and img.dtype == dt and img.is_contiguous()
    n = weight.shape[0]
    assert weight.dtype == dt and weight.is_contiguous() and weight.shape[1] == cin * patch * patch
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous())
    assert pos is None or (pos.dtype == torch.float32 and pos.is_contiguous() and pos.numel() == (s // patch) ** 2 * n)
    g = s // patch
    if out is None:
        out = torch.empty((b, g, g, n), dtype=torch.float32, device=img.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == b * g * g * n
    fn = _lib.load().samq_patch_embed_f32 if f32 else _lib.load().samq_patch_embed
    _lib.check(fn(_ptr(img), _ptr(weight), _ptr(bias), _ptr(pos), _ptr(out), b, cin, s, patch, n, _stream()),
               "patch_embed")
    return out


def patch_embed_u8(img: torch.Tensor, pixel_mean: torch.Tensor, pixel_std: torch.Tensor, weight: torch.Tensor,
                   bias: Optional[torch.Tensor], pos: Optional[torch.Tensor], patch: int, img_size: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Raw uint8 pixels (B, Cin, h, w), h, w <= img_size -> f32 (B, S/p, S/p, N): Sam.preprocess
    (normalise by pixel mean / std, zero-pad to img_size) fused into the patch-embedding GEMM.
    weight f16 (fp16 MFMA) or f32 (fp32 MFMA, the W4A8 embedding)."""
    _need_cuda(img, pixel_mean, pixel_std, weight, bias, pos)
    assert img.dtype == torch.uint8 and img.dim() == 4 and img.is_contiguous()
    b, cin, h, w = img.shape
    mean = pixel_mean.reshape(-1).float().contiguous()
    std = pixel_std.reshape(-1).float().contiguous()
    assert mean.numel() == cin and std.numel() == cin
    n = weight.shape[0]
    assert weight.dtype in (torch.float16, torch.float32) and weight.is_contiguous()
    assert weight.shape[1] == cin * patch * patch
    g = img_size // patch
    if out is None:
        out = torch.empty((b, g, g, n), dtype=torch.float32, device=img.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == b * g * g * n
    _lib.check(_lib.load().samq_patch_embed_u8(_ptr(img), h, w, _ptr(mean), _ptr(std), _ptr(weight),
                                               int(weight.dtype == torch.float32), _ptr(bias), _ptr(pos), _ptr(out),
                                               b, cin, img_size, patch, n, _stream()), "patch_embed_u8")
    return out


def conv1x1_f32(x: torch.Tensor, weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x f32 (..., K) tokens -> f16 (..., N) = x . weight^T (1x1 conv, no bias); weight f16 (N, K)."""
    _need_cuda(x, weight)
    k = x.shape[-1]
    n = weight.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous() and weight.dtype == torch.float16 and weight.shape[1] == k
    if out is None:
        out = torch.empty(x.shape[:-1] + (n,), dtype=torch.float16, device=x.device)
    assert out.dtype == torch.float16 and out.is_contiguous()
    _lib.check(_lib.load().samq_conv1x1_f32(_ptr(x), _ptr(weight.contiguous()), _ptr(out), x.numel() // k, n, k,
                                            _stream()), "conv1x1")
    return out


def conv3x3_nhwc(x: torch.Tensor, weight_tap_major: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x f16 (B, G, G, Cin) -> f16 (B, G, G, N): 3x3 conv, padding 1, no bias; weight f16 (N, 3, 3, Cin)."""
    _need_cuda(x, weight_tap_major)
    b, g, g2, cin = x.shape
    assert g == g2 and x.dtype == torch.float16 and x.is_contiguous()
    w = weight_tap_major
    n = w.shape[0]
    assert w.dtype == torch.float16 and w.is_contiguous() and tuple(w.shape[1:]) == (3, 3, cin)
    if out is None:
        out = torch.empty((b, g, g, n), dtype=torch.float16, device=x.device)
    assert out.dtype == torch.float16 and out.is_contiguous()
    _lib.check(_lib.load().samq_conv3x3_nhwc(_ptr(x), _ptr(w), _ptr(out), b, g, cin, n, _stream()), "conv3x3")
    return out


# ----------------------------------------------------------------------------- attention
def rel_attention(qkv: torch.Tensor, qkv_bias: Optional[torch.Tensor], rel_pos_h: torch.Tensor,
                  rel_pos_w: torch.Tensor, heads: int, window: int, sm_scale: float,
                  out: Optional[torch.Tensor] = None, out_scale: float = 0.0) -> torch.Tensor:
    """qkv f16 (B, H, W, 3C) -> out f16 (B, H, W, C); windowed (window > 0) or global.
    out_scale > 0: out int8 codes of the fp16 output quantised with out_scale (samq_rel_attention_q,
    the W4A8 proj-input QAct folded into the store)."""
    _need_cuda(qkv, qkv_bias, rel_pos_h, rel_pos_w)
    b, h, w, c3 = qkv.shape
    c = c3 // 3
    hd = c // heads
    assert qkv.dtype == torch.float16 and qkv.is_contiguous()
    assert rel_pos_h.dtype == torch.float16 and rel_pos_w.dtype == torch.float16
    odt = torch.int8 if out_scale > 0 else torch.float16
    if out is None:
        out = torch.empty((b, h, w, c), dtype=odt, device=qkv.device)
    assert out.dtype == odt and out.is_contiguous()
    # named, so a copy made here lives until the launch is queued (a temporary's block would be handed
    # to the next copy, and the kernel would read that one's data)
    rel_pos_h, rel_pos_w = rel_pos_h.contiguous(), rel_pos_w.contiguous()
    args = (_ptr(qkv), _ptr(qkv_bias), _ptr(rel_pos_h), _ptr(rel_pos_w), _ptr(out),
            b, h, w, heads, hd, window, float(sm_scale))
    if out_scale > 0:
        _lib.check(_lib.load().samq_rel_attention_q(*args, float(out_scale), _stream()), "rel_attention_q")
    else:
        _lib.check(_lib.load().samq_rel_attention(*args, _stream()), "rel_attention")
    return out


def attention_relbias(inp: torch.Tensor, rel_h: torch.Tensor, rel_w: torch.Tensor, heads: int, hd: int,
                      sm_scale: float) -> torch.Tensor:
    """Reference ``fused_attention.forward`` semantics with precomputed rel_h / rel_w."""
    _need_cuda(inp, rel_h, rel_w)
    b, h, w, c3 = inp.shape
    assert h == w, "the reference kernel requires square grids (emb_len = rel.shape[-1])"
    out = torch.empty((b, h, w, c3 // 3), dtype=inp.dtype, device=inp.device)
    # named, so the fp16 / contiguous copies live until the launch is queued: the block of a temporary
    # rel_h copy would be handed to the rel_w copy, and the kernel would read rel_w for both
    inp, rel_h, rel_w = inp.contiguous(), rel_h.half().contiguous(), rel_w.half().contiguous()
    _lib.check(_lib.load().samq_attention_relbias(_ptr(inp), _ptr(rel_h), _ptr(rel_w), _ptr(out), b, h, heads, hd,
                                                  float(sm_scale), _stream()), "attention_relbias")
    return out


# ----------------------------------------------------------------------------- int8 activations
def quantize(x: torch.Tensor, scale: float, fake: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fq_vit QAct (quant mode): int8 codes ``clamp(round(x / s), -128, 127)`` (or, with
    ``fake``, the f32 value ``codes * s``).  x f32 / f16 contiguous."""
    _need_cuda(x)
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.float16)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32 if fake else torch.int8, device=x.device)
    flags = (_lib.Q_IN_F16 if x.dtype == torch.float16 else 0) | (_lib.Q_OUT_FQ if fake else 0)
    _lib.check(_lib.load().samq_quantize(_ptr(x), _ptr(out), x.numel(), float(scale), flags, _stream()), "quantize")
    return out


def minmax_update(x2d: torch.Tensor, axis: int, max_val: Optional[torch.Tensor] = None,
                  min_val: Optional[torch.Tensor] = None):
    """fq_vit ``MinmaxObserver.update`` core on the GPU (``samq_minmax``): running max / min of a
    contiguous (rows, C) f32 / f16 tensor per row (``MM_PER_ROW``), per column (``MM_PER_COL``)
    or over everything (``MM_ALL``, 0-dim results).  ``max_val`` / ``min_val`` None -> fresh f32
    tensors; else they are merged in place (f32, contiguous, matching shape)."""
    _need_cuda(x2d)
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype in (torch.float32, torch.float16)
    rows, c = x2d.shape
    shape = {_lib.MM_PER_ROW: (rows,), _lib.MM_PER_COL: (c,), _lib.MM_ALL: ()}[axis]
    init = max_val is None
    if init:
        max_val = torch.empty(shape, dtype=torch.float32, device=x2d.device)
        min_val = torch.empty(shape, dtype=torch.float32, device=x2d.device)
    for t in (max_val, min_val):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape and t.device == x2d.device
    lib = _lib.load()
    nws = lib.samq_minmax_workspace(rows, c, axis)
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=x2d.device)
    _lib.check(lib.samq_minmax(_ptr(x2d), rows, c, int(x2d.dtype == torch.float16), axis, _ptr(max_val),
                               _ptr(min_val), int(init), _ptr(ws), nws, _stream()), "minmax")
    return max_val, min_val


def order_stats(x: torch.Tensor, ranks):
    """Exact order statistics (``samq_order_stats``): the values at the zero-based ``ranks`` (1 to 4
    Python ints) of the sorted flat f32 / f16 tensor ``x``.  Returns ``(values, nan_flag)``, an f32
    tensor of ``len(ranks)`` values and a 0-dim int32 tensor (1 if ``x`` holds a NaN), both on the
    device: nothing is synchronised here."""
    _need_cuda(x)
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.float16) and x.numel() > 0
    ranks = [int(r) for r in ranks]
    n = x.numel()
    assert 1 <= len(ranks) <= 4 and all(0 <= r < n for r in ranks), "order_stats: 1 to 4 ranks in [0, n)"
    import ctypes
    lib = _lib.load()
    out = torch.empty(len(ranks), dtype=torch.float32, device=x.device)
    flag = torch.empty((), dtype=torch.int32, device=x.device)
    nws = lib.samq_order_stats_workspace(n, len(ranks))
    ws = torch.empty((nws + 7) // 8, dtype=torch.int64, device=x.device)
    host_ranks = (ctypes.c_int64 * len(ranks))(*ranks)
    _lib.check(lib.samq_order_stats(_ptr(x), n, int(x.dtype == torch.float16), host_ranks, len(ranks), _ptr(out),
                                    _ptr(flag), _ptr(ws), nws, _stream()), "order_stats")
    return out, flag


def omse_scores(x: torch.Tensor, cand: torch.Tensor, qmin: float, qmax: float) -> torch.Tensor:
    """fq_vit ``OmseObserver`` candidate scores (``samq_omse_scores``): for each row (scale,
    zero_point) of the f32 (ncand <= 96, 2) tensor ``cand``, the float64 sum over the flat f32 / f16
    tensor ``x`` of ``(x - (clamp(round(x / s + zp), qmin, qmax) - zp) * s) ** 2``, every f32 step
    rounded as torch's separate ops round it.  Returns a float64 (ncand,) tensor on the device."""
    _need_cuda(x, cand)
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.float16) and x.numel() > 0
    assert cand.dtype == torch.float32 and cand.is_contiguous() and cand.dim() == 2 and cand.shape[1] == 2
    ncand = cand.shape[0]
    assert 1 <= ncand <= 96
    lib = _lib.load()
    sums = torch.empty(ncand, dtype=torch.float64, device=x.device)
    nws = lib.samq_omse_scores_workspace(x.numel(), ncand)
    ws = torch.empty((nws + 7) // 8, dtype=torch.float64, device=x.device)
    _lib.check(lib.samq_omse_scores(_ptr(x), x.numel(), int(x.dtype == torch.float16), _ptr(cand), ncand,
                                    float(qmin), float(qmax), _ptr(sums), _ptr(ws), nws, _stream()), "omse_scores")
    return sums


def layernorm_q(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, in_scale: float = 0.0,
                out_scale: float = 0.0, out_dtype: torch.dtype = torch.int8,
                out: Optional[torch.Tensor] = None, rows_per_wave: int = 0,
                rowsum: Optional[torch.Tensor] = None, zero_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm with int8 codes on either side: x int8 (codes * in_scale) / f32 / f16;
    out int8 codes (q(y, out_scale)), f32 fake-quant (out_dtype f32 with out_scale > 0), f16 or f32.
    ``rows_per_wave`` (1, 2, 4; 0 = library default) as in ``layernorm``.  ``rowsum`` (int32 [rows],
    int8-code output only): the output rows' code sums (``samq_layernorm_q_rs``, the W4A8 GEMM's
    row sums); ``zero_rows`` (int32 [rows]) is zeroed on the way."""
    if rowsum is not None:
        return _layernorm_q_rs(x, gamma, beta, eps, in_scale, out_scale, out, rows_per_wave, rowsum, zero_rows)
    if zero_rows is not None:
        raise AssertionError("layernorm_q: zero_rows is zeroed on the row-sum path only (pass rowsum too)")
    _need_cuda(x, gamma, beta)
    c = x.shape[-1]
    assert x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    flags = 0
    if x.dtype == torch.int8:
        flags |= _lib.LN_IN_I8
    elif x.dtype == torch.float16:
        flags |= _lib.LN_IN_F16
    if out.dtype == torch.int8:
        flags |= _lib.LN_OUT_I8
    elif out.dtype == torch.float32:
        flags |= _lib.LN_OUT_F32 | (_lib.LN_OUT_I8 if out_scale > 0 else 0)
    flags |= rows_per_wave << 16
    _lib.check(_lib.load().samq_layernorm_q(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), x.numel() // c, c,
                                            float(eps), flags, float(in_scale), float(out_scale), _stream()),
               "layernorm_q")
    return out


def _rows_i32(t: Optional[torch.Tensor], rows: int, what: str) -> None:
    if t is not None:
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= rows, f"{what}: int32 [rows] expected"


def _layernorm_q_rs(x, gamma, beta, eps, in_scale, out_scale, out, rows_per_wave, rowsum, zero_rows):
    _need_cuda(x, gamma, beta, rowsum, zero_rows)
    c = x.shape[-1]
    rows = x.numel() // c
    assert x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    _rows_i32(rowsum, rows, "layernorm_q rowsum")
    _rows_i32(zero_rows, rows, "layernorm_q zero_rows")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    assert out.dtype == torch.int8, "layernorm_q: row sums need int8-code output"
    flags = _lib.LN_OUT_I8 | (rows_per_wave << 16)
    if x.dtype == torch.int8:
        flags |= _lib.LN_IN_I8
    elif x.dtype == torch.float16:
        flags |= _lib.LN_IN_F16
    _lib.check(_lib.load().samq_layernorm_q_rs(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), rows, c, float(eps), flags,
                                               float(in_scale), float(out_scale), _ptr(rowsum), _ptr(zero_rows),
                                               _stream()), "layernorm_q_rs")
    return out


def w8_repack(w: torch.Tensor) -> torch.Tensor:
    """int8 weight codes [N, K] (QLinear / flattened QConv2d layout) -> int8 MFMA fragment order."""
    _need_cuda(w)
    assert w.dtype == torch.int8 and w.dim() == 2
    w = w.contiguous()
    n, k = w.shape
    out = torch.empty(n * k, dtype=torch.int8, device=w.device)
    _lib.check(_lib.load().samq_w8_repack(_ptr(w), _ptr(out), k, n, _stream()), "w8_repack")
    return out


def _i8_out(a2, n, epilogue, out, shape):
    if out is None:
        if epilogue in _Q8_EPIS:
            dt = torch.int8
        elif epilogue in (EPI_RESADD_F32, EPI_F32):
            dt = torch.float32
        else:
            dt = torch.float16
        assert epilogue != EPI_RESADD_F32, "residual epilogue needs an out tensor"
        out = torch.empty(shape + (n,), dtype=dt, device=a2.device)
    o2 = out.reshape(-1, n)
    assert o2.stride(-1) == 1 and o2.shape[0] == a2.shape[0]
    return out, o2


def i8_gemm(a: torch.Tensor, bfmt: int, wpacked: torch.Tensor, wscale: torch.Tensor, n: int,
            bias: Optional[torch.Tensor] = None, qzeros: Optional[torch.Tensor] = None, epilogue: int = EPI_BIAS,
            a_scale: float = 1.0, out_scale: float = 0.0, mid_scale: float = 0.0, res_scale: float = 0.0,
            res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, cfg: int = 0) -> torch.Tensor:
    """int8 codes a (..., K) x packed weights (bfmt 0: W8 from w8_repack, 1: GPTQ W4 layout 3)."""
    _need_cuda(a, wpacked, wscale, bias, qzeros, res)
    assert a.dtype == torch.int8 and wscale.dtype == torch.float32
    assert bias is None or bias.dtype == torch.float32
    k = a.shape[-1]
    a2 = a.reshape(-1, k)
    out, o2 = _i8_out(a2, n, epilogue, out, tuple(a.shape[:-1]))
    r2 = None if res is None else res.reshape(-1, n)
    status = _lib.load().samq_i8_gemm_cfg(
        _ptr(a2), a2.stride(0), bfmt, _ptr(wpacked), _ptr(wscale), _ptr(qzeros), _ptr(bias), _ptr(o2), o2.stride(0),
        _ptr(r2), 0 if r2 is None else r2.stride(0), a2.shape[0], n, k, epilogue, float(a_scale), float(mid_scale),
        float(res_scale), float(out_scale), cfg, _stream())
    _lib.check(status, "i8_gemm")
    return out


def w8a8_gemm(a, wpacked, wscale, n, bias=None, epilogue=EPI_Q8, a_scale=1.0, out_scale=0.0, mid_scale=0.0,
              res_scale=0.0, res=None, out=None, cfg=0):
    """fq_vit QLinear on int8 codes: ``epilogue(float(sum a w) * a_scale * wscale[n] + bias[n])``."""
    return i8_gemm(a, _lib.BF_W8, wpacked, wscale, n, bias, None, epilogue, a_scale, out_scale, mid_scale,
                   res_scale, res, out, cfg)


def w8a8_gemm_v16(a, wpacked, wscale, n, bias, a_scale, out_scale, v16, v_col0, out=None, cfg=0):
    """``w8a8_gemm`` with the Q8 epilogue that also stores the codes of columns [v_col0, n) as fp16
    into ``v16`` (rows x (n - v_col0)): the fq_vit qkv projection feeding ``rel_attention_q8(v16=)``."""
    _need_cuda(a, wpacked, wscale, bias, v16)
    assert a.dtype == torch.int8 and wscale.dtype == torch.float32 and v16.dtype == torch.float16
    k = a.shape[-1]
    a2 = a.reshape(-1, k)
    out, o2 = _i8_out(a2, n, EPI_Q8, out, tuple(a.shape[:-1]))
    v2 = v16.reshape(a2.shape[0], -1)
    assert v2.is_contiguous() and v2.shape[1] >= n - v_col0
    _lib.check(_lib.load().samq_w8a8_gemm_v16(
        _ptr(a2), a2.stride(0), _ptr(wpacked), _ptr(wscale), _ptr(bias), _ptr(o2), o2.stride(0), a2.shape[0], n, k,
        float(a_scale), float(out_scale), _ptr(v2), int(v_col0), v2.stride(0), cfg, _stream()), "w8a8_gemm_v16")
    return out


def w8a8_conv_gemm(x: torch.Tensor, mode: int, wpacked: torch.Tensor, wscale: torch.Tensor, n: int,
                   bias: Optional[torch.Tensor] = None, epilogue: int = EPI_Q8, a_scale: float = 1.0,
                   out_scale: float = 0.0, mid_scale: float = 0.0, res_scale: float = 0.0,
                   res: Optional[torch.Tensor] = None, rmod: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fq_vit QConv2d on int8 codes as an implicit GEMM (``samq_w8a8_conv_gemm``): mode 1 = the
    16x16 / stride-16 PatchEmbed on NCHW codes (B, Cin, S, S); mode 2 = the 3x3 / pad-1 neck conv on
    NHWC codes (B, G, G, Cin).  Returns int8 codes (B, G, G, n) (``out``: caller-owned, contiguous)."""
    _need_cuda(x, wpacked, wscale, bias, res)
    assert x.dtype == torch.int8 and x.is_contiguous() and wscale.dtype == torch.float32
    if mode == 1:
        b, cin, side, _ = x.shape
        g = side // 16
    else:
        b, g, _, cin = x.shape
        side = g
    if out is None:
        out = torch.empty((b, g, g, n), dtype=torch.int8, device=x.device)
    assert out.is_cuda and out.dtype == torch.int8 and out.is_contiguous() and out.numel() == b * g * g * n
    _lib.check(_lib.load().samq_w8a8_conv_gemm(_ptr(x), mode, b, cin, side, _ptr(wpacked), _ptr(wscale), _ptr(bias),
                                               _ptr(out), _ptr(res), rmod, n, epilogue, float(a_scale),
                                               float(mid_scale), float(res_scale), float(out_scale), _stream()),
               "w8a8_conv_gemm")
    return out


# ---- activation zero points: a quantiser is (scale, zp), code = clamp(rint(fl(x / s) + zp), -128, 127),
# value = (code - zp) * s (fq_vit quantizer/uniform.py:23-45); zp an integer in [-128, 127]
def _zp(*zps) -> None:
    for z in zps:
        assert int(z) == z and -128 <= z <= 127, f"zero point {z!r}: an integer in [-128, 127] expected"


def quantize_zp(x: torch.Tensor, scale: float, zp: int, fake: bool = False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``quantize`` with a zero point: int8 codes ``clamp(rint(x / s + zp), -128, 127)`` (the zero point
    added to the fp32 quotient BEFORE the rounding) or, with ``fake``, the f32 value ``(code - zp) * s``."""
    _need_cuda(x)
    _zp(zp)
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.float16)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32 if fake else torch.int8, device=x.device)
    flags = (_lib.Q_IN_F16 if x.dtype == torch.float16 else 0) | (_lib.Q_OUT_FQ if fake else 0)
    _lib.check(_lib.load().samq_quantize_zp(_ptr(x), _ptr(out), x.numel(), float(scale), int(zp), flags, _stream()),
               "quantize_zp")
    return out


def layernorm_q_zp(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, in_scale: float = 0.0,
                   out_scale: float = 0.0, zp_in: int = 0, zp_out: int = 0, out_dtype: torch.dtype = torch.int8,
                   out: Optional[torch.Tensor] = None, rows_per_wave: int = 0) -> torch.Tensor:
    """``layernorm_q`` with zero points: int8 input ``(code - zp_in) * in_scale``; int8 output codes of
    the quantiser (out_scale, zp_out), or (out_dtype f32 with out_scale > 0) the fake-quant value
    ``(code - zp_out) * out_scale``."""
    _need_cuda(x, gamma, beta)
    _zp(zp_in, zp_out)
    c = x.shape[-1]
    assert x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    flags = 0
    if x.dtype == torch.int8:
        flags |= _lib.LN_IN_I8
    elif x.dtype == torch.float16:
        flags |= _lib.LN_IN_F16
    if out.dtype == torch.int8:
        flags |= _lib.LN_OUT_I8
    elif out.dtype == torch.float32:
        flags |= _lib.LN_OUT_F32 | (_lib.LN_OUT_I8 if out_scale > 0 else 0)
    flags |= rows_per_wave << 16
    _lib.check(_lib.load().samq_layernorm_q_zp(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), x.numel() // c, c,
                                               float(eps), flags, float(in_scale), float(out_scale), int(zp_in),
                                               int(zp_out), _stream()), "layernorm_q_zp")
    return out


def _col_offset(col_offset: Optional[torch.Tensor], n: int) -> None:
    if col_offset is not None:
        assert col_offset.dtype == torch.int32 and col_offset.is_contiguous() and col_offset.numel() == n, \
            "col_offset: int32 [N] expected"


def w8a8_col_offset(w: torch.Tensor, zp_a: int) -> torch.Tensor:
    """The zero-point GEMMs' ``col_offset`` of int8 weight codes w [N, K] under the input zero point
    zp_a: int32 [N] = -zp_a * sum_k w[n, k] (exact: |sum| <= 128 K)."""
    _zp(zp_a)
    return (w.to(torch.int32).sum(1, dtype=torch.int32) * (-int(zp_a))).contiguous()


def i8_gemm_zp(a: torch.Tensor, wpacked: torch.Tensor, wscale: torch.Tensor, n: int,
               bias: Optional[torch.Tensor] = None, epilogue: int = EPI_Q8, a_scale: float = 1.0,
               out_scale: float = 0.0, mid_scale: float = 0.0, res_scale: float = 0.0,
               res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, cfg: int = 0,
               col_offset: Optional[torch.Tensor] = None, mid_zp: int = 0, res_zp: int = 0, out_zp: int = 0,
               rmod: int = 0) -> torch.Tensor:
    """``w8a8_gemm`` on activations with zero points (``samq_i8_gemm_zp``; W8 weights, epilogues Q8 /
    Q8_GELU / Q8_RES): ``col_offset`` (int32 [N], ``w8a8_col_offset``) is added to every row's int32
    sum before the scaling -- the input's zero point; the residual is ``(R - res_zp) * res_scale``
    (row ``r % rmod`` of R when rmod > 0), the mid and output quantisers carry mid_zp / out_zp."""
    _need_cuda(a, wpacked, wscale, bias, res, col_offset)
    _zp(mid_zp, res_zp, out_zp)
    assert a.dtype == torch.int8 and wscale.dtype == torch.float32
    assert bias is None or bias.dtype == torch.float32
    _col_offset(col_offset, n)
    k = a.shape[-1]
    a2 = a.reshape(-1, k)
    out, o2 = _i8_out(a2, n, epilogue, out, tuple(a.shape[:-1]))
    r2 = None if res is None else res.reshape(-1, n)
    assert r2 is None or rmod == 0 or r2.shape[0] >= rmod, "i8_gemm_zp: the residual has fewer than rmod rows"
    assert r2 is None or rmod > 0 or r2.shape[0] >= a2.shape[0], "i8_gemm_zp: the residual has fewer rows than A"
    status = _lib.load().samq_i8_gemm_zp(
        _ptr(a2), a2.stride(0), _ptr(wpacked), _ptr(wscale), _ptr(bias), _ptr(o2), o2.stride(0), _ptr(r2),
        0 if r2 is None else r2.stride(0), a2.shape[0], n, k, epilogue, float(a_scale), float(mid_scale),
        float(res_scale), float(out_scale), cfg, _ptr(col_offset), int(mid_zp), int(res_zp), int(out_zp), int(rmod),
        _stream())
    _lib.check(status, "i8_gemm_zp")
    return out


def w8a8_conv_gemm_zp(x: torch.Tensor, mode: int, wpacked: torch.Tensor, wscale: torch.Tensor, n: int,
                      bias: Optional[torch.Tensor] = None, epilogue: int = EPI_Q8, a_scale: float = 1.0,
                      out_scale: float = 0.0, mid_scale: float = 0.0, res_scale: float = 0.0,
                      res: Optional[torch.Tensor] = None, rmod: int = 0, out: Optional[torch.Tensor] = None,
                      col_offset: Optional[torch.Tensor] = None, mid_zp: int = 0, res_zp: int = 0, out_zp: int = 0,
                      pad16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``w8a8_conv_gemm`` on activations with zero points (``samq_w8a8_conv_gemm_zp``).  ``pad16`` (mode
    2): 16 int8 device bytes, each the input's zero-point code -- what the 3x3 gather reads outside
    the map (a padded 0.0 is the code zp), so ``col_offset`` holds for border pixels too."""
    _need_cuda(x, wpacked, wscale, bias, res, col_offset, pad16)
    _zp(mid_zp, res_zp, out_zp)
    assert x.dtype == torch.int8 and x.is_contiguous() and wscale.dtype == torch.float32
    _col_offset(col_offset, n)
    assert pad16 is None or (pad16.dtype == torch.int8 and pad16.is_contiguous() and pad16.numel() >= 16), \
        "pad16: 16 int8 bytes expected"
    if mode == 1:
        b, cin, side, _ = x.shape
        g = side // 16
    else:
        b, g, _, cin = x.shape
        side = g
    assert res is None or res.numel() >= (rmod if rmod > 0 else b * g * g) * n, "w8a8_conv_gemm_zp: residual too small"
    if out is None:
        out = torch.empty((b, g, g, n), dtype=torch.int8, device=x.device)
    assert out.is_cuda and out.dtype == torch.int8 and out.is_contiguous() and out.numel() == b * g * g * n
    _lib.check(_lib.load().samq_w8a8_conv_gemm_zp(
        _ptr(x), mode, b, cin, side, _ptr(wpacked), _ptr(wscale), _ptr(bias), _ptr(out), _ptr(res), rmod, n, epilogue,
        float(a_scale), float(mid_scale), float(res_scale), float(out_scale), _ptr(col_offset), int(mid_zp),
        int(res_zp), int(out_zp), _ptr(pad16), _stream()), "w8a8_conv_gemm_zp")
    return out


# ---- Power-of-Two Factor activations (fq_vit observer/ptf.py): a quantiser is (s0, zp, exp[C]), channel c
# under the scale s0 * 2^exp[c]; exp a uint8 device tensor with values 0..3
def _exp(t: Optional[torch.Tensor], n: int, what: str) -> None:
    if t is not None:
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n, \
            f"{what}: uint8 [{n}] on the GPU expected"


def ptf_scores(x2d: torch.Tensor, scale1: float, zero_point: float, qmin: float, qmax: float) -> torch.Tensor:
    """fq_vit ``PtfObserver`` scores (``samq_ptf_scores``): for every column of the contiguous f32 / f16
    (rows, C) tensor the float64 sums over the rows of the squared fake-quant error under the scales
    ``scale1 * (1, 2, 4, 8)`` and the zero point.  Returns a float64 (C, 4) tensor on the device."""
    _need_cuda(x2d)
    assert x2d.dim() == 2 and x2d.is_contiguous() and x2d.dtype in (torch.float32, torch.float16) and x2d.numel() > 0
    rows, c = x2d.shape
    lib = _lib.load()
    sums = torch.empty((c, 4), dtype=torch.float64, device=x2d.device)
    nws = lib.samq_ptf_scores_workspace(rows, c)
    ws = torch.empty((nws + 7) // 8, dtype=torch.float64, device=x2d.device)
    _lib.check(lib.samq_ptf_scores(_ptr(x2d), rows, c, int(x2d.dtype == torch.float16), float(scale1),
                                   float(zero_point), float(qmin), float(qmax), _ptr(sums), _ptr(ws), nws, _stream()),
               "ptf_scores")
    return sums


def layernorm_q_ptf(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, in_scale: float,
                    out_scale: float, zp_in: int, zp_out: int, in_exp: torch.Tensor,
                    out_dtype: torch.dtype = torch.int8, out: Optional[torch.Tensor] = None,
                    rows_per_wave: int = 0) -> torch.Tensor:
    """``layernorm_q_zp`` on int8 codes under a PTF quantiser: ``x = ((code - zp_in) << in_exp[c]) * in_scale``."""
    _need_cuda(x, gamma, beta, in_exp)
    _zp(zp_in, zp_out)
    c = x.shape[-1]
    assert x.dtype == torch.int8 and x.is_contiguous() and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    assert in_exp is not None, "layernorm_q_ptf: in_exp is required"
    _exp(in_exp, c, "in_exp")
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    flags = _lib.LN_IN_I8
    if out.dtype == torch.int8:
        flags |= _lib.LN_OUT_I8
    elif out.dtype == torch.float32:
        flags |= _lib.LN_OUT_F32 | (_lib.LN_OUT_I8 if out_scale > 0 else 0)
    flags |= rows_per_wave << 16
    _lib.check(_lib.load().samq_layernorm_q_ptf(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), x.numel() // c, c,
                                                float(eps), flags, float(in_scale), float(out_scale), int(zp_in),
                                                int(zp_out), _ptr(in_exp), _stream()), "layernorm_q_ptf")
    return out


def ptf_stack_weight(w: torch.Tensor, in_exp: torch.Tensor, zp_a: int):
    """The replay operands of ``i8_gemm_ptf`` for int8 weight codes w [N, K] whose input has the per-k
    exponents ``in_exp`` (uint8 [K], 0..3): the distinct exponents e_0 > ... > e_{P-1} = 0 (0 always
    included), the P masked copies of w stacked along K, the shifts e_p - e_{p+1} and
    ``col_offset[n] = -zp_a * sum_k 2^exp[k] w[n, k]`` (int64 arithmetic, checked to fit int32).
    Returns ``(stacked [N, P * K] int8, (s0, s1, s2), col_offset int32 [N])``."""
    _zp(zp_a)
    n, k = w.shape
    e = in_exp.to(w.device).to(torch.int64).reshape(-1)
    assert e.numel() == k and int(e.min()) >= 0 and int(e.max()) <= 3, "in_exp: K values in 0..3"
    levels = sorted(set(e.unique().tolist()) | {0}, reverse=True)
    assert 255 * 128 * 2 ** levels[0] * k < 2 ** 31 or len(levels) == 1, "ptf replay: the int32 sums could overflow"
    stacked = torch.cat([w * (e == lv).to(w.dtype)[None, :] for lv in levels], dim=1).contiguous()
    shifts = [levels[p] - levels[p + 1] for p in range(len(levels) - 1)] + [0] * (4 - len(levels))
    off = -int(zp_a) * (w.to(torch.int64) * (2 ** e)[None, :]).sum(1)
    assert int(off.abs().max()) < 2 ** 31, "ptf replay: col_offset outside int32"
    return stacked, tuple(shifts), off.to(torch.int32).contiguous()


def i8_gemm_ptf(a: torch.Tensor, wpacked: torch.Tensor, wscale: torch.Tensor, n: int,
                bias: Optional[torch.Tensor] = None, epilogue: int = EPI_Q8, a_scale: float = 1.0,
                out_scale: float = 0.0, mid_scale: float = 0.0, res_scale: float = 0.0,
                res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, cfg: int = 0,
                col_offset: Optional[torch.Tensor] = None, mid_zp: int = 0, res_zp: int = 0, out_zp: int = 0,
                rmod: int = 0, out_exp: Optional[torch.Tensor] = None, res_exp: Optional[torch.Tensor] = None,
                passes: int = 1, k_shift=(0, 0, 0)) -> torch.Tensor:
    """``i8_gemm_zp`` on PTF activations (``samq_i8_gemm_ptf``): ``out_exp`` / ``res_exp`` (uint8 [N]) are the
    output quantiser's and the residual's exponents; ``passes`` > 1 with ``k_shift``: ``wpacked`` is the
    repack of ``ptf_stack_weight``'s stacked copies (K of the weight = passes * a.shape[-1])."""
    _need_cuda(a, wpacked, wscale, bias, res, col_offset, out_exp, res_exp)
    _zp(mid_zp, res_zp, out_zp)
    assert a.dtype == torch.int8 and wscale.dtype == torch.float32
    assert bias is None or bias.dtype == torch.float32
    _col_offset(col_offset, n)
    _exp(out_exp, n, "out_exp")
    _exp(res_exp, n, "res_exp")
    ka = a.shape[-1]
    assert ka % 128 == 0 and 1 <= passes <= 4 and wpacked.numel() == n * ka * passes, "i8_gemm_ptf: weight size"
    a2 = a.reshape(-1, ka)
    out, o2 = _i8_out(a2, n, epilogue, out, tuple(a.shape[:-1]))
    r2 = None if res is None else res.reshape(-1, n)
    assert r2 is None or rmod == 0 or r2.shape[0] >= rmod, "i8_gemm_ptf: the residual has fewer than rmod rows"
    assert r2 is None or rmod > 0 or r2.shape[0] >= a2.shape[0], "i8_gemm_ptf: the residual has fewer rows than A"
    ks = tuple(int(s) for s in k_shift) + (0, 0, 0)
    status = _lib.load().samq_i8_gemm_ptf(
        _ptr(a2), a2.stride(0), _ptr(wpacked), _ptr(wscale), _ptr(bias), _ptr(o2), o2.stride(0), _ptr(r2),
        0 if r2 is None else r2.stride(0), a2.shape[0], n, ka * passes, epilogue, float(a_scale), float(mid_scale),
        float(res_scale), float(out_scale), cfg, _ptr(col_offset), int(mid_zp), int(res_zp), int(out_zp), int(rmod),
        _ptr(out_exp), _ptr(res_exp), ka // 128, ks[0], ks[1], ks[2], _stream())
    _lib.check(status, "i8_gemm_ptf")
    return out


def w8a8_conv_gemm_ptf(x: torch.Tensor, mode: int, wpacked: torch.Tensor, wscale: torch.Tensor, n: int,
                       bias: Optional[torch.Tensor] = None, epilogue: int = EPI_Q8, a_scale: float = 1.0,
                       out_scale: float = 0.0, mid_scale: float = 0.0, res_scale: float = 0.0,
                       res: Optional[torch.Tensor] = None, rmod: int = 0, out: Optional[torch.Tensor] = None,
                       col_offset: Optional[torch.Tensor] = None, mid_zp: int = 0, res_zp: int = 0, out_zp: int = 0,
                       pad16: Optional[torch.Tensor] = None, out_exp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``w8a8_conv_gemm_zp`` with the output quantiser's exponents ``out_exp`` (``samq_w8a8_conv_gemm_ptf``)."""
    _need_cuda(x, wpacked, wscale, bias, res, col_offset, pad16, out_exp)
    _zp(mid_zp, res_zp, out_zp)
    assert x.dtype == torch.int8 and x.is_contiguous() and wscale.dtype == torch.float32
    _col_offset(col_offset, n)
    _exp(out_exp, n, "out_exp")
    assert pad16 is None or (pad16.dtype == torch.int8 and pad16.is_contiguous() and pad16.numel() >= 16), \
        "pad16: 16 int8 bytes expected"
    if mode == 1:
        b, cin, side, _ = x.shape
        g = side // 16
    else:
        b, g, _, cin = x.shape
        side = g
    assert res is None or res.numel() >= (rmod if rmod > 0 else b * g * g) * n, "w8a8_conv_gemm_ptf: residual too small"
    if out is None:
        out = torch.empty((b, g, g, n), dtype=torch.int8, device=x.device)
    assert out.is_cuda and out.dtype == torch.int8 and out.is_contiguous() and out.numel() == b * g * g * n
    _lib.check(_lib.load().samq_w8a8_conv_gemm_ptf(
        _ptr(x), mode, b, cin, side, _ptr(wpacked), _ptr(wscale), _ptr(bias), _ptr(out), _ptr(res), rmod, n, epilogue,
        float(a_scale), float(mid_scale), float(res_scale), float(out_scale), _ptr(col_offset), int(mid_zp),
        int(res_zp), int(out_zp), _ptr(pad16), _ptr(out_exp), _stream()), "w8a8_conv_gemm_ptf")
    return out


def w4a8_gemm(a, wpacked3, wscale, qzeros, n, bias=None, epilogue=EPI_BIAS, a_scale=1.0, out_scale=0.0,
              out=None, groupsize=-1, cfg=0, rowsum=None, rowsum_out=None):
    """GPTQ int4 weights (repacked layout 3) x int8 activation codes (cfg 0 = library pick).
    ``groupsize`` -1 (per-channel, ``wscale`` f32 [N]) or a multiple of 128 (grouped:
    ``wscale`` f32 [G, N], ``qzeros`` [G, N/8]; samq_w4a8_gemm_cfg).  Per-channel only:
    ``rowsum`` (int32 [M]) = the input rows' code sums from their producer (the zero-point
    ping-pong then skips its own), ``rowsum_out`` (int32 [M], zeroed by the caller; int8-code
    epilogues) accumulates the output rows' code sums (``samq_w4a8_gemm_rs``)."""
    if (rowsum is not None or rowsum_out is not None) and groupsize in (-1, a.shape[-1]):
        _need_cuda(a, wpacked3, wscale, bias, qzeros, rowsum, rowsum_out)
        assert a.dtype == torch.int8 and wscale.dtype == torch.float32
        assert bias is None or bias.dtype == torch.float32
        k = a.shape[-1]
        a2 = a.reshape(-1, k)
        _rows_i32(rowsum, a2.shape[0], "w4a8_gemm rowsum")
        _rows_i32(rowsum_out, a2.shape[0], "w4a8_gemm rowsum_out")
        out, o2 = _i8_out(a2, n, epilogue, out, tuple(a.shape[:-1]))
        status = _lib.load().samq_w4a8_gemm_rs(
            _ptr(a2), a2.stride(0), _ptr(wpacked3), _ptr(wscale), _ptr(qzeros), _ptr(bias), _ptr(o2), o2.stride(0),
            a2.shape[0], n, k, epilogue, float(a_scale), float(out_scale), _ptr(rowsum), _ptr(rowsum_out), cfg,
            _stream())
        _lib.check(status, "w4a8_gemm_rs")
        return out
    if groupsize in (-1, a.shape[-1]):
        return i8_gemm(a, _lib.BF_W4, wpacked3, wscale, n, bias, qzeros, epilogue, a_scale, out_scale, out=out,
                       cfg=cfg)
    if groupsize <= 0 or groupsize % 128:
        raise NotImplementedError("w4a8_gemm: grouped weights need groupsize % 128 == 0 (the int8 K tile)")
    if rowsum is not None or rowsum_out is not None:
        raise AssertionError("w4a8_gemm: rowsum / rowsum_out are per-channel only (grouped weights have no row-sum path)")
    _need_cuda(a, wpacked3, wscale, bias, qzeros)
    assert a.dtype == torch.int8 and wscale.dtype == torch.float32
    assert bias is None or bias.dtype == torch.float32
    k = a.shape[-1]
    assert wscale.numel() == ((k + groupsize - 1) // groupsize) * n, "w4a8_gemm: wscale must be f32 [G, N]"
    a2 = a.reshape(-1, k)
    out, o2 = _i8_out(a2, n, epilogue, out, tuple(a.shape[:-1]))
    status = _lib.load().samq_w4a8_gemm_cfg(
        _ptr(a2), a2.stride(0), _ptr(wpacked3), _ptr(wscale), _ptr(qzeros), _ptr(bias), _ptr(o2), o2.stride(0),
        a2.shape[0], n, k, groupsize, epilogue, float(a_scale), float(out_scale), cfg, _stream())
    _lib.check(status, "w4a8_gemm")
    return out


def rel_attention_q8(qkv: torch.Tensor, qkv_bias: Optional[torch.Tensor], rel_pos_h: torch.Tensor,
                     rel_pos_w: torch.Tensor, heads: int, window: int, sm_scale: float, s_qkv: float, s_a1: float,
                     s_a2: float, s_out: float, out: Optional[torch.Tensor] = None,
                     rows: Optional[tuple] = None, v16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W8A8 attention on int8 qkv codes (B, H, W, 3C) -> int8 output codes (B, H, W, C).
    ``rows = (row0, n)``: only the queries (global) / windows (windowed) of grid rows
    [row0, row0 + n) are computed (``samq_rel_attention_q8_rows``).  ``v16``: the V codes as fp16
    (B, H, W, C) from ``w8a8_gemm_v16`` (the global kernel then stages V unconverted)."""
    if v16 is not None:
        _need_cuda(v16)
        assert v16.dtype == torch.float16 and v16.is_contiguous() and v16.numel() == qkv.numel() // 3
    _need_cuda(qkv, qkv_bias, rel_pos_h, rel_pos_w)
    b, h, w, c3 = qkv.shape
    c = c3 // 3
    assert qkv.dtype == torch.int8 and qkv.is_contiguous()
    assert rel_pos_h.dtype == torch.float32 and rel_pos_w.dtype == torch.float32
    assert qkv_bias is None or qkv_bias.dtype == torch.float32
    if out is None:
        out = torch.empty((b, h, w, c), dtype=torch.int8, device=qkv.device)
    r0, nr = rows if rows is not None else (0, -1)
    rel_pos_h, rel_pos_w = rel_pos_h.contiguous(), rel_pos_w.contiguous()   # named: see rel_attention
    _lib.check(_lib.load().samq_rel_attention_q8_rows(
        _ptr(qkv), _ptr(qkv_bias), _ptr(rel_pos_h), _ptr(rel_pos_w), _ptr(out), b, h, w,
        heads, c // heads, window, float(sm_scale), float(s_qkv), float(s_a1), float(s_a2), float(s_out), int(r0),
        int(nr), _ptr(v16), _stream()), "rel_attention_q8")
    return out


def rel_attention_q8_zp(qkv: torch.Tensor, qkv_bias: Optional[torch.Tensor], rel_pos_h: torch.Tensor,
                        rel_pos_w: torch.Tensor, heads: int, window: int, sm_scale: float, s_qkv: float, s_a1: float,
                        s_a2: float, s_out: float, zp_qkv: int, zp_a1: int, zp_a2: int, zp_out: int,
                        out: Optional[torch.Tensor] = None, rows: Optional[tuple] = None,
                        v16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rel_attention_q8`` on codes with zero points (``samq_rel_attention_q8_zp``): qkv codes under
    (s_qkv, zp_qkv), score quantisers (s_a1, zp_a1) / (s_a2, zp_a2), output codes under (s_out, zp_out).
    ``v16`` is refused (NotImplementedError): the 64 x 64 kernel runs on the int8 V codes."""
    _need_cuda(qkv, qkv_bias, rel_pos_h, rel_pos_w, v16)
    _zp(zp_qkv, zp_a1, zp_a2, zp_out)
    b, h, w, c3 = qkv.shape
    c = c3 // 3
    assert qkv.dtype == torch.int8 and qkv.is_contiguous()
    assert rel_pos_h.dtype == torch.float32 and rel_pos_w.dtype == torch.float32
    assert qkv_bias is None or qkv_bias.dtype == torch.float32
    if out is None:
        out = torch.empty((b, h, w, c), dtype=torch.int8, device=qkv.device)
    r0, nr = rows if rows is not None else (0, -1)
    rel_pos_h, rel_pos_w = rel_pos_h.contiguous(), rel_pos_w.contiguous()   # named: see rel_attention
    _lib.check(_lib.load().samq_rel_attention_q8_zp(
        _ptr(qkv), _ptr(qkv_bias), _ptr(rel_pos_h), _ptr(rel_pos_w), _ptr(out), b, h, w,
        heads, c // heads, window, float(sm_scale), float(s_qkv), float(s_a1), float(s_a2), float(s_out), int(r0),
        int(nr), _ptr(v16), int(zp_qkv), int(zp_a1), int(zp_a2), int(zp_out), _stream()), "rel_attention_q8_zp")
    return out



# ----------------------------------------------------------------------------- mask decoder (fq_vit W8A8)
def attention_q8_plain(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, s_q: float, s_k: float,
                       s_v: float, s_a1: float, s_out: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mask decoder's attention on int8 codes (``samq_attention_q8_plain``): q (B, Nq, C), k / v
    (B, Nk, C) codes of qact1_1 / qact1_2 / qact1_3 -> codes of qact2 (B, Nq, C); C = heads * head_dim."""
    _need_cuda(q, k, v, out)
    for t in (q, k, v):
        assert t.dtype == torch.int8 and t.dim() == 3 and t.is_contiguous()
    b, nq, c = q.shape
    nk = k.shape[1]
    assert k.shape == (b, nk, c) and v.shape == (b, nk, c) and c % heads == 0
    if out is None:
        out = torch.empty((b, nq, c), dtype=torch.int8, device=q.device)
    assert out.dtype == torch.int8 and out.is_contiguous() and out.numel() == b * nq * c
    _lib.check(_lib.load().samq_attention_q8_plain(_ptr(q), _ptr(k), _ptr(v), _ptr(out), b, nq, nk, heads, c // heads,
                                                   float(s_q), float(s_k), float(s_v), float(s_a1), float(s_out),
                                                   _stream()), "attention_q8_plain")
    return out


def add_q8(a: torch.Tensor, s_a: float, b: Optional[torch.Tensor], s_b: float, s_out: float, fake: bool = False,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``q8(a * s_a + b * s_b, s_out)`` on int8 codes (``samq_add_q8``), bit-identical to torch's f32 add of
    the two fake-quant tensors + UniformQuantizer.  ``b`` None: the requantisation ``q8(a * s_a, s_out)``;
    a ``b`` with fewer elements is repeated (its numel must divide into whole rows of ``a``: the positional
    encoding shared over the batch).  ``fake``: f32 ``codes * s_out`` instead of int8 codes."""
    _need_cuda(a, b, out)
    assert a.dtype == torch.int8 and a.is_contiguous()
    n = a.numel()
    bmod = n
    if b is not None:
        assert b.dtype == torch.int8 and b.is_contiguous()
        bmod = b.numel()
        assert 0 < bmod <= n and n % bmod == 0 and tuple(b.shape[-1:]) == tuple(a.shape[-1:]), \
            "add_q8: b must tile a along its leading dims"
    if out is None:
        out = torch.empty(a.shape, dtype=torch.float32 if fake else torch.int8, device=a.device)
    assert out.is_contiguous() and out.numel() == n and out.dtype == (torch.float32 if fake else torch.int8)
    _lib.check(_lib.load().samq_add_q8(_ptr(a), float(s_a), _ptr(b), float(s_b), bmod, _ptr(out), n, float(s_out),
                                       _lib.Q_OUT_FQ if fake else 0, _stream()), "add_q8")
    return out


def relu_q8(x: torch.Tensor) -> torch.Tensor:
    """In-place ``max(codes, 0)`` (``samq_relu_q8``): the ReLU of lin1 -> ReLU -> QAct on ``EPI_Q8`` codes."""
    _need_cuda(x)
    assert x.dtype == torch.int8 and x.is_contiguous()
    _lib.check(_lib.load().samq_relu_q8(_ptr(x), x.numel(), _stream()), "relu_q8")
    return x


# ----------------------------------------------------------------------------- mask decoder tail (fq_vit W8A8)
def convt_split_weight(weight: torch.Tensor):
    """A ``ConvTranspose2d(k2 s2)`` fp32 weight [Cin, Cout, 2, 2] -> the (hi, lo) fp16 planes the tail
    kernels read: the GEMM matrix W[n][k] = weight[k][co][kh][kw], n = (2 kh + kw) Cout + co, split
    w = hi + lo 2^-11 and put in MFMA fragment order [4 Cout / 32][Cin / 16][64][8]."""
    cin, cout, kh, kw = weight.shape
    assert (kh, kw) == (2, 2) and cin % 16 == 0 and (4 * cout) % 32 == 0
    w = weight.detach().float().permute(2, 3, 1, 0).reshape(4 * cout, cin)
    hi = w.to(torch.float16)
    lo = ((w - hi.float()) * 2048.0).to(torch.float16)

    def frag(p):   # [N, K] -> [N/32, K/16, khalf, n, 8]: lane = 32 khalf + n
        return p.reshape(4 * cout // 32, 32, cin // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)
    return frag(hi), frag(lo)


def mlp_pack_weight(codes: torch.Tensor, n_pad: int = 0) -> torch.Tensor:
    """int8 weight codes [N, K] of a QLinear -> ``samq_decoder_mlps_q8``'s [K/4][max(N, n_pad)][4]
    (4 consecutive k of an output column in one dword; columns past N zero)."""
    n, k = codes.shape
    assert codes.dtype == torch.int8 and k % 4 == 0
    if n_pad > n:
        codes = torch.cat([codes, codes.new_zeros((n_pad - n, k))])
    return codes.reshape(codes.shape[0], k // 4, 4).permute(1, 0, 2).contiguous()


def upscale0_q8(x: torch.Tensor, w_hi: torch.Tensor, w_lo: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor,
                beta: torch.Tensor, eps: float, b: int, h: int, w: int, s_in: float, s0: float, s1: float, s2: float,
                out: Optional[torch.Tensor] = None, dbg_q0: Optional[torch.Tensor] = None,
                dbg_q1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``samq_upscale0_q8``: key codes (b*h*w, Cin) -> codes of ``qacts[2]`` (b, 2h, 2w, Cout) NHWC;
    ``dbg_q0`` / ``dbg_q1`` (int8, out's shape) receive the codes of ``qacts[0]`` / ``qacts[1]``."""
    _need_cuda(x, w_hi, w_lo, bias, gamma, beta, out, dbg_q0, dbg_q1)
    cout = bias.numel()
    cin = x.shape[-1]
    assert x.dtype == torch.int8 and x.is_contiguous() and x.numel() == b * h * w * cin
    assert w_hi.dtype == torch.float16 and w_lo.dtype == torch.float16
    assert w_hi.numel() == 4 * cout * cin and w_lo.numel() == 4 * cout * cin
    for t in (bias, gamma, beta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == cout
    if out is None:
        out = torch.empty((b, 2 * h, 2 * w, cout), dtype=torch.int8, device=x.device)
    for t in (out, dbg_q0, dbg_q1):
        assert t is None or (t.dtype == torch.int8 and t.is_contiguous() and t.numel() == b * 4 * h * w * cout)
    _lib.check(_lib.load().samq_upscale0_q8(_ptr(x), _ptr(w_hi), _ptr(w_lo), _ptr(bias), _ptr(gamma), _ptr(beta),
                                            _ptr(out), _ptr(dbg_q0), _ptr(dbg_q1), b, h, w, cin, cout, float(eps),
                                            float(s_in), float(s0), float(s1), float(s2), _stream()), "upscale0_q8")
    return out


def decoder_mlps_q8(q: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor, b1: torch.Tensor,
                    b2: torch.Tensor, b3: torch.Tensor, scales: torch.Tensor, n_hyper: int, no_hyper: int, no_iou: int,
                    s_in: float, hyper: Optional[torch.Tensor] = None, iou: Optional[torch.Tensor] = None,
                    dbg: Optional[torch.Tensor] = None):
    """``samq_decoder_mlps_q8``: q (B, Nt, C) codes of the transformer's ``qact4`` -> (hyper codes
    (B, n_hyper, no_hyper) int8, iou_pred (B, no_iou) f32).  Weights from ``mlp_pack_weight`` stacked
    over the n_hyper + 1 MLPs (the IoU head last); ``scales`` (n_hyper + 1, 8) f32 on the device."""
    _need_cuda(q, w1, w2, w3, b1, b2, b3, scales, hyper, iou, dbg)
    assert q.dtype == torch.int8 and q.dim() == 3 and q.is_contiguous()
    b, nt, c = q.shape
    nm = n_hyper + 1
    hd = w2.shape[-2]
    no = max(no_hyper, no_iou)
    assert all(t.dtype == torch.int8 and t.is_contiguous() for t in (w1, w2, w3))
    assert tuple(w1.shape) == (nm, c // 4, hd, 4) and tuple(w2.shape) == (nm, hd // 4, hd, 4)
    assert tuple(w3.shape) == (nm, hd // 4, no, 4)
    for t, shp in ((b1, (nm, hd)), (b2, (nm, hd)), (b3, (nm, no)), (scales, (nm, 8))):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shp
    if hyper is None:
        hyper = torch.empty((b, n_hyper, no_hyper), dtype=torch.int8, device=q.device)
    if iou is None:
        iou = torch.empty((b, no_iou), dtype=torch.float32, device=q.device)
    assert hyper.dtype == torch.int8 and hyper.is_contiguous() and hyper.numel() == b * n_hyper * no_hyper
    assert iou.dtype == torch.float32 and iou.is_contiguous() and iou.numel() == b * no_iou
    assert dbg is None or (dbg.dtype == torch.int8 and dbg.is_contiguous() and dbg.numel() == b * nm * 4 * hd)
    _lib.check(_lib.load().samq_decoder_mlps_q8(_ptr(q), _ptr(w1), _ptr(w2), _ptr(w3), _ptr(b1), _ptr(b2), _ptr(b3),
                                                _ptr(scales), _ptr(hyper), _ptr(iou), _ptr(dbg), b, nt, c, hd, n_hyper,
                                                no_hyper, no_iou, float(s_in), _stream()), "decoder_mlps_q8")
    return hyper, iou


def upscale1_masks_q8(x: torch.Tensor, w_hi: torch.Tensor, w_lo: torch.Tensor, bias: torch.Tensor,
                      hyper: torch.Tensor, s_hyper: torch.Tensor, s_in: float, s3: float, s4: float, s_q1: float,
                      masks: Optional[torch.Tensor] = None, dbg_q3: Optional[torch.Tensor] = None,
                      x4: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``samq_upscale1_masks_q8``: x (B, H, W, Cin) NHWC codes of ``qacts[2]``, hyper (B, M, Cout) codes
    with scales ``s_hyper`` (M,) f32 on the device -> masks (B, M, 2H, 2W) fake-quant f32 (``qact1``);
    ``dbg_q3`` / ``x4`` (int8 (B, 2H, 2W, Cout)) receive the codes of ``qacts[3]`` / ``qacts[4]``."""
    _need_cuda(x, w_hi, w_lo, bias, hyper, s_hyper, masks, dbg_q3, x4)
    assert x.dtype == torch.int8 and x.dim() == 4 and x.is_contiguous()
    b, hh, ww, cin = x.shape
    cout = bias.numel()
    assert w_hi.dtype == torch.float16 and w_lo.dtype == torch.float16
    assert w_hi.numel() == 4 * cout * cin and w_lo.numel() == 4 * cout * cin
    assert bias.dtype == torch.float32 and bias.is_contiguous()
    assert hyper.dtype == torch.int8 and hyper.dim() == 3 and hyper.is_contiguous()
    nm = hyper.shape[1]
    assert tuple(hyper.shape) == (b, nm, cout), "upscale1_masks_q8: hyper must be (B, masks, Cout)"
    assert s_hyper.dtype == torch.float32 and s_hyper.is_contiguous() and s_hyper.numel() == nm
    if masks is None:
        masks = torch.empty((b, nm, 2 * hh, 2 * ww), dtype=torch.float32, device=x.device)
    assert masks.dtype == torch.float32 and masks.is_contiguous() and masks.numel() == b * nm * 4 * hh * ww
    for t in (dbg_q3, x4):
        assert t is None or (t.dtype == torch.int8 and t.is_contiguous() and t.numel() == b * 4 * hh * ww * cout)
    _lib.check(_lib.load().samq_upscale1_masks_q8(_ptr(x), _ptr(w_hi), _ptr(w_lo), _ptr(bias), _ptr(hyper),
                                                  _ptr(s_hyper), _ptr(masks), _ptr(dbg_q3), _ptr(x4), b, hh, ww, cin,
                                                  cout, nm, float(s_in), float(s3), float(s4), float(s_q1), _stream()),
               "upscale1_masks_q8")
    return masks
