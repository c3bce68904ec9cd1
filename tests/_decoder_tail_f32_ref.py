"""Shared pieces of ``test_decoder_tail_f32``: a seeded float decoder whose transformer hands back the test's own
``hs`` / ``keys``, the module tail in float64 / fp32 on the CPU, and the issue's error measure and condition."""
import copy

import torch
import torch.nn as nn


class FixedTransformer(nn.Module):
    """Stands in for the two-way transformer: returns preset tokens and keys (moved / cast with the module)."""

    def __init__(self, hs, keys):
        super().__init__()
        self.register_buffer("hs", hs)
        self.register_buffer("keys", keys)

    def forward(self, src, pos, tokens):
        assert tokens.shape[:2] == self.hs.shape[:2] and src.shape[0] == self.keys.shape[0]
        return self.hs, self.keys


def seeded_decoder(seed):
    """``build_prompt_decoder()``'s mask decoder with seeded random weights (LayerNorm2d's affine included)."""
    from samq.sam_decoder import build_prompt_decoder
    torch.manual_seed(seed)
    dec = build_prompt_decoder()[1].eval()
    with torch.no_grad():
        ln = dec.output_upscaling[1]
        ln.weight.copy_(1.0 + 0.5 * torch.randn(ln.weight.shape))
        ln.bias.copy_(0.5 * torch.randn(ln.bias.shape))
    return dec


def run(dec, b, n_tokens, h, w):
    """``predict_masks`` on inputs of the right shapes (their values never reach a FixedTransformer's outputs)."""
    p = next(dec.parameters())
    z = lambda *s: torch.zeros(s, dtype=p.dtype, device=p.device)
    with torch.no_grad():
        return dec.predict_masks(z(1, 256, h, w), z(1, 256, h, w), z(b, n_tokens - 5, 256), z(b, 256, h, w))


def tail_case(seed, b, n_tokens, h, w, scale=1.0):
    """(decoder fp32 on the CPU with a FixedTransformer, masks64, iou64, hyper64): the float64 module on the same
    ``hs`` / ``keys``."""
    dec = seeded_decoder(seed)
    g = torch.Generator().manual_seed(seed + 1)
    dec.transformer = FixedTransformer(torch.randn((b, n_tokens, 256), generator=g),
                                       scale * torch.randn((b, h * w, 256), generator=g))
    d64 = copy.deepcopy(dec).double()
    masks, iou = run(d64, b, n_tokens, h, w)
    with torch.no_grad():
        hyper = torch.stack([m(d64.transformer.hs[:, 1 + i]) for i, m in enumerate(d64.output_hypernetworks_mlps)], 1)
    return dec, masks, iou, hyper


def err(x, ref64):
    return ((x.detach().double().cpu() - ref64).abs().max() / ref64.abs().max()).item()


def check(name, fused, module32, ref64):
    """The accuracy condition: e(fused) <= 4 e(fp32 module) + 2^-22, both against the float64 module."""
    e_f, e_m = err(fused, ref64), err(module32, ref64)
    print(f"[decoder_tail_f32] {name}: e(fused) {e_f:.3e}  e(module fp32) {e_m:.3e}")
    assert torch.isfinite(fused).all()
    assert e_f <= 4 * e_m + 2.0 ** -22, (name, e_f, e_m)
