"""Inputs and references of the fq_vit W8A8 mask decoder tests (``test_fq_decoder.py``) and of the
golden generator ``golden/make_golden_fq_decoder.py``.

* ``decoder_state`` / ``prompt_set`` / ``image_embedding``: the seeded weights (rounded through
  fp16, like the encoder fixtures), prompts and image embeddings both the reference run (the
  generator) and the tests build, so the fixture needs to store results only.
* ``attention_ref`` / ``transformer_ref``: plain torch restatements of one decoder attention
  (``fq_vit/models/sam/transformer.py:511-541``) and of the two-way transformer (``:103-149``,
  ``:332-371``) on fake-quant values, in fp32 or fp64 -- what ``tests/_attn_q8_ref.py`` is for the
  encoder's attention.
* ``attn_inputs`` / ``exact_attn_inputs``: the attention kernel's test inputs.
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

GRID = 16                      # embedding grid of the fixture (input 256, patch 16)
IMG = GRID * 16
STATE_SEED = 4100
CALIB_SEEDS, TEST_SEED = (41, 42, 43), 44
STAGE_SHAPE = "point_box"      # the prompt shape of the stage-local test
STAGE_ROWS_MAX = 20000         # QAct outputs up to this size (the token rows) are stored in the golden
PROMPT_SHAPES = ("point", "point_box")   # N_tokens = 5 + 2 and 5 + 4, see prompt_set


# ----------------------------------------------------------------------------- seeded model inputs
def decoder_state(shapes: dict, seed: int = STATE_SEED) -> dict:
    """name -> f32 array (every value exactly representable in fp16) for the parameters / buffers of
    the prompt encoder + mask decoder, given their shapes.  One generator per name (seed + crc32 of
    the name), so the values do not depend on the iteration order of the dict."""
    out = {}
    for name, shape in shapes.items():
        rng = np.random.Generator(np.random.PCG64(seed + zlib.crc32(name.encode())))
        shape = tuple(shape)
        leaf = name.rsplit(".", 1)[-1]
        norm = any(t in name for t in (".norm", "norm_final_attn", "output_upscaling.1.", "mask_downscaling.1.",
                                       "mask_downscaling.4."))
        if name.endswith("positional_encoding_gaussian_matrix"):
            v = rng.standard_normal(shape)
        elif norm and leaf == "weight":
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif leaf == "bias":
            v = 0.05 * rng.standard_normal(shape)
        elif len(shape) >= 2 and not any(t in name for t in ("iou_token", "mask_tokens", "point_embeddings",
                                                             "not_a_point_embed", "no_mask_embed")):
            fan_in = int(np.prod(shape[1:])) if "output_upscaling" not in name else shape[0] * 4
            v = rng.standard_normal(shape) * (1.5 / math.sqrt(fan_in))
        else:   # embeddings / tokens
            v = 0.5 * rng.standard_normal(shape)
        out[name] = v.astype(np.float16).astype(np.float32)
    return out


def image_embedding(seed: int, grid: int = GRID, c: int = 256) -> np.ndarray:
    """A (1, C, grid, grid) f32 image embedding: smooth per-channel structure + noise, O(1) values."""
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    yy, xx = np.meshgrid(np.linspace(-1, 1, grid), np.linspace(-1, 1, grid), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, (c, 1, 1))
    fx, fy = rng.uniform(0.5, 3, (c, 1, 1)), rng.uniform(0.5, 3, (c, 1, 1))
    e = np.sin(fx * xx[None] * np.pi + ph) * np.cos(fy * yy[None] * np.pi) + 0.3 * rng.standard_normal((c, grid, grid))
    return e[None].astype(np.float16).astype(np.float32)


def prompt_set(seed: int, shape: str, img: int = IMG):
    """(point coords (1, P, 2), labels (1, P), box (1, 4) or None) in input-image pixels.
    ``point``: one positive point, padded by the prompt encoder -> 5 + 2 tokens; ``point_box``: a
    positive and a negative point and a box (no padding point) -> 5 + 4 tokens."""
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    npt = 2 if shape == "point_box" else 1
    pt = rng.uniform(0.15 * img, 0.85 * img, (1, npt, 2)).astype(np.float32)
    lab = np.array([[1, 0][:npt]], np.int32)
    box = None
    if shape == "point_box":
        c = rng.uniform(0.3 * img, 0.7 * img, 2)
        half = rng.uniform(0.1 * img, 0.25 * img, 2)
        box = np.concatenate([c - half, c + half])[None].astype(np.float32)
    return pt, lab, box


# ----------------------------------------------------------------------------- restatements
def fake_quant(x: torch.Tensor, s) -> torch.Tensor:
    s = torch.as_tensor(float(s), dtype=x.dtype)
    return torch.clamp(torch.round(x / s), -128, 127) * s


def attention_ref(qc, kc, vc, heads, s_q, s_k, s_v, s_a1, s_out, dtype=torch.float32):
    """Output codes (float array) of the decoder attention core on int8 codes (B, N, C)."""
    t = lambda a, s: torch.from_numpy(np.asarray(a).astype(np.float32)).to(dtype) * torch.tensor(float(s), dtype=dtype)
    q, k, v = t(qc, s_q), t(kc, s_k), t(vc, s_v)
    b, nq, c = q.shape
    d = c // heads
    sp = lambda x: x.reshape(b, x.shape[1], heads, d).transpose(1, 2)
    q, k, v = sp(q), sp(k), sp(v)
    attn = fake_quant((q @ k.permute(0, 1, 3, 2)) / math.sqrt(d), s_a1)
    o = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(b, nq, c)
    return np.clip(np.round((o / torch.tensor(float(s_out), dtype=dtype)).numpy()), -128, 127)


def transformer_ref(sd: dict, tokens, src, pos, dtype=torch.float32, prefix="transformer.", depth=2, heads=8,
                    taps=None):
    """The two-way transformer in quant mode on fake-quant inputs: ``tokens`` (B, Nt, C), ``src``
    (B, hw, C), ``pos`` (1, hw, C) (the values of qact_embed1 / qact_embed2 / pos_src_qact as token
    rows).  ``sd``: the mask decoder's state dict (f32 tensors, ``...quantizer.scale`` included).
    Weight codes are computed in f32 as the reference does; everything else in ``dtype``."""
    cast = lambda a: torch.as_tensor(a).to(dtype)

    def scale(name):
        return float(torch.as_tensor(sd[prefix + name + ".quantizer.scale"]).reshape(-1)[0])

    def act(x, name):
        return fake_quant(x, scale(name))

    def lin(x, name):
        w = torch.as_tensor(sd[prefix + name + ".weight"]).float()
        s = torch.as_tensor(sd[prefix + name + ".quantizer.scale"]).float().reshape(-1, 1)
        wq = torch.clamp(torch.round(w / s), -128, 127) * s
        return x @ cast(wq).T + cast(sd[prefix + name + ".bias"])

    def ln(x, name):
        return F.layer_norm(x, (x.shape[-1],), cast(sd[prefix + name + ".weight"]), cast(sd[prefix + name + ".bias"]),
                            1e-5)

    def attn(p, q, k, v):
        q, k, v = act(lin(q, p + "q_proj"), p + "qact1_1"), act(lin(k, p + "k_proj"), p + "qact1_2"), \
            act(lin(v, p + "v_proj"), p + "qact1_3")
        b, _, c = q.shape
        d = c // heads
        sp = lambda x: x.reshape(b, x.shape[1], heads, d).transpose(1, 2)
        q, k, v = sp(q), sp(k), sp(v)
        a = act((q @ k.permute(0, 1, 3, 2)) / math.sqrt(d), p + "qact_attn1")
        o = (torch.softmax(a, dim=-1) @ v).transpose(1, 2).reshape(b, -1, c)
        return act(lin(act(o, p + "qact2"), p + "out_proj"), p + "qact3")

    tokens, keys, pos = cast(tokens), cast(src), cast(pos)
    queries = tokens
    for i in range(depth):
        L = f"layers.{i}."
        if i == 0:
            queries = act(attn(L + "self_attn.", queries, queries, queries), L + "qact2")
        else:
            q = act(queries + act(tokens, L + "qact_pos"), L + "qact1")
            queries = act(queries + attn(L + "self_attn.", q, q, queries), L + "qact2")
        queries = act(ln(queries, L + "norm1"), L + "qact3")
        q, k = act(queries + tokens, L + "qact4"), act(keys + pos, L + "qact5")
        queries = act(queries + attn(L + "cross_attn_token_to_image.", q, k, keys), L + "qact6")
        queries = act(ln(queries, L + "norm2"), L + "qact7")
        h = act(torch.relu(lin(queries, L + "mlp.lin1")), L + "mlp.qact1")
        queries = act(queries + act(act(lin(h, L + "mlp.lin2"), L + "mlp.qact2"), L + "qact8"), L + "qact9")
        queries = act(ln(queries, L + "norm3"), L + "qact10")
        q, k = act(queries + tokens, L + "qact11"), act(keys + pos, L + "qact12")
        keys = act(keys + attn(L + "cross_attn_image_to_token.", k, q, queries), L + "qact13")
        keys = act(ln(keys, L + "norm4"), L + "qact14")
        if taps is not None:
            taps[L + "queries"], taps[L + "keys"] = queries, keys
    q, k = act(queries + tokens, "qact1"), act(keys + pos, "qact2")
    queries = act(queries + attn("final_attn_token_to_image.", q, k, keys), "qact3")
    return act(ln(queries, "norm_final_attn"), "qact4"), keys


# ----------------------------------------------------------------------------- attention kernel inputs
# (B, H, D, Nq, Nk): one case per launch branch of samq_attention_q8_plain and its tails --
# one lane per query at D = 32 (tokens x tokens) and D = 16 (image x tokens; Nq past one 256-lane
# block, Nk past one 64-key LDS tile), keys over the lanes at 1 / 2 / 4 / 8 waves (Nk = 515 and 4096:
# not a multiple of the lane count, several strides), at D = 16 and D = 32
ATTN_CASES = [(1, 8, 32, 7, 7), (2, 8, 32, 9, 9), (1, 8, 16, 7, 256), (1, 8, 16, 7, 515), (1, 8, 16, 9, 4096),
              (2, 8, 16, 1, 300), (1, 8, 16, 5, 67), (1, 8, 32, 5, 130), (1, 8, 16, 256, 7), (1, 8, 16, 200, 9),
              (1, 4, 16, 300, 70)]
# score side exact in fp32 (power-of-two s_q, s_k, s_a1: the kernel's and both restatements' score
# codes agree bit for bit at D = 16, so the comparison measures the softmax and the output
# quantiser); s_v arbitrary, s_out sized to the output's spread (the softmax averages ~Nk / 6 of
# the random values: std ~ 1.48 / sqrt(Nk / 6)) so the codes fill the int8 range and a few clamp
def attn_scales(case):
    """(s_q, s_k, s_v, s_a1, s_out) of an ATTN_CASES entry."""
    nk = case[4]
    s_out = np.float32(2.5 * 1.48 / math.sqrt(max(1.0, nk / 6.0)) / 127.5)
    return 2.0 ** -6, 2.0 ** -6, np.float32(0.02), 2.0 ** -5, s_out


def attn_inputs(case, seed=0):
    """Full-range random codes; query 0 of every batch is all zero (an all-equal-scores row: its
    softmax is uniform over every key chunk)."""
    b, h, d, nq, nk = case
    rng = np.random.Generator(np.random.PCG64(1234 + seed + zlib.crc32(repr(case).encode())))
    q = rng.integers(-128, 128, (b, nq, h * d), dtype=np.int8)
    k = rng.integers(-128, 128, (b, nk, h * d), dtype=np.int8)
    v = rng.integers(-128, 128, (b, nk, h * d), dtype=np.int8)
    q[:, 0, :] = 0
    return q, k, v


EXACT_CASES = [(1, 8, 16, 7, 192), (1, 8, 16, 100, 9), (1, 8, 32, 6, 6)]


# "peaked" scale set: s_q = s_k = 1, s_a1 = 2^-1 -- q.k s_q s_k / sqrt(D) / s_a1 is dot / 2 as with the
# plain set (the same integer score codes, the same exact ties), the softmax argument code * s_a1
# 16 times larger: one code step is a factor e^0.5, rows are near one-hot, and the running maxima of
# the lanes, waves and workgroup partial states lie many e-folds apart.  With the two larger cases:
# keys over the lanes at 8 waves (Nk = 4096) and one lane per query past one block (Nq = 300).
EXACT_PEAKED_CASES = EXACT_CASES + [(1, 8, 16, 9, 4096), (1, 8, 16, 300, 70)]
EXACT_PEAKED_SCORE_SCALES = (1.0, 1.0, 2.0 ** -1)     # s_q, s_k, s_a1


def exact_attn_inputs(case, seed=0, peaked=False):
    """Small integer codes and power-of-two scales: q.k * s_q s_k / sqrt(D) / s_a1 = dot / 2 at
    D = 16 (every odd dot an exact tie of the score quantiser, D = 32: dot / (2 sqrt 2)), scores a
    few codes apart so many keys carry weight; v codes * 2^-3.  s_out is NOT a power of two: after the
    softmax no output quotient is exact, and a power-of-two s_out would put the uniform rows' (query 0,
    all zero) quotients sum(v) / (Nk / 2) on exact .5 ties that neither fp32 nor fp64 resolves the
    same way -- the condition test_exact_attention_inputs_fp32_vs_fp64 checks.
    ``peaked``: the same codes with EXACT_PEAKED_SCORE_SCALES.
    Returns (q, k, v, scales)."""
    b, h, d, nq, nk = case
    rng = np.random.Generator(np.random.PCG64(4321 + seed + zlib.crc32(repr(case).encode())))
    q = rng.integers(-3, 4, (b, nq, h * d), dtype=np.int8)
    k = rng.integers(-3, 4, (b, nk, h * d), dtype=np.int8)
    v = rng.integers(-128, 128, (b, nk, h * d), dtype=np.int8)
    q[:, 0, :] = 0
    s_q, s_k, s_a1 = EXACT_PEAKED_SCORE_SCALES if peaked else (2.0 ** -2, 2.0 ** -2, 2.0 ** -5)
    return q, k, v, (s_q, s_k, 2.0 ** -3, s_a1, float(np.float32(0.0371)))


# (B, H, D, Nq, Nk): uniform softmax rows whose output quotients are exact, ties included -- one lane per
# query (Nk = 1, 2, 64) and keys over the lanes at 1 and 2 waves (Nk = 128, 256)
TIE_CASES = [(1, 8, 16, 3, 1), (1, 8, 32, 3, 2), (2, 8, 16, 20, 64), (1, 8, 16, 3, 128), (1, 8, 32, 2, 256)]
TIE_DIV = {1: 2, 2: 2, 64: 16, 128: 32, 256: 32}      # output quotient = sum(v) / TIE_DIV[Nk]


def tie_scales(case):
    """(s_q, s_k, s_v, s_a1, s_out), all powers of two, s_out = s_v * TIE_DIV[Nk] / Nk."""
    nk = case[4]
    return 2.0 ** -2, 2.0 ** -2, 2.0 ** -3, 2.0 ** -5, 2.0 ** -3 * TIE_DIV[nk] / nk


def output_tie_inputs(case, seed=0):
    """All-zero queries: every score code is 0, the softmax weights are exactly 1 / Nk (Nk a power of
    two), so with ``tie_scales`` every output quotient is sum(v) / TIE_DIV[Nk] exactly -- in fp32, in
    fp64 and in the kernel (integer sums below 2^24) -- and lands on exact .5 ties (and some clamps)
    that the output quantiser must round half to even.  Returns (q, k, v, expected codes, quotients)."""
    b, h, d, nq, nk = case
    rng = np.random.Generator(np.random.PCG64(999 + seed + zlib.crc32(repr(case).encode())))
    q = np.zeros((b, nq, h * d), np.int8)
    k = rng.integers(-128, 128, (b, nk, h * d), dtype=np.int8)
    v = rng.integers(-128, 128, (b, nk, h * d), dtype=np.int8)
    quot = v.astype(np.float64).sum(axis=1, keepdims=True) / TIE_DIV[nk]
    want = np.clip(np.round(quot), -128, 127)            # numpy rounds half to even
    return q, k, v, np.broadcast_to(want, (b, nq, h * d)), quot


def off_by_one(a, b):
    """(max |a - b|, fraction of codes that differ)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(d.max()), float((d > 0).mean())
