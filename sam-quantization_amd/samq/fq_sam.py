"""fq_vit W8A8 SAM prompt encoder + mask decoder: module API of the reference + the fused HIP engine
of the two-way transformer.

Mirrors (module and attribute names, constructor arguments, QAct positions, ``quantizer.scale``
buffers) the decoder half of the reference's "fully quantised" SAM, so a calibrated state dict loads
key for key:

* ``PromptEncoder`` (``fq_vit/models/sam/prompt_encoder.py:17-246``);
* ``MaskDecoder`` / ``MLP`` (``mask_decoder.py:17-362``), ``QConvTranspose2d`` (``ptq/layers.py:77-157``);
* ``TwoWayTransformer`` / ``TwoWayAttentionBlock`` / ``Attention`` (``transformer.py:17-541``);
* ``Sam`` with its five switches (``sam.py:20-235``) and ``build_fq_sam`` (``build_sam.py``).

Quirks of the reference kept as they are (``tests/golden/fq_decoder.npz`` pins them):

* ``Sam.model_quant`` and the other switches select ``type(m) in [QConv2d, QLinear, QAct,
  QIntSoftmax]`` -- ``QConvTranspose2d`` is not in the list, so the two output-upscaling transposed
  convolutions are never calibrated and always run their float weights;
* ``MLP`` builds its layers as bare ``QLinear(n, k)``: layer-wise (one scalar) int8 weight scales;
  it assigns ``qact3`` twice, as ``MaskDecoder`` does ``pos_src_qact``;
* ``final_attn_token_to_image`` is constructed without ``quant`` / ``calibrate`` (the switches set
  them afterwards all the same);
* the quantised ``MaskDecoder`` does not repeat the image embedding per prompt: ``src`` is
  ``image_embeddings + dense_prompt_embeddings`` by broadcasting (``mask_decoder.py:244-246``);
* attention scores are ``q @ k^T / sqrt(c_per_head)`` then ``qact_attn1``; ``QIntSoftmax`` and
  ``QIntLayerNorm`` (eps 1e-5) are the float ops; the MLP activation is ReLU.

Supported configuration as for the encoder: ``Config(False, False, m)`` with ``BIT_TYPE_A = int8``.
Float / calibration forwards and the CPU run the module graph with torch ops.  In quant mode on a
GPU ``MaskDecoder.predict_masks`` runs through ``W8A8DecoderEngine``: int8 codes between HIP kernels
from ``qact_embed1`` to the low-res masks and ``iou_pred`` (the two-way transformer, then three
kernels for the output upscaling, the hypernetwork MLPs, the IoU head and the mask product), one
HIP graph per token count.  ``use_fused_tail = False`` keeps the module graph (``heads_forward``,
HIP fake-quant ``QAct``) behind the transformer; the prompt encoder is the module graph.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple, Type

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import sam_decoder
from .build_sam import Sam as _FloatSam
from .fq_vit import (BIT_TYPE_DICT, Config, QAct, QConv2d, QIntLayerNorm, QIntLayerNorm2D, QIntSoftmax, QLinear,
                     _QFlags, _qact, _qconv, _qlinear, _s, build_fq_image_encoder, sam_w8a8_config)


class QConvTranspose2d(nn.ConvTranspose2d, _QFlags):
    """``layers.py:77-157``.  Not in the switches' type list: stays float and uncalibrated."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, dilation=1,
                 groups=1, bias=True, quant=False, calibrate=False, last_calibrate=False,
                 bit_type=BIT_TYPE_DICT["int8"], calibration_mode="layer_wise", observer_str="minmax",
                 quantizer_str="uniform"):
        nn.ConvTranspose2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                                    output_padding=output_padding, dilation=dilation, groups=groups, bias=bias)
        self._init_q(quant, calibrate, last_calibrate, bit_type, calibration_mode, observer_str, quantizer_str,
                     "conv_weight")

    def forward(self, x, output_size=None):
        self._observe(self.weight, x)
        w = self.quantizer(self.weight) if self.quant else self.weight
        op = self._output_padding(x, output_size, self.stride, self.padding, self.kernel_size, 2, self.dilation)
        return F.conv_transpose2d(x, w, self.bias, self.stride, self.padding, op, self.groups, self.dilation)


def _refuse_ptf(cfg, who: str) -> None:
    """The prompt encoder / mask decoder mirror has no Power-of-Two Factor quantisers (``Config(ptf=True)``):
    its ``ln=True`` QActs are not at the reference's places and the decoder engine and tail are layer-wise."""
    if cfg is not None and cfg.INT_NORM:
        raise NotImplementedError(f"{who}: Config(ptf=True) (INT_NORM, Power-of-Two Factor activations) is "
                                  "supported by the image encoder only")


def _qconvT(cfg, i, o, quant, calibrate):
    return QConvTranspose2d(i, o, kernel_size=2, stride=2, quant=quant, calibrate=calibrate, bit_type=cfg.BIT_TYPE_W,
                            calibration_mode=cfg.CALIBRATION_MODE_W, observer_str=cfg.OBSERVER_W,
                            quantizer_str=cfg.QUANTIZER_W)


# ----------------------------------------------------------------------------- prompt encoder
class PromptEncoder(sam_decoder.PromptEncoder):
    """``prompt_encoder.py:17-246``: the float prompt encoder's point / box embedding with the mask
    branch as ``QConv2d`` / ``QIntLayerNorm2D`` / GELU, a ``QAct`` after each of the seven."""

    def __init__(self, embed_dim: int, image_embedding_size: Tuple[int, int], input_image_size: Tuple[int, int],
                 mask_in_chans: int, activation: Type[nn.Module] = nn.GELU, quant=False, calibrate=False,
                 input_quant=False, cfg: Optional[Config] = None):
        nn.Module.__init__(self)
        cfg = cfg or sam_w8a8_config()
        _refuse_ptf(cfg, "PromptEncoder")
        self.embed_dim = embed_dim
        self.input_image_size = input_image_size
        self.image_embedding_size = image_embedding_size
        self.pe_layer = sam_decoder.PositionEmbeddingRandom(embed_dim // 2)
        self.num_point_embeddings = 4
        self.point_embeddings = nn.ModuleList([nn.Embedding(1, embed_dim) for _ in range(4)])
        self.not_a_point_embed = nn.Embedding(1, embed_dim)
        self.mask_input_size = (4 * image_embedding_size[0], 4 * image_embedding_size[1])
        c4 = mask_in_chans // 4
        self.mask_downscaling = nn.ModuleList([
            _qconv(cfg, 1, c4, 2, stride=2, quant=quant, calibrate=calibrate), QIntLayerNorm2D(c4), activation(),
            _qconv(cfg, c4, mask_in_chans, 2, stride=2, quant=quant, calibrate=calibrate),
            QIntLayerNorm2D(mask_in_chans), activation(),
            _qconv(cfg, mask_in_chans, embed_dim, 1, quant=quant, calibrate=calibrate)])
        self.qacts = nn.ModuleList([_qact(cfg, quant, calibrate, ln=i in (0, 3)) for i in range(7)])
        self.no_mask_embed = nn.Embedding(1, embed_dim)

    def get_dense_pe(self) -> torch.Tensor:
        """The same tensor on every call while the Gaussian matrix is unchanged: the decoder engine
        recognises the image side it has already quantised by its tensors."""
        g = self.pe_layer.positional_encoding_gaussian_matrix
        key = (g.data_ptr(), _tensor_version(g), g.device, g.dtype)
        if self.__dict__.get("_dense_pe_key") != key or key[1] is None:
            self.__dict__["_dense_pe"] = super().get_dense_pe()
            self.__dict__["_dense_pe_key"] = key
        return self.__dict__["_dense_pe"]

    def _embed_masks(self, masks: torch.Tensor) -> torch.Tensor:
        x = masks
        for i, mod in enumerate(self.mask_downscaling):
            x = self.qacts[i](mod(x))
        return x

    def forward(self, points, boxes, masks):
        sparse, dense = super().forward(points, boxes, None)
        if masks is not None:
            dense = self._embed_masks(masks)
        return sparse, dense


# ----------------------------------------------------------------------------- two-way transformer
class MLPBlock(nn.Module):
    """``common.py:15-71`` with the reference's positional arguments (``transformer.py:317``)."""

    def __init__(self, embedding_dim, mlp_dim, act: Type[nn.Module] = nn.GELU, quant=False, calibrate=False,
                 cfg: Optional[Config] = None):
        super().__init__()
        self.lin1 = _qlinear(cfg, embedding_dim, mlp_dim, True, quant, calibrate)
        self.qact1 = _qact(cfg, quant, calibrate)
        self.lin2 = _qlinear(cfg, mlp_dim, embedding_dim, True, quant, calibrate)
        self.qact2 = _qact(cfg, quant, calibrate)
        self.act = act()

    def forward(self, x):
        return self.qact2(self.lin2(self.qact1(self.act(self.lin1(x)))))


class Attention(nn.Module):
    """``transformer.py:374-541``."""

    def __init__(self, embedding_dim: int, num_heads: int, downsample_rate: int = 1, quant=False, calibrate=False,
                 cfg: Optional[Config] = None):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.internal_dim = embedding_dim // downsample_rate
        self.num_heads = num_heads
        assert self.internal_dim % num_heads == 0, "num_heads must divide embedding_dim."
        self.q_proj = _qlinear(cfg, embedding_dim, self.internal_dim, True, quant, calibrate)
        self.k_proj = _qlinear(cfg, embedding_dim, self.internal_dim, True, quant, calibrate)
        self.v_proj = _qlinear(cfg, embedding_dim, self.internal_dim, True, quant, calibrate)
        self.qact1_1 = _qact(cfg, quant, calibrate, permute=False)
        self.qact1_2 = _qact(cfg, quant, calibrate, permute=False)
        self.qact1_3 = _qact(cfg, quant, calibrate, permute=False)
        self.qact2 = _qact(cfg, quant, calibrate, permute=False)
        self.out_proj = _qlinear(cfg, self.internal_dim, embedding_dim, True, quant, calibrate)
        self.qact3 = _qact(cfg, quant, calibrate, permute=False)
        self.qact_attn1 = _qact(cfg, quant, calibrate, permute=False)
        self.log_int_softmax = QIntSoftmax(log_i_softmax=cfg.INT_SOFTMAX, quant=quant, calibrate=calibrate,
                                           bit_type=cfg.BIT_TYPE_S, calibration_mode=cfg.CALIBRATION_MODE_S,
                                           observer_str=cfg.OBSERVER_S, quantizer_str=cfg.QUANTIZER_S)

    def _separate_heads(self, x, num_heads):
        b, n, c = x.shape
        return x.reshape(b, n, num_heads, c // num_heads).transpose(1, 2)

    def forward(self, q, k, v):
        q = self._separate_heads(self.qact1_1(self.q_proj(q)), self.num_heads)
        k = self._separate_heads(self.qact1_2(self.k_proj(k)), self.num_heads)
        v = self._separate_heads(self.qact1_3(self.v_proj(v)), self.num_heads)
        attn = q @ k.permute(0, 1, 3, 2)
        attn = self.qact_attn1(attn / math.sqrt(q.shape[-1]))
        attn = self.log_int_softmax(attn, self.qact_attn1.quantizer.scale)
        out = (attn @ v).transpose(1, 2)
        out = out.reshape(out.shape[0], out.shape[1], -1)
        return self.qact3(self.out_proj(self.qact2(out)))


class TwoWayAttentionBlock(nn.Module):
    """``transformer.py:152-371``."""

    def __init__(self, embedding_dim: int, num_heads: int, mlp_dim: int = 2048,
                 activation: Type[nn.Module] = nn.ReLU, attention_downsample_rate: int = 2,
                 skip_first_layer_pe: bool = False, quant=False, calibrate=False, cfg: Optional[Config] = None):
        super().__init__()
        _refuse_ptf(cfg, "TwoWayAttentionBlock")
        if not skip_first_layer_pe:
            self.qact_pos = _qact(cfg, quant, calibrate, permute=False)
            self.qact1 = _qact(cfg, quant, calibrate, permute=False)
        for i in range(2, 15):   # qact2, 6, 9, 13 take the LayerNorm-input settings
            setattr(self, f"qact{i}", _qact(cfg, quant, calibrate, ln=i in (2, 6, 9, 13)))
        self.self_attn = Attention(embedding_dim, num_heads, quant=quant, calibrate=calibrate, cfg=cfg)
        self.norm1 = QIntLayerNorm(embedding_dim)
        self.cross_attn_token_to_image = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate,
                                                   quant=quant, calibrate=calibrate, cfg=cfg)
        self.norm2 = QIntLayerNorm(embedding_dim)
        self.mlp = MLPBlock(embedding_dim, mlp_dim, activation, quant, calibrate, cfg)
        self.norm3 = QIntLayerNorm(embedding_dim)
        self.norm4 = QIntLayerNorm(embedding_dim)
        self.cross_attn_image_to_token = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate,
                                                   quant=quant, calibrate=calibrate, cfg=cfg)
        self.skip_first_layer_pe = skip_first_layer_pe

    def forward(self, queries, keys, query_pe, key_pe):
        if self.skip_first_layer_pe:
            queries = self.qact2(self.self_attn(q=queries, k=queries, v=queries))
        else:
            q = self.qact1(queries + self.qact_pos(query_pe))
            queries = self.qact2(queries + self.self_attn(q=q, k=q, v=queries))
        queries = self.qact3(self.norm1(queries))
        q = self.qact4(queries + query_pe)
        k = self.qact5(keys + key_pe)
        queries = self.qact6(queries + self.cross_attn_token_to_image(q=q, k=k, v=keys))
        queries = self.qact7(self.norm2(queries))
        queries = self.qact9(queries + self.qact8(self.mlp(queries)))
        queries = self.qact10(self.norm3(queries))
        q = self.qact11(queries + query_pe)
        k = self.qact12(keys + key_pe)
        keys = self.qact13(keys + self.cross_attn_image_to_token(q=k, k=q, v=queries))
        keys = self.qact14(self.norm4(keys))
        return queries, keys


class TwoWayTransformer(nn.Module):
    """``transformer.py:17-149``."""

    def __init__(self, depth: int, embedding_dim: int, num_heads: int, mlp_dim: int,
                 activation: Type[nn.Module] = nn.ReLU, attention_downsample_rate: int = 2, quant=False,
                 calibrate=False, cfg: Optional[Config] = None):
        super().__init__()
        _refuse_ptf(cfg, "TwoWayTransformer")
        self.depth, self.embedding_dim, self.num_heads, self.mlp_dim = depth, embedding_dim, num_heads, mlp_dim
        self.layers = nn.ModuleList([
            TwoWayAttentionBlock(embedding_dim=embedding_dim, num_heads=num_heads, mlp_dim=mlp_dim,
                                 activation=activation, attention_downsample_rate=attention_downsample_rate,
                                 skip_first_layer_pe=(i == 0), quant=quant, calibrate=calibrate, cfg=cfg)
            for i in range(depth)])
        self.final_attn_token_to_image = Attention(embedding_dim, num_heads, downsample_rate=attention_downsample_rate,
                                                   cfg=cfg)
        self.norm_final_attn = QIntLayerNorm(embedding_dim)
        self.qact1 = _qact(cfg, quant, calibrate)
        self.qact2 = _qact(cfg, quant, calibrate)
        self.qact4 = _qact(cfg, quant, calibrate, permute=False)
        self.qact3 = _qact(cfg, quant, calibrate, ln=True, permute=False)

    def forward(self, image_embedding, image_pe, point_embedding, taps: Optional[dict] = None):
        """``taps`` (tests): receives every block's output ``layers.<i>.queries`` / ``.keys``."""
        image_embedding = image_embedding.flatten(2).permute(0, 2, 1)
        image_pe = image_pe.flatten(2).permute(0, 2, 1)
        queries, keys = point_embedding, image_embedding
        for i, layer in enumerate(self.layers):
            queries, keys = layer(queries=queries, keys=keys, query_pe=point_embedding, key_pe=image_pe)
            if taps is not None:
                taps[f"layers.{i}.queries"], taps[f"layers.{i}.keys"] = queries, keys
        q = self.qact1(queries + point_embedding)
        k = self.qact2(keys + image_pe)
        queries = self.qact3(queries + self.final_attn_token_to_image(q=q, k=k, v=keys))
        return self.qact4(self.norm_final_attn(queries)), keys


# ----------------------------------------------------------------------------- mask decoder
class MLP(nn.Module):
    """``mask_decoder.py:284-362``: bare ``QLinear(n, k)`` layers (layer-wise weight scales)."""

    def __init__(self, input_dim: int, hidden_dim: int, output_dim: int, num_layers: int, sigmoid_output: bool = False,
                 quant=False, calibrate=False, cfg: Optional[Config] = None):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(QLinear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))
        self.sigmoid_output = sigmoid_output
        self.qacts1 = nn.ModuleList([_qact(cfg, quant, calibrate) for _ in range(num_layers - 1)])
        self.qacts2 = nn.ModuleList([_qact(cfg, quant, calibrate) for _ in range(num_layers - 1)])
        self.qact3 = _qact(cfg, quant, calibrate)
        self.qact3 = _qact(cfg, quant, calibrate)
        self.qact4 = _qact(cfg, quant, calibrate)

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            if i < self.num_layers - 1:
                x = self.qacts2[i](F.relu(self.qacts1[i](layer(x))))
            else:
                x = self.qact3(layer(x))
        if self.sigmoid_output:
            x = self.qact4(torch.sigmoid(x))
        return x


class MaskDecoder(nn.Module):
    """``mask_decoder.py:17-279``."""

    def __init__(self, *, transformer_dim: int, transformer: nn.Module, num_multimask_outputs: int = 3,
                 activation: Type[nn.Module] = nn.GELU, iou_head_depth: int = 3, iou_head_hidden_dim: int = 256,
                 quant=False, calibrate=False, cfg: Optional[Config] = None):
        super().__init__()
        cfg = cfg or sam_w8a8_config()
        _refuse_ptf(cfg, "MaskDecoder")
        self.cfg = cfg
        self.transformer_dim = transformer_dim
        self.transformer = transformer
        self.num_multimask_outputs = num_multimask_outputs
        self.iou_token = nn.Embedding(1, transformer_dim)
        self.num_mask_tokens = num_multimask_outputs + 1
        self.mask_tokens = nn.Embedding(self.num_mask_tokens, transformer_dim)
        self.qact_embed1 = _qact(cfg, quant, calibrate)
        self.qact_embed2 = _qact(cfg, quant, calibrate)
        self.pos_src_qact = _qact(cfg, quant, calibrate)
        self.pos_src_qact = _qact(cfg, quant, calibrate)
        c4, c8 = transformer_dim // 4, transformer_dim // 8
        self.output_upscaling = nn.ModuleList([
            _qconvT(cfg, transformer_dim, c4, quant, calibrate), QIntLayerNorm2D(c4), activation(),
            _qconvT(cfg, c4, c8, quant, calibrate), activation()])
        self.qacts = nn.ModuleList([_qact(cfg, quant, calibrate, ln=i == 0) for i in range(5)])
        self.output_hypernetworks_mlps = nn.ModuleList([
            MLP(transformer_dim, transformer_dim, c8, 3, quant=quant, calibrate=calibrate, cfg=cfg)
            for _ in range(self.num_mask_tokens)])
        self.qact1 = _qact(cfg, quant, calibrate)
        self.iou_prediction_head = MLP(transformer_dim, iou_head_hidden_dim, self.num_mask_tokens, iou_head_depth,
                                       quant=quant, calibrate=calibrate, cfg=cfg)
        self.use_engine = True   # False: the module graph on the GPU too (tools/bench_decoder.py)
        self.use_fused_tail = True   # False: the engine's transformer, then heads_forward (the module-graph tail)
        self._engine = None

    def _qmods(self):
        return [m for m in self.modules() if type(m) in (QConv2d, QLinear, QAct, QIntSoftmax)]

    def is_quant(self) -> bool:
        """All quantisers on, none calibrating.  The walk over the ~300 modules is done once and kept
        until ``refresh()`` -- which the five ``Sam`` switches and a state-dict load call; call it after
        setting ``quant`` / ``calibrate`` flags on the modules by hand."""
        state = self.__dict__.get("_quant_state")
        if state is None:
            mods = self._qmods()
            state = (all(m.quant for m in mods if not isinstance(m, QIntSoftmax))
                     and not any(m.calibrate for m in mods))
            self.__dict__["_quant_state"] = state
        return state

    def refresh(self) -> None:
        """Forget the engine (its weight codes and scales are a snapshot) and the cached mode."""
        self._engine = None
        self.__dict__["_quant_state"] = None

    def _load_from_state_dict(self, *args, **kwargs):
        self.refresh()   # a loaded checkpoint brings new weights / scales: the next quant forward rebuilds the engine
        super()._load_from_state_dict(*args, **kwargs)

    def engine(self) -> "W8A8DecoderEngine":
        if self._engine is None:
            self._engine = W8A8DecoderEngine(self)
        return self._engine

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings,
                multimask_output: bool, taps: Optional[dict] = None):
        masks, iou_pred = self.predict_masks(image_embeddings, image_pe, sparse_prompt_embeddings,
                                             dense_prompt_embeddings, taps=taps)
        sl = slice(1, None) if multimask_output else slice(0, 1)
        return masks[:, sl, :, :], iou_pred[:, sl]

    def predict_masks(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings,
                      taps: Optional[dict] = None):
        """``taps`` (tests): the fake-quant f32 values of ``qact_embed1`` / ``qact_embed2`` /
        ``pos_src_qact``, every block's ``layers.<i>.queries`` / ``.keys``, the transformer's
        ``queries`` / ``keys`` and the low-res masks ``qact1``; through the engine's fused tail also
        ``upscaling.qacts.0`` .. ``.4`` and ``hyper_in``.

        Through the fused tail, once ``engine().capture(n_tokens)`` has recorded a graph for this token
        count, ``masks`` / ``iou_pred`` (and the slices ``forward`` returns) are the graph's own output
        buffers: the next click of that token count overwrites them -- clone what must outlive it (a
        low-res mask fed back as the next click's mask input).  Without a captured graph they are fresh."""
        output_tokens = torch.cat([self.iou_token.weight, self.mask_tokens.weight], dim=0)
        output_tokens = output_tokens.unsqueeze(0).expand(sparse_prompt_embeddings.size(0), -1, -1)
        raw_tokens = torch.cat((output_tokens, sparse_prompt_embeddings), dim=1)
        if self.use_engine and raw_tokens.is_cuda and self.is_quant():
            if self.use_fused_tail:
                return self.engine().forward_masks(image_embeddings, dense_prompt_embeddings, image_pe, raw_tokens,
                                                   taps=taps)
            hs, src = self.engine().forward(image_embeddings, dense_prompt_embeddings, image_pe, raw_tokens, taps=taps)
            b, c, h, w = src.shape[0], image_embeddings.shape[1], image_embeddings.shape[2], image_embeddings.shape[3]
        else:
            tokens = self.qact_embed1(raw_tokens)
            src = self.qact_embed2(image_embeddings + dense_prompt_embeddings)
            pos_src = self.pos_src_qact(image_pe)
            b, c, h, w = src.shape
            if taps is not None:
                taps["qact_embed1"], taps["qact_embed2"], taps["pos_src_qact"] = tokens, src, pos_src
            hs, src = self.transformer(src, pos_src, tokens, taps=taps)
            if taps is not None:
                taps["queries"], taps["keys"] = hs, src
        return self.heads_forward(hs, src, (b, c, h, w), taps=taps)

    def heads_forward(self, hs, src, shape, taps: Optional[dict] = None):
        """``mask_decoder.py:251-279``: output upscaling, hypernetwork MLPs, low-res masks (``qact1``)
        and the IoU head from the transformer's ``queries`` (B, Nt, C) / ``keys`` (B, hw, C)."""
        b, c, h, w = shape
        iou_token_out = hs[:, 0, :]
        mask_tokens_out = hs[:, 1:(1 + self.num_mask_tokens), :]
        x = src.transpose(1, 2).view(b, c, h, w)
        for i, mod in enumerate(self.output_upscaling):
            x = self.qacts[i](mod(x))
        hyper_in: List[torch.Tensor] = [self.output_hypernetworks_mlps[i](mask_tokens_out[:, i, :])
                                        for i in range(self.num_mask_tokens)]
        hyper_in = torch.stack(hyper_in, dim=1)
        b, c, h, w = x.shape
        masks = self.qact1((hyper_in @ x.reshape(b, c, h * w)).view(b, -1, h, w))
        if taps is not None:
            taps["qact1"] = masks
        return masks, self.iou_prediction_head(iou_token_out)


# ----------------------------------------------------------------------------- the model
class Sam(_FloatSam):
    """``fq_vit/models/sam/sam.py:20-235``: the container with the five calibration switches over
    every ``QConv2d`` / ``QLinear`` / ``QAct`` / ``QIntSoftmax`` of encoder, prompt encoder and
    mask decoder (exact type match, as the reference)."""

    def __init__(self, image_encoder, prompt_encoder, mask_decoder, pixel_mean=(123.675, 116.28, 103.53),
                 pixel_std=(58.395, 57.12, 57.375), quant=False, calibrate=False, cfg: Optional[Config] = None):
        super().__init__(image_encoder, prompt_encoder, mask_decoder, pixel_mean, pixel_std)
        self.cfg = cfg or sam_w8a8_config()

    def _qmods(self):
        return [m for m in self.modules() if type(m) in (QConv2d, QLinear, QAct, QIntSoftmax)]

    def _drop_engines(self):
        self.image_encoder._engine = None
        self.image_encoder._engine_zp = None
        self.image_encoder._pick_zp = None
        if hasattr(self.mask_decoder, "refresh"):
            self.mask_decoder.refresh()

    def model_quant(self):
        for m in self._qmods():
            m.quant = True
        self._drop_engines()

    def model_dequant(self):
        for m in self._qmods():
            m.quant = False
        self._drop_engines()

    def model_open_calibrate(self):
        for m in self._qmods():
            m.calibrate = True
        self._drop_engines()

    def model_open_last_calibrate(self):
        for m in self._qmods():
            m.last_calibrate = True
        self._drop_engines()

    def model_close_calibrate(self):
        for m in self._qmods():
            m.calibrate = False
        self._drop_engines()


def build_fq_prompt_decoder(cfg: Optional[Config] = None, prompt_embed_dim: int = 256, image_size: int = 1024,
                            patch: int = 16, quant=False, calibrate=False,
                            image_embedding_size: Optional[Tuple[int, int]] = None):
    """The reference's prompt encoder / mask decoder hyper-parameters (``build_sam.py``, fq_vit)."""
    cfg = cfg or sam_w8a8_config()
    emb = image_embedding_size or (image_size // patch, image_size // patch)
    pe = PromptEncoder(embed_dim=prompt_embed_dim, image_embedding_size=tuple(emb),
                       input_image_size=(image_size, image_size), mask_in_chans=16, quant=quant, calibrate=calibrate,
                       cfg=cfg)
    md = MaskDecoder(num_multimask_outputs=3, transformer_dim=prompt_embed_dim, iou_head_depth=3,
                     iou_head_hidden_dim=256, quant=quant, calibrate=calibrate, cfg=cfg,
                     transformer=TwoWayTransformer(depth=2, embedding_dim=prompt_embed_dim, mlp_dim=2048, num_heads=8,
                                                   quant=quant, calibrate=calibrate, cfg=cfg))
    return pe, md


def build_fq_sam(name: str = "vit_b", cfg: Optional[Config] = None, img_size: int = 1024,
                 depth: Optional[int] = None, quant=False, calibrate=False) -> Sam:
    """fq_vit ``build_sam_vit_*`` (``fq_vit/models/sam/build_sam.py``): the W8A8 encoder of
    ``build_fq_image_encoder`` with the quantised prompt encoder and mask decoder."""
    cfg = cfg or sam_w8a8_config()
    enc = build_fq_image_encoder(name, img_size=img_size, cfg=cfg, depth=depth, quant=quant, calibrate=calibrate)
    pe, md = build_fq_prompt_decoder(cfg, 256, img_size, 16, quant=quant, calibrate=calibrate)
    sam = Sam(enc, pe, md, quant=quant, calibrate=calibrate, cfg=cfg)
    sam.eval()
    return sam


# ----------------------------------------------------------------------------- fused W8A8 decoder engine
def _tensor_version(t: torch.Tensor):
    """``t._version``, or None for an inference-mode tensor (which tracks none and raises)."""
    try:
        return t._version
    except RuntimeError:
        return None


class W8A8DecoderEngine:
    """Fused HIP forward of a calibrated ``TwoWayTransformer`` (quant mode): int8 codes between the
    kernels, every QAct folded into the kernel that produces its input.

    Per block: [add (qact_pos / qact1)] -> q / k / v GEMMs (qact1_1..3) -> attention (qact_attn1,
    softmax, attn.qact2) -> out_proj GEMM + attn.qact3 + residual + qact2 -> LayerNorm + qact3 |
    adds (qact4, qact5) -> 3 GEMMs -> attention -> out_proj + residual + qact6 -> LN + qact7 |
    lin1 GEMM + mlp.qact1, ReLU -> lin2 GEMM + mlp.qact2 (= qact8) + residual + qact9 -> LN + qact10 |
    adds (qact11, qact12) -> 3 GEMMs -> attention (image queries) -> out_proj + residual + qact13 ->
    LN + qact14.  Then the final token-to-image attention the same way and LN + qact4 -> f32
    (``forward``) or int8 codes (``forward_masks``).

    ``forward_masks`` goes on to the masks in three more kernels (``csrc/decoder_tail.hip``):
    ``upscale0_q8`` (convT 256 -> 64, qacts[0], LayerNorm2D, qacts[1], GELU, qacts[2]) on the key codes,
    ``decoder_mlps_q8`` (the four hypernetwork MLPs and the IoU head) on the query codes and
    ``upscale1_masks_q8`` (convT 64 -> 32, qacts[3], GELU, qacts[4], hyper_in @ x, qact1).  The tail's
    weights are a snapshot too: the float transposed-convolution weights split into two fp16 planes,
    the MLP weight codes quantised once.

    The image side (``qact_embed2(image_embeddings + dense)`` and ``pos_src_qact(image_pe)`` as token
    rows of codes) is quantised once per image and cached; a forward quantises the prompt tokens
    and runs the kernels.  No host synchronisation in ``forward``; ``capture(n_tokens)`` records it
    into HIP graphs, two per token count: one that ends in the f32 ``queries`` / ``keys`` (``forward``) and
    one that ends in ``masks`` / ``iou_pred`` (``forward_masks``) -- a click replays the second only and
    does not pay for the f32 outputs it does not read.
    """

    def __init__(self, dec: MaskDecoder):
        from . import ops
        cfg = dec.cfg
        if not (cfg.BIT_TYPE_A.signed and cfg.BIT_TYPE_A.bits == 8) or cfg.INT_NORM or cfg.INT_SOFTMAX:
            raise NotImplementedError("W8A8 decoder engine supports Config(ptf=False, lis=False) with BIT_TYPE_A=int8")
        tr = dec.transformer
        dev = dec.iou_token.weight.device
        if dev.type != "cuda":
            raise RuntimeError("W8A8 decoder engine: move the decoder to the GPU first")
        self.dec, self.dev, self.ops = dec, dev, ops
        self.c = tr.embedding_dim
        self.heads = tr.num_heads
        self.s_tok, self.s_src, self.s_pos = _s(dec.qact_embed1), _s(dec.qact_embed2), _s(dec.pos_src_qact)
        self.layers = []
        for blk in tr.layers:
            d = dict(skip_pe=blk.skip_first_layer_pe, self_attn=self._attn(blk.self_attn),
                     t2i=self._attn(blk.cross_attn_token_to_image), i2t=self._attn(blk.cross_attn_image_to_token),
                     lin1=self._weight(blk.mlp.lin1), lin2=self._weight(blk.mlp.lin2),
                     s_h=_s(blk.mlp.qact1), s_l2=_s(blk.mlp.qact2),
                     norms=[self._norm(n) for n in (blk.norm1, blk.norm2, blk.norm3, blk.norm4)])
            for i in range(2, 15):
                d[f"s{i}"] = _s(getattr(blk, f"qact{i}"))
            if not blk.skip_first_layer_pe:
                d["s_qpos"], d["s1"] = _s(blk.qact_pos), _s(blk.qact1)
            self.layers.append(d)
        self.final = self._attn(tr.final_attn_token_to_image)
        self.norm_final = self._norm(tr.norm_final_attn)
        self.sf = [None] + [_s(getattr(tr, f"qact{i}")) for i in range(1, 5)]
        # the tail's snapshot: now when the decoder uses it -- an unsupported tail (sigmoid_output, a
        # per-channel tail QAct) is refused here, also for callers of forward() alone: set
        # use_fused_tail = False before engine() to run such a decoder -- else on the first forward_masks
        self._tail = self._snapshot_tail() if dec.use_fused_tail else None
        self._image = None      # (image_embeddings, dense, image_pe, their versions) -> cached codes
        self._graphs = {}       # (n_tokens, batch, hw) -> (graph, static tokens, outputs)
        self.forwards = 0       # engine forwards (eager or replayed); the tests' "the engine ran" counter
        self.image_quantisations = 0

    # -- construction helpers
    def _weight(self, mod):
        """``W8A8Engine._weight`` for a QLinear (per-output-channel codes of ``quantizer(weight)``)."""
        w = mod.weight.detach().float()
        s = mod.quantizer.scale
        if s is None:
            raise RuntimeError("fq_vit: weight quantizer is not calibrated")
        s = s.detach().float().reshape(-1).to(w.device)
        if s.numel() == 1:
            s = s.expand(w.shape[0])
        codes = torch.clamp(torch.round((w.double() / s.double()[:, None]).float()), -128, 127).to(torch.int8)
        bias = None if mod.bias is None else mod.bias.detach().float().contiguous()
        return dict(packed=self.ops.w8_repack(codes), scale=s.contiguous(), bias=bias, n=w.shape[0], k=w.shape[1])

    def _attn(self, a: Attention):
        return dict(q=self._weight(a.q_proj), k=self._weight(a.k_proj), v=self._weight(a.v_proj),
                    o=self._weight(a.out_proj), s_q=_s(a.qact1_1), s_k=_s(a.qact1_2), s_v=_s(a.qact1_3),
                    s_a1=_s(a.qact_attn1), s_ao=_s(a.qact2), s_o=_s(a.qact3), heads=a.num_heads)

    @staticmethod
    def _norm(n):
        return n.weight.detach().float().contiguous(), n.bias.detach().float().contiguous(), n.eps

    def _snapshot_tail(self):
        """Output upscaling, hypernetwork MLPs and IoU head for the three tail kernels."""
        ops, dec, dev = self.ops, self.dec, self.dev
        up = dec.output_upscaling
        if not (len(up) == 5 and isinstance(up[0], QConvTranspose2d) and isinstance(up[1], QIntLayerNorm2D)
                and isinstance(up[3], QConvTranspose2d) and all(isinstance(up[i], nn.GELU) for i in (2, 4))
                and all(getattr(up[i], "approximate", "none") == "none" for i in (2, 4))):
            raise NotImplementedError("W8A8 decoder tail: output_upscaling must be convT, LayerNorm2D, GELU, convT, GELU")

        def convt(m):
            if (tuple(m.kernel_size), tuple(m.stride), tuple(m.padding), tuple(m.output_padding), tuple(m.dilation),
                    m.groups) != ((2, 2), (2, 2), (0, 0), (0, 0), (1, 1), 1):
                raise NotImplementedError("W8A8 decoder tail: transposed convolutions must be kernel 2, stride 2")
            w = (m.quantizer(m.weight) if m.quant else m.weight).detach().float()   # float unless set by hand
            hi, lo = ops.convt_split_weight(w)
            bias = torch.zeros(w.shape[1], device=dev) if m.bias is None else m.bias.detach().float().contiguous()
            return dict(hi=hi, lo=lo, bias=bias, cin=w.shape[0], cout=w.shape[1])
        mlps = list(dec.output_hypernetworks_mlps) + [dec.iou_prediction_head]
        if any(m.num_layers != 3 for m in mlps):
            raise NotImplementedError("W8A8 decoder tail: 3-layer MLPs (iou_head_depth = 3)")
        hid, cin = mlps[0].layers[1].in_features, mlps[0].layers[0].in_features
        no_h, no_i = mlps[0].layers[2].out_features, mlps[-1].layers[2].out_features
        no = max(no_h, no_i)
        w1, w2, w3, b1, b2, b3, sc = [], [], [], [], [], [], []
        for i, m in enumerate(mlps):
            if m.sigmoid_output:
                raise NotImplementedError("W8A8 decoder tail: MLP(sigmoid_output=True) is not supported")
            want = [(cin, hid), (hid, hid), (hid, no_i if i == len(mlps) - 1 else no_h)]
            if [(l.in_features, l.out_features) for l in m.layers] != want:
                raise NotImplementedError("W8A8 decoder tail: MLPs of one input / hidden width")
            ws = []
            for lay, dst, bdst, pad in zip(m.layers, (w1, w2, w3), (b1, b2, b3), (0, 0, no)):
                s = lay.quantizer.scale
                if s is None:
                    raise RuntimeError("fq_vit: weight quantizer is not calibrated")
                if s.numel() != 1:
                    raise NotImplementedError("W8A8 decoder tail: the MLPs' QLinears have one weight scale each")
                w = lay.weight.detach().float()
                s = s.detach().float().reshape(-1).to(w.device)   # the rounding of _weight
                codes = torch.clamp(torch.round((w.double() / s.double()[:, None]).float()), -128, 127).to(torch.int8)
                dst.append(ops.mlp_pack_weight(codes, pad))
                bias = torch.zeros(w.shape[0], device=dev) if lay.bias is None else lay.bias.detach().float()
                bdst.append(F.pad(bias, (0, max(pad, w.shape[0]) - w.shape[0])))
                ws.append(float(s[0]))
            sc.append(ws + [_s(m.qacts1[0]), _s(m.qacts2[0]), _s(m.qacts1[1]), _s(m.qacts2[1]), _s(m.qact3)])
        ln = up[1]
        return dict(up0=convt(up[0]), up1=convt(up[3]), gamma=ln.weight.detach().float().contiguous(),
                    beta=ln.bias.detach().float().contiguous(), eps=ln.eps, su=[_s(q) for q in dec.qacts],
                    s_q1=_s(dec.qact1), w1=torch.stack(w1), w2=torch.stack(w2), w3=torch.stack(w3),
                    b1=torch.stack(b1).contiguous(), b2=torch.stack(b2).contiguous(), b3=torch.stack(b3).contiguous(),
                    scales=torch.tensor(sc, dtype=torch.float32, device=dev),
                    s_hyper=torch.tensor([r[7] for r in sc[:-1]], dtype=torch.float32, device=dev),
                    s_hyper_host=[r[7] for r in sc[:-1]], n_hyper=len(mlps) - 1, no_h=no_h, no_i=no_i)

    def _gemm(self, a, lw, epi, a_scale, out_scale, mid=0.0, res=None, res_scale=0.0, out=None):
        return self.ops.w8a8_gemm(a, lw["packed"], lw["scale"], lw["n"], lw["bias"], epi, a_scale, out_scale, mid,
                                  res_scale, res, out)

    # -- the image side, once per image
    def set_image(self, image_embeddings, dense, image_pe):
        """Token rows of codes of ``qact_embed2(image_embeddings + dense)`` (B * hw, C) and of
        ``pos_src_qact(image_pe)`` (hw, C), cached while the three tensors stay the same storage and
        version (the predictor's features, the expanded ``no_mask_embed``, the dense PE).  The cache
        holds those three tensors until the next image replaces them.  Tensors without a version
        counter (made under ``torch.inference_mode``) are not recognised: every call requantises."""
        key = tuple((t.data_ptr(), _tensor_version(t), tuple(t.shape), t.stride())
                    for t in (image_embeddings, dense, image_pe))
        if self._image is not None and self._image["key"] == key and None not in (k[1] for k in key):
            return self._image
        ops = self.ops
        src = (image_embeddings + dense).float().flatten(2).permute(0, 2, 1).contiguous()
        pos = image_pe.float().flatten(2).permute(0, 2, 1).contiguous()
        if pos.shape[0] != 1:
            raise NotImplementedError("W8A8 decoder engine: one positional encoding for the batch")
        b, hw, c = src.shape
        old = self._image
        if old is not None and (old["b"], old["hw"]) == (b, hw):
            # same geometry: the codes go into the same buffers, so the captured graphs stay valid
            src_q, pos_q = old["src"], old["pos"]
            ops.quantize(src, self.s_src, out=src_q.view(b, hw, c))
            ops.quantize(pos, self.s_pos, out=pos_q.view(1, hw, c))
        else:
            src_q = ops.quantize(src, self.s_src).view(b * hw, c)
            pos_q = ops.quantize(pos, self.s_pos).view(hw, c)
            self._graphs.clear()
        # the cache keeps the tensors alive, so an equal data pointer is the same storage
        self._image = dict(key=key, hold=(image_embeddings, dense, image_pe), b=b, hw=hw, src=src_q, pos=pos_q,
                           grid=tuple(image_embeddings.shape[-2:]))
        self.image_quantisations += 1
        return self._image

    # -- forward
    @torch.no_grad()
    def forward(self, image_embeddings, dense, image_pe, raw_tokens, taps: Optional[dict] = None):
        """``raw_tokens`` f32 (B, Nt, C): the concatenated output / prompt tokens BEFORE ``qact_embed1``.
        Returns the fake-quant f32 ``queries`` (B, Nt, C), ``keys`` (B, hw, C).  Replays the captured
        graph of this token count if there is one (and no ``taps``); the two tensors are then the
        graph's own output buffers, which the next replay for that token count overwrites -- clone
        them to keep them across clicks (``predict_masks`` consumes them at once)."""
        img = self.set_image(image_embeddings, dense, image_pe)
        b, nt, c = raw_tokens.shape
        if b != img["b"]:
            raise ValueError(f"W8A8 decoder engine: {b} prompt sets for {img['b']} image-side batches")
        self.forwards += 1
        g = self._graphs.get((nt, b, img["hw"])) if taps is None else None
        if g is not None and g["src"] is img["src"]:
            g["tokens"].copy_(raw_tokens)
            g["graph"].replay()
            return g["out"]
        return self._run(raw_tokens.float().contiguous(), img, taps)

    __call__ = forward

    @torch.no_grad()
    def forward_masks(self, image_embeddings, dense, image_pe, raw_tokens, taps: Optional[dict] = None):
        """The whole decoder behind the prompt encoder: ``(masks, iou_pred)`` -- the fake-quant f32 low-res
        masks (B, 4, 4h, 4w) of ``qact1`` and the IoU head's (B, 4) -- from the same inputs as ``forward``.
        The transformer's ``qact4`` and the keys stay int8 codes; three tail kernels follow on the same
        stream.  Replays the captured graph of this token count if there is one (and no ``taps``): the
        two tensors are then the graph's own buffers, overwritten by the next replay.  ``taps`` also
        receives ``upscaling.qacts.0`` .. ``.4`` (NCHW), ``hyper_in`` and ``qact1``."""
        img = self.set_image(image_embeddings, dense, image_pe)
        b, nt, c = raw_tokens.shape
        if b != img["b"]:
            raise ValueError(f"W8A8 decoder engine: {b} prompt sets for {img['b']} image-side batches")
        self.forwards += 1
        g = self._graphs.get((nt, b, img["hw"])) if taps is None else None
        if g is not None and g["src"] is img["src"] and g.get("graph_masks") is not None:
            g["tokens"].copy_(raw_tokens)
            g["graph_masks"].replay()
            return g["masks"], g["iou_pred"]
        return self._run(raw_tokens.float().contiguous(), img, taps, tail=True)

    def _attention(self, a, q_in, s_qin, k_in, s_kin, v_in, s_vin, b):
        """q / k / v projections + attention: codes of attn.qact2 (rows of q_in, internal dim)."""
        ops = self.ops
        q = self._gemm(q_in, a["q"], ops.EPI_Q8, s_qin, a["s_q"])
        k = self._gemm(k_in, a["k"], ops.EPI_Q8, s_kin, a["s_k"])
        v = self._gemm(v_in, a["v"], ops.EPI_Q8, s_vin, a["s_v"])
        d = q.shape[-1]
        return ops.attention_q8_plain(q.view(b, -1, d), k.view(b, -1, d), v.view(b, -1, d), a["heads"], a["s_q"],
                                      a["s_k"], a["s_v"], a["s_a1"], a["s_ao"]).view(-1, d)

    def _tail_run(self, qc, K, s_K, s_q, img, taps):
        """The three tail kernels: query codes (B, Nt, C) of qact4, key codes (B * hw, C) -> masks, iou_pred."""
        ops = self.ops
        if self._tail is None:
            self._tail = self._snapshot_tail()
        t = self._tail
        b = qc.shape[0]
        h, w = img["grid"]
        u0, u1, su = t["up0"], t["up1"], t["su"]
        dbg = None
        if taps is not None:
            i8 = lambda ch, k: torch.empty((b, k * h, k * w, ch), dtype=torch.int8, device=self.dev)
            dbg = [i8(u0["cout"], 2), i8(u0["cout"], 2), None, i8(u1["cout"], 4), i8(u1["cout"], 4)]
        x2 = ops.upscale0_q8(K, u0["hi"], u0["lo"], u0["bias"], t["gamma"], t["beta"], t["eps"], b, h, w, s_K,
                             su[0], su[1], su[2], dbg_q0=dbg and dbg[0], dbg_q1=dbg and dbg[1])
        hyper, iou = ops.decoder_mlps_q8(qc, t["w1"], t["w2"], t["w3"], t["b1"], t["b2"], t["b3"], t["scales"],
                                         t["n_hyper"], t["no_h"], t["no_i"], s_q)
        masks = ops.upscale1_masks_q8(x2, u1["hi"], u1["lo"], u1["bias"], hyper, t["s_hyper"], su[2], su[3], su[4],
                                      t["s_q1"], dbg_q3=dbg and dbg[3], x4=dbg and dbg[4])
        if taps is not None:
            dbg[2] = x2
            for i, codes in enumerate(dbg):   # NCHW fake-quant values, as the module graph's
                taps[f"upscaling.qacts.{i}"] = codes.permute(0, 3, 1, 2).float() * su[i]
            taps["hyper_in"] = hyper.float() * t["s_hyper"][None, :, None]
            taps["qact1"] = masks
        return masks, iou

    def _run(self, raw_tokens, img, taps, tail=False):
        ops = self.ops
        b, nt, c = raw_tokens.shape
        hw = img["hw"]

        def tap(name, codes, s, rows):
            if taps is not None:
                taps[name] = codes.view(b, rows, -1).float() * s
        T = ops.quantize(raw_tokens, self.s_tok).view(b * nt, c)     # qact_embed1: point_embedding = query_pe
        K, P = img["src"], img["pos"]
        s_T, s_K, s_P = self.s_tok, self.s_src, self.s_pos
        if taps is not None:
            taps["qact_embed1"] = T.view(b, nt, c).float() * s_T
            # NCHW, as the module graph's taps of the same names
            nchw = lambda t, n: t.permute(0, 2, 1).reshape(n, c, *img["grid"])
            taps["qact_embed2"] = nchw(K.view(b, hw, c).float() * s_K, b)
            taps["pos_src_qact"] = nchw(P.view(1, hw, c).float() * s_P, 1)
        Q, s_Q = T, s_T
        zero = None
        for li, L in enumerate(self.layers):
            pre = f"layers.{li}."
            # ---- self attention of the tokens
            a = L["self_attn"]
            if L["skip_pe"]:
                o = self._attention(a, Q, s_Q, Q, s_Q, Q, s_Q, b)
                if zero is None:
                    zero = torch.zeros_like(Q)
                # qact2(attn_out): the residual epilogue on a zero residual (0 * 1 + x = x)
                Q = self._gemm(o, a["o"], ops.EPI_Q8_RES, a["s_ao"], L["s2"], mid=a["s_o"], res=zero, res_scale=1.0)
            else:
                qp = T if L["s_qpos"] == s_T else ops.add_q8(T, s_T, None, 0.0, L["s_qpos"])   # qact_pos(query_pe)
                qin = ops.add_q8(Q, s_Q, qp, L["s_qpos"], L["s1"])
                tap(pre + "qact1", qin, L["s1"], nt)
                o = self._attention(a, qin, L["s1"], qin, L["s1"], Q, s_Q, b)
                Q = self._gemm(o, a["o"], ops.EPI_Q8_RES, a["s_ao"], L["s2"], mid=a["s_o"], res=Q, res_scale=s_Q)
            tap(pre + "qact2", Q, L["s2"], nt)
            Q = ops.layernorm_q(Q, *L["norms"][0], in_scale=L["s2"], out_scale=L["s3"])
            tap(pre + "qact3", Q, L["s3"], nt)
            # ---- tokens attend to the image
            a = L["t2i"]
            qin = ops.add_q8(Q, L["s3"], T, s_T, L["s4"])
            kin = ops.add_q8(K, s_K, P, s_P, L["s5"])
            tap(pre + "qact4", qin, L["s4"], nt)
            tap(pre + "qact5", kin, L["s5"], hw)
            o = self._attention(a, qin, L["s4"], kin, L["s5"], K, s_K, b)
            tap(pre + "cross_attn_token_to_image.qact2", o, a["s_ao"], nt)
            Q = self._gemm(o, a["o"], ops.EPI_Q8_RES, a["s_ao"], L["s6"], mid=a["s_o"], res=Q, res_scale=L["s3"])
            tap(pre + "qact6", Q, L["s6"], nt)
            Q = ops.layernorm_q(Q, *L["norms"][1], in_scale=L["s6"], out_scale=L["s7"])
            tap(pre + "qact7", Q, L["s7"], nt)
            # ---- MLP: lin1 + mlp.qact1 (ReLU on the codes), lin2 + mlp.qact2 + qact8 + residual + qact9
            hbuf = ops.relu_q8(self._gemm(Q, L["lin1"], ops.EPI_Q8, L["s7"], L["s_h"]))
            tap(pre + "mlp.qact1", hbuf, L["s_h"], nt)
            if L["s8"] == L["s_l2"]:   # qact8 on mlp.qact2's output at the same scale: the identity on its codes
                Q = self._gemm(hbuf, L["lin2"], ops.EPI_Q8_RES, L["s_h"], L["s9"], mid=L["s_l2"], res=Q,
                               res_scale=L["s7"])
            else:                      # both quantisers in order, then the residual add
                y = self._gemm(hbuf, L["lin2"], ops.EPI_Q8, L["s_h"], L["s_l2"])
                y = ops.add_q8(y, L["s_l2"], None, 0.0, L["s8"])
                Q = ops.add_q8(Q, L["s7"], y, L["s8"], L["s9"])
            tap(pre + "qact9", Q, L["s9"], nt)
            Q = ops.layernorm_q(Q, *L["norms"][2], in_scale=L["s9"], out_scale=L["s10"])
            tap(pre + "qact10", Q, L["s10"], nt)
            # ---- the image attends to the tokens
            a = L["i2t"]
            qin = ops.add_q8(Q, L["s10"], T, s_T, L["s11"])
            kin = kin if L["s12"] == L["s5"] else ops.add_q8(K, s_K, P, s_P, L["s12"])   # the same keys + key_pe
            tap(pre + "qact11", qin, L["s11"], nt)
            tap(pre + "qact12", kin, L["s12"], hw)
            o = self._attention(a, kin, L["s12"], qin, L["s11"], Q, L["s10"], b)
            tap(pre + "cross_attn_image_to_token.qact2", o, a["s_ao"], hw)
            K = self._gemm(o, a["o"], ops.EPI_Q8_RES, a["s_ao"], L["s13"], mid=a["s_o"], res=K, res_scale=s_K)
            tap(pre + "qact13", K, L["s13"], hw)
            K = ops.layernorm_q(K, *L["norms"][3], in_scale=L["s13"], out_scale=L["s14"])
            s_Q, s_K = L["s10"], L["s14"]
            tap(pre + "queries", Q, s_Q, nt)
            tap(pre + "keys", K, s_K, hw)
        # ---- final attention of the tokens to the image
        sf, a = self.sf, self.final
        qin = ops.add_q8(Q, s_Q, T, s_T, sf[1])
        kin = ops.add_q8(K, s_K, P, s_P, sf[2])
        tap("transformer.qact1", qin, sf[1], nt)
        tap("transformer.qact2", kin, sf[2], hw)
        o = self._attention(a, qin, sf[1], kin, sf[2], K, s_K, b)
        Q = self._gemm(o, a["o"], ops.EPI_Q8_RES, a["s_ao"], sf[3], mid=a["s_o"], res=Q, res_scale=s_Q)
        tap("transformer.qact3", Q, sf[3], nt)
        if tail:   # qact4 and the keys stay codes; no f32 pass over the keys
            qc = ops.layernorm_q(Q, *self.norm_final, in_scale=sf[3], out_scale=sf[4]).view(b, nt, c)
            if taps is not None:
                taps["queries"], taps["keys"] = qc.float() * sf[4], K.view(b, hw, c).float() * s_K
            return self._tail_run(qc, K, s_K, sf[4], img, taps)
        queries = ops.layernorm_q(Q, *self.norm_final, in_scale=sf[3], out_scale=sf[4],
                                  out_dtype=torch.float32).view(b, nt, c)
        keys = ops.add_q8(K, s_K, None, 0.0, s_K, fake=True).view(b, hw, c)   # codes * scale as f32
        if taps is not None:
            taps["queries"], taps["keys"] = queries, keys
        return queries, keys

    # -- HIP graph
    def capture(self, n_tokens: int, image_embeddings=None, dense=None, image_pe=None):
        """Record the forward for ``n_tokens`` tokens (5 + prompt points) on the current image into HIP
        graphs; ``forward`` / ``forward_masks`` then replay them for that token count while the image stays
        cached.  Two graphs on one static token buffer: the transformer with its f32 ``queries`` / ``keys``
        (returned) and, when the decoder uses the fused tail, the whole click to ``masks`` / ``iou_pred``.
        One graph for both would make every click compute and store the f32 queries / keys (a pass over
        B * hw * C floats) that only ``forward``'s callers read.  ``use_fused_tail`` is read here: captured
        while it is False, the entry has no masks graph and ``forward_masks`` for that token count runs its
        kernels eagerly until ``capture`` is called again.
        Call after a ``forward`` (or with the image tensors) so the image side is quantised."""
        if image_embeddings is not None:
            self.set_image(image_embeddings, dense, image_pe)
        img = self._image
        if img is None:
            raise RuntimeError("W8A8 decoder engine: capture needs an image (run a forward first)")
        b, hw = img["b"], img["hw"]
        tokens = torch.zeros((b, n_tokens, self.c), dtype=torch.float32, device=self.dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._run(tokens, img, None)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._run(tokens, img, None)
        entry = dict(graph=graph, tokens=tokens, out=out, src=img["src"], graph_masks=None)
        if self.dec.use_fused_tail:
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._run(tokens, img, None, tail=True)
            torch.cuda.current_stream().wait_stream(s)
            gm = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gm):
                entry["masks"], entry["iou_pred"] = self._run(tokens, img, None, tail=True)
            entry["graph_masks"] = gm
        self._graphs[(n_tokens, b, hw)] = entry
        return graph

    def drop_graphs(self):
        self._graphs.clear()
