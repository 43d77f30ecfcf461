"""Transformer ASR on gfx950: the plain CTC / attention encoder-decoder of the model zoo (`model: Transformer`;
funasr/models/transformer/model.py, the class the reference's Conformer subclasses with nothing added).

  * `TransformerEncoder` (encoder_classes; funasr/models/transformer/encoder.py): Conv2dSubsampling, x sqrt(D) + the absolute
    sinusoid, pre-LayerNorm blocks of masked self-attention (`MultiHeadedAttention`) and a ReLU feed-forward, `after_norm`. One
    `pf_tfencoder` handle (csrc/engine_conformer.hip): the Conformer's subsampling front, the plain attention kernel of
    csrc/attention_abs.hip, two-mode GEMMs.
  * `Transformer` (model_classes): everything else is `funasr_amd.conformer.AttentionEncoderDecoder` -- the `TransformerDecoder`
    stepper, the CTC head, greedy CTC for `batch_size > 1` and the joint CTC-prefix / attention beam search otherwise.

As for the Conformer the padded-batch result is the contract: the reference runs Conv2dSubsampling over the zero-padded batch
without masking, so a clip's frames and its output length depend on the longest clip it is batched with.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .conformer import (MAX_LEN, _PRECISIONS, AttentionEncoderDecoder, Conv2dSubsampledEncoder, TooShortUttError, _attention, _ffn,  # noqa: F401
                        abs_pos_table, subsampled_length)
from .hip_module import Holder, ParamHolder, _truthy, layer_norm, linear
from .register import tables


@tables.register("encoder_classes", "TransformerEncoder")
class TransformerEncoder(Conv2dSubsampledEncoder):
    _prefix = "pf_tfencoder"

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048, num_blocks: int = 6,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0,
                 input_layer: str = "conv2d", pos_enc_class=None, normalize_before: bool = True, concat_after: bool = False,
                 positionwise_layer_type: str = "linear", positionwise_conv_kernel_size: int = 1, padding_idx: int = -1,
                 interctc_layer_idx=(), interctc_use_conditioning: bool = False, precision: str = None, **kwargs):
        super().__init__()
        D, H = int(output_size), int(attention_heads)
        refusals = [
            (input_layer != "conv2d", f"input_layer: {input_layer} (only conv2d, the 1/4 subsampling)"),
            (pos_enc_class is not None, "pos_enc_class (only the default PositionalEncoding)"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (positionwise_layer_type != "linear", f"positionwise_layer_type: {positionwise_layer_type} (only linear)"),
            (len(list(interctc_layer_idx or ())) > 0, "interctc_layer_idx"),
            (_truthy(interctc_use_conditioning), "interctc_use_conditioning: true"),
            (H < 1 or D != 64 * H, f"attention_heads: {attention_heads} with output_size {output_size} (only a head dim of 64 is built)"),
            (int(linear_units) % 32 != 0, f"linear_units: {linear_units} (a multiple of 32)"),
            (not 7 <= int(input_size) <= 256, f"input_size: {input_size} (7 .. 256 features)"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"TransformerEncoder(HIP): {why} is not built")
        mode = precision or "f16x2"
        if mode not in _PRECISIONS:
            raise NotImplementedError(f"TransformerEncoder(HIP): precision {mode!r}: built are {sorted(_PRECISIONS)}")
        self.precision = mode
        self.input_size, self._output_size, self.attention_heads, self.linear_units = int(input_size), D, H, int(linear_units)
        self.num_blocks = int(num_blocks)
        self.interctc_use_conditioning = False
        f2 = ((self.input_size - 1) // 2 - 1) // 2
        embed = Holder()
        conv = nn.Module()
        conv.add_module("0", ParamHolder((D, 1, 3, 3), (D,)))
        conv.add_module("2", ParamHolder((D, D, 3, 3), (D,)))
        embed.conv = conv
        out = nn.Module()
        out.add_module("0", linear(D, D * f2))
        embed.out = out
        self.embed = embed
        blocks = nn.ModuleList()
        for _ in range(self.num_blocks):
            b = Holder()
            b.self_attn = _attention(D, rel=False)
            b.feed_forward = _ffn(D, self.linear_units)
            b.norm1, b.norm2 = layer_norm(D), layer_norm(D)
            blocks.append(b)
        self.encoders = blocks
        self.after_norm = layer_norm(D)
        for p in self.parameters():
            p.requires_grad_(False)
        # the reference's `pe`, built as it builds it (float32 torch ops on the host); a plain attribute there and here, so not in the
        # state dict. The last bit of div_term depends on the host's float32 exp(), exactly as the reference's own table does.
        self.pos_table = abs_pos_table(D)

    def pos_rows(self, T: int):
        """the rows of the table a forward over T encoder frames reads (a view)"""
        return self.pos_table[:T]

    def _make_config(self):
        c = _lib.pf_tfencoder_config()
        c.input_dim, c.d_model, c.n_heads, c.ffn_dim, c.n_blocks = (self.input_size, self._output_size, self.attention_heads, self.linear_units,
                                                                    self.num_blocks)
        c.precision, c.ln_eps = _PRECISIONS[self.precision], 1e-12
        return c


@tables.register("model_classes", "Transformer")
class Transformer(AttentionEncoderDecoder):
    """funasr/models/transformer/model.py Transformer"""
    _encoder = "TransformerEncoder"
    _other_encoders = "ConformerEncoder belongs to model: Conformer, the Branchformer family is another model"
