"""E-Branchformer ASR on gfx950: the third encoder of the CTC / attention encoder-decoder family (`model: EBranchformer` and
`model: Branchformer` with `encoder: EBranchformerEncoder`, the layout of funasr/models/e_branchformer/template.yaml;
funasr/models/e_branchformer/model.py and funasr/models/branchformer/model.py are empty subclasses of the Transformer model).

  * `EBranchformerEncoder` (encoder_classes; funasr/models/e_branchformer/encoder.py): Conv2dSubsampling, then blocks of two
    parallel branches -- the Conformer's relative-position self-attention and the convolutional gating MLP of
    funasr/models/branchformer/cgmlp.py -- merged by a depthwise conv over their concatenation and a Linear, between optional
    (macaron) Swish feed-forwards. One `pf_ebranchformer` handle (csrc/engine_conformer.hip): the Conformer's subsampling front and
    attention kernel, the GELU / gating-unit / merge kernels of csrc/ebranchformer.hip, two-mode GEMMs (`precision: f16x2` runs the
    block GEMMs from two-plane fp16 operands except `merge_proj`, which stays exact fp32: DESIGN 3.16).
  * `EBranchformer` (model_classes, under both names): everything else is `funasr_amd.conformer.AttentionEncoderDecoder` -- the
    `TransformerDecoder` stepper, the CTC head, greedy CTC for `batch_size > 1`, the joint CTC-prefix / attention beam search otherwise.

The padded-batch result is the contract, more so than for the Conformer: besides Conv2dSubsampling, the reference runs BOTH
depthwise convs of every block (the gating unit's and the merge's) over the zero-padded batch without masking, so the frames near a
shorter clip's end read the rows behind it, which are not zero after the first bias. A clip batched with a longer one does not get
the frames it gets alone; this package reproduces the reference's batched frames. A batch of equal-length clips has no padding and
there a clip's result is bitwise what it is alone.

The plain `BranchformerEncoder` (other merge methods, FastSelfAttention, branch dropout) is not built.
"""
from __future__ import annotations

import torch.nn as nn

from . import _lib
from .conformer import (MAX_LEN, _PRECISIONS, AttentionEncoderDecoder, Conv2dSubsampledEncoder, TooShortUttError, _attention, _ffn,  # noqa: F401
                        latest_rel_pos_table, legacy_rel_pos_table, subsampled_length)
from .hip_module import Holder, ParamHolder, _truthy, layer_norm, linear
from .register import tables


def _odd_kernel(k) -> bool:
    return int(k) % 2 == 1 and 1 <= int(k) <= 31


@tables.register("encoder_classes", "EBranchformerEncoder")
class EBranchformerEncoder(Conv2dSubsampledEncoder):
    _prefix = "pf_ebranchformer"

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, attention_layer_type: str = "rel_selfattn",
                 pos_enc_layer_type: str = "rel_pos", rel_pos_type: str = "latest", cgmlp_linear_units: int = 2048,
                 cgmlp_conv_kernel: int = 31, use_linear_after_conv: bool = False, gate_activation: str = "identity", num_blocks: int = 12,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0,
                 input_layer: str = "conv2d", zero_triu: bool = False, padding_idx: int = -1, layer_drop_rate: float = 0.0,
                 max_pos_emb_len: int = 5000, use_ffn: bool = False, macaron_ffn: bool = False, ffn_activation_type: str = "swish",
                 linear_units: int = 2048, positionwise_layer_type: str = "linear", merge_conv_kernel: int = 3, interctc_layer_idx=None,
                 interctc_use_conditioning: bool = False, precision: str = None, **kwargs):
        super().__init__()
        if rel_pos_type not in ("legacy", "latest"):
            raise ValueError("unknown rel_pos_type: " + str(rel_pos_type))
        D, H = int(output_size), int(attention_heads)
        refusals = [
            (input_layer != "conv2d", f"input_layer: {input_layer} (only conv2d, the 1/4 subsampling)"),
            (pos_enc_layer_type != "rel_pos", f"pos_enc_layer_type: {pos_enc_layer_type} (only rel_pos)"),
            (attention_layer_type != "rel_selfattn", f"attention_layer_type: {attention_layer_type} (only rel_selfattn)"),
            (_truthy(use_linear_after_conv), "use_linear_after_conv: true"),
            (gate_activation != "identity", f"gate_activation: {gate_activation} (only identity)"),
            (_truthy(zero_triu), "zero_triu: true"),
            (ffn_activation_type != "swish", f"ffn_activation_type: {ffn_activation_type} (only swish)"),
            (positionwise_layer_type != "linear", f"positionwise_layer_type: {positionwise_layer_type} (only linear)"),
            (int(max_pos_emb_len) != MAX_LEN, f"max_pos_emb_len: {max_pos_emb_len} (only {MAX_LEN})"),
            (len(list(interctc_layer_idx or ())) > 0, "interctc_layer_idx"),
            (_truthy(interctc_use_conditioning), "interctc_use_conditioning: true"),
            (not _odd_kernel(cgmlp_conv_kernel), f"cgmlp_conv_kernel: {cgmlp_conv_kernel} (odd, at most 31)"),
            (not _odd_kernel(merge_conv_kernel), f"merge_conv_kernel: {merge_conv_kernel} (odd, at most 31)"),
            (H < 1 or D != 64 * H, f"attention_heads: {attention_heads} with output_size {output_size} (only a head dim of 64 is built)"),
            (int(linear_units) < 64 or int(linear_units) % 64 != 0, f"linear_units: {linear_units} (a multiple of 64)"),
            (int(cgmlp_linear_units) < 64 or int(cgmlp_linear_units) % 64 != 0, f"cgmlp_linear_units: {cgmlp_linear_units} (a multiple of 64)"),
            (not 7 <= int(input_size) <= 256, f"input_size: {input_size} (7 .. 256 features)"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"EBranchformerEncoder(HIP): {why} is not built")
        mode = precision or "f16x2"
        if mode not in _PRECISIONS:
            raise NotImplementedError(f"EBranchformerEncoder(HIP): precision {mode!r}: built are {sorted(_PRECISIONS)}")
        self.precision = mode
        self.input_size, self._output_size, self.attention_heads, self.linear_units = int(input_size), D, H, int(linear_units)
        self.num_blocks, self.cgmlp_units = int(num_blocks), int(cgmlp_linear_units)
        self.cgmlp_kernel, self.merge_kernel = int(cgmlp_conv_kernel), int(merge_conv_kernel)
        self.use_ffn = _truthy(use_ffn)
        self.macaron = self.use_ffn and _truthy(macaron_ffn)
        self.legacy = rel_pos_type == "legacy"
        self.interctc_use_conditioning = False                       # layer_drop_rate: training only, accepted and ignored
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
        U = self.cgmlp_units
        blocks = nn.ModuleList()
        for _ in range(self.num_blocks):
            b = Holder()
            b.attn = _attention(D, rel=True)
            mlp = Holder()
            proj1 = nn.Module()
            proj1.add_module("0", linear(U, D))                       # Sequential(Linear, GELU)
            mlp.channel_proj1 = proj1
            csgu = Holder()
            csgu.norm = layer_norm(U // 2)
            csgu.conv = ParamHolder((U // 2, 1, self.cgmlp_kernel), (U // 2,))
            mlp.csgu = csgu
            mlp.channel_proj2 = linear(D, U // 2)
            b.cgmlp = mlp
            if self.use_ffn:
                b.feed_forward = _ffn(D, self.linear_units)
            if self.macaron:
                b.feed_forward_macaron = _ffn(D, self.linear_units)
            if self.use_ffn:
                b.norm_ff = layer_norm(D)
            if self.macaron:
                b.norm_ff_macaron = layer_norm(D)
            b.norm_mha, b.norm_mlp, b.norm_final = layer_norm(D), layer_norm(D), layer_norm(D)
            b.depthwise_conv_fusion = ParamHolder((2 * D, 1, self.merge_kernel), (2 * D,))
            b.merge_proj = linear(D, 2 * D)
            blocks.append(b)
        self.encoders = blocks
        self.after_norm = layer_norm(D)
        for p in self.parameters():
            p.requires_grad_(False)
        # the reference's table, built as it builds it (float32 torch ops on the host); a plain attribute there and here, so not in
        # the state dict
        self.pos_table = legacy_rel_pos_table(D) if self.legacy else latest_rel_pos_table(D)

    def pos_rows(self, T: int):
        """the rows of the table a forward over T encoder frames reads (a view)"""
        return self.pos_table[:T] if self.legacy else self.pos_table[MAX_LEN - T: MAX_LEN + T - 1]

    def _make_config(self):
        c = _lib.pf_ebranchformer_config()
        c.input_dim, c.d_model, c.n_heads, c.ffn_dim, c.n_blocks = (self.input_size, self._output_size, self.attention_heads, self.linear_units,
                                                                    self.num_blocks)
        c.cgmlp_units, c.cgmlp_kernel, c.merge_kernel = self.cgmlp_units, self.cgmlp_kernel, self.merge_kernel
        c.use_ffn, c.macaron, c.legacy = int(self.use_ffn), int(self.macaron), int(self.legacy)
        c.precision, c.ln_eps = _PRECISIONS[self.precision], 1e-12
        return c


@tables.register("model_classes", "Branchformer")
@tables.register("model_classes", "EBranchformer")
class EBranchformer(AttentionEncoderDecoder):
    """funasr/models/e_branchformer/model.py EBranchformer(Transformer) and funasr/models/branchformer/model.py
    Branchformer(Transformer): the reference's own template names `model: Branchformer` with `encoder: EBranchformerEncoder`"""
    _encoder = "EBranchformerEncoder"
    _other_encoders = ("the plain BranchformerEncoder is not built; ConformerEncoder / TransformerEncoder belong to model: Conformer / "
                       "Transformer")
