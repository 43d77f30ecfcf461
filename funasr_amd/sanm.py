"""SAN-M ASR on gfx950: the autoregressive SAN-M encoder-decoder of the model zoo (`model: SANM`; funasr/models/sanm/model.py, an
empty subclass of the reference's `Transformer`).

  * `FsmnDecoder` (decoder_classes; funasr/models/sanm/decoder.py): the SAN-M decoder as a device-resident stepper (`begin` /
    `step` / `reorder`, handle `pf_fsmndecoder`): a bare token embedding, per layer the feed-forward FIRST (w_1, ReLU, a LayerNorm over
    the hidden units, w_2 without bias), then the FSMN memory block over a K-column window per hypothesis slot, then cross-attention
    through linear_q / linear_k_v / linear_out; `decoders2` layers without cross-attention, one FFN-only `decoders3` layer without
    residual. Cross-attention K | V once per utterance.
  * `SANM` (model_classes): `SANMEncoder` (funasr_amd/sanm_encoder.py) with the clips' true lengths -- NOT the zero-padded-batch
    contract of the conv2d encoders -- and everything else of `funasr_amd.conformer.AttentionEncoderDecoder`: the CTC head where
    `ctc_weight` > 0, greedy CTC for `batch_size > 1`, the joint CTC-prefix / attention beam search otherwise.

What a step computes is the reference's `forward_one_step`, cache rule included: the FSMN window at step n is the last K columns of
[0] * L + [x_0] + [0] * R + [x_1 .. x_n], L = (K - 1) // 2 (+ sanm_shfit when positive), R = K - 1 - L. That is the causal memory,
and equal to the teacher-forced `forward`, only when R == 0 (the constructor's default sanm_shfit with an odd K); the template's
`sanm_shfit: 0` has R = 5 zeros between the first token and the second. Inference runs the step, so the step is the contract.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from . import sanm_encoder as _sanm_encoder  # noqa: F401  (registers SANMEncoder)
from .conformer import AttentionEncoderDecoder, BeamStepper
from .hip_module import HipModule, Holder, ParamHolder, _truthy, layer_norm, linear
from .paraformer_decoder import _block, _block2, _ffn
from .register import tables

MAX_HYP = 256             # hypothesis slots of one pf_fsmndecoder handle


def fsmn_paddings(kernel_size: int, sanm_shfit) -> "tuple[int, int]":
    """(L, R) of MultiHeadedAttentionSANMDecoder (attention.py:576-580) for FsmnDecoder's sanm_shfit (None: (K - 1) // 2)"""
    K = int(kernel_size)
    shift = (K - 1) // 2 if sanm_shfit is None else int(sanm_shfit)
    left = (K - 1) // 2 + (shift if shift > 0 else 0)
    return left, K - 1 - left


@tables.register("decoder_classes", "FsmnDecoder")
class FsmnDecoder(BeamStepper, HipModule):
    _prefix = "pf_fsmndecoder"
    _max_len_why = "one utterance holds at most"          # (no positional table: the embedding is bare)

    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4, linear_units: int = 2048, num_blocks: int = 6,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, self_attention_dropout_rate: float = 0.0,
                 src_attention_dropout_rate: float = 0.0, input_layer: str = "embed", use_output_layer: bool = True, pos_enc_class=None,
                 normalize_before: bool = True, concat_after: bool = False, att_layer_num: int = 6, kernel_size: int = 21,
                 sanm_shfit: int = None, concat_embeds: bool = False, attention_dim: int = None,
                 tf2torch_tensor_name_prefix_torch: str = "decoder", tf2torch_tensor_name_prefix_tf: str = "seq2seq/decoder",
                 embed_tensor_name_prefix_tf: str = None, **kwargs):
        super().__init__()
        D, H, K = int(encoder_output_size), int(attention_heads), int(kernel_size)
        shift = (K - 1) // 2 if sanm_shfit is None else int(sanm_shfit)
        left, right = fsmn_paddings(K, sanm_shfit)
        refusals = [
            (input_layer != "embed", f"input_layer: {input_layer} (only embed)"),
            (not _truthy(use_output_layer), "use_output_layer: false"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (_truthy(concat_embeds), "concat_embeds: true"),
            (attention_dim is not None and int(attention_dim) != D, f"attention_dim: {attention_dim} (only the encoder's width, {D})"),
            (H < 1 or D not in (64 * H, 128 * H), f"attention_heads: {attention_heads} with encoder_output_size {encoder_output_size} "
                                                  "(only a head dim of 64 or 128 is built)"),
            (D > 2048, f"encoder_output_size: {encoder_output_size} (at most 2048)"),
            (int(linear_units) % 32 != 0 or not 32 <= int(linear_units) <= 2048, f"linear_units: {linear_units} (a multiple of 32, at most 2048)"),
            (not 1 <= K <= 32, f"kernel_size: {kernel_size} (1 .. 32)"),
            (shift < 0 or right < 0, f"sanm_shfit: {sanm_shfit} with kernel_size {kernel_size} (a right padding of {right})"),
            (not 1 <= int(att_layer_num) <= int(num_blocks), f"att_layer_num: {att_layer_num} of num_blocks {num_blocks} (1 .. num_blocks)"),
            (int(vocab_size) < 1, f"vocab_size: {vocab_size}"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"FsmnDecoder(HIP): {why} is not built")
        self.vocab_size, self.d_model, self.attention_heads, self.linear_units = int(vocab_size), D, H, int(linear_units)
        self.num_blocks, self.att_layer_num, self.kernel_size, self.sanm_shfit = int(num_blocks), int(att_layer_num), K, shift
        self.left_padding, self.right_padding = left, right
        emb = nn.Module()
        emb.add_module("0", ParamHolder((self.vocab_size, D)))
        self.embed = emb
        self.after_norm = layer_norm(D)
        self.output_layer = linear(self.vocab_size, D)
        self.decoders = nn.ModuleList([_block(D, self.linear_units, K) for _ in range(self.att_layer_num)])
        self.decoders2 = (nn.ModuleList([_block2(D, self.linear_units, K) for _ in range(self.num_blocks - self.att_layer_num)])
                          if self.num_blocks - self.att_layer_num > 0 else None)
        last = Holder()
        _ffn(last, D, self.linear_units)
        self.decoders3 = nn.ModuleList([last])
        self._memory = None

    def _make_config(self):
        c = _lib.pf_fsmndecoder_config()
        c.vocab_size, c.d_model, c.n_heads, c.ffn_dim, c.n_blocks = self.vocab_size, self.d_model, self.attention_heads, self.linear_units, self.num_blocks
        c.att_layer_num, c.kernel_size, c.sanm_shift, c.ln_eps = self.att_layer_num, self.kernel_size, self.sanm_shfit, 1e-12
        return c

    def _check_begin(self, max_len: int, max_hyp: int):
        super()._check_begin(max_len, max_hyp)
        if max_hyp > MAX_HYP:
            raise ValueError(f"FsmnDecoder: {max_hyp} hypotheses; one handle holds at most {MAX_HYP}")


@tables.register("model_classes", "SANM")
class SANM(AttentionEncoderDecoder):
    """funasr/models/sanm/model.py SANM(Transformer)"""
    _encoder = "SANMEncoder"
    _other_encoders = "the conv2d encoders belong to model: Conformer / Transformer"
    _decoder = "FsmnDecoder"
    _PRECISIONS = ("f16x2", "fp32")

    def set_precision(self, mode=None):
        """"f16x2": the encoder's GEMMs and attention and the CTC head on the fp16 matrix cores from two-plane operands (fp32-class
        results); "fp32": exact fp32; None: the encoder's own default, which is f16x2 where its kernels cover the width (d_k 128,
        output_size and linear_units multiples of 256) and fp32 elsewhere. The decoder step is exact fp32 in every mode."""
        if mode is not None and mode not in self._PRECISIONS:
            raise NotImplementedError(f"SANM(HIP): precision {mode!r}: built are {sorted(self._PRECISIONS)}")
        if mode == "f16x2" and self.encoder._default_precision() != "f16x2":
            raise NotImplementedError("SANM(HIP): precision 'f16x2' at this encoder width is not built (its kernels cover attention heads of "
                                      "128 dims with output_size and linear_units multiples of 256); use 'fp32' or None")
        self.encoder.set_precision(mode)
        if self.ctc is not None:
            self.ctc.set_precision(mode)
        return self

    def encode(self, speech: torch.Tensor, speech_lengths, **kwargs):
        """(normalisation +) SANMEncoder.forward with the true lengths -> (encoder_out [B, T, D], lengths): a clip's valid frames do not
        depend on what it is batched with (the encoder masks by length)"""
        if self.normalize is not None:
            dev = self.encoder._device()
            speech, speech_lengths = self.normalize(speech.to(device=dev, dtype=torch.float32).contiguous(), speech_lengths)
        out, olens, _ = self.encoder(speech, speech_lengths)
        return out, olens.to(torch.int64)

    def _features(self, data_in, data_lengths, frontend, kwargs):
        from .audio import batch_to_features

        speech, speech_lengths, meta = batch_to_features(data_in, data_lengths, frontend, kwargs)
        lens = [int(v) for v in (speech_lengths.tolist() if isinstance(speech_lengths, torch.Tensor) else
                                 ([speech_lengths] if isinstance(speech_lengths, int) else speech_lengths))]
        return speech.to(dtype=torch.float32), lens, meta
