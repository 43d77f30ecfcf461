"""Conformer ASR on gfx950: the CTC / attention encoder-decoder family of the model zoo (`model: Conformer`;
funasr/models/conformer/model.py over funasr/models/transformer/model.py).

  * `ConformerEncoder` (encoder_classes): Conv2dSubsampling, relative-position self-attention in the reference's two variants
    (`rel_pos_type: legacy` -- the default, what the released checkpoints use -- and `latest`), macaron feed-forwards, the
    GLU / depthwise-conv / BatchNorm / Swish convolution module. One `pf_conformer` handle (csrc/engine_conformer.hip).
  * `TransformerDecoder` (decoder_classes): the autoregressive decoder as a device-resident stepper (`begin` / `step` / `reorder`,
    handle `pf_tdecoder`): cross-attention K / V once per utterance, a self-attention K / V cache per hypothesis slot.
  * `Conformer` (model_classes): the reference's `inference` dispatch -- `batch_size > 1`: greedy CTC over the padded batch, text
    only; otherwise the joint CTC-prefix / attention beam search (funasr_amd/transformer_search.py), `nbest` records with `token`
    and `text`.

The reference runs Conv2dSubsampling and the convolution module over the ZERO-PADDED batch without masking, so a clip's encoder
frames (and, through the mask rule, its output length) depend on the longest clip it is batched with. This package is a drop-in:
the padded-batch result is the contract, every row of the batch is computed. A batch of equal-length clips has no padding and
there a clip's result is bitwise what it is alone.

`Conv2dSubsampledEncoder` (the forward over the padded batch) and `AttentionEncoderDecoder` (the model: everything but the encoder)
are the bases this module shares with funasr_amd/transformer.py, the plain-Transformer sibling.

All modules hold the reference's parameters under the reference's state_dict keys (BatchNorm's running statistics included);
the positional tables are built on the host exactly as the reference builds them (float32 torch ops) and uploaded.
"""
from __future__ import annotations

import math
import time
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib
from .hip_module import Holder, HipModule, ParamHolder, _truthy, layer_norm, linear, stream_ptr
from .register import tables

_PRECISIONS = {"fp32": 0, "f16x2": 3}
MAX_LEN = 5000            # rows of the reference's positional tables (PositionalEncoding(max_len=5000))


def _sinusoid(position: torch.Tensor, d_model: int) -> torch.Tensor:
    """embedding.py:66-76 for a column of float32 positions"""
    pe = torch.zeros(position.shape[0], d_model)
    div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def abs_pos_table(d_model: int, max_len: int = MAX_LEN) -> torch.Tensor:
    """PositionalEncoding.pe (embedding.py:59-78): row p = the sinusoid of position p"""
    return _sinusoid(torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1), d_model)


def legacy_rel_pos_table(d_model: int, max_len: int = MAX_LEN) -> torch.Tensor:
    """LegacyRelPositionalEncoding.pe (reverse=True): row m = the sinusoid of position max_len - 1 - m; a forward over T frames takes
    its FIRST T rows (embedding.py:250-252), i.e. positions 4999, 4998, ..."""
    return _sinusoid(torch.arange(max_len - 1, -1, -1.0, dtype=torch.float32).unsqueeze(1), d_model)


def latest_rel_pos_table(d_model: int, max_len: int = MAX_LEN) -> torch.Tensor:
    """RelPositionalEncoding.pe (embedding.py:279-309): 2 max_len - 1 rows, row k = position max_len - 1 - k (the negative half is
    computed as sin / cos of -1 * position * div_term); a forward over T frames takes rows [max_len - T, max_len + T - 1)"""
    position = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / d_model))
    pos = torch.zeros(max_len, d_model)
    neg = torch.zeros(max_len, d_model)
    pos[:, 0::2] = torch.sin(position * div_term)
    pos[:, 1::2] = torch.cos(position * div_term)
    neg[:, 0::2] = torch.sin(-1 * position * div_term)
    neg[:, 1::2] = torch.cos(-1 * position * div_term)
    return torch.cat([torch.flip(pos, [0]), neg[1:]], dim=0)


def subsampled_length(n: int, padded: int) -> int:
    """encoder frames of a clip of n feature frames in a batch padded to `padded` frames: x_mask[:, :, :-2:2][:, :, :-2:2]"""
    def sub(L, m):
        k = min(L, m - 2)
        return 0 if k <= 0 else (k + 1) // 2
    return sub(sub(n, padded), sub(padded, padded))


class TooShortUttError(Exception):
    """funasr/models/transformer/utils/nets_utils.py TooShortUttError"""

    def __init__(self, message, actual_size, limit):
        super().__init__(message)
        self.actual_size, self.limit = actual_size, limit


def _attention(D: int, rel: bool) -> Holder:
    a = Holder()
    a.linear_q, a.linear_k, a.linear_v, a.linear_out = linear(D, D), linear(D, D), linear(D, D), linear(D, D)
    if rel:
        a.linear_pos = linear(D, D, bias=False)
        a.pos_bias_u = nn.Parameter(torch.zeros(D // 64, 64), requires_grad=False)
        a.pos_bias_v = nn.Parameter(torch.zeros(D // 64, 64), requires_grad=False)
    return a


def _ffn(D: int, units: int) -> Holder:
    f = Holder()
    f.w_1, f.w_2 = linear(units, D), linear(D, units)
    return f


class Conv2dSubsampledEncoder(HipModule):
    """what the two encoders behind Conv2dSubsampling share: the precision switch and the forward over the zero-padded batch (the C
    entry points `<_prefix>_set_precision` / `<_prefix>_forward` have one signature). A subclass holds the parameters, `pos_table`,
    `precision` and `_output_size`."""

    def output_size(self) -> int:
        return self._output_size

    def _extra_tensors(self):
        return (("pos_table", self.pos_table),)

    def set_precision(self, mode=None):
        mode = mode or "f16x2"
        if mode not in _PRECISIONS:
            raise NotImplementedError(f"{type(self).__name__}(HIP): precision {mode!r}: built are {sorted(_PRECISIONS)}")
        self.precision = mode
        if self._handle is not None:
            _lib.check(getattr(_lib.load(), self._prefix + "_set_precision")(self._handle, _PRECISIONS[mode]), self._prefix + "_set_precision")
        return self

    def forward(self, xs_pad: torch.Tensor, ilens, prev_states=None, ctc=None):
        """xs_pad [B, L, input_size] zero-padded features, ilens [B] -> (out [B, T, D], olens [B] int64 on the device, None): every
        row of the padded batch, lengths by the reference's mask rule (funasr/models/conformer/encoder.py:559-636)"""
        lens = [int(v) for v in (ilens.tolist() if isinstance(ilens, torch.Tensor) else ilens)]
        B, L = int(xs_pad.shape[0]), int(xs_pad.shape[1])
        if L < 7:
            raise TooShortUttError(f"has {L} frames and is too short for subsampling (it needs more than 7 frames), return empty results", L, 7)
        T = subsampled_length(L, L)
        if T > MAX_LEN:
            raise ValueError(f"{type(self).__name__}: {T} encoder frames in one batch; the positional tables hold {MAX_LEN} (200 s of audio). "
                             "Split the input (the reference's result beyond that depends on the process's call history)")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = xs_pad.to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty(B, T, self._output_size, device=dev)
        ln = (_lib.C.c_int32 * B)(*lens)
        ol = (_lib.C.c_int32 * B)()
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, self._prefix + "_forward")(h, x.data_ptr(), ln, B, L, out.data_ptr(), ol, stream_ptr()), self._prefix + "_forward")
            torch.cuda.current_stream(dev).synchronize()           # the lengths are staged asynchronously
        olens = torch.tensor(list(ol), dtype=torch.int64, device=dev)
        return out, olens, None


@tables.register("encoder_classes", "ConformerEncoder")
class ConformerEncoder(Conv2dSubsampledEncoder):
    _prefix = "pf_conformer"
    _push_buffers = True

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048, num_blocks: int = 6,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0,
                 input_layer: str = "conv2d", normalize_before: bool = True, concat_after: bool = False,
                 positionwise_layer_type: str = "linear", positionwise_conv_kernel_size: int = 3, macaron_style: bool = False,
                 rel_pos_type: str = "legacy", pos_enc_layer_type: str = "rel_pos", selfattention_layer_type: str = "rel_selfattn",
                 activation_type: str = "swish", use_cnn_module: bool = True, zero_triu: bool = False, cnn_module_kernel: int = 31,
                 padding_idx: int = -1, interctc_layer_idx=(), interctc_use_conditioning: bool = False, stochastic_depth_rate=0.0,
                 precision: str = None, **kwargs):
        super().__init__()
        if rel_pos_type not in ("legacy", "latest"):
            raise ValueError("unknown rel_pos_type: " + str(rel_pos_type))
        D, H = int(output_size), int(attention_heads)
        refusals = [
            (input_layer != "conv2d", f"input_layer: {input_layer} (only conv2d, the 1/4 subsampling)"),
            (pos_enc_layer_type != "rel_pos", f"pos_enc_layer_type: {pos_enc_layer_type} (only rel_pos)"),
            (selfattention_layer_type != "rel_selfattn", f"selfattention_layer_type: {selfattention_layer_type} (only rel_selfattn)"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (positionwise_layer_type != "linear", f"positionwise_layer_type: {positionwise_layer_type} (only linear)"),
            (activation_type != "swish", f"activation_type: {activation_type} (only swish)"),
            (not _truthy(use_cnn_module), "use_cnn_module: false"),
            (_truthy(zero_triu), "zero_triu: true"),
            (len(list(interctc_layer_idx or ())) > 0, "interctc_layer_idx"),
            (_truthy(interctc_use_conditioning), "interctc_use_conditioning: true"),
            (int(cnn_module_kernel) % 2 != 1 or int(cnn_module_kernel) > 31, f"cnn_module_kernel: {cnn_module_kernel} (odd, at most 31)"),
            (H < 1 or D != 64 * H, f"attention_heads: {attention_heads} with output_size {output_size} (only a head dim of 64 is built)"),
            (int(linear_units) % 32 != 0, f"linear_units: {linear_units} (a multiple of 32)"),
            (not 7 <= int(input_size) <= 256, f"input_size: {input_size} (7 .. 256 features)"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"ConformerEncoder(HIP): {why} is not built")
        mode = precision or "f16x2"
        if mode not in _PRECISIONS:
            raise NotImplementedError(f"ConformerEncoder(HIP): precision {mode!r}: built are {sorted(_PRECISIONS)}")
        self.precision = mode
        self.input_size, self._output_size, self.attention_heads, self.linear_units = int(input_size), D, H, int(linear_units)
        self.num_blocks, self.kernel, self.macaron, self.legacy = int(num_blocks), int(cnn_module_kernel), _truthy(macaron_style), rel_pos_type == "legacy"
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
            b.self_attn = _attention(D, rel=True)
            b.feed_forward = _ffn(D, self.linear_units)
            if self.macaron:
                b.feed_forward_macaron = _ffn(D, self.linear_units)
            cm = Holder()
            cm.pointwise_conv1 = ParamHolder((2 * D, D, 1), (2 * D,))
            cm.depthwise_conv = ParamHolder((D, 1, self.kernel), (D,))
            cm.norm = nn.BatchNorm1d(D)                                  # a holder like the others: eval-mode statistics, never executed
            cm.pointwise_conv2 = ParamHolder((D, D, 1), (D,))
            b.conv_module = cm
            b.norm_ff, b.norm_mha = layer_norm(D), layer_norm(D)
            if self.macaron:
                b.norm_ff_macaron = layer_norm(D)
            b.norm_conv, b.norm_final = layer_norm(D), layer_norm(D)
            blocks.append(b)
        self.encoders = blocks
        self.after_norm = layer_norm(D)
        for p in self.parameters():
            p.requires_grad_(False)
        # the reference's table, built as it builds it: float32 torch ops on the host. Not a parameter and not in the state dict
        # (the reference keeps `pe` as a plain attribute). Its values depend on the host's float32 exp() in the last bit of
        # div_term -- a sinusoid of position ~5000 moves by up to 5e-4 with it -- exactly as the reference's own table does.
        self.pos_table = legacy_rel_pos_table(D) if self.legacy else latest_rel_pos_table(D)

    def pos_rows(self, T: int) -> torch.Tensor:
        """the rows of the table a forward over T encoder frames reads (a view)"""
        return self.pos_table[:T] if self.legacy else self.pos_table[MAX_LEN - T: MAX_LEN + T - 1]

    def _make_config(self):
        c = _lib.pf_conformer_config()
        c.input_dim, c.d_model, c.n_heads, c.ffn_dim = self.input_size, self._output_size, self.attention_heads, self.linear_units
        c.n_blocks, c.kernel_size, c.macaron, c.legacy = self.num_blocks, self.kernel, int(self.macaron), int(self.legacy)
        c.precision, c.ln_eps = _PRECISIONS[self.precision], 1e-12
        return c


class BeamStepper:
    """the stepper of funasr_amd.transformer_search.BeamSearchTransformer over the C calls `<_prefix>_begin / _step / _reorder` (a
    mix-in of the HipModule decoders that hold `vocab_size`); messages carry the class's own name"""
    _max_len_why = "the positional table holds"

    def set_precision(self, mode=None):
        """accepted for symmetry: every GEMM of a step has M = n_hyp rows and runs the fp32 weight-streaming kernel in every mode"""
        return self

    def set_memory(self, memory: torch.Tensor):
        """memory [T, D]: the encoder output of ONE utterance (its valid frames)"""
        self._ensure_handle()
        self._memory = memory.to(device=self._handle_device, dtype=torch.float32).contiguous()
        return self

    def _check_begin(self, max_len: int, max_hyp: int):
        """the limits of the handle that the class refuses in its own words"""
        if max_len > MAX_LEN:
            raise ValueError(f"{type(self).__name__}: {max_len} output positions; {self._max_len_why} {MAX_LEN}")

    def _call(self, what: str, *args):
        """`<_prefix>_<what>(handle, *args, stream)` on the handle's device"""
        lib, h = self._ensure_handle()
        name = f"{self._prefix}_{what}"
        with torch.cuda.device(self._handle_device):
            _lib.check(getattr(lib, name)(h, *args, stream_ptr()), name)
            if what != "begin":
                torch.cuda.current_stream(self._handle_device).synchronize()      # the ids / parents are staged asynchronously

    def begin(self, max_len: int, max_hyp: int):
        if self._memory is None:
            raise RuntimeError(f"{type(self).__name__}.begin: set_memory(encoder_out) first")
        self._check_begin(max_len, max_hyp)
        self._call("begin", self._memory.data_ptr(), int(self._memory.shape[0]), int(max_len), int(max_hyp))

    def step(self, tokens: List[int], pos: int) -> torch.Tensor:
        self._ensure_handle()                                                     # (the handle's device is known from here on)
        n = len(tokens)
        out = torch.empty(n, self.vocab_size, device=self._handle_device)
        self._call("step", (_lib.C.c_int32 * n)(*[int(t) for t in tokens]), int(pos), n, out.data_ptr())
        return out

    def reorder(self, parents: List[int]):
        n = len(parents)
        self._call("reorder", (_lib.C.c_int32 * n)(*[int(p) for p in parents]), n)


@tables.register("decoder_classes", "TransformerDecoder")
class TransformerDecoder(BeamStepper, HipModule):
    _prefix = "pf_tdecoder"

    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4, linear_units: int = 2048, num_blocks: int = 6,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, self_attention_dropout_rate: float = 0.0,
                 src_attention_dropout_rate: float = 0.0, input_layer: str = "embed", use_output_layer: bool = True,
                 normalize_before: bool = True, concat_after: bool = False, **kwargs):
        super().__init__()
        D, H = int(encoder_output_size), int(attention_heads)
        refusals = [
            (input_layer != "embed", f"input_layer: {input_layer} (only embed)"),
            (not _truthy(use_output_layer), "use_output_layer: false"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (H < 1 or D != 64 * H, f"attention_heads: {attention_heads} with encoder_output_size {encoder_output_size} (only a head dim of 64 is built)"),
            (int(linear_units) % 32 != 0, f"linear_units: {linear_units} (a multiple of 32)"),
            (int(vocab_size) < 1, f"vocab_size: {vocab_size}"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"TransformerDecoder(HIP): {why} is not built")
        self.vocab_size, self.d_model, self.attention_heads, self.linear_units, self.num_blocks = int(vocab_size), D, H, int(linear_units), int(num_blocks)
        emb = nn.Module()
        emb.add_module("0", ParamHolder((self.vocab_size, D)))
        self.embed = emb
        self.after_norm = layer_norm(D)
        self.output_layer = linear(self.vocab_size, D)
        layers = nn.ModuleList()
        for _ in range(self.num_blocks):
            b = Holder()
            b.self_attn, b.src_attn = _attention(D, rel=False), _attention(D, rel=False)
            b.feed_forward = _ffn(D, self.linear_units)
            b.norm1, b.norm2, b.norm3 = layer_norm(D), layer_norm(D), layer_norm(D)
            layers.append(b)
        self.decoders = layers
        self._memory = None

    def _extra_tensors(self):
        return (("pos_table", abs_pos_table(self.d_model)),)

    def _make_config(self):
        c = _lib.pf_tdecoder_config()
        c.vocab_size, c.d_model, c.n_heads, c.ffn_dim, c.n_blocks, c.ln_eps = (self.vocab_size, self.d_model, self.attention_heads,
                                                                              self.linear_units, self.num_blocks, 1e-12)
        return c


class PaddedBatchFront:
    """the head every model over a `Conv2dSubsampledEncoder` shares (a mix-in of nn.Module classes that hold `encoder` and
    `normalize`): features of the ZERO-padded batch, (normalisation +) encoder, the lazily made result writer. Used by
    `AttentionEncoderDecoder` below and by funasr_amd.transducer.Transducer."""

    def encode(self, speech: torch.Tensor, speech_lengths, **kwargs):
        """transformer/model.py:288-325: (normalisation +) encoder over the padded batch -> (encoder_out [B, T, D], lengths)"""
        if self.normalize is not None:
            dev = self.encoder._device()
            speech, speech_lengths = self.normalize(speech.to(device=dev, dtype=torch.float32).contiguous(), speech_lengths)
        out, olens, _ = self.encoder(speech, speech_lengths)
        return out, olens

    def _features(self, data_in, data_lengths, frontend, kwargs):
        from .audio import batch_to_features

        speech, speech_lengths, meta = batch_to_features(data_in, data_lengths, frontend, kwargs)
        lens = [int(v) for v in (speech_lengths.tolist() if isinstance(speech_lengths, torch.Tensor) else
                                 ([speech_lengths] if isinstance(speech_lengths, int) else speech_lengths))]
        speech = speech.to(dtype=torch.float32)
        if any(n < speech.shape[1] for n in lens):                    # the contract is the ZERO-padded batch
            speech = speech.clone()
            for b, n in enumerate(lens):
                speech[b, n:] = 0
        return speech, lens, meta

    def _writer(self, kwargs, name):
        if kwargs.get("output_dir") is None:
            return None
        if not hasattr(self, "writer"):
            from .datadir_writer import DatadirWriter
            self.writer = DatadirWriter(kwargs.get("output_dir"))
        return self.writer[name]


class AttentionEncoderDecoder(PaddedBatchFront, nn.Module):
    """funasr/models/transformer/model.py Transformer, the CTC / attention encoder-decoder the reference's `Conformer` subclasses
    with nothing added: everything but the encoder. A model class names the one encoder it accepts (`_encoder`) and what its
    refusal of another says (`_other_encoders`), and the one decoder (`_decoder`); funasr_amd.transformer.Transformer and
    funasr_amd.sanm.SANM are the others."""
    _encoder = None                # the encoder_classes key
    _other_encoders = ""
    _decoder = "TransformerDecoder"    # the decoder_classes key (funasr_amd.sanm.SANM names "FsmnDecoder")

    def __init__(self, specaug: Optional[str] = None, specaug_conf: Optional[Dict] = None, normalize: str = None,
                 normalize_conf: Optional[Dict] = None, encoder: str = None, encoder_conf: Optional[Dict] = None, decoder: str = None,
                 decoder_conf: Optional[Dict] = None, ctc: str = None, ctc_conf: Optional[Dict] = None, ctc_weight: float = 0.5,
                 interctc_weight: float = 0.0, input_size: int = 80, vocab_size: int = -1, ignore_id: int = -1, blank_id: int = 0,
                 sos: int = 1, eos: int = 2, lsm_weight: float = 0.0, length_normalized_loss: bool = False, report_cer: bool = True,
                 report_wer: bool = True, sym_space: str = "<space>", sym_blank: str = "<blank>", share_embedding: bool = False, **kwargs):
        super().__init__()
        me = type(self).__name__
        if encoder != self._encoder:
            raise NotImplementedError(f"{me}(HIP): encoder: {encoder} is not built (only {self._encoder}; {self._other_encoders})")
        if decoder is None or float(ctc_weight) == 1.0:
            raise NotImplementedError(f"{me}(HIP): a model without decoder (decoder: null or ctc_weight: 1.0) is not built")
        if decoder != self._decoder:
            raise NotImplementedError(f"{me}(HIP): decoder: {decoder} is not built (only {self._decoder})")
        if float(interctc_weight) != 0.0:
            raise NotImplementedError(f"{me}(HIP): interctc_weight is not built")
        if _truthy(share_embedding):
            raise NotImplementedError(f"{me}(HIP): share_embedding: true is not built")
        enc_conf = dict(encoder_conf or {})
        enc_conf.pop("input_size", None)
        self.encoder = tables.encoder_classes[self._encoder](input_size=input_size, **enc_conf)
        d = self.encoder.output_size()
        dec_conf = dict(decoder_conf or {})
        dec_conf.pop("vocab_size", None)
        dec_conf.pop("encoder_output_size", None)
        self.decoder = tables.decoder_classes[self._decoder](vocab_size=vocab_size, encoder_output_size=d, **dec_conf)
        self.ctc = None
        if float(ctc_weight) > 0.0:                                   # transformer/model.py:118-123,163-166
            from .ctc import CTC
            self.ctc = CTC(odim=vocab_size, encoder_output_size=d, **(ctc_conf or {}))
        self.normalize = None
        if normalize is not None:
            from . import normalize as _normalize  # noqa: F401  (registers normalize_classes)
            self.normalize = tables.normalize_classes.get(normalize)(**(normalize_conf or {}))
        self.specaug = None                                           # training-time augmentation: accepted, never applied
        self.blank_id, self.vocab_size, self.ignore_id, self.ctc_weight = blank_id, vocab_size, ignore_id, float(ctc_weight)
        self.sos = sos if sos is not None else vocab_size - 1
        self.eos = eos if eos is not None else vocab_size - 1
        self.beam_search = None
        self.nbest = 1
        if kwargs.get("precision"):
            self.set_precision(kwargs["precision"])

    def set_precision(self, mode=None):
        """"f16x2" (default): the encoder blocks' GEMMs on the fp16 matrix cores from two-plane operands (fp32-class results);
        "fp32": exact-fp32 MFMA GEMMs everywhere"""
        self.encoder.set_precision(mode)
        self.decoder.set_precision(mode)
        if self.ctc is not None:
            self.ctc.set_precision(mode)
        return self

    # ------------------------------------------------------------------------------------------------ device pipeline
    def ctc_greedy(self, encoder_out: torch.Tensor, olens) -> List[List[int]]:
        """arg-max of the CTC head over each clip's valid frames, repeats collapsed, blanks dropped (model.py:442-447)"""
        ids = self.ctc.argmax(encoder_out).cpu()
        res = []
        for i, n in enumerate([int(v) for v in olens.tolist()]):
            y = torch.unique_consecutive(ids[i, :n], dim=-1)
            res.append(y[y != self.blank_id].tolist())
        return res

    def init_beam_search(self, **kwargs):
        """transformer/model.py:464-512"""
        from .transformer_search import BeamSearchTransformer

        token_list = kwargs.get("token_list")
        n_vocab = len(token_list) if token_list is not None else self.vocab_size
        w = kwargs.get("decoding_ctc_weight", 0.5)
        self.beam_search = BeamSearchTransformer(beam_size=kwargs.get("beam_size", 10), vocab_size=n_vocab, sos=self.sos, eos=self.eos,
                                                 ctc_weight=w if self.ctc is not None else 0.0,
                                                 length_bonus_weight=kwargs.get("penalty", 0.0), blank=0,
                                                 pre_beam=self.ctc_weight != 1.0)
        if self.ctc is None:                                          # the reference keeps `decoder = 1 - decoding_ctc_weight` even then
            self.beam_search.w_dec = 1.0 - w

    def beam_search_features(self, encoder_out: torch.Tensor, maxlenratio: float = 0.0, minlenratio: float = 0.0):
        """encoder_out [T, D] of one utterance -> the n-best hypotheses (transformer_search.Hypothesis), best first"""
        ctc_logp = None
        if self.beam_search.w_ctc != 0 and self.ctc is not None:      # CTCPrefixScorer.init_state (scorers/ctc.py:26-38)
            ctc_logp = self.ctc.log_softmax(encoder_out[None])[0].cpu().numpy()
        self.decoder.set_memory(encoder_out)
        return self.beam_search(self.decoder, int(encoder_out.shape[0]), ctc_logp, maxlenratio, minlenratio)

    # ------------------------------------------------------------------------------------------------ inference
    def inference_batch_ctc(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """transformer/model.py:390-462"""
        from .tokenizer import sentence_postprocess

        if self.ctc is None:
            raise RuntimeError(f"{type(self).__name__}.inference(batch_size > 1) decodes the CTC head; this model has none (ctc_weight 0)")
        speech, lens, meta = self._features(data_in, data_lengths, frontend, kwargs)
        encoder_out, olens = self.encode(speech, lens)
        ids = self.ctc_greedy(encoder_out, olens)
        if key is None:
            key = [f"utt_{i}" for i in range(len(ids))]
        writer = self._writer(kwargs, "1best_recog")
        results = []
        for i, token_int in enumerate(ids):
            token = tokenizer.ids2tokens(token_int)
            text, _ = sentence_postprocess(token)
            results.append({"key": key[i], "text": text})
            if writer is not None:
                writer["token"][key[i]] = " ".join(token)
                writer["text"][key[i]] = text
        return results, meta

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """transformer/model.py:514-629: batch_size > 1 -> greedy CTC; otherwise beam search over the attention decoder"""
        from .tokenizer import sentence_postprocess

        if kwargs.get("batch_size", 1) > 1:
            return self.inference_batch_ctc(data_in, data_lengths=data_lengths, key=key, tokenizer=tokenizer, frontend=frontend, **kwargs)
        if self.beam_search is None:
            if kwargs.get("token_list") is None and tokenizer is not None and getattr(tokenizer, "token_list", None) is not None:
                kwargs = dict(kwargs, token_list=tokenizer.token_list)
            self.init_beam_search(**kwargs)
            self.nbest = kwargs.get("nbest", 1)
        t0 = time.perf_counter()
        speech, lens, meta = self._features(data_in, data_lengths, frontend, kwargs)
        encoder_out, olens = self.encode(speech, lens)
        nbest = self.beam_search_features(encoder_out[0], kwargs.get("maxlenratio", 0.0), kwargs.get("minlenratio", 0.0))[: self.nbest]
        meta.setdefault("decode", f"{time.perf_counter() - t0:0.3f}")
        if key is None:
            key = [f"utt_{i}" for i in range(encoder_out.shape[0])]
        results = []
        for i in range(encoder_out.shape[0]):
            for nbest_idx, hyp in enumerate(nbest):
                writer = self._writer(kwargs, f"{nbest_idx + 1}best_recog")
                token_int = [t for t in hyp.yseq[1:-1] if t != self.eos and t != self.sos and t != self.blank_id]
                token = tokenizer.ids2tokens(token_int)
                text, _ = sentence_postprocess(token)
                results.append({"key": key[i], "token": token, "text": text})
                if writer is not None:
                    writer["token"][key[i]] = " ".join(token)
                    writer["text"][key[i]] = text
        return results, meta


@tables.register("model_classes", "Conformer")
class Conformer(AttentionEncoderDecoder):
    """funasr/models/conformer/model.py Conformer(Transformer)"""
    _encoder = "ConformerEncoder"
    _other_encoders = "the Transformer / Branchformer families are other models"
