"""LCB-Net on gfx950: long-context biasing ASR (`model: LCBNet`, the zoo's iic/LCB-NET; funasr/models/lcbnet/). It takes audio plus
the OCR text of the slides and returns text: `AutoModel.generate(input=(wav, ocr_txt), data_type=("sound", "text"))`.

The audio side is the Transformer family (funasr_amd/transformer.py: `TransformerEncoder`, `TransformerDecoder`, the CTC head, the
joint CTC-prefix / attention beam search). This module adds the text side:

  * `TransformerTextEncoder` (encoder_classes; lcbnet/encoder.py:130-241): Embedding x sqrt(D) + the absolute sinusoid, pre-LayerNorm
    blocks of masked self-attention and a ReLU feed-forward, `after_norm`. One `pf_textencoder` handle: the block loop of the audio
    encoder behind another front (token rows instead of the subsampling; csrc/lcbnet.hip, csrc/engine_conformer.hip).
  * `FusionSANEncoder` (encoder_classes; lcbnet/encoder.py:244-370, `SelfSrcAttention`): ONE layer whose queries are audio frames and
    whose keys are text tokens -- self-attention, cross-attention over the text encoder's rows (`tf_cross_attention_kernel`),
    feed-forward. One `pf_fusion` handle.
  * `ConvBiasPredictor` (encoder_classes): parameter holders only. The reference constructs it, keeps it in the state dict and never
    calls it at inference.
  * `LCBNet` (model_classes): `encoder_out + fusion_encoder(encoder_out, text_encoder(ocr))`, then the family's beam search.

Both new handles run exact-fp32 GEMMs in every mode; `precision: f16x2 | fp32` means the audio encoder, the decoder and the CTC head,
as in `Transformer`.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib
from .conformer import MAX_LEN, AttentionEncoderDecoder, _attention, _ffn, abs_pos_table
from .hip_module import HipModule, Holder, ParamHolder, _truthy, layer_norm, linear, stream_ptr
from .register import tables
from .transformer import TransformerEncoder  # noqa: F401  (registers the audio encoder the model names)

DEFAULT_OCR_IDS = (294, 0)        # lcbnet/model.py:501-504: the ids the reference decodes with when no text comes with the audio


def _refuse(who: str, refusals):
    for bad, why in refusals:
        if bad:
            raise NotImplementedError(f"{who}(HIP): {why} is not built")


def _lengths(lens, n: int, full: int, what: str):
    """None -> NULL (every row); otherwise n lengths in [0, full] as a ctypes array"""
    if lens is None:
        return None
    vals = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    if len(vals) != n or any(v < 0 or v > full for v in vals):
        raise ValueError(f"{what}: {n} lengths in 0 .. {full} expected, got {vals}")
    return (_lib.C.c_int32 * n)(*vals)


@tables.register("encoder_classes", "TransformerTextEncoder")
class TransformerTextEncoder(HipModule):
    _prefix = "pf_textencoder"

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048, num_blocks: int = 6,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0, pos_enc_class=None,
                 normalize_before: bool = True, concat_after: bool = False, **kwargs):
        super().__init__()
        D, H = int(output_size), int(attention_heads)
        _refuse("TransformerTextEncoder", [
            (pos_enc_class is not None, "pos_enc_class (only the default PositionalEncoding)"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (H < 1 or D != 64 * H, f"attention_heads: {attention_heads} with output_size {output_size} (only a head dim of 64 is built)"),
            (int(linear_units) % 32 != 0, f"linear_units: {linear_units} (a multiple of 32)"),
            (int(input_size) < 1, f"input_size: {input_size} (the vocabulary size)"),
        ])
        self.vocab_size, self._output_size, self.attention_heads, self.linear_units = int(input_size), D, H, int(linear_units)
        self.num_blocks = int(num_blocks)
        emb = nn.Module()
        emb.add_module("0", ParamHolder((self.vocab_size, D)))
        self.embed = emb
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
        self.pos_table = abs_pos_table(D)          # the reference's `pe`: a plain attribute there and here, not in the state dict

    def output_size(self) -> int:
        return self._output_size

    def pos_rows(self, L: int):
        return self.pos_table[:L]

    def _extra_tensors(self):
        return (("pos_table", self.pos_table),)

    def _make_config(self):
        c = _lib.pf_textencoder_config()
        c.vocab_size, c.d_model, c.n_heads, c.ffn_dim, c.n_blocks, c.ln_eps = (self.vocab_size, self._output_size, self.attention_heads,
                                                                              self.linear_units, self.num_blocks, 1e-12)
        return c

    def forward(self, xs_pad, ilens):
        """xs_pad [B, L] token ids (a tensor or lists of equal length), ilens [B] -> (out [B, L, D] on the device, olens [B] int64,
        None): every row is computed, keys at or past ilens[b] are masked (lcbnet/encoder.py:219-241)"""
        ids = xs_pad.detach().cpu().to(torch.int64) if isinstance(xs_pad, torch.Tensor) else torch.tensor(xs_pad, dtype=torch.int64)
        if ids.dim() != 2:
            raise ValueError(f"TransformerTextEncoder: token ids [B, L] expected, got {tuple(ids.shape)}")
        B, L = int(ids.shape[0]), int(ids.shape[1])
        if not 1 <= L <= MAX_LEN:
            raise ValueError(f"TransformerTextEncoder: {L} tokens; 1 .. {MAX_LEN} (the positional table holds {MAX_LEN})")
        bad = ids[(ids < 0) | (ids >= self.vocab_size)]
        if bad.numel():
            raise ValueError(f"TransformerTextEncoder: token id {int(bad[0])} is outside the vocabulary of {self.vocab_size}")
        ln = _lengths(ilens, B, L, "TransformerTextEncoder")
        if ln is None:
            raise ValueError("TransformerTextEncoder: ilens is required")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        out = torch.empty(B, L, self._output_size, device=dev)
        flat = (_lib.C.c_int32 * (B * L))(*ids.reshape(-1).tolist())
        with torch.cuda.device(dev):
            _lib.check(lib.pf_textencoder_forward(h, flat, ln, B, L, out.data_ptr(), stream_ptr()), "pf_textencoder_forward")
        return out, torch.tensor(list(ln), dtype=torch.int64, device=dev), None


@tables.register("encoder_classes", "FusionSANEncoder")
class FusionSANEncoder(HipModule):
    """lcbnet/encoder.py SelfSrcAttention, registered under the reference's key"""
    _prefix = "pf_fusion"

    def __init__(self, size: int, attention_heads: int, attention_dim: int, linear_units: int, self_attention_dropout_rate: float = 0.0,
                 src_attention_dropout_rate: float = 0.0, positional_dropout_rate: float = 0.0, dropout_rate: float = 0.0,
                 normalize_before: bool = True, concat_after: bool = False, **kwargs):
        super().__init__()
        D, H = int(size), int(attention_heads)
        _refuse("FusionSANEncoder", [
            (int(attention_dim) != D, f"attention_dim: {attention_dim} with size {size} (only attention_dim == size)"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (H < 1 or D != 64 * H, f"attention_heads: {attention_heads} with size {size} (only a head dim of 64 is built)"),
            (int(linear_units) % 32 != 0, f"linear_units: {linear_units} (a multiple of 32)"),
        ])
        self.size, self.attention_heads, self.linear_units = D, H, int(linear_units)
        self.self_attn, self.src_attn = _attention(D, rel=False), _attention(D, rel=False)
        self.feed_forward = _ffn(D, self.linear_units)
        self.norm1, self.norm2, self.norm3 = layer_norm(D), layer_norm(D), layer_norm(D)
        for p in self.parameters():
            p.requires_grad_(False)

    def output_size(self) -> int:
        return self.size

    def _make_config(self):
        c = _lib.pf_fusion_config()
        c.d_model, c.n_heads, c.ffn_dim, c.ln_eps = self.size, self.attention_heads, self.linear_units, 1e-12
        return c

    def forward(self, tgt: torch.Tensor, tgt_mask, memory: torch.Tensor, memory_mask, add_input: bool = False):
        """tgt [B, T, D] audio rows, memory [B, L, D] text rows -> (out [B, T, D], tgt_mask, memory, memory_mask) as the reference's
        layer. The masks are LENGTHS here ([B], or None = every row / every key: what the model passes, as the reference does).
        add_input: out = tgt + layer(tgt, memory), the model's `encoder_out + fusion_out`, summed inside the last GEMM."""
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = tgt.to(device=dev, dtype=torch.float32).contiguous()
        mem = memory.to(device=dev, dtype=torch.float32).contiguous()
        if x.dim() != 3 or mem.dim() != 3 or x.shape[0] != mem.shape[0] or x.shape[2] != self.size or mem.shape[2] != self.size:
            raise ValueError(f"FusionSANEncoder: tgt [B, T, {self.size}] and memory [B, L, {self.size}] expected, got {tuple(x.shape)} and "
                             f"{tuple(mem.shape)}")
        B, T, L = int(x.shape[0]), int(x.shape[1]), int(mem.shape[1])
        xl = _lengths(tgt_mask, B, T, "FusionSANEncoder tgt_mask")
        ml = _lengths(memory_mask, B, L, "FusionSANEncoder memory_mask")
        out = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.check(lib.pf_fusion_forward(h, x.data_ptr(), xl, mem.data_ptr(), ml, B, T, L, int(bool(add_input)), out.data_ptr(),
                                             stream_ptr()), "pf_fusion_forward")
        return out, tgt_mask, memory, memory_mask


@tables.register("encoder_classes", "ConvBiasPredictor")
class ConvBiasPredictor(nn.Module):
    """lcbnet/encoder.py ConvPredictor: the parameters under the reference's keys, so that `load_state_dict(strict=True)` takes a real
    checkpoint. `LCBNet.inference` never runs it (it is a training-time head), so no kernel exists."""

    def __init__(self, size: int = 256, l_order: int = 3, r_order: int = 3, attention_heads: int = 4, attention_dropout_rate: float = 0.1,
                 linear_units: int = 2048, **kwargs):
        super().__init__()
        D = int(size)
        self.atten = _attention(D, rel=False)
        self.norm1 = layer_norm(D)
        self.feed_forward = _ffn(D, int(linear_units))
        self.norm2 = layer_norm(D)
        self.conv1d = ParamHolder((D, 1, int(l_order) + int(r_order) + 1), (D,))
        self.output_linear = linear(1, D)
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("ConvBiasPredictor(HIP): inference never runs the bias predictor (the reference's LCBNet.inference does not "
                                  "call it); its forward is not built")


@tables.register("model_classes", "LCBNet")
class LCBNet(AttentionEncoderDecoder):
    """funasr/models/lcbnet/model.py LCBNet: inference"""
    _encoder = "TransformerEncoder"
    _other_encoders = "the reference's LCB-Net is built on the plain Transformer encoder"

    def __init__(self, text_encoder: str = None, text_encoder_conf: Optional[Dict] = None, bias_predictor: str = None,
                 bias_predictor_conf: Optional[Dict] = None, fusion_encoder: str = None, fusion_encoder_conf: Optional[Dict] = None,
                 select_num: int = 2, select_length: int = 3, insert_blank: bool = True, **kwargs):
        super().__init__(**kwargs)
        for opt, name, want in (("text_encoder", text_encoder, "TransformerTextEncoder"), ("fusion_encoder", fusion_encoder, "FusionSANEncoder"),
                                ("bias_predictor", bias_predictor, "ConvBiasPredictor")):
            if name != want:
                raise NotImplementedError(f"LCBNet(HIP): {opt}: {name} is not built (only {want})")
        d = self.encoder.output_size()
        tconf = dict(text_encoder_conf or {})
        tconf.pop("input_size", None)
        self.text_encoder = TransformerTextEncoder(input_size=self.vocab_size, **tconf)
        self.fusion_encoder = FusionSANEncoder(**dict(fusion_encoder_conf or {}))
        self.bias_predictor = ConvBiasPredictor(**dict(bias_predictor_conf or {}))
        if self.text_encoder.output_size() != d:
            raise NotImplementedError(f"LCBNet(HIP): text_encoder_conf output_size: {self.text_encoder.output_size()} is not built (only the "
                                      f"audio encoder's {d})")
        if self.fusion_encoder.output_size() != d:
            raise NotImplementedError(f"LCBNet(HIP): fusion_encoder_conf size: {self.fusion_encoder.output_size()} is not built (only the audio "
                                      f"encoder's {d})")
        self.sos = self.eos = self.vocab_size - 1                     # model.py:153-154: the constructor's sos / eos are ignored
        self.select_num, self.select_length, self.insert_blank = select_num, select_length, insert_blank      # training only

    def init_beam_search(self, **kwargs):
        """lcbnet/model.py:400-448: the family's search with this model's defaults (beam 20, decoding_ctc_weight 0.3)"""
        super().init_beam_search(**dict({"beam_size": 20, "decoding_ctc_weight": 0.3}, **kwargs))

    # ------------------------------------------------------------------------------------------------ the OCR text
    def ocr_ids(self, token_ids=None) -> List[int]:
        """the ids the text encoder reads (model.py:501-504,520): the tokenizer's ids of the OCR text (None: the reference's literal
        default [294, 0]), every id but 0 shifted by +1"""
        ids = list(DEFAULT_OCR_IDS) if token_ids is None else [int(t) for t in token_ids]
        if not ids:
            raise ValueError("LCBNet: the OCR text is empty (no token ids); pass the audio alone to decode with the default ids")
        out = []
        for t in ids:
            s = t + 1 if t != 0 else 0
            if t < 0 or s >= self.vocab_size:
                raise ValueError(f"LCBNet: OCR token id {t} (read as {s} after the shift by one) is outside the vocabulary of {self.vocab_size}"
                                 + (" (the default ids [294, 0] need a vocabulary of at least 296)" if token_ids is None else ""))
            out.append(s)
        return out

    def fuse(self, encoder_out: torch.Tensor, ocr: List[int]) -> torch.Tensor:
        """model.py:521-527: encoder_out [1, T, D] + fusion_encoder(encoder_out, text_encoder(ocr)); `ocr`: the shifted ids"""
        text, _, _ = self.text_encoder([list(ocr)], [len(ocr)])
        fused, _, _, _ = self.fusion_encoder(encoder_out, None, text, None, add_input=True)
        return fused

    # ------------------------------------------------------------------------------------------------ inference
    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """lcbnet/model.py:450-574, one utterance per call. `data_type=("sound", "text")`: data_in holds one (audio, text) pair, the
        text a string or a path to a text file. Plain "sound" input decodes with the reference's default ids [294, 0]. So does
        `data_type="fbank"`, which goes beyond the reference: its fbank route raises UnboundLocalError (`ocr_sample_list` is unbound)."""
        from .audio import load_audio_text
        from .tokenizer import sentence_postprocess

        if kwargs.get("batch_size", 1) > 1:
            raise NotImplementedError("batch decoding is not implemented")
        if self.beam_search is None:
            if kwargs.get("token_list") is None and tokenizer is not None and getattr(tokenizer, "token_list", None) is not None:
                kwargs = dict(kwargs, token_list=tokenizer.token_list)
            self.init_beam_search(**kwargs)
            self.nbest = kwargs.get("nbest", 1)
        t0 = time.perf_counter()
        data_type = kwargs.get("data_type", "sound")
        token_ids = None
        if isinstance(data_type, (list, tuple)):
            if tuple(data_type) != ("sound", "text"):
                raise NotImplementedError(f'LCBNet(HIP): data_type {tuple(data_type)} is not built (("sound", "text"), "sound", "fbank")')
            if frontend is None:
                raise ValueError("LCBNet.inference needs the frontend of the model directory")
            audio_list, text_list = load_audio_text(data_in, fs=frontend.fs, audio_fs=kwargs.get("fs", 16000), data_type=data_type,
                                                    tokenizer=tokenizer)
            if len(audio_list) != 1:
                raise NotImplementedError("batch decoding is not implemented")
            token_ids = text_list[0]
            data_in, kwargs = audio_list, dict(kwargs, data_type="sound")
        ocr = self.ocr_ids(token_ids)
        speech, lens, meta = self._features(data_in, data_lengths, frontend, kwargs)
        if speech.shape[0] != 1:
            raise NotImplementedError("batch decoding is not implemented")
        encoder_out, olens = self.encode(speech, lens)
        encoder_out = self.fuse(encoder_out, ocr)
        nbest = self.beam_search_features(encoder_out[0], kwargs.get("maxlenratio", 0.0), kwargs.get("minlenratio", 0.0))[: self.nbest]
        meta.setdefault("decode", f"{time.perf_counter() - t0:0.3f}")
        if key is None:
            key = ["utt_0"]
        results = []
        for nbest_idx, hyp in enumerate(nbest):
            writer = self._writer(kwargs, f"{nbest_idx + 1}best_recog")
            token_int = [t for t in hyp.yseq[1:-1] if t != self.eos and t != self.sos and t != self.blank_id]
            token = tokenizer.ids2tokens(token_int)
            text, _ = sentence_postprocess(token)
            results.append({"key": key[0], "token": token, "text": text})
            if writer is not None:
                writer["token"][key[0]] = " ".join(token)
                writer["text"][key[0]] = text
        return results, meta
