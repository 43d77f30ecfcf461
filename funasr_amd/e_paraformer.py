"""E-Paraformer on gfx950: the non-autoregressive successor of Paraformer in the model zoo (`model: EParaformer`;
funasr/models/e_paraformer/, Interspeech 2024; recipe examples/aishell/e_paraformer/conf/e_paraformer_conformer_12e_6d_2048_256.yaml).
It decodes a whole padded batch in ONE pass: encoder -> predictor -> decoder over all tokens -> arg-max per clip.

  * encoder: `ConformerEncoder` (funasr_amd/conformer.py, handle `pf_conformer`), within its limits.
  * `PifPredictor` (predictor_classes; pif_predictor.py): parallel integrate-and-fire. The alphas come from a depthwise conv and a
    Linear as in CIF; the sequential scan is replaced by an attention from the fire positions l + 0.5 to the frames whose scores are
    -((l + 0.5 - cumsum(alphas)[t]) sigma_g)^2 per sigma head g. Handle `pf_pif` (kernels in csrc/pif.hip): two calls around one host
    read of the B token sums. Exact fp32 in every precision mode.
  * `ParaformerSANDecoder` (decoder_classes; decoder.py:1129-1251): plain Transformer decoder layers run once over the predictor's
    embeddings -- no embedding lookup, no positional encoding (the `embed.*` parameters exist and are unused), self-attention masked by
    the clips' token counts only (not causal). Handle `pf_sandecoder` (csrc/engine_conformer.hip) over the kernels of the
    Transformer family.
  * `EParaformer` (model_classes): `encode`, `calc_predictor`, `cal_decoder_with_predictor`, `inference` (greedy).

The padded-batch result is the contract: besides the Conformer's unmasked convs, the predictor's depthwise conv is not masked and
every clip gets the batch's longest token count of fire positions, so a clip's rows depend on its batch. This package reproduces the
reference's batched result; a batch of equal-length clips has no padding and there a clip's result is bitwise what it is alone.

Beyond the reference: a batch in which no clip has a token returns one empty record per key (the reference returns a bare `[]`
that its own AutoModel cannot unpack); a clip whose alpha sum is zero gets zero alphas instead of 0 / 0.
Not built: the `BeamSearchPara` path (`decoding_ctc_weight` / `lm_weight`), `pred_timestamp` (the reference hands `cif_peak = None`
to `ts_prediction_lfr6_standard` and fails there), `share_embedding`, the SANM-encoder variants, streaming, training, bf16 modes.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib
from .conformer import _PRECISIONS, PaddedBatchFront, _attention, _ffn
from .hip_module import Holder, HipModule, ParamHolder, _truthy, host_i32, layer_norm, linear, stream_ptr
from .register import tables

MAX_TOKENS = 2048          # fire positions per batch (PIF_MAX_L of csrc/pif.h)


@tables.register("predictor_classes", "PifPredictor")
class PifPredictor(HipModule):
    _prefix = "pf_pif"

    def __init__(self, idim, l_order, r_order, threshold=1.0, dropout=0.1, smooth_factor=1.0, noise_threshold=0, sigma=0.5, bias=0.0,
                 sigma_heads=4, **kwargs):
        super().__init__()
        D, H = int(idim), int(sigma_heads)
        refusals = [
            (not 1 <= H <= 8 or D % max(H, 1) != 0 or (D // max(H, 1)) % 32 != 0,
             f"sigma_heads: {sigma_heads} with idim {idim} (1 .. 8 heads of a multiple of 32 channels)"),
            (not 0 < D <= 1024, f"idim: {idim} (at most 1024)"),
            (not 0 <= int(l_order) <= 15, f"l_order: {l_order} (0 .. 15)"),
            (not 0 <= int(r_order) <= 15, f"r_order: {r_order} (0 .. 15)"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"PifPredictor(HIP): {why} is not built")
        self.idim, self.l_order, self.r_order, self.sigma_heads = D, int(l_order), int(r_order), H
        self.threshold, self.smooth_factor, self.noise_threshold = threshold, smooth_factor, noise_threshold
        self.cif_conv1d = ParamHolder((D, 1, self.l_order + self.r_order + 1), (D,))
        self.cif_output = ParamHolder((1, D), (1,))
        self.sigma = nn.Parameter(torch.tensor([float(sigma)] * H), requires_grad=False)
        self.bias = nn.Parameter(torch.tensor([float(bias)] * H), requires_grad=False)

    def _make_config(self):
        return _lib.pf_pif_config(self.idim, self.l_order, self.r_order, self.sigma_heads, float(self.threshold), float(self.smooth_factor),
                                  float(self.noise_threshold))

    def forward(self, hidden, target_label=None, mask=None, ignore_id=-1, mask_chunk_predictor=None, target_label_length=None,
                lengths=None, return_align=False):
        """hidden [B, T, D], mask [B, 1, T] (or `lengths`) -> (acoustic_embeds [B, Lmax, D], token_num [B] -- the sums BEFORE the
        normalisation --, alphas [B, T] normalised to the rounded counts, None), all on the device. Lmax = the largest rounded count;
        (B, 0, D) embeddings when no clip has a token."""
        if target_label is not None or target_label_length is not None or mask_chunk_predictor is not None:
            raise NotImplementedError("PifPredictor(HIP) implements the inference path (no target labels)")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        hid = hidden.to(device=dev, dtype=torch.float32).contiguous()
        B, T, D = hid.shape
        if lengths is None:
            lengths = [T] * B if mask is None else mask.reshape(B, -1).to(torch.float32).sum(-1).round().to(torch.int32)
        lens_c, _ = host_i32(lengths, B)
        alphas = torch.empty(B, T, device=dev, dtype=torch.float32)
        token_num = torch.empty(B, device=dev, dtype=torch.float32)
        align = torch.zeros(B, T, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.pf_pif_alphas(h, hid.data_ptr(), lens_c, B, T, alphas.data_ptr(), token_num.data_ptr(), stream_ptr()), "pf_pif_alphas")
            counts = [int(v) for v in token_num.cpu().round().tolist()]          # the one host read; torch.round: half to even, on fp32
            L = max(counts)
            if L > MAX_TOKENS:
                raise ValueError(f"PifPredictor: {L} tokens in one clip; at most {MAX_TOKENS} fire positions are built. Split the input")
            embeds = torch.empty(B, L, D, device=dev, dtype=torch.float32)
            cnt_c = (_lib.C.c_int32 * B)(*counts)
            if L > 0:
                _lib.check(lib.pf_pif_embeds(h, hid.data_ptr(), alphas.data_ptr(), token_num.data_ptr(), cnt_c, lens_c, B, T, L, align.data_ptr(),
                                             embeds.data_ptr(), stream_ptr()), "pf_pif_embeds")
            else:
                alphas.zero_()                                                    # every count is 0: n / token_num = 0 everywhere
        if return_align:
            return embeds, token_num, alphas, None, align
        return embeds, token_num, alphas, None


@tables.register("decoder_classes", "ParaformerSANDecoder")
class ParaformerSANDecoder(HipModule):
    _prefix = "pf_sandecoder"
    _skip_keys = ("embed.",)                  # built by the reference's base class, never read by its forward

    def __init__(self, vocab_size: int, encoder_output_size: int, attention_heads: int = 4, linear_units: int = 2048, num_blocks: int = 6,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, self_attention_dropout_rate: float = 0.0,
                 src_attention_dropout_rate: float = 0.0, input_layer: str = "embed", use_output_layer: bool = True,
                 normalize_before: bool = True, concat_after: bool = False, embeds_id: int = -1, precision: str = None, **kwargs):
        super().__init__()
        D, H = int(encoder_output_size), int(attention_heads)
        refusals = [
            (input_layer != "embed", f"input_layer: {input_layer} (only embed)"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (not _truthy(use_output_layer), "use_output_layer: false"),
            (int(embeds_id) >= 0, f"embeds_id: {embeds_id} (the intermediate embeddings are a training output)"),
            (H < 1 or D != 64 * H, f"attention_heads: {attention_heads} with encoder_output_size {encoder_output_size} (only a head dim of 64 is built)"),
            (int(linear_units) < 32 or int(linear_units) % 32 != 0, f"linear_units: {linear_units} (a multiple of 32)"),
            (int(num_blocks) < 1, f"num_blocks: {num_blocks}"),
            (int(vocab_size) < 1, f"vocab_size: {vocab_size}"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"ParaformerSANDecoder(HIP): {why} is not built")
        self.vocab_size, self.d_model, self.attention_heads, self.linear_units, self.num_blocks = int(vocab_size), D, H, int(linear_units), int(num_blocks)
        self.precision = "f16x2"
        self.set_precision(precision)
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

    def set_precision(self, mode=None):
        mode = mode or "f16x2"
        if mode not in _PRECISIONS:
            raise NotImplementedError(f"ParaformerSANDecoder(HIP): precision {mode!r}: built are {sorted(_PRECISIONS)}")
        self.precision = mode
        if self._handle is not None:
            _lib.check(_lib.load().pf_sandecoder_set_precision(self._handle, _PRECISIONS[mode]), "pf_sandecoder_set_precision")
        return self

    def _make_config(self):
        return _lib.pf_sandecoder_config(self.d_model, self.attention_heads, self.linear_units, self.num_blocks, self.vocab_size,
                                         _PRECISIONS[self.precision], 1e-12)

    def decode(self, hs_pad, hlens, ys_in_pad, ys_in_lens, want_logp: bool = True):
        """memory [B, T, D] with lengths, embeddings [B, L, D] with token counts -> (log-probabilities [B, L, V] or None, arg-max ids
        [B, L] int32, their log-probabilities [B, L])"""
        lib, h = self._ensure_handle()
        dev = self._handle_device
        mem = hs_pad.to(device=dev, dtype=torch.float32).contiguous()
        emb = ys_in_pad.to(device=dev, dtype=torch.float32).contiguous()
        B, T, D = mem.shape
        L = int(emb.shape[1])
        ml, _ = host_i32(hlens, B)
        tl, _ = host_i32(ys_in_lens, B)
        logp = torch.empty(B, L, self.vocab_size, device=dev, dtype=torch.float32) if want_logp else None
        ids = torch.empty(B, L, device=dev, dtype=torch.int32)
        best = torch.empty(B, L, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.pf_sandecoder_forward(h, mem.data_ptr(), ml, emb.data_ptr(), tl, B, T, L, logp.data_ptr() if want_logp else None,
                                                 ids.data_ptr(), best.data_ptr(), stream_ptr()), "pf_sandecoder_forward")
        return logp, ids, best

    def forward(self, hs_pad, hlens, ys_in_pad, ys_in_lens):
        """as the reference's forward, except that the scores are already log-softmaxed (what `cal_decoder_with_predictor` makes of them):
        (log-probabilities [B, L, V], the token counts)"""
        logp, _, _ = self.decode(hs_pad, hlens, ys_in_pad, ys_in_lens)
        _, lens = host_i32(ys_in_lens, int(logp.shape[0]))
        return logp, torch.tensor(lens, dtype=torch.int64, device=logp.device)


@tables.register("model_classes", "EParaformer")
class EParaformer(PaddedBatchFront, nn.Module):
    """funasr/models/e_paraformer/model.py EParaformer, inference path"""

    def __init__(self, specaug: Optional[str] = None, specaug_conf: Optional[Dict] = None, normalize: str = None,
                 normalize_conf: Optional[Dict] = None, encoder: str = None, encoder_conf: Optional[Dict] = None, decoder: str = None,
                 decoder_conf: Optional[Dict] = None, ctc: str = None, ctc_conf: Optional[Dict] = None, predictor: str = None,
                 predictor_conf: Optional[Dict] = None, ctc_weight: float = 0.5, input_size: int = 80, vocab_size: int = -1, ignore_id: int = -1,
                 blank_id: int = 0, sos: int = 1, eos: int = 2, lsm_weight: float = 0.0, length_normalized_loss: bool = False,
                 predictor_weight: float = 0.0, predictor_bias: int = 2, sampling_ratio: float = 0.2, share_embedding: bool = False,
                 use_1st_decoder_loss: bool = True, **kwargs):
        super().__init__()
        if encoder != "ConformerEncoder":
            raise NotImplementedError(f"EParaformer(HIP): encoder: {encoder} is not built (only ConformerEncoder, the published recipe; "
                                      "SANMEncoder belongs to model: Paraformer)")
        if decoder != "ParaformerSANDecoder" or float(ctc_weight) == 1.0:
            raise NotImplementedError(f"EParaformer(HIP): decoder: {decoder if float(ctc_weight) != 1.0 else 'none (ctc_weight: 1.0)'} is not "
                                      "built (only ParaformerSANDecoder; ParaformerSANMDecoder belongs to model: Paraformer)")
        if predictor != "PifPredictor":
            raise NotImplementedError(f"EParaformer(HIP): predictor: {predictor} is not built (only PifPredictor; the CIF predictors belong "
                                      "to model: Paraformer)")
        if _truthy(share_embedding):
            raise NotImplementedError("EParaformer(HIP): share_embedding: true is not built")
        if kwargs.get("bf16", False) or kwargs.get("precision") in ("bf16", "bf16x3"):
            raise NotImplementedError("EParaformer(HIP): the bf16 modes are not built (precision: f16x2 or fp32)")
        enc_conf = dict(encoder_conf or {})
        enc_conf.pop("input_size", None)
        self.encoder = tables.encoder_classes["ConformerEncoder"](input_size=input_size, **enc_conf)
        d = self.encoder.output_size()
        dec_conf = dict(decoder_conf or {})
        dec_conf.pop("vocab_size", None)
        dec_conf.pop("encoder_output_size", None)
        self.decoder = ParaformerSANDecoder(vocab_size=vocab_size, encoder_output_size=d, **dec_conf)
        self.ctc = None
        if float(ctc_weight) > 0.0:               # its parameters load; greedy decoding does not read them
            from .ctc import CTC
            self.ctc = CTC(odim=vocab_size, encoder_output_size=d, **(ctc_conf or {}))
        pred_conf = dict(predictor_conf or {})
        if int(pred_conf.get("idim", d)) != d:
            raise NotImplementedError(f"EParaformer(HIP): predictor_conf.idim: {pred_conf.get('idim')} differs from the encoder's output_size {d}")
        self.predictor = PifPredictor(**pred_conf)
        self.normalize = None
        if normalize is not None:
            from . import normalize as _normalize  # noqa: F401  (registers normalize_classes)
            self.normalize = tables.normalize_classes.get(normalize)(**(normalize_conf or {}))
        self.specaug = None                       # training-time augmentation: accepted, never applied
        self.blank_id, self.vocab_size, self.ignore_id, self.ctc_weight = blank_id, vocab_size, ignore_id, float(ctc_weight)
        self.sos = sos if sos is not None else vocab_size - 1
        self.eos = eos if eos is not None else vocab_size - 1
        self.beam_search = None
        if kwargs.get("precision"):
            self.set_precision(kwargs["precision"])

    def set_precision(self, mode=None):
        """"f16x2" (default): the encoder blocks' GEMMs and the decoder GEMMs with an a-priori operand bound on the fp16 matrix cores
        from two-plane operands (fp32-class results); "fp32": exact-fp32 MFMA GEMMs everywhere. The predictor is exact fp32 in both."""
        if mode in ("bf16", "bf16x3"):
            raise NotImplementedError("EParaformer(HIP): the bf16 modes are not built (precision: f16x2 or fp32)")
        self.encoder.set_precision(mode)
        self.decoder.set_precision(mode)
        if self.ctc is not None:
            self.ctc.set_precision(mode)
        return self

    # ------------------------------------------------------------------------------------------------ device pipeline
    def calc_predictor(self, encoder_out, encoder_out_lens):
        """model.py:321-335 -> (acoustic_embeds, token_num, alphas, None)"""
        return self.predictor(encoder_out, None, None, ignore_id=self.ignore_id, lengths=encoder_out_lens)

    def cal_decoder_with_predictor(self, encoder_out, encoder_out_lens, sematic_embeds, ys_pad_lens):
        """model.py:337-352 -> (log-probabilities [B, L, V], ys_pad_lens)"""
        logp, _, _ = self.decoder.decode(encoder_out, encoder_out_lens, sematic_embeds, ys_pad_lens)
        return logp, ys_pad_lens

    def greedy(self, speech, lens):
        """zero-padded features -> per clip the arg-max ids of its own token rows (host lists) and the rounded counts"""
        encoder_out, olens = self.encode(speech, lens)
        embeds, token_num, _, _ = self.calc_predictor(encoder_out, olens)
        counts = [int(v) for v in token_num.cpu().round().tolist()]
        if max(counts) < 1:
            return [[] for _ in counts], counts
        _, ids, _ = self.decoder.decode(encoder_out, olens, embeds, counts, want_logp=False)
        ids = ids.cpu()
        return [ids[b, :n].tolist() for b, n in enumerate(counts)], counts

    # ------------------------------------------------------------------------------------------------ inference
    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """model.py:600-763, the greedy path: any batch_size, data_type sound / fbank, output_dir writers, tokenizer=None -> token_int"""
        from .tokenizer import sentence_postprocess

        if float(kwargs.get("decoding_ctc_weight", 0.0) or 0.0) > 0.00001:
            raise NotImplementedError("EParaformer(HIP): decoding_ctc_weight > 0 (the BeamSearchPara path) is not built")
        if float(kwargs.get("lm_weight", 0.0) or 0.0) > 0.00001:
            raise NotImplementedError("EParaformer(HIP): lm_weight > 0 (the BeamSearchPara path) is not built")
        if kwargs.get("pred_timestamp", False):
            raise NotImplementedError("EParaformer(HIP): pred_timestamp is not built (the reference passes cif_peak = None into "
                                      "ts_prediction_lfr6_standard and fails there)")
        if kwargs.get("bf16", False):
            raise NotImplementedError("EParaformer(HIP): the bf16 modes are not built (precision: f16x2 or fp32)")
        speech, lens, meta = self._features(data_in, data_lengths, frontend, kwargs)
        ids, _ = self.greedy(speech, lens)
        b = len(ids)
        if key is None:
            key = [f"utt_{i}" for i in range(b)]
        if isinstance(key[0], (list, tuple)):
            key = key[0]
        if len(key) < b:
            key = key * b
        writer = self._writer(kwargs, "1best_recog")
        drop = (self.eos, self.sos, self.blank_id)
        results = []
        for i in range(b):
            token_int = [t for t in ids[i] if t not in drop]
            if tokenizer is None:
                results.append({"key": key[i], "token_int": token_int})
                continue
            token = tokenizer.ids2tokens(token_int)
            text = tokenizer.tokens2text(token)
            if not hasattr(tokenizer, "bpemodel"):
                text, _ = sentence_postprocess(token)
            results.append({"key": key[i], "text": text})
            if writer is not None:
                writer["token"][key[i]] = " ".join(token)
                writer["text"][key[i]] = text
        return results, meta
