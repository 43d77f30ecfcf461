"""Keyword spotting on gfx950: `FsmnKWS` (funasr/models/fsmn_kws/model.py, `encoder: FSMN` with a right context and no softmax) and
`SanmKWS` (funasr/models/sanm_kws/model.py, `encoder: SANMEncoder` plus a `CTC` head), both over `KwsCtcPrefixDecoder`
(funasr_amd/kws_utils.py).

One call of `inference` takes the whole batch through ONE encoder pass, ONE candidate launch (`pf_kws_candidates`: the softmax,
the top 3 and the keyword filter of every frame of every clip) and ONE read-back of 7 x B x T words; the prefix search and the hit
test then run per clip in the library's host code. Records are the reference's: `{"key", "text"}` with `text` =
`"detected <keyword> <str(score)>"` or `"rejected"`; with `output_dir` the `detect` file is written (without it the reference dies
on `self.writer`; here nothing is written).

The FSMN gets no lengths, as in the reference (`self.encoder(speech)`): every row of the zero-padded feature batch is computed and
the last `rorder * rstride` frames of a shorter clip read the padding frames behind it, so a clip decoded in a batch and alone may
differ -- as it does there. The SAN-M encoder masks by length.

Precision: fp32 for both (the KWS SAN-M sizes have no f16x2 kernels, the FSMN GEMMs are tiny); `bf16` is refused by name.
Not built, each refused by name: `FsmnKWSMT`, `SanmKWSStreaming`, `FsmnKWSConvert` / `FsmnKWSMTConvert` (the Kaldi-net converters), export.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import fsmn_vad as _fsmn_vad  # noqa: F401  (registers encoder_classes FSMN)
from . import sanm_encoder as _sanm_encoder  # noqa: F401  (registers SANMEncoder)
from .conformer import PaddedBatchFront
from .hip_module import Holder, _truthy
from .kws_utils import KwsCtcPrefixDecoder, candidates
from .register import tables

NOT_BUILT = {
    "FsmnKWSMT": "the multi-task FSMN keyword spotter (two output heads) is not built; model: FsmnKWS is",
    "SanmKWSStreaming": "the chunk-streaming SAN-M keyword spotter is not built; model: SanmKWS is",
    "FsmnKWSConvert": "the Kaldi-net converter classes are not built (to_kaldi_net / to_pytorch_net); model: FsmnKWS is",
    "FsmnKWSMTConvert": "the Kaldi-net converter classes are not built (to_kaldi_net / to_pytorch_net); model: FsmnKWS is",
}


def _refuse_precision(who: str, kwargs: dict):
    if _truthy(kwargs.get("bf16", False)) or kwargs.get("precision") in ("bf16", "bf16x3", "f16x2"):
        raise NotImplementedError(f"{who}(HIP): bf16 / precision: {kwargs.get('precision', 'bf16')} is not built (the keyword "
                                  "spotters run in fp32)")


class _NoProjection(Holder):
    """`CTC(extra_linear=False)` (ctc.py:43-46): no `ctc_lo`, no parameters; the encoder output is the logits"""
    ctc_lo = None


class _KwsBase(PaddedBatchFront, torch.nn.Module):
    def _init_common(self, specaug, normalize, normalize_conf, vocab_size, ignore_id, blank_id, ctc_weight, kwargs):
        me = type(self).__name__
        _refuse_precision(me, kwargs)
        if int(blank_id) != 0:
            raise NotImplementedError(f"{me}(HIP): blank_id: {blank_id} is not built (the keyword search takes token 0 as the blank)")
        self.normalize = None
        if normalize is not None:
            from . import normalize as _normalize  # noqa: F401  (registers normalize_classes)
            self.normalize = tables.normalize_classes.get(normalize)(**(normalize_conf or {}))
        self.specaug = None                                       # training-time augmentation: accepted, never applied
        self.vocab_size, self.ignore_id, self.blank_id, self.ctc_weight = int(vocab_size), ignore_id, int(blank_id), ctc_weight
        self.keywords = kwargs.get("keywords")
        self.error_calculator = None

    def _make_ctc(self, d: int, ctc_conf: Optional[Dict]):
        conf = dict(ctc_conf or {})
        if not _truthy(conf.pop("extra_linear", True)):
            if d != self.vocab_size:
                raise ValueError(f"ctc_conf.extra_linear: false needs an encoder of vocab_size outputs ({d} != {self.vocab_size})")
            return _NoProjection()
        from .ctc import CTC
        return CTC(odim=self.vocab_size, encoder_output_size=d, **conf).set_precision("fp32")

    def _logits(self, speech: torch.Tensor, lens):  # pragma: no cover - abstract
        raise NotImplementedError

    def set_precision(self, mode=None):
        if mode not in (None, "fp32"):
            raise NotImplementedError(f"{type(self).__name__}(HIP): precision: {mode} is not built (the keyword spotters run in fp32)")
        return self

    def make_decoder(self, keywords, tokenizer) -> KwsCtcPrefixDecoder:
        if keywords is None:
            raise ValueError("keywords: a comma-separated keyword string is required (AutoModel(keywords=...) or generate(keywords=...))")
        if tokenizer is None or getattr(tokenizer, "token_list", None) is None:
            raise ValueError(f"{type(self).__name__}.inference needs the tokenizer of the model directory (its token_list)")
        if len(tokenizer.token_list) != self.vocab_size:
            raise ValueError(f"token_list has {len(tokenizer.token_list)} entries, the model {self.vocab_size} outputs")
        key = (str(keywords), id(tokenizer))
        if self.__dict__.get("_kws_key") != key:                  # the reference rebuilds it per call; the result is the same
            self.__dict__["kws_decoder"] = KwsCtcPrefixDecoder(ctc=self.ctc, keywords=keywords, token_list=tokenizer.token_list,
                                                               seg_dict=getattr(tokenizer, "seg_dict", None))
            self.__dict__["_kws_key"] = key
        return self.__dict__["kws_decoder"]

    def detect(self, speech: torch.Tensor, lens, decoder: KwsCtcPrefixDecoder):
        """features [B, T, F] (zero-padded) -> [(detected, keyword | None, score | None)] per clip: one encoder pass, one candidate
        launch, one read-back"""
        logits, olens = self._logits(speech, lens)
        B, T = int(logits.shape[0]), int(logits.shape[1])
        cand = candidates(logits.reshape(B * T, -1) if logits.is_contiguous() else logits.flatten(0, 1), decoder.mask_on(logits.device),
                          self.vocab_size)
        return decoder.decode_candidates(cand.cpu().numpy().reshape(B, T, 7), olens)

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        _refuse_precision(type(self).__name__, kwargs)
        decoder = self.make_decoder(kwargs.get("keywords", self.keywords), tokenizer)
        speech, lens, meta = self._features(data_in, data_lengths, frontend, kwargs)
        results = self.detect(speech, lens, decoder)
        if key is None:
            key = [f"utt_{i}" for i in range(len(results))]
        writer = self._writer(kwargs, "detect")
        out = []
        for i, (hit, keyword, score) in enumerate(results):
            info = "detected " + keyword + " " + str(score) if hit else "rejected"
            if writer is not None:
                writer[key[i]] = info
            out.append({"key": key[i], "text": info})
        return out, meta

    def export(self, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}(HIP): export is not built")

    def forward(self, *a, **k):  # pragma: no cover
        raise NotImplementedError("use inference(); training is not built")


@tables.register("model_classes", "FsmnKWS")
class FsmnKWS(_KwsBase):
    """funasr/models/fsmn_kws/model.py FsmnKWS (inference)"""

    def __init__(self, specaug: Optional[str] = None, specaug_conf: Optional[Dict] = None, normalize: str = None,
                 normalize_conf: Optional[Dict] = None, encoder: str = None, encoder_conf: Optional[Dict] = None, ctc: str = None,
                 ctc_conf: Optional[Dict] = None, ctc_weight: float = 1.0, input_size: int = 360, vocab_size: int = -1,
                 ignore_id: int = -1, blank_id: int = 0, **kwargs):
        super().__init__()
        if encoder != "FSMN":
            raise NotImplementedError(f"FsmnKWS(HIP): encoder: {encoder} is not built (only FSMN; FSMNConvert is the Kaldi-net converter)")
        self._init_common(specaug, normalize, normalize_conf, vocab_size, ignore_id, blank_id, ctc_weight, kwargs)
        self.encoder = tables.encoder_classes["FSMN"](**(encoder_conf or {}))
        self.ctc = self._make_ctc(self.encoder.output_size(), ctc_conf)
        if self.encoder.use_softmax:
            raise NotImplementedError("FsmnKWS(HIP): encoder_conf.use_softmax: true is not built (the search normalises the encoder output itself)")
        for p in self.parameters():
            p.requires_grad_(False)

    def _logits(self, speech, lens):
        if self.normalize is not None:
            speech, lens = self.normalize(speech.to(device=self.encoder._device(), dtype=torch.float32).contiguous(), lens)
        out = self.encoder.logits(speech)                          # no lengths: all B x T rows, as the reference's encoder(speech)
        return (out if self.ctc.ctc_lo is None else self.ctc.logits(out.contiguous())), [int(v) for v in lens]


@tables.register("model_classes", "SanmKWS")
class SanmKWS(_KwsBase):
    """funasr/models/sanm_kws/model.py SanmKWS (inference)"""

    def __init__(self, specaug: Optional[str] = None, specaug_conf: Optional[Dict] = None, normalize: str = None,
                 normalize_conf: Optional[Dict] = None, encoder: str = None, encoder_conf: Optional[Dict] = None, ctc: str = None,
                 ctc_conf: Optional[Dict] = None, ctc_weight: float = 1.0, input_size: int = 360, vocab_size: int = -1,
                 ignore_id: int = -1, blank_id: int = 0, sos: int = 1, eos: int = 2, **kwargs):
        super().__init__()
        if encoder != "SANMEncoder":
            raise NotImplementedError(f"SanmKWS(HIP): encoder: {encoder} is not built (only SANMEncoder; SANMEncoderChunkOpt belongs "
                                      "to SanmKWSStreaming)")
        self._init_common(specaug, normalize, normalize_conf, vocab_size, ignore_id, blank_id, ctc_weight, kwargs)
        enc_conf = dict(encoder_conf or {})
        enc_conf.pop("input_size", None)
        self.encoder = tables.encoder_classes["SANMEncoder"](input_size=input_size, **enc_conf)
        self.encoder.set_precision("fp32")
        self.ctc = self._make_ctc(self.encoder.output_size(), ctc_conf)
        self.sos = sos if sos is not None else vocab_size - 1
        self.eos = eos if eos is not None else vocab_size - 1
        for p in self.parameters():
            p.requires_grad_(False)

    def _logits(self, speech, lens):
        out, _ = self.encode(speech, lens)                         # (the encoder keeps the lengths it is given)
        return (out if self.ctc.ctc_lo is None else self.ctc.logits(out)), [int(v) for v in lens]


def refuse_not_built(name: str):
    """AutoModel: the keyword-spotting classes of the reference that are not built are refused by name"""
    if name in NOT_BUILT:
        raise NotImplementedError(f"model: {name} is not built ({NOT_BUILT[name]})")
