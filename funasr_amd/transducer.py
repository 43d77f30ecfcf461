"""Transducer (RNN-T) ASR on gfx950: the fourth decoding family of the model zoo (`model: Transducer`;
funasr/models/transducer/model.py, rnnt_decoder.py, joint_network.py, beam_search_transducer.py).

  * `RNNTDecoder` (decoder_classes "rnnt_decoder"): the prediction network -- an embedding and `num_layers` one-layer LSTMs -- as a
    parameter holder under the reference's keys (`embed.weight`, `rnn.{l}.weight_ih_l0` ...).
  * `JointNetwork` (joint_network_classes "joint_network"): `lin_enc`, `lin_dec` (no bias), `lin_out`, tanh.
  * `Transducer` (model_classes): the encoder is the Conformer's, the Transformer's, the RWKV encoder's (the reference template's own,
    funasr_amd/rwkv_encoder.py) or the chunk Conformer's HIP handle (funasr_amd/chunk_conformer.py); the model itself owns ONE
    `pf_transducer` handle (csrc/engine_transducer.hip) that holds both networks and runs the reference's one decoding path --
    `BeamSearchTransducer(decoder, joint_network, beam_size, nbest=1)` with the default search, one utterance per call, no LM --
    inside the library: a prediction step (csrc/transducer.hip) only for a new label prefix, two launches per joint evaluation,
    one small read-back, scores in double.

The search arithmetic is exact fp32 whatever `precision` the encoder runs in. The reference's `while True` has no guard; here a
non-finite joint value and more than `max_expansions_per_frame` (default 64 x beam_size) joint evaluations in one frame raise
RuntimeError.

Not built (each refused by name): `rnn_type: gru`, joint activations other than tanh, encoders other than ConformerEncoder /
TransformerEncoder / RWKVEncoder / ChunkConformerEncoder (and, for the last two, encoder_conf keys their constructors do not name), `model: BAT` (refused where AutoModel resolves the name), `beam_size > 16`; the tsd / alsd / maes searches, LM fusion, chunk-by-chunk search and batched
search do not exist here. `use_embed_mask: true` is a training-time augmentation: accepted and ignored.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from .conformer import PaddedBatchFront
from .hip_module import HipModule, Holder, ParamHolder, linear, stream_ptr
from .register import tables

MAX_DIM, MAX_LAYERS, MAX_BEAM = 1024, 4, 16           # csrc/transducer.h
_ENCODERS = ("ConformerEncoder", "TransformerEncoder", "RWKVEncoder", "ChunkConformerEncoder")


def _check_dim(who: str, name: str, value: int):
    if int(value) < 4 or int(value) % 4 != 0 or int(value) > MAX_DIM:
        raise NotImplementedError(f"{who}(HIP): {name}: {value} is not built (a multiple of 4, at most {MAX_DIM})")


class _LstmHolder(nn.Module):
    """the parameters of torch.nn.LSTM(in, hidden, 1) in its order and under its names; never executed"""

    def __init__(self, in_dim: int, hidden: int):
        super().__init__()
        self.weight_ih_l0 = nn.Parameter(torch.zeros(4 * hidden, in_dim), requires_grad=False)
        self.weight_hh_l0 = nn.Parameter(torch.zeros(4 * hidden, hidden), requires_grad=False)
        self.bias_ih_l0 = nn.Parameter(torch.zeros(4 * hidden), requires_grad=False)
        self.bias_hh_l0 = nn.Parameter(torch.zeros(4 * hidden), requires_grad=False)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: computation happens inside libparaformer_hip.so")


@tables.register("decoder_classes", "rnnt_decoder")
class RNNTDecoder(Holder):
    """funasr/models/transducer/rnnt_decoder.py RNNTDecoder: parameters only; the step runs in the model's pf_transducer handle.
    `embed_pad` is the reference's padding_idx, which has no effect at inference: row 0 is a weight row like any other."""

    def __init__(self, vocab_size: int, embed_size: int = 256, hidden_size: int = 256, rnn_type: str = "lstm", num_layers: int = 1,
                 dropout_rate: float = 0.0, embed_dropout_rate: float = 0.0, embed_pad: int = 0, use_embed_mask: bool = False):
        super().__init__()
        if rnn_type not in ("lstm", "gru"):
            raise ValueError(f"Not supported: rnn_type={rnn_type}")
        if rnn_type != "lstm":
            raise NotImplementedError(f"RNNTDecoder(HIP): rnn_type: {rnn_type} is not built (only lstm)")
        _check_dim("RNNTDecoder", "embed_size", embed_size)
        _check_dim("RNNTDecoder", "hidden_size", hidden_size)
        if not 1 <= int(num_layers) <= MAX_LAYERS:
            raise NotImplementedError(f"RNNTDecoder(HIP): num_layers: {num_layers} is not built (1 .. {MAX_LAYERS})")
        if int(vocab_size) < 2:
            raise NotImplementedError(f"RNNTDecoder(HIP): vocab_size: {vocab_size} is not built (at least 2)")
        self.vocab_size, self.embed_size, self.output_size = int(vocab_size), int(embed_size), int(hidden_size)
        self.dlayers, self.dtype = int(num_layers), rnn_type
        self.use_embed_mask = use_embed_mask                      # training-time augmentation: accepted, never applied
        self.embed = ParamHolder((self.vocab_size, self.embed_size))
        self.rnn = nn.ModuleList([_LstmHolder(self.embed_size if l == 0 else self.output_size, self.output_size)
                                  for l in range(self.dlayers)])


@tables.register("joint_network_classes", "joint_network")
class JointNetwork(Holder):
    """funasr/models/transducer/joint_network.py JointNetwork: parameters only"""

    def __init__(self, output_size: int, encoder_size: int, decoder_size: int, joint_space_size: int = 256,
                 joint_activation_type: str = "tanh", **activation_parameters):
        super().__init__()
        if joint_activation_type != "tanh":
            raise NotImplementedError(f"JointNetwork(HIP): joint_activation_type: {joint_activation_type} is not built (only tanh)")
        _check_dim("JointNetwork", "joint_space_size", joint_space_size)
        _check_dim("JointNetwork", "encoder_size (the encoder's output_size)", encoder_size)
        self.joint_space_size = int(joint_space_size)
        self.lin_enc = linear(self.joint_space_size, int(encoder_size))
        self.lin_dec = linear(self.joint_space_size, int(decoder_size), bias=False)
        self.lin_out = linear(int(output_size), self.joint_space_size)


class TransducerSearchError(RuntimeError):
    """the search ended on one of its guards (a non-finite joint value, the per-frame expansion cap)"""


@tables.register("model_classes", "Transducer")
class Transducer(PaddedBatchFront, HipModule):
    """funasr/models/transducer/model.py Transducer (inference)"""
    _prefix = "pf_transducer"
    _set_tensor_name = "pf_transducer_set_weights"
    _skip_keys = ("encoder.", "ctc_lin.", "lm_lin.")             # the encoder has its own handle; the auxiliary heads are training-only

    def __init__(self, frontend: Optional[str] = None, frontend_conf: Optional[Dict] = None, specaug: Optional[str] = None,
                 specaug_conf: Optional[Dict] = None, normalize: str = None, normalize_conf: Optional[Dict] = None, encoder: str = None,
                 encoder_conf: Optional[Dict] = None, decoder: str = None, decoder_conf: Optional[Dict] = None, joint_network: str = None,
                 joint_network_conf: Optional[Dict] = None, transducer_weight: float = 1.0, fastemit_lambda: float = 0.0,
                 auxiliary_ctc_weight: float = 0.0, auxiliary_ctc_dropout_rate: float = 0.0, auxiliary_lm_loss_weight: float = 0.0,
                 auxiliary_lm_loss_smoothing: float = 0.0, input_size: int = 80, vocab_size: int = -1, ignore_id: int = -1,
                 blank_id: int = 0, sos: int = 1, eos: int = 2, lsm_weight: float = 0.0, length_normalized_loss: bool = False,
                 share_embedding: bool = False, **kwargs):
        super().__init__()
        if encoder not in _ENCODERS:
            raise NotImplementedError(f"Transducer(HIP): encoder: {encoder} is not built (only {' / '.join(_ENCODERS)})")
        if decoder != "rnnt_decoder":
            raise NotImplementedError(f"Transducer(HIP): decoder: {decoder} is not built (only rnnt_decoder)")
        if joint_network != "joint_network":
            raise NotImplementedError(f"Transducer(HIP): joint_network: {joint_network} is not built (only joint_network)")
        if int(blank_id) != 0:
            raise NotImplementedError(f"Transducer(HIP): blank_id: {blank_id} is not built (the search takes row 0 as the blank)")
        if encoder == "ConformerEncoder":
            from . import conformer  # noqa: F401  (registers it)
        elif encoder == "TransformerEncoder":
            from . import transformer  # noqa: F401
        elif encoder == "ChunkConformerEncoder":
            from . import chunk_conformer
            foreign = chunk_conformer.foreign_keys(encoder_conf)
            if foreign:                                           # the reference's constructor has no **kwargs: TypeError there
                raise NotImplementedError(f"Transducer(HIP): encoder: ChunkConformerEncoder does not take encoder_conf keys {foreign} (its "
                                          f"constructor's are {', '.join(chunk_conformer.CONF_KEYS)})")
        else:
            from . import rwkv_encoder
            foreign = rwkv_encoder.foreign_keys(encoder_conf)
            if foreign:                                           # the reference swallows them in **kwargs and builds another geometry
                raise NotImplementedError(f"Transducer(HIP): encoder: RWKVEncoder does not take encoder_conf keys {foreign} (its "
                                          f"constructor's are {', '.join(rwkv_encoder.CONF_KEYS)}); the reference ignores them silently")
        enc_conf = dict(encoder_conf or {})
        enc_conf.pop("input_size", None)
        self.encoder = tables.encoder_classes[encoder](input_size=input_size, **enc_conf)
        d = self.encoder.output_size()
        dec_conf = dict(decoder_conf or {})
        dec_conf.pop("vocab_size", None)
        self.decoder = RNNTDecoder(vocab_size=vocab_size, **dec_conf)
        self.joint_network = JointNetwork(vocab_size, d, self.decoder.output_size, **(joint_network_conf or {}))
        self.use_auxiliary_ctc = float(auxiliary_ctc_weight) > 0
        self.use_auxiliary_lm_loss = float(auxiliary_lm_loss_weight) > 0
        if self.use_auxiliary_ctc:                                # held under the reference's keys, unused at inference
            self.ctc_lin = linear(int(vocab_size), d)
        if self.use_auxiliary_lm_loss:
            self.lm_lin = linear(int(vocab_size), self.decoder.output_size)
        self.normalize = None
        if normalize is not None:
            from . import normalize as _normalize  # noqa: F401  (registers normalize_classes)
            self.normalize = tables.normalize_classes.get(normalize)(**(normalize_conf or {}))
        self.specaug = None                                       # training-time augmentation: accepted, never applied
        self.vocab_size, self.ignore_id, self.blank_id = int(vocab_size), ignore_id, int(blank_id)
        self.sos = sos if sos is not None else vocab_size - 1
        self.eos = eos if eos is not None else vocab_size - 1
        self.ctc = None
        self.beam_size, self.nbest = None, 1
        for p in self.parameters():
            p.requires_grad_(False)
        if kwargs.get("precision"):
            self.set_precision(kwargs["precision"])

    def set_precision(self, mode=None):
        """the encoder's arithmetic ("f16x2" default, "fp32"; the RWKV and chunk Conformer encoders have fp32 only, and None leaves them there); the search is
        exact fp32 in both"""
        self.encoder.set_precision(mode)
        return self

    def encode(self, speech: torch.Tensor, speech_lengths, **kwargs):
        """transducer/model.py encode: (encoder_out [B, T, D], lengths). With a unified-mode ChunkConformerEncoder the reference
        unpacks (x_utt, x_chunk, olens) positionally and hands x_chunk on as "lengths", which its inference never reads; here the
        utt branch runs alone and the lengths are the true ones."""
        if not hasattr(self.encoder, "forward_utt"):
            return super().encode(speech, speech_lengths, **kwargs)
        if self.normalize is not None:
            dev = self.encoder._device()
            speech, speech_lengths = self.normalize(speech.to(device=dev, dtype=torch.float32).contiguous(), speech_lengths)
        return self.encoder.forward_utt(speech, speech_lengths)

    def _make_config(self):
        c = _lib.pf_transducer_config()
        c.vocab, c.enc_dim, c.embed_dim, c.hidden = self.vocab_size, self.encoder.output_size(), self.decoder.embed_size, self.decoder.output_size
        c.n_layers, c.joint_dim, c.blank_id = self.decoder.dlayers, self.joint_network.joint_space_size, self.blank_id
        return c

    # ------------------------------------------------------------------------------------------------ search
    def init_beam_search(self, **kwargs):
        """transducer/model.py:455-491: BeamSearchTransducer(decoder, joint_network, beam_size (default 2), nbest=1)"""
        beam = int(kwargs.get("beam_size", 2))
        if beam > MAX_BEAM:
            raise NotImplementedError(f"Transducer(HIP): beam_size: {beam} is not built (at most {MAX_BEAM})")
        if beam < 1 or beam > self.vocab_size:
            raise ValueError(f"beam_size ({beam}) should be smaller than or equal to vocabulary size ({self.vocab_size}).")
        self.beam_size = beam

    def search(self, encoder_out: torch.Tensor, beam_size: int = 2, nbest: int = 1, max_expansions_per_frame: int = None
               ) -> Tuple[List[Tuple[List[int], float]], Dict[str, int]]:
        """encoder_out [T, D] of ONE utterance -> ([(yseq with its leading blank, score)] best first, at most `nbest` of them,
        {"joint_evals", "pred_steps", "max_frame_evals"}). Raises TransducerSearchError on a guard."""
        if int(beam_size) > MAX_BEAM:
            raise NotImplementedError(f"Transducer(HIP): beam_size: {beam_size} is not built (at most {MAX_BEAM})")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        enc = encoder_out.to(device=dev, dtype=torch.float32).contiguous()
        T = int(enc.shape[0])
        max_len = 1 + 8 * T + 64
        nb = max(1, int(nbest))
        ids = (C.c_int32 * (nb * max_len))()
        lens = (C.c_int32 * nb)()
        scores = (C.c_double * nb)()
        n_out = C.c_int32(0)
        stats = (C.c_int64 * 3)()
        cap = 0 if max_expansions_per_frame is None else int(max_expansions_per_frame)
        if max_expansions_per_frame is not None and cap < 1:
            raise ValueError(f"max_expansions_per_frame must be positive, got {max_expansions_per_frame}")
        with torch.cuda.device(dev):
            rc = lib.pf_transducer_search(h, enc.data_ptr(), T, int(beam_size), nb, cap, ids, lens, scores, max_len, C.byref(n_out), stats,
                                          stream_ptr())
        info = {"joint_evals": int(stats[0]), "pred_steps": int(stats[1]), "max_frame_evals": int(stats[2])}
        if rc in (_lib.TRANSDUCER_NONFINITE, _lib.TRANSDUCER_CAP):
            err = TransducerSearchError((lib.pf_transducer_last_error(h) or b"").decode("utf-8", "replace"))
            err.stats = info
            raise err
        _lib.check(rc, "pf_transducer_search")
        out = [([int(v) for v in ids[i * max_len: i * max_len + int(lens[i])]], float(scores[i])) for i in range(int(n_out.value))]
        return out, info

    # ------------------------------------------------------------------------------------------------ inference
    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """transducer/model.py:493-595: one utterance, one search over encoder_out[0]; the reference builds its searcher with nbest=1,
        so there is one record whatever `nbest` is passed"""
        from .tokenizer import sentence_postprocess

        if kwargs.get("batch_size", 1) > 1:
            raise NotImplementedError("batch decoding is not implemented")
        self.init_beam_search(**kwargs)
        self.nbest = kwargs.get("nbest", 1)
        t0 = time.perf_counter()
        speech, lens, meta = self._features(data_in, data_lengths, frontend, kwargs)
        encoder_out, _ = self.encode(speech, lens)
        hyps, _ = self.search(encoder_out[0], beam_size=self.beam_size, nbest=1,
                              max_expansions_per_frame=kwargs.get("max_expansions_per_frame"))
        hyps = hyps[: self.nbest]
        meta.setdefault("decode", f"{time.perf_counter() - t0:0.3f}")
        if key is None:
            key = [f"utt_{i}" for i in range(encoder_out.shape[0])]
        results = []
        for i in range(encoder_out.shape[0]):
            for nbest_idx, (yseq, _score) in enumerate(hyps):
                writer = self._writer(kwargs, f"{nbest_idx + 1}best_recog")
                token_int = [t for t in yseq if t != self.eos and t != self.sos and t != self.blank_id]
                token = tokenizer.ids2tokens(token_int)
                text = tokenizer.tokens2text(token)
                text_postprocessed, _ = sentence_postprocess(token)
                results.append({"key": key[i], "token": token, "text": text, "text_postprocessed": text_postprocessed})
                if writer is not None:
                    writer["token"][key[i]] = " ".join(token)
                    writer["text"][key[i]] = text
                    writer["text_postprocessed"][key[i]] = text_postprocessed
        return results, meta

