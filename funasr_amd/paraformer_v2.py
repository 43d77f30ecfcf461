"""Paraformer-v2 on gfx950: the CTC posterior embedder in front of the SAN-M decoder.

Host-side mirrors of `Paraformer_v2_community` and `ParaformerSANMDecoder_v2_community`
(funasr/models/paraformer_v2_community/{model,decoder}.py). The model has no CIF predictor: the decoder input comes from the CTC
head -- frame-wise softmax, greedy path, consecutive equal labels merged, blank runs dropped, the posterior vectors of each
remaining run averaged (model.py:451-482) -- and goes through the decoder's input layer `embed` = Linear(V -> D), LayerNorm(1e-5),
ReLU, PositionalEncoding (decoder.py:318-325, :434). The encoder is the SANMEncoder and everything behind `embed` is the
ParaformerSANMDecoder of this package; the new device stage between them is `pf_posterior_embed_*` (csrc/ctc_merge.hip,
csrc/engine_posterior.hip), which works in the frame domain: Linear(mean_t p_t) = mean_t(p_t W^T) + b.

Unlike the reference's `inference` (model.py:484-590: a Python loop that runs the decoder one clip at a time with `.item()` calls
per run) the stage is batched, the decoder runs once for the whole batch and there is one device->host copy of the token ids.

Two deliberate divergences from the reference:

(a) Ragged batches run, and give for each clip what the reference gives for that clip alone at batch size 1. The reference hands
    `encoder_out[b:b+1]` to the decoder without slicing it to the clip's length, so a batch whose clips differ in length dies in
    the cross-attention mask ("The size of tensor a (31) must match the size of tensor b (40)").
(b) A clip whose CTC path is all blank yields the record {"key", "token_int": [], "text": ""}. The reference appends NO record for
    such a clip (model.py:563-588: the append sits in the else branch), which shifts every later key of the batch.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib
from .audio import batch_to_features
from .conformer import abs_pos_table
from .ctc import CTC
from .hip_module import HipModule, HostCopyRing, StagedUpload, host_i32, layer_norm, linear, stream_ptr
from .paraformer_decoder import ParaformerSANMDecoder
from .register import tables
from .tokenizer import sentence_postprocess

from . import sanm_encoder as _sanm_encoder  # noqa: F401  (registers SANMEncoder)
from . import wav_frontend as _wav_frontend  # noqa: F401


class PosteriorRuns(NamedTuple):
    """what `PosteriorEmbed.runs` found, and what `PosteriorEmbed.embeds` needs to finish the stage"""
    N: int                              # the largest run count of the batch (0: every clip is blank)
    counts: List[int]                   # runs per clip
    path: Optional[torch.Tensor]        # greedy path int32 [B, T] when asked for
    B: int
    T: int
    hidden: torch.Tensor                # the stage's input (kept alive until the embeds are enqueued)


class PosteriorEmbed(HipModule):
    """The decoder's input layer `embed` (keys 0.weight [D, V], 0.bias, 1.weight, 1.bias below `decoder.embed.`) and the handle of
    the device stage that applies it to the CTC posteriors (include/paraformer_hip.h pf_posterior_embed_*)."""
    _prefix = "pf_posterior_embed"

    def __init__(self, vocab_size: int, d_model: int, blank_id: int = 0):
        super().__init__()
        self.vocab_size, self.d_model, self.blank_id = vocab_size, d_model, blank_id
        self.add_module("0", linear(d_model, vocab_size))
        self.add_module("1", layer_norm(d_model))

    def _make_config(self):
        return None

    def _create_args(self):
        return (self.vocab_size, self.d_model, self.blank_id)

    def _push_weights(self, lib):
        with torch.cuda.device(self._handle_device):
            named = [("embed." + n, p) for n, p in self.named_parameters()] + [("pos_table", abs_pos_table(self.d_model))]
            for name, p in named:
                t = p.detach().to(device=self._handle_device, dtype=torch.float32).contiguous()
                _lib.check(lib.pf_posterior_embed_set_tensor(self._handle, name.encode(), t.data_ptr(), t.numel()),
                           f"pf_posterior_embed_set_tensor({name})")
            torch.cuda.synchronize()

    def set_blank_id(self, blank_id: int):
        if blank_id != self.blank_id:
            self.blank_id = blank_id
            self._free()                      # the id is fixed at creation of the handle
        return self

    def reference_forward(self, probs: torch.Tensor) -> torch.Tensor:
        """`embed(probs)` with torch on the tensor's device: merged posteriors [B, N, V] -> [B, N, D] (decoder.py:318-325). The route
        of `forward`, whose input is already merged; the fast route never builds [B, N, V]."""
        w0, b0 = getattr(self, "0").weight, getattr(self, "0").bias
        g, b = getattr(self, "1").weight, getattr(self, "1").bias
        dev = probs.device
        x = torch.nn.functional.linear(probs.float(), w0.to(dev), b0.to(dev))
        x = torch.relu(torch.nn.functional.layer_norm(x, (self.d_model,), g.to(dev), b.to(dev), 1e-5))
        return x * (self.d_model ** 0.5) + abs_pos_table(self.d_model)[: x.shape[1]].to(dev)

    def runs(self, ctc: CTC, hs_pad: torch.Tensor, hlens, mode: str, want_path: bool = False, chunk_rows: int = 0) -> PosteriorRuns:
        """the stage up to its one host wait (the run counts)"""
        lib, h = self._ensure_handle()
        _, hc = ctc._ensure_handle()
        dev = self._handle_device
        _lib.check(lib.pf_posterior_embed_set_precision(h, {"fp32": 0, "f16x2": 3}[mode]), "pf_posterior_embed_set_precision")
        _lib.check(lib.pf_posterior_embed_set_chunk_rows(h, int(chunk_rows)), "pf_posterior_embed_set_chunk_rows")
        x = hs_pad.to(device=dev, dtype=torch.float32).contiguous()
        B, T, _ = x.shape
        lens_c, _ = host_i32(hlens, B)
        counts_c = (C.c_int32 * B)()
        path = torch.empty(B, T, device=dev, dtype=torch.int32) if want_path else None
        with torch.cuda.device(dev):
            n = lib.pf_posterior_embed_runs(h, hc, x.data_ptr(), lens_c, B, T, counts_c, path.data_ptr() if want_path else None, stream_ptr())
        if n < 0:
            _lib.check(n, "pf_posterior_embed_runs")
        return PosteriorRuns(int(n), [int(v) for v in counts_c], path, B, T, x)

    def embeds(self, runs: PosteriorRuns, want_ranges: bool = False):
        """the rest of the stage for the LAST `runs` of this module: (embeds [B, N, D], run ranges int32 [B, N, 2] or None); nothing is
        enqueued for N == 0"""
        lib, h = self._ensure_handle()
        dev = self._handle_device
        emb = torch.empty(runs.B, runs.N, self.d_model, device=dev, dtype=torch.float32)
        ranges = torch.empty(runs.B, runs.N, 2, device=dev, dtype=torch.int32) if want_ranges else None
        with torch.cuda.device(dev):
            _lib.check(lib.pf_posterior_embed_embeds(h, runs.B, runs.T, runs.N, emb.data_ptr(), ranges.data_ptr() if want_ranges else None,
                                                     stream_ptr()), "pf_posterior_embed_embeds")
        return emb, ranges


@tables.register("decoder_classes", "ParaformerSANMDecoder_v2_community")
class ParaformerSANMDecoder_v2_community(ParaformerSANMDecoder):
    """`ParaformerSANMDecoder` whose `forward` applies the input layer: x = embed(tgt) instead of x = tgt (decoder.py:434, the one
    line in which the file differs from paraformer/decoder.py). `embed.{0,1}.{weight,bias}` are real state_dict entries here: they
    live in the `embed` child (a HipModule of its own), which owns the posterior-embedder handle and pushes them there. The parent's
    `_skip_keys = ("embed.",)` is therefore NOT overridden: it keeps these tensors away from the pf_decoder handle, which has no such
    names, while strict loading sees them through the child."""

    def __init__(self, vocab_size: int, encoder_output_size: int, input_layer: str = "embed", wo_input_layer: bool = False,
                 blank_id: int = 0, **kwargs):
        if wo_input_layer or input_layer != "linear":
            raise NotImplementedError(f"ParaformerSANMDecoder_v2_community(HIP): input_layer='linear' is the only input layer built "
                                      f"(got input_layer={input_layer!r}, wo_input_layer={wo_input_layer})")
        super().__init__(vocab_size, encoder_output_size, input_layer="linear", wo_input_layer=False, **kwargs)
        self.embed = PosteriorEmbed(vocab_size, encoder_output_size, blank_id)

    def set_precision(self, mode=None):
        if mode in ("bf16", "bf16x3"):
            raise ValueError("ParaformerSANMDecoder_v2_community: precision must be 'f16x2' or 'fp32'")
        return super().set_precision(mode)

    def _embed_mode(self) -> str:
        return "f16x2" if self._mode() == "f16x2" else "fp32"

    def forward(self, hs_pad, hlens, ys_in_pad, ys_in_lens, chunk_mask=None, return_hidden: bool = False, return_both: bool = False):
        """the reference contract: merged posteriors [B, N, V] in, logits out"""
        dev = self._device()
        x = self.embed.reference_forward(ys_in_pad.to(device=dev, dtype=torch.float32))
        return super().forward(hs_pad, hlens, x, ys_in_lens, chunk_mask=chunk_mask, return_hidden=return_hidden, return_both=return_both)

    def decode_from_ctc(self, ctc: CTC, hs_pad, hlens, want_path: bool = False, want_hidden: bool = False, chunk_rows: int = 0) -> dict:
        """The fast route: posterior embedder (one host wait: the run counts size the decoder) -> pf_decoder_forward with the fused
        arg-max. -> dict(ids int32 [B, N] on the device, None when every clip is blank; counts list; and, None unless asked for / when
        every clip is blank: path [B, T], ranges [B, N, 2], embeds [B, N, D], hidden [B, N, D])"""
        runs = self.embed.runs(ctc, hs_pad, hlens, self._embed_mode(), want_path=want_path, chunk_rows=chunk_rows)
        out = dict(ids=None, counts=runs.counts, path=runs.path, ranges=None, embeds=None, hidden=None)
        if runs.N == 0:
            return out
        out["embeds"], out["ranges"] = self.embed.embeds(runs, want_ranges=want_path)
        _, out["ids"], out["hidden"], _ = self._run(hs_pad, hlens, out["embeds"], runs.counts, want_logits=False, want_ids=True,
                                                    want_hidden=want_hidden)
        return out

    def greedy_from_ctc(self, ctc: CTC, hs_pad, hlens):
        """-> (ids int32 [B, N] on the device or None when every clip is blank, counts list)"""
        out = self.decode_from_ctc(ctc, hs_pad, hlens)
        return out["ids"], out["counts"]


@tables.register("model_classes", "Paraformer_v2_community")
class Paraformer_v2_community(nn.Module):
    def __init__(self, specaug: Optional[str] = None, specaug_conf: Optional[Dict] = None, normalize: str = None,
                 normalize_conf: Optional[Dict] = None, encoder: str = None, encoder_conf: Optional[Dict] = None,
                 decoder: str = None, decoder_conf: Optional[Dict] = None, ctc: str = None, ctc_conf: Optional[Dict] = None,
                 ctc_weight: float = 0.5, input_size: int = 80, vocab_size: int = -1, ignore_id: int = -1, blank_id: int = 0,
                 sos: int = 1, eos: int = 2, lsm_weight: float = 0.0, length_normalized_loss: bool = False,
                 share_embedding: bool = False, use_1st_decoder_loss: bool = False, **kwargs):
        super().__init__()
        if ctc_weight == 0.0 or ctc_weight == 1.0 or decoder is None:
            raise NotImplementedError("Paraformer_v2_community(HIP): ctc_weight 0.0 leaves the model without a CTC head and 1.0 (or no decoder) "
                                      "without a decoder; the reference's inference cannot run either")
        if share_embedding:
            raise NotImplementedError("Paraformer_v2_community(HIP): share_embedding removes the decoder's input layer")
        enc_conf = dict(encoder_conf or {})
        enc_conf.pop("input_size", None)
        self.encoder = tables.encoder_classes.get(encoder)(input_size=input_size, **enc_conf)
        d = self.encoder.output_size()
        dec_conf = dict(decoder_conf or {})
        dec_conf.pop("vocab_size", None)
        dec_conf.pop("encoder_output_size", None)
        self.decoder = tables.decoder_classes.get(decoder)(vocab_size=vocab_size, encoder_output_size=d, **dec_conf)
        if not hasattr(self.decoder, "decode_from_ctc"):
            raise NotImplementedError("Paraformer_v2_community(HIP): the decoder must be ParaformerSANMDecoder_v2_community")
        self.ctc = CTC(odim=vocab_size, encoder_output_size=d, **(ctc_conf or {}))
        self.normalize, self.specaug = None, None                 # specaug: training-time augmentation, accepted and never applied
        if normalize is not None:
            from . import normalize as _normalize  # noqa: F401  (registers normalize_classes)
            self.normalize = tables.normalize_classes.get(normalize)(**(normalize_conf or {}))
        self.blank_id, self.vocab_size, self.ignore_id, self.ctc_weight = blank_id, vocab_size, ignore_id, float(ctc_weight)
        self.sos = sos if sos is not None else vocab_size - 1
        self.eos = eos if eos is not None else vocab_size - 1
        self.decoder.embed.set_blank_id(blank_id)
        if kwargs.get("precision"):                              # model_conf: {precision: f16x2 | fp32}
            self.set_precision(kwargs["precision"])

    def set_precision(self, mode=None):
        """"f16x2" (the default where the shape rules of SANMEncoder / ParaformerSANMDecoder / CTC allow: fp32-class results from
        two-plane fp16 operands) or "fp32" (exact-fp32 MFMA everywhere). None restores the default."""
        if mode is not None and mode not in ("f16x2", "fp32"):
            raise ValueError("Paraformer_v2_community: precision must be 'f16x2' or 'fp32' (the bf16 modes are not built for this model)")
        self.encoder.set_precision(mode)
        self.decoder.set_precision(mode)
        self.ctc.set_precision(mode)
        return self

    def encode(self, speech: torch.Tensor, speech_lengths, **kwargs):
        """model.py:250-277. The CTC head and the cross-attention read a clip's valid rows only, so in the f16x2 mode only those are
        computed (`all_rows` keeps every row)."""
        if hasattr(self.encoder, "set_row_packing"):
            self.encoder.set_row_packing(self.encoder.ALL_ROWS if kwargs.get("all_rows") else 0)
        if self.normalize is not None:
            dev = self.encoder._device()
            speech, speech_lengths = self.normalize(speech.to(device=dev, dtype=torch.float32).contiguous(), speech_lengths)
        out, olens, _ = self.encoder(speech, speech_lengths)
        return out, olens

    def enqueue_features(self, speech: torch.Tensor, speech_lengths, return_intermediate: bool = False) -> dict:
        """[B, T, 560] features -> encoder, posterior embedder, decoder with the fused arg-max and the ids' D2H copy, all ENQUEUED on
        the current HIP stream; the one host wait inside is for the run counts. `collect()` brings the ids to the host."""
        enc, olens = self.encode(speech, speech_lengths, all_rows=return_intermediate)
        out = self.decoder.decode_from_ctc(self.ctc, enc, olens, want_path=return_intermediate, want_hidden=return_intermediate)
        ids = out["ids"]
        pending = dict(tok=out["counts"], ids=ids, B=enc.shape[0])
        if ids is not None:
            pending["ids_host"] = self.__dict__.setdefault("_host_ring", HostCopyRing()).start(ids)
        if return_intermediate:
            pending["extra"] = dict(path=out["path"], ranges=out["ranges"], embeds=out["embeds"], hidden=out["hidden"], enc=enc, olens=olens)
        return pending

    def collect(self, pending: dict) -> dict:
        tok, B = pending["tok"], pending["B"]
        raw: List[List[int]] = [[] for _ in range(B)]
        if pending["ids"] is not None:
            ids_host = HostCopyRing.wait(pending["ids_host"])
            raw = [ids_host[b, : tok[b]].tolist() for b in range(B)]
        drop = (self.eos, self.sos, self.blank_id)                # model.py:581-585
        out = dict(token_num=tok, raw_ids=raw, ids=[[t for t in r if t not in drop] for r in raw])
        out.update(pending.get("extra", {}))
        return out

    def recognize_features(self, speech: torch.Tensor, speech_lengths, return_intermediate: bool = False) -> dict:
        return self.collect(self.enqueue_features(speech, speech_lengths, return_intermediate))

    def __getstate__(self):
        st = dict(self.__dict__)
        for k in ("_host_ring", "_upload"):
            st.pop(k, None)
        return st

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """model.py:484-590 -> (results, meta_data): one record {"key", "token_int"} per clip (+ "text" with a tokenizer)"""
        speech, speech_lengths, meta_data = batch_to_features(data_in, data_lengths, frontend, kwargs,
                                                              uploader=self.__dict__.setdefault("_upload", StagedUpload()))
        res = self.recognize_features(speech, speech_lengths)
        B = len(res["ids"])
        if key is None:
            key = [f"utt_{i}" for i in range(B)]
        if isinstance(key[0], (list, tuple)):                    # model.py:550-553
            key = key[0]
        if len(key) < B:
            key = list(key) * B
        results = []
        for i in range(B):
            token_int = res["ids"][i]
            rec = {"key": key[i], "token_int": token_int}
            if tokenizer is not None:
                text = ""
                if token_int:
                    token = tokenizer.ids2tokens(token_int)
                    text = tokenizer.tokens2text(token)
                    if not hasattr(tokenizer, "bpemodel"):
                        text, _ = sentence_postprocess(token)
                rec["text"] = text
            results.append(rec)
        return results, meta_data

    def forward(self, *args, **kwargs):  # pragma: no cover
        raise NotImplementedError("training forward() is out of scope; use inference()/recognize_features()")
