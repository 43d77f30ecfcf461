"""UniASR two-pass ASR on gfx950 (`model: UniASR`; funasr/models/uniasr/model.py), offline inference in its three modes.

  * `ChunkLayout`: the chunk geometry of `overlap_chunk` (funasr/models/scama/chunk_utilis.py) for one (length, ind) as index maps and
    0 / 1 vectors on the host -- split_chunk and remove_chunk are row gathers, the three masks are periodic in the chunk -- plus
    `frame_alignments` (CifPredictorV2.gen_frame_alignments) and `scama_mask` (build_scama_mask_for_cross_attention_decoder).
  * `chunked_forward`: `SANMEncoderChunkOpt.forward(xs, lens, ind=)` (scama/encoder.py:393-478): features and positional rows gathered
    into the chunked layout, then the SAN-M blocks with the chunk masks worked out from the geometry on the device
    (`pf_encoder_set_chunk_mask`, csrc/uniasr.hip). Exact fp32.
  * `StrideConv`: `Conv1dSubsampling` over [features | pass-1 output], read from its two sources (`pf_uniasr_stride_conv`).
  * `FsmnDecoderSCAMAOpt` (decoder_classes): the SAN-M stepper whose step takes the memory mask row of its position (`pf_scamadecoder`).
  * `UniASR` (model_classes): decoding_model "fast" (ind 0, pass 1), "normal" (ind 0, pass 2), "offline" (ind 1, pass 2); the search is
    `BeamSearchScama` (uniasr/beam_search.py), which is funasr_amd.transformer_search.BeamSearchTransformer over the decoder and the
    length bonus with the predictor's token count as the length bound (UniASR never builds a CTC head: model.py:186-187).
"""
from __future__ import annotations

import time
from typing import List

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import cif_predictor as _cif_predictor  # noqa: F401  (registers CifPredictorV2)
from . import paraformer_streaming as _paraformer_streaming  # noqa: F401  (registers SANMEncoderChunkOpt)
from .hip_module import ParamHolder, _truthy, stream_ptr
from .register import tables
from .sanm import FsmnDecoder


def _per_ind(x, n: int) -> List[int]:
    """overlap_chunk.check_chunk_size_args: a shorter list repeats its first entry"""
    x = [int(v) for v in (x if isinstance(x, (list, tuple)) else [x])]
    return x if len(x) >= n else [x[0]] * n


class ChunkLayout:
    """overlap_chunk.gen_chunk_mask for ONE sequence of T frames: chunk c holds `shift` FSMN shift rows, then `chunk` rows for the
    frames c stride - pad_left .. c stride - pad_left + chunk - 1 (zero rows outside 0 .. T - 1); the last chunk ends with frame T - 1."""

    def __init__(self, T: int, chunk: int, stride: int, pad_left: int, shift: int, enc_look_back: int, dec_look_back: int):
        if not (T >= 1 and 1 <= stride <= chunk and pad_left >= 0 and chunk - stride - pad_left >= 0 and shift >= 0):
            raise ValueError(f"chunk geometry: chunk_size {chunk}, stride {stride}, pad_left {pad_left} need 1 <= stride and "
                             "stride + pad_left <= chunk_size")
        self.T, self.chunk, self.stride, self.pad_left, self.shift = int(T), int(chunk), int(stride), int(pad_left), int(shift)
        self.enc_look_back, self.dec_look_back = int(enc_look_back), int(dec_look_back)
        self.period = self.chunk + self.shift
        self.n_chunks = -(-self.T // self.stride)
        self.Tc = (self.n_chunks - 1) * self.period + self.shift + self.pad_left + self.T - (self.n_chunks - 1) * self.stride
        r = np.arange(self.Tc)
        c, i = r // self.period, r % self.period - self.shift
        src = c * self.stride + i - self.pad_left
        self.add_index = np.where((i >= 0) & (src >= 0) & (src < self.T), src, -1).astype(np.int32)       # x_add_mask as a gather
        t = np.arange(self.T)
        self.rm_index = ((t // self.stride) * self.period + self.shift + self.pad_left + t % self.stride).astype(np.int32)   # x_rm_mask
        self.mask_shift = (i >= 0).astype(np.float32)                                                      # mask_shfit_chunk
        self.mask_predictor = ((i >= self.pad_left) & (i < self.pad_left + self.stride)).astype(np.float32)  # mask_chunk_predictor

    def att_visible(self, r: int, k: int) -> bool:
        """mask_att_chunk_encoder[r, k] -- the rule csrc/uniasr.hip evaluates per key"""
        c, j = r // self.period, r % self.period - self.shift
        if j < 0 or k >= self.Tc:
            return False
        own = c * self.period + self.shift
        if own <= k < own + self.chunk:
            return True
        if j >= self.stride or k >= own:
            return False
        ck, jk = k // self.period, k % self.period - self.shift
        return ck >= max(c - self.enc_look_back, 0) and 0 <= jk < self.stride

    def att_mask(self) -> np.ndarray:
        return np.asarray([[self.att_visible(r, k) for k in range(self.Tc)] for r in range(self.Tc)], np.float32)

    def frame_alignments(self, alphas: torch.Tensor) -> np.ndarray:
        """CifPredictorV2.gen_frame_alignments (paraformer/cif_predictor.py:448-509) for one sequence in eval mode: alphas [Tc] ->
        how many tokens fire at each row. Token i (1-based) fires at row #(floor(cumsum) < i), clamped to the last row."""
        a = alphas.detach().to("cpu", torch.float32).reshape(-1)
        n_tok = int(torch.floor(a.sum()))
        cum = torch.floor(torch.cumsum(a, 0)).to(torch.int32).numpy()
        out = np.zeros(a.numel(), np.int32)
        for i in range(1, n_tok + 1):
            pos = min(int((cum // i == 0).sum()) + 1, self.Tc)
            if pos - 1 < out.shape[0]:
                out[pos - 1] += 1
        return out

    def scama_mask(self, alignments: np.ndarray) -> np.ndarray:
        """build_scama_mask_for_cross_attention_decoder (chunk_utilis.py:482-624) as UniASR.calc_predictor_mask calls it (chunk_size 1,
        encoder_chunk_size = attention_chunk_size = chunk + shift, eval mode) -> [N, Tc]: token i sees the chunk that fired it whole,
        of the `dec_look_back` chunks before it the predictor's frames, and no shift row."""
        L, P = self.Tc, self.period
        al = np.asarray(alignments, np.int64)
        N = int(al.sum())
        cum = np.cumsum(al)
        cols = np.arange(L)
        mask = np.zeros((N, L), np.float32)
        for i in range(1, N + 1):
            cnt = min(max(int((cum // i == 0).sum()) + 1, 1), L)
            e = min(max(cnt - 1, 0), L)
            end = (e // P + 1) * P
            beg1, beg2 = max(end - P, 0), max(end - P * (self.dec_look_back + 1), 0)
            own = (cols >= beg1) & (cols < end)
            back = (cols + P < end) & (self.mask_predictor > 0)      # (the reference's `t > chunk_size` holds: chunk_size is 1)
            mask[i - 1] = ((own | back) & (cols >= beg2) & (self.mask_shift > 0)).astype(np.float32)
        return mask


def chunk_layout(encoder, T: int, ind: int) -> ChunkLayout:
    n = len(_per_ind(encoder.chunk_size, 1))
    ind = int(ind)
    if not 0 <= ind < n:
        raise ValueError(f"ind {ind}: the encoder holds {n} chunk geometries")
    pick = lambda x: _per_ind(x, n)[ind]                               # noqa: E731
    return ChunkLayout(T, pick(encoder.chunk_size), pick(encoder.stride), pick(encoder.pad_left), (encoder.kernel_size - 1) // 2,
                       pick(encoder.encoder_att_look_back_factor), pick(encoder.decoder_att_look_back_factor))


def gather_rows(src: torch.Tensor, index: np.ndarray) -> torch.Tensor:
    """out[r] = src[index[r]], a zero row where index[r] < 0 (device gather, csrc/uniasr.hip); src [n, D] on the device"""
    src = src.contiguous()
    dev = src.device
    idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
    out = torch.empty(idx.numel(), src.shape[1], device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pf_uniasr_gather_rows(src.data_ptr(), src.shape[1], src.shape[0], idx.data_ptr(), out.data_ptr(), idx.numel(),
                                                     src.shape[1], stream_ptr()), "pf_uniasr_gather_rows")
    return out


def chunked_forward(encoder, xs_pad: torch.Tensor, ilens, ind: int):
    """SANMEncoderChunkOpt.forward(xs_pad, ilens, ind=ind) for ONE sequence -> (out [1, Tc, D], [Tc], layout)"""
    if xs_pad.dim() != 3 or xs_pad.shape[0] != 1:
        raise NotImplementedError("SANMEncoderChunkOpt(HIP): the chunked forward takes one sequence ([1, T, input_size])")
    if encoder._mode() != "fp32":
        raise NotImplementedError(f"SANMEncoderChunkOpt(HIP): the chunked forward runs in the fp32 mode, not {encoder._mode()!r}")
    T = int(ilens[0]) if not isinstance(ilens, int) else int(ilens)
    lay = chunk_layout(encoder, T, ind)
    lib, h = encoder._ensure_handle()
    dev = encoder._handle_device
    x = xs_pad[0, :T].to(device=dev, dtype=torch.float32)
    # the reference adds the positional rows BEFORE it splits: row r carries the position of its source frame, a zero row stays zero
    xc = gather_rows(x, lay.add_index)
    pe = gather_rows(encoder._pe_table(T, dev)[:T], lay.add_index)
    out = torch.empty(1, lay.Tc, encoder.output_size(), device=dev, dtype=torch.float32)
    encoder._apply_settings(lib, h)
    lens_c = (_lib.C.c_int32 * 1)(lay.Tc)
    with torch.cuda.device(dev):
        _lib.check(lib.pf_encoder_set_chunk_mask(h, lay.chunk, lay.stride, lay.shift, lay.enc_look_back), "pf_encoder_set_chunk_mask")
        try:
            _lib.check(lib.pf_encoder_forward(h, xc.data_ptr(), lens_c, 1, lay.Tc, pe.data_ptr(), out.data_ptr(), -1, stream_ptr()),
                       "pf_encoder_forward")
        finally:
            _lib.check(lib.pf_encoder_set_chunk_mask(h, 0, 0, 0, 0), "pf_encoder_set_chunk_mask")
    return out, [lay.Tc], lay


class StrideConv(nn.Module):
    """Conv1dSubsampling (transformer/utils/subsampling.py:332-388): pad, conv1d(kernel_size, stride), ReLU; state_dict keys conv.*"""

    def __init__(self, idim: int, odim: int, kernel_size: int, stride: int, pad, **kwargs):
        super().__init__()
        pad = [int(v) for v in pad] if isinstance(pad, (list, tuple)) else [int(pad), int(pad)]
        if len(pad) != 2 or min(pad) < 0:
            raise NotImplementedError(f"UniASR(HIP): stride_conv_conf pad: {pad} is not built (an int or a (left, right) pair, not negative)")
        if not 1 <= int(kernel_size) <= 8 or int(stride) < 1:
            raise NotImplementedError(f"UniASR(HIP): stride_conv_conf kernel_size: {kernel_size} / stride: {stride} is not built (1 .. 8 taps)")
        if int(kernel_size) * int(idim) * 4 > 48 * 1024:
            raise NotImplementedError(f"UniASR(HIP): stride_conv_conf kernel_size: {kernel_size} over {idim} features is not built "
                                      "(kernel_size * features floats within 48 KiB)")
        self.idim, self.odim, self.kernel_size, self.stride, self.pad = int(idim), int(odim), int(kernel_size), int(stride), pad
        self.conv = ParamHolder((self.odim, self.idim, self.kernel_size), (self.odim,))

    def output_size(self) -> int:
        return self.odim

    def out_len(self, T: int) -> int:
        """the length the reference reports, (T - 1) // stride + 1 -- the rows the second encoder keeps"""
        return (T - 1) // self.stride + 1

    def forward(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a [T, Da], b [T, Db] on the device (Da + Db == idim) -> [out_len(T), odim]"""
        dev = self.conv.weight.device
        if dev.type != "cuda":
            raise RuntimeError("UniASR.stride_conv runs only on an AMD GPU through libparaformer_hip.so (no CPU fallback by design)")
        a, b = a.to(dev, torch.float32).contiguous(), b.to(dev, torch.float32).contiguous()
        T = a.shape[0]
        if a.shape[1] + b.shape[1] != self.idim or b.shape[0] != T:
            raise ValueError(f"stride_conv: {a.shape[1]} + {b.shape[1]} features over {T} / {b.shape[0]} rows; expected {self.idim} in all")
        Tout, full = self.out_len(T), (T + sum(self.pad) - self.kernel_size) // self.stride + 1
        if Tout > full:
            raise ValueError(f"stride_conv: {T} frames with pad {self.pad} yield {full} rows but the length rule keeps {Tout} "
                             "(the reference fails on this geometry too)")
        w, bias = self.conv.weight.detach().contiguous(), self.conv.bias.detach().contiguous()
        out = torch.empty(Tout, self.odim, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pf_uniasr_stride_conv(a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1], T, w.data_ptr(), bias.data_ptr(),
                                                         self.odim, self.kernel_size, self.stride, self.pad[0], self.pad[1], out.data_ptr(),
                                                         Tout, stream_ptr()), "pf_uniasr_stride_conv")
        return out


@tables.register("decoder_classes", "FsmnDecoderSCAMAOpt")
class FsmnDecoderSCAMAOpt(FsmnDecoder):
    """funasr/models/scama/decoder.py FsmnDecoderSCAMAOpt without `concat_embeds`: FsmnDecoder's parameters and step, with the memory
    mask of the position in every `decoders` cross-attention. `set_memory(memory, mask)`: mask [N, T] 0 / 1 rows (None: no mask);
    the step at position i takes row min(i, N - 1) (uniasr/beam_search.py:391-394); N == 0: nothing is visible."""
    _prefix = "pf_scamadecoder"

    def __init__(self, *args, **kwargs):
        try:
            super().__init__(*args, **kwargs)
        except NotImplementedError as e:
            raise NotImplementedError(str(e).replace("FsmnDecoder(HIP)", "FsmnDecoderSCAMAOpt(HIP)")) from None
        self._mask = self._windows = None

    def set_memory(self, memory: torch.Tensor, mask=None):
        super().set_memory(memory)
        T = int(self._memory.shape[0])
        if mask is None:
            self._mask, self._windows = None, None
            return self
        m = np.ascontiguousarray(np.asarray(mask, np.float32).reshape(-1, T))
        self._windows = []
        for row in m:
            nz = np.flatnonzero(row)
            self._windows.append((int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0))
        self._mask = torch.from_numpy(m).to(self._handle_device) if m.shape[0] else torch.zeros(1, T, device=self._handle_device)
        return self

    def step(self, tokens: List[int], pos: int) -> torch.Tensor:
        self._ensure_handle()
        n = len(tokens)
        out = torch.empty(n, self.vocab_size, device=self._handle_device)
        ids = (_lib.C.c_int32 * n)(*[int(t) for t in tokens])
        if self._mask is None:
            self._call("step", ids, int(pos), n, None, 0, int(self._memory.shape[0]), out.data_ptr())
        else:
            row = min(int(pos), len(self._windows) - 1)
            lo, hi = self._windows[row] if row >= 0 else (0, 0)
            self._call("step", ids, int(pos), n, self._mask[max(row, 0)].data_ptr(), lo, hi, out.data_ptr())
        return out


@tables.register("model_classes", "UniASR")
class UniASR(nn.Module):
    """funasr/models/uniasr/model.py UniASR: inference"""
    _PRECISIONS = ("f16x2", "fp32")

    def __init__(self, specaug: str = None, specaug_conf: dict = None, normalize: str = None, normalize_conf: dict = None, encoder: str = None,
                 encoder_conf: dict = None, encoder2: str = None, encoder2_conf: dict = None, decoder: str = None, decoder_conf: dict = None,
                 decoder2: str = None, decoder2_conf: dict = None, predictor: str = None, predictor_conf: dict = None, predictor_bias: int = 0,
                 predictor_weight: float = 0.0, predictor2: str = None, predictor2_conf: dict = None, predictor2_bias: int = 0,
                 predictor2_weight: float = 0.0, ctc: str = None, ctc_conf: dict = None, ctc_weight: float = 0.5, ctc2: str = None,
                 ctc2_conf: dict = None, ctc2_weight: float = 0.5, decoder_attention_chunk_type: str = "chunk",
                 decoder_attention_chunk_type2: str = "chunk", stride_conv=None, stride_conv_conf: dict = None, loss_weight_model1: float = 0.5,
                 input_size: int = 80, vocab_size: int = -1, ignore_id: int = -1, blank_id: int = 0, sos: int = 1, eos: int = 2,
                 lsm_weight: float = 0.0, length_normalized_loss: bool = False, share_embedding: bool = False, **kwargs):
        super().__init__()
        refusals = [
            (encoder != "SANMEncoderChunkOpt", f"encoder: {encoder} (only SANMEncoderChunkOpt)"),
            (encoder2 != "SANMEncoderChunkOpt", f"encoder2: {encoder2} (only SANMEncoderChunkOpt)"),
            (decoder != "FsmnDecoderSCAMAOpt", f"decoder: {decoder} (only FsmnDecoderSCAMAOpt)"),
            (decoder2 != "FsmnDecoderSCAMAOpt", f"decoder2: {decoder2} (only FsmnDecoderSCAMAOpt)"),
            (predictor != "CifPredictorV2", f"predictor: {predictor} (only CifPredictorV2)"),
            (predictor2 != "CifPredictorV2", f"predictor2: {predictor2} (only CifPredictorV2)"),
            (decoder_attention_chunk_type != "chunk", f"decoder_attention_chunk_type: {decoder_attention_chunk_type} (only chunk)"),
            (decoder_attention_chunk_type2 != "chunk", f"decoder_attention_chunk_type2: {decoder_attention_chunk_type2} (only chunk)"),
            (stride_conv_conf is None, "stride_conv_conf: null (the reference needs it too)"),
            (_truthy(share_embedding), "share_embedding: true"),
        ]
        for which, conf in (("predictor_conf", predictor_conf), ("predictor2_conf", predictor2_conf)):
            # the reference's gen_frame_alignments multiplies the [1, T + 1] alignments of a tail frame with a [1, T] mask and fails
            refusals.append((float((conf or {}).get("tail_threshold", 0.0)) > 0.0,
                             f"{which} tail_threshold: {(conf or {}).get('tail_threshold')} (the reference's frame alignments fail on the tail frame)"))
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"UniASR(HIP): {why} is not built")
        enc_cls, dec_cls, pre_cls = tables.encoder_classes[encoder], tables.decoder_classes[decoder], tables.predictor_classes[predictor]

        def _enc(conf, size, which):
            conf = dict(conf or {})
            conf.pop("input_size", None)
            if conf.get("input_layer", "conv2d") != "pe":
                raise NotImplementedError(f"UniASR(HIP): {which} input_layer: {conf.get('input_layer', 'conv2d')} is not built (only pe)")
            return enc_cls(input_size=size, **conf)

        def _dec(conf, d):
            conf = dict(conf or {})
            conf.pop("vocab_size", None)
            conf.pop("encoder_output_size", None)
            return dec_cls(vocab_size=vocab_size, encoder_output_size=d, **conf)

        self.encoder = _enc(encoder_conf, input_size, "encoder_conf")
        d1 = self.encoder.output_size()
        self.decoder = _dec(decoder_conf, d1)
        self.predictor = pre_cls(**(predictor_conf or {}))
        self.stride_conv = StrideConv(idim=input_size + d1, odim=input_size + d1, **dict(stride_conv_conf))
        self.encoder2 = _enc(encoder2_conf, self.stride_conv.output_size(), "encoder2_conf")
        self.decoder2 = _dec(decoder2_conf, self.encoder2.output_size())
        self.predictor2 = pre_cls(**(predictor2_conf or {}))
        self.normalize = None
        if normalize is not None:
            from . import normalize as _normalize  # noqa: F401  (registers normalize_classes)
            self.normalize = tables.normalize_classes.get(normalize)(**(normalize_conf or {}))
        self.specaug = None                                           # training-time augmentation: accepted, never applied
        self.ctc = self.ctc2 = None                                   # model.py:186-187: never built, whatever ctc_weight says
        self.blank_id, self.sos, self.eos, self.vocab_size, self.ignore_id = blank_id, sos, eos, vocab_size, ignore_id
        self.ctc_weight, self.ctc2_weight = float(ctc_weight), float(ctc2_weight)
        self.beam_search, self.nbest = None, 1
        self.set_precision(kwargs.get("precision") or None)

    def set_precision(self, mode=None):
        """"fp32": exact fp32 everywhere. The chunk-masked attention exists in exact fp32 only, so that is also what None means;
        "f16x2" is refused by name (the rule of funasr_amd.sanm.SANM: a mode is refused where its kernels do not exist)."""
        if mode is not None and mode not in self._PRECISIONS:
            raise NotImplementedError(f"UniASR(HIP): precision {mode!r}: built are {sorted(self._PRECISIONS)}")
        if mode == "f16x2":
            raise NotImplementedError("UniASR(HIP): precision 'f16x2' is not built for the chunk-masked encoder (its attention and FSMN "
                                      "kernels are exact fp32); use 'fp32' or None")
        self.encoder.set_precision("fp32")
        self.encoder2.set_precision("fp32")
        return self

    # ------------------------------------------------------------------------------------------------ stages
    def encode(self, speech: torch.Tensor, speech_lengths, ind: int = 0):
        """model.py:381-409 -> (normalised features [1, T, F], pass-1 output [1, Tc, D1], [Tc])"""
        dev = self.encoder._device()
        speech = speech.to(device=dev, dtype=torch.float32).contiguous()
        if self.normalize is not None:
            speech, speech_lengths = self.normalize(speech, speech_lengths)
        lens = [int(v) for v in (speech_lengths.tolist() if isinstance(speech_lengths, torch.Tensor) else speech_lengths)]
        out, olens, lay = chunked_forward(self.encoder, speech, lens, ind)
        self._layout1 = lay
        return speech[:, : lens[0]], out, olens

    def encode2(self, encoder_out: torch.Tensor, speech: torch.Tensor, ind: int = 0):
        """model.py:411-447: remove_chunk, [features | pass-1 output] through stride_conv, the second chunked encoder"""
        rm = gather_rows(encoder_out[0], self._layout1.rm_index)
        self._stride_out = x2 = self.stride_conv(speech[0], rm)
        out, olens, lay = chunked_forward(self.encoder2, x2[None], [x2.shape[0]], ind)
        self._layout2 = lay
        return out, olens

    def calc_predictor_mask(self, encoder_out: torch.Tensor, lay: ChunkLayout, predictor):
        """model.py:787-965 for one sequence -> (alphas [Tc] on the host, token count as the reference sums it, alignments, scama mask)"""
        masked = gather_rows(encoder_out[0], np.where(lay.mask_shift > 0, np.arange(lay.Tc), -1))
        _, _, alphas, _ = predictor(masked[None], None, None, lengths=[lay.Tc])
        alphas = alphas[0, : lay.Tc].to("cpu", torch.float32) * torch.from_numpy(lay.mask_predictor)
        token_num = float(alphas.sum())
        align = lay.frame_alignments(alphas)
        return alphas, token_num, align, lay.scama_mask(align)

    def init_beam_search(self, **kwargs):
        """model.py:967-1020"""
        from .transformer_search import BeamSearchTransformer

        for k in ("lm_weight", "ngram_weight"):
            if float(kwargs.get(k, 0.0) or 0.0) != 0.0:
                raise NotImplementedError(f"UniASR(HIP): {k} is not built (the reference builds no such scorer either)")
        token_list = kwargs.get("token_list")
        n_vocab = len(token_list) if token_list is not None else self.vocab_size
        self.beam_search = BeamSearchTransformer(beam_size=kwargs.get("beam_size", 5), vocab_size=n_vocab, sos=self.sos, eos=self.eos,
                                                 ctc_weight=0.0, length_bonus_weight=kwargs.get("penalty", 0.0), blank=0, pre_beam=False)
        self.beam_search.w_dec = 1.0 - float(kwargs.get("decoding_ctc_weight", 0.0))     # kept even without a CTC scorer

    @staticmethod
    def decoding(decoding_model: str):
        """-> (ind, which pass decodes) (model.py:1042-1052: anything but fast / offline is normal)"""
        return {"fast": (0, 1), "offline": (1, 2)}.get(decoding_model, (0, 2))

    def recognize(self, speech: torch.Tensor, speech_lengths, decoding_model: str = "normal", token_num_relax: int = 5):
        """features of one utterance -> n-best hypotheses (transformer_search.Hypothesis), best first"""
        ind, which = self.decoding(decoding_model)
        raw, out, _ = self.encode(speech, speech_lengths, ind=ind)
        if which == 1:
            lay, decoder, predictor = self._layout1, self.decoder, self.predictor
        else:
            out, _ = self.encode2(out, raw, ind=ind)
            lay, decoder, predictor = self._layout2, self.decoder2, self.predictor2
        alphas, token_num, align, mask = self.calc_predictor_mask(out, lay, predictor)
        self._stages = dict(encoder_out=out, alphas=alphas, token_num=token_num, alignments=align, scama_mask=mask)
        maxlen = int(token_num + token_num_relax)
        if maxlen < 1:
            return []
        decoder.set_memory(out[0], mask)
        return self.beam_search(decoder, maxlen, None, 0.0, 0.0)

    def _features(self, data_in, data_lengths, frontend, kwargs):
        from .audio import batch_to_features

        speech, speech_lengths, meta = batch_to_features(data_in, data_lengths, frontend, kwargs)
        lens = [int(v) for v in (speech_lengths.tolist() if isinstance(speech_lengths, torch.Tensor) else
                                 ([speech_lengths] if isinstance(speech_lengths, int) else speech_lengths))]
        return speech.to(dtype=torch.float32), lens, meta

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """model.py:1022-1143"""
        from .tokenizer import sentence_postprocess

        if kwargs.get("batch_size", 1) > 1:
            raise NotImplementedError("UniASR(HIP): batch_size > 1 is not built (the reference decodes encoder_out[0] only)")
        if self.beam_search is None:
            if kwargs.get("token_list") is None and tokenizer is not None and getattr(tokenizer, "token_list", None) is not None:
                kwargs = dict(kwargs, token_list=tokenizer.token_list)
            self.init_beam_search(**kwargs)
            self.nbest = kwargs.get("nbest", 1)
        t0 = time.perf_counter()
        speech, lens, meta = self._features(data_in, data_lengths, frontend, kwargs)
        if speech.shape[0] != 1:
            raise NotImplementedError("UniASR(HIP): one utterance per call (the reference decodes encoder_out[0] only)")
        nbest = self.recognize(speech, lens, kwargs.get("decoding_model", "normal"), kwargs.get("token_num_relax", 5))[: self.nbest]
        meta.setdefault("decode", f"{time.perf_counter() - t0:0.3f}")
        if key is None:
            key = ["utt_0"]
        results = []
        for hyp in nbest:
            token_int = [t for t in hyp.yseq[1:-1] if t != 0]
            token = tokenizer.ids2tokens(token_int)
            text = tokenizer.tokens2text(token)
            if not hasattr(tokenizer, "bpemodel"):
                text, _ = sentence_postprocess(token)
            results.append({"key": key[0], "text": text})
        return results, meta
