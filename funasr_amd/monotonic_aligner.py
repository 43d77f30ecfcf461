"""MonotonicAligner on gfx950: forced alignment (`model: MonotonicAligner`, the zoo's `fa-zh`,
speech_timestamp_prediction-v1-16k-offline): audio and its transcript in, one [begin_ms, end_ms] per token out.

Host-side mirror of funasr/models/monotonic_aligner/model.py: the same constructor arguments, the reference's state-dict names
(`encoder.*`, `predictor.*`) under a strict load, `encode`, `calc_predictor_timestamp` and `inference`. The model is a
`SANMEncoder` (funasr_amd/sanm_encoder.py; the template's 4 heads of d_k = 80 run csrc/attention_mid.hip, fp32 mode only) and the
timestamp head of `CifPredictorV3` (funasr_amd/cif_predictor.py: upsampling GEMM, BLSTM, second alpha head, scale-and-scan) called
with the transcript's token count + 1. `ts_prediction_lfr6_standard` (funasr_amd/timestamps.py) turns the fires into spans and
`sentence_postprocess` merges them with the tokens.

`inference` takes the two-input batches of `AutoModel.generate(input=(wav, text), data_type=("sound", "text"))`: a list of
(sound, text) tuples. All device work of a batch (frontend, encoder, timestamp head) is enqueued before anything is read back,
and the encoder gets the clips' true lengths, so a clip's record does not depend on what it is batched with.
"""
from __future__ import annotations

import copy
import time
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import cif_predictor as _cif_predictor  # noqa: F401  (registers CifPredictorV3)
from . import sanm_encoder as _sanm_encoder  # noqa: F401  (registers SANMEncoder)
from .hip_module import host_i32
from .register import tables
from .timestamps import cif_timestamps
from .tokenizer import sentence_postprocess

# hidden sizes csrc/lstm.hip is instantiated for (launch_lstm)
LSTM_HIDDEN_SIZES = (16, 32, 48, 64, 96, 128, 256, 320, 512)
# heads the SAN-M encoder takes (pf_encoder_create): 128, 80 / 96 (fp32 mode only), multiples of 4 up to 64
FP32_ONLY_HEADS = (80, 96)


def _head_size_ok(d_k: int) -> bool:
    return d_k == 128 or d_k in FP32_ONLY_HEADS or (0 < d_k <= 64 and d_k % 4 == 0)


@tables.register("model_classes", "MonotonicAligner")
class MonotonicAligner(nn.Module):
    def __init__(self, input_size: int = 80, specaug: Optional[str] = None, specaug_conf: Optional[Dict] = None,
                 normalize: str = None, normalize_conf: Optional[Dict] = None, encoder: str = None,
                 encoder_conf: Optional[Dict] = None, predictor: str = None, predictor_conf: Optional[Dict] = None,
                 predictor_bias: int = 0, length_normalized_loss: bool = False, precision: Optional[str] = None, **kwargs):
        super().__init__()
        me = "MonotonicAligner(HIP)"
        encoder_conf, predictor_conf = dict(encoder_conf or {}), dict(predictor_conf or {})
        if encoder != "SANMEncoder":
            raise NotImplementedError(f"{me}: encoder: {encoder} is not built (only SANMEncoder)")
        if predictor != "CifPredictorV3":
            raise NotImplementedError(f"{me}: predictor: {predictor} is not built (only CifPredictorV3, whose timestamp head this model is)")
        if predictor_conf.get("upsample_type", "cnn") == "cnn_attn":
            raise NotImplementedError(f"{me}: upsample_type: cnn_attn is not built (cnn, cnn_blstm; the reference's cnn_attn fails on its own mask)")
        idim = int(predictor_conf.get("idim", 0))
        if predictor_conf.get("upsample_type", "cnn") == "cnn_blstm" and idim not in LSTM_HIDDEN_SIZES:
            raise NotImplementedError(f"{me}: idim: {idim} is not built with upsample_type cnn_blstm (the LSTM kernel is instantiated for "
                                      f"hidden sizes {list(LSTM_HIDDEN_SIZES)})")
        D, H = int(encoder_conf.get("output_size", 256)), int(encoder_conf.get("attention_heads", 4))
        if H < 1 or D % H or not _head_size_ok(D // H):
            raise NotImplementedError(f"{me}: attention_heads: {H} with output_size {D} is not built (a head size of 128, 96, 80, or a "
                                      "multiple of 4 up to 64)")
        if precision not in (None, "fp32") and D // H in FP32_ONLY_HEADS:
            raise NotImplementedError(f"{me}: precision: {precision} is not built for heads of d_k = {D // H} (fp32 only)")
        if idim != D:
            raise NotImplementedError(f"{me}: idim: {idim} differs from the encoder's output_size {D}")
        self.normalize = None
        if normalize is not None:
            from . import normalize as _normalize  # noqa: F401  (registers normalize_classes)
            self.normalize = tables.normalize_classes.get(normalize)(**(normalize_conf or {}))
        self.specaug = None                                           # training-time augmentation: accepted, never applied
        self.encoder = tables.encoder_classes.get(encoder)(input_size=input_size, **encoder_conf)
        self.predictor = tables.predictor_classes.get(predictor)(**predictor_conf)
        self.predictor_bias = predictor_bias
        self.length_normalized_loss = length_normalized_loss
        if precision is not None:
            self.set_precision(precision)

    def set_precision(self, mode=None):
        """"fp32" or None (the encoder's default) at heads of d_k = 80 / 96; the encoder's modes elsewhere"""
        d_k = self.encoder.output_size() // self.encoder.attention_heads
        if mode not in (None, "fp32") and d_k in FP32_ONLY_HEADS:
            raise NotImplementedError(f"MonotonicAligner(HIP): precision: {mode} is not built for heads of d_k = {d_k} (fp32 only)")
        self.encoder.set_precision(mode)
        return self

    def forward(self, *args, **kwargs):
        raise NotImplementedError("MonotonicAligner(HIP): training forward is not built (inference only)")

    def encode(self, speech: torch.Tensor, speech_lengths, **kwargs):
        """(normalisation +) SANMEncoder.forward with the true lengths -> (encoder_out [B, T, D], lengths)"""
        if self.normalize is not None:
            dev = self.encoder._device()
            speech, speech_lengths = self.normalize(speech.to(device=dev, dtype=torch.float32).contiguous(), speech_lengths)
        out, olens, _ = self.encoder(speech, speech_lengths)
        return out, olens

    def calc_predictor_timestamp(self, encoder_out, encoder_out_lens, token_num):
        """-> (None, None, us_alphas [B, U T], us_peaks [B, U T]): the re-downsampled pair of the reference is unused at inference"""
        return self.predictor.get_upsample_timestamp(encoder_out, None, token_num, lengths=encoder_out_lens)

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        from .audio import batch_to_features, load_audio_text

        data_type = kwargs.get("data_type", "sound")
        if not isinstance(data_type, (list, tuple)) or tuple(data_type) != ("sound", "text"):
            raise ValueError('MonotonicAligner.inference: pass input=(sound, text) with data_type=("sound", "text")')
        if frontend is None or tokenizer is None:
            raise ValueError("MonotonicAligner.inference needs the frontend and the tokenizer of the model directory")
        t1 = time.perf_counter()
        audio_list, token_int_list = load_audio_text(data_in, fs=frontend.fs, audio_fs=kwargs.get("fs", 16000), data_type=data_type,
                                                     tokenizer=tokenizer)
        # (an empty transcript returns in the reference -- text "", no spans; tests/golden/aligner.npz `empty_transcript` -- and here:
        #  token_num 1, `cif_timestamps` and `sentence_postprocess` hand back their empty results)
        load_s = time.perf_counter() - t1
        speech, speech_lengths, meta_data = batch_to_features(audio_list, None, frontend, dict(kwargs, data_type="sound"))
        meta_data["load_data"] = f"{load_s:0.3f}"
        lens = host_i32(speech_lengths)[1]

        # ---- device work, all of it enqueued before the first read-back
        encoder_out, encoder_out_lens = self.encode(speech.to(dtype=torch.float32), lens)
        token_num = [len(t) + 1 for t in token_int_list]
        # The BLSTM of the timestamp head runs over every row it is given, and its reverse pass starts at the LAST one: behind a
        # shorter clip of a padded batch that is padding, in the reference as here (`calc_predictor_timestamp` on a padded batch
        # gives the reference's padded-batch result), and what it leaves in the state moves the clip's weights enough to move a fire
        # by a frame. `inference` therefore calls the head once per group of clips of EQUAL length, without padding rows: a clip's
        # record is that of the clip alone (the reference's at its default batch_size 1), whatever it is batched with. Clips of one
        # length -- a corpus cut into fixed windows -- make one group; a ragged batch pays one LSTM chain per distinct length.
        groups: Dict[int, list] = {}
        for i, n in enumerate(lens):
            groups.setdefault(int(n), []).append(i)
        pending = []
        for n, idx in groups.items():
            hid = encoder_out[:, :n] if len(idx) == len(lens) else torch.stack([encoder_out[i, :n] for i in idx])
            _, _, usa, usp = self.calc_predictor_timestamp(hid, [n] * len(idx), [token_num[i] for i in idx])
            pending.append((idx, usa, usp))
        us_alphas, us_peaks = [None] * len(lens), [None] * len(lens)
        for idx, usa, usp in pending:
            usa, usp = usa.cpu(), usp.cpu()
            for j, i in enumerate(idx):
                us_alphas[i], us_peaks[i] = usa[j], usp[j]

        ibest_writer = None
        if kwargs.get("output_dir") is not None:
            if not hasattr(self, "writer"):
                from .datadir_writer import DatadirWriter
                self.writer = DatadirWriter(kwargs.get("output_dir"))
            ibest_writer = self.writer["tp_res"]
        results = []
        for i, token_int in enumerate(token_int_list):
            token = tokenizer.ids2tokens(token_int)
            n = int(lens[i]) * 3            # the reference's literal 3 (model.py:248-249), as in bicif_paraformer.py
            timestamp_str, timestamp = cif_timestamps(us_alphas[i][:n], us_peaks[i][:n], copy.copy(token))
            text, stamps, _ = sentence_postprocess(token, timestamp)
            results.append({"key": key[i], "text": text, "timestamp": stamps})
            if ibest_writer is not None:
                ibest_writer["timestamp_list"][key[i]] = stamps
                ibest_writer["timestamp_str"][key[i]] = timestamp_str
        return results, meta_data
