"""CAM++ speaker embedding on gfx950 (funasr/models/campplus/model.py, components.py).

`CAMPPlus` is registered as model_classes/"CAMPPlus". It holds the reference's parameters AND BatchNorm buffers under the
reference's state_dict keys (937 of them, `num_batches_tracked` included), so `load_pretrained_model(strict=True)` loads a
published `campplus_cn_common.bin`; all arithmetic runs in csrc/campplus.hip through the `pf_campplus` handle:
  * `forward(x [B, T, 80]) -> [B, 192]`: the reference's forward on ready features (extract_feature's mean-normalised fbank);
  * `embed_chunks(wav, starts, chunk_len, valid=None)`: chunks of a waveform already in GPU memory straight to embeddings
    (gather, kaldi fbank with the CAM++ options, mean removal, network) in one library call -- the diarization path;
  * `inference(data_in, ...)`: the reference's contract -> ([{"spk_embedding": [B, 192]}], meta).
The model directory's `frontend: WavFrontend` is NOT applied: CAM++ uses its own fbank (campplus/utils.py:119-137: 80 bins,
povey window, no 2^15 scaling, dither 0), computed by the library's fbank kernel.
"""
from __future__ import annotations

import time
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .hip_module import Holder, HipModule, ParamHolder, stream_ptr
from .register import tables

LAYERS = (12, 24, 16)
SAMPLE_RATE = 16000


class _BN(torch.nn.Module):
    """BatchNorm parameter / buffer holder with torch's names (weight, bias, running_mean, running_var, num_batches_tracked)."""

    def __init__(self, c: int, affine: bool = True):
        super().__init__()
        if affine:
            self.weight = torch.nn.Parameter(torch.ones(c), requires_grad=False)
            self.bias = torch.nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: computation happens inside libparaformer_hip.so")


def _nonlinear(c: int, affine: bool = True) -> Holder:
    h = Holder()
    h.batchnorm = _BN(c, affine)
    return h


def _conv(*shape) -> ParamHolder:
    return ParamHolder(shape)


def _res_block(cin: int, c: int, stride: int) -> Holder:
    b = Holder()
    b.conv1 = _conv(c, cin, 3, 3)
    b.bn1 = _BN(c)
    b.conv2 = _conv(c, c, 3, 3)
    b.bn2 = _BN(c)
    if stride != 1 or cin != c:
        b.shortcut = torch.nn.Sequential(_conv(c, cin, 1, 1), _BN(c))
    return b


@tables.register("model_classes", "CAMPPlus")
class CAMPPlus(HipModule):
    _prefix = "pf_campplus"
    _push_buffers = True      # BatchNorm running statistics: the library folds them into the convs

    def __init__(self, feat_dim: int = 80, embedding_size: int = 192, growth_rate: int = 32, bn_size: int = 4,
                 init_channels: int = 128, config_str: str = "batchnorm-relu", memory_efficient: bool = True,
                 output_level: str = "segment", max_batch: int = 256, **kwargs):
        super().__init__()
        if config_str != "batchnorm-relu":
            raise NotImplementedError(f"CAMPPlus(HIP): config_str {config_str!r} is not built; the published models use "
                                      "'batchnorm-relu', whose BatchNorms fold into the convs")
        if output_level != "segment":
            raise NotImplementedError("CAMPPlus(HIP): output_level 'frame' (frame-level features) is not built; the embedding "
                                      "path ends in the stats pool")
        if (feat_dim, growth_rate, bn_size, init_channels) != (80, 32, 4, 128):
            raise NotImplementedError("CAMPPlus(HIP): only the published shape is built (feat_dim 80, growth_rate 32, bn_size 4, "
                                      "init_channels 128)")
        self.feat_dim, self.embedding_size = feat_dim, embedding_size
        self.growth_rate, self.bn_size, self.init_channels = growth_rate, bn_size, init_channels
        self.m_channels, self.bn_eps, self.max_batch = 32, 1e-5, int(max_batch)
        mc = self.m_channels
        head = Holder()
        head.conv1 = _conv(mc, 1, 3, 3)
        head.bn1 = _BN(mc)
        head.layer1 = torch.nn.Sequential(_res_block(mc, mc, 2), _res_block(mc, mc, 1))
        head.layer2 = torch.nn.Sequential(_res_block(mc, mc, 2), _res_block(mc, mc, 1))
        head.conv2 = _conv(mc, mc, 3, 3)
        head.bn2 = _BN(mc)
        self.head = head
        xv = torch.nn.Module()
        tdnn = Holder()
        tdnn.linear = _conv(init_channels, mc * (feat_dim // 8), 5)
        tdnn.nonlinear = _nonlinear(init_channels)
        xv.add_module("tdnn", tdnn)
        ch, bnc = init_channels, bn_size * growth_rate
        for i, n in enumerate(LAYERS):
            block = torch.nn.Module()
            for j in range(n):
                layer = Holder()
                layer.nonlinear1 = _nonlinear(ch + j * growth_rate)
                layer.linear1 = _conv(bnc, ch + j * growth_rate, 1)
                layer.nonlinear2 = _nonlinear(bnc)
                cam = Holder()
                cam.linear_local = _conv(growth_rate, bnc, 3)
                cam.linear1 = ParamHolder((bnc // 2, bnc, 1), (bnc // 2,))
                cam.linear2 = ParamHolder((growth_rate, bnc // 2, 1), (growth_rate,))
                layer.cam_layer = cam
                block.add_module(f"tdnnd{j + 1}", layer)
            xv.add_module(f"block{i + 1}", block)
            ch += n * growth_rate
            transit = Holder()
            transit.nonlinear = _nonlinear(ch)
            transit.linear = _conv(ch // 2, ch, 1)
            xv.add_module(f"transit{i + 1}", transit)
            ch //= 2
        xv.add_module("out_nonlinear", _nonlinear(ch))
        dense = Holder()
        dense.linear = _conv(embedding_size, ch * 2, 1)
        dense.nonlinear = _nonlinear(embedding_size, affine=False)
        xv.add_module("dense", dense)
        self.xvector = xv

    # ------------------------------------------------------------------------------------------------ handle
    def _make_config(self):
        return _lib.pf_campplus_config(self.feat_dim, self.embedding_size, self.growth_rate, self.bn_size, self.init_channels,
                                       self.m_channels, self.bn_eps)

    def _after_create(self, lib, handle):
        _lib.check(lib.pf_campplus_set_max_batch(handle, self.max_batch), "pf_campplus_set_max_batch")

    def set_max_batch(self, n: int):
        """chunks per launch sequence (never changes a result). The workspace is about 31 KB per frame of a sub-batch (4.6 MB per
        1.5-s chunk): it is bounded by this for equal-length chunks, but one long utterance through forward() needs its whole
        length at once (about 11 GB for an hour)."""
        self.max_batch = int(n)
        if self._handle is not None:
            _lib.check(_lib.load().pf_campplus_set_max_batch(self._handle, self.max_batch), "pf_campplus_set_max_batch")

    # ------------------------------------------------------------------------------------------------ compute
    @staticmethod
    def frames_after_tdnn(T: int) -> int:
        return (T - 1) // 2 + 1

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        if x.dim() != 3 or x.shape[2] != self.feat_dim:
            raise ValueError(f"CAMPPlus: expected features [B, T, {self.feat_dim}], got {tuple(x.shape)}")
        B, T, _ = x.shape
        if self.frames_after_tdnn(T) < 2:
            raise ValueError(f"CAMPPlus: {T} frames leave fewer than 2 after the stride-2 TDNN: the standard deviation of the "
                             "stats pool is undefined (the reference returns NaN)")
        emb = torch.empty(B, self.embedding_size, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.pf_campplus_forward(h, x.data_ptr(), B, T, emb.data_ptr(), stream_ptr()), "pf_campplus_forward")
        return emb

    def embed_chunks(self, wav: torch.Tensor, starts: Sequence[int], chunk_len: int,
                     valid: Optional[Sequence[int]] = None) -> torch.Tensor:
        """embeddings of chunks of one waveform in GPU memory: chunk i = wav[starts[i] : starts[i] + valid[i]] zero-padded to
        chunk_len samples (sv_chunk's padding of a short segment, campplus/utils.py:76-116) -> [N, 192]"""
        lib, h = self._ensure_handle()
        dev = self._handle_device
        w = wav.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        n = len(starts)
        emb = torch.empty(n, self.embedding_size, device=dev, dtype=torch.float32)
        if n == 0:
            return emb
        if int(chunk_len) < 400:
            raise ValueError("CAMPPlus: a chunk must hold at least one 25-ms analysis window")
        T = (int(chunk_len) - 400) // 160 + 1
        if self.frames_after_tdnn(T) < 2:
            raise ValueError(f"CAMPPlus: chunks of {chunk_len} samples give {T} frames, fewer than 2 after the TDNN")
        st = (_lib.C.c_int64 * n)(*[int(s) for s in starts])
        va = None
        if valid is not None:
            if len(valid) != n:
                raise ValueError("CAMPPlus: one valid length per chunk")
            va = (_lib.C.c_int32 * n)(*[int(v) for v in valid])
        with torch.cuda.device(dev):
            _lib.check(lib.pf_campplus_embed_chunks(h, w.data_ptr(), w.numel(), st, va, n, int(chunk_len), emb.data_ptr(),
                                                    stream_ptr()), "pf_campplus_embed_chunks")
            torch.cuda.current_stream(dev).synchronize()      # the host arrays above are staged asynchronously
        return emb

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """the reference's CAMPPlus.inference (model.py): waveforms (paths, arrays, tensors, a list of numpy chunks as AutoModel
        passes them) -> ([{"spk_embedding": [B, 192]}], meta). Each waveform gets its own kaldi fbank and time-mean removal; a
        batch of unequal lengths is zero-padded after that and the network runs over the padding (extract_feature + pad_list)."""
        return speaker_inference(self, data_in, **kwargs)

    def fbank(self, wav: torch.Tensor) -> torch.Tensor:
        """extract_feature for one waveform on the device: kaldi fbank (CAM++ options) minus its time mean -> [T, 80]"""
        return speaker_fbank(self, wav)


# The feature path of the reference's speaker models (campplus/utils.py extract_feature), shared by every module that has `feat_dim`,
# `forward` and HipModule's `_device` (CAMPPlus, ERes2NetV2SV).
def speaker_fbank(module, wav: torch.Tensor) -> torch.Tensor:
    """extract_feature for one waveform on the device: kaldi fbank (povey window, no 2^15 scaling, dither 0) minus its time mean"""
    n = int(wav.numel())
    if n < 400:
        raise ValueError(f"{type(module).__name__}: a waveform must hold at least one 25-ms analysis window")
    dev = module._device()
    fe = module.__dict__.setdefault("_fe", {}).get(dev)         # one frontend per device the module has lived on
    if fe is None:
        from .wav_frontend import WavFrontend

        fe = WavFrontend(window="povey", n_mels=module.feat_dim, frame_length=25, frame_shift=10, lfr_m=1, lfr_n=1, dither=0.0,
                         upsacle_samples=False, device=dev)
        module.__dict__["_fe"][dev] = fe
    feats, flens = fe(wav.to(torch.float32).reshape(1, -1), [n])
    f = feats[0, : int(flens[0])]
    return f - f.mean(dim=0, keepdim=True)


def speaker_inference(module, data_in, **kwargs):
    """waveforms -> ([{"spk_embedding": [B, E]}], meta): per-waveform fbank and mean removal, zero-padding to the longest, forward"""
    from .audio import load_audio_list

    meta = {}
    t1 = time.perf_counter()
    if isinstance(data_in, (list, tuple)):
        audio = [torch.as_tensor(np.asarray(d, dtype=np.float32)) if isinstance(d, np.ndarray) and d.dtype.kind == "f"
                 else load_audio_list([d], fs=SAMPLE_RATE, audio_fs=kwargs.get("fs", SAMPLE_RATE))[0] for d in data_in]
    else:
        audio = load_audio_list(data_in, fs=SAMPLE_RATE, audio_fs=kwargs.get("fs", SAMPLE_RATE))
    t2 = time.perf_counter()
    meta["load_data"] = f"{t2 - t1:0.3f}"
    dev = module._device()
    feats = [module.fbank(a.to(dev)) for a in audio]
    T = max(f.shape[0] for f in feats)
    x = torch.zeros(len(feats), T, module.feat_dim, device=dev)
    for i, f in enumerate(feats):
        x[i, : f.shape[0]] = f
    meta["extract_feat"] = f"{time.perf_counter() - t2:0.3f}"
    meta["batch_data_time"] = float(sum(int(a.shape[0]) for a in audio)) / SAMPLE_RATE
    return [{"spk_embedding": module.forward(x)}], meta
