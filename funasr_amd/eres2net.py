"""ERes2NetV2 speaker embedding on gfx950 (funasr/models/eres2net/model.py, eres2netv2.py, fusion.py).

`ERes2NetV2SV` is registered as model_classes/"ERes2NetV2" and "iic/speech_eres2netv2_sv_zh-cn_16k-common". It holds the reference's
parameters AND BatchNorm buffers under the reference's state_dict keys ("model.conv1.weight", ...; 557 of them at the default
configuration, `num_batches_tracked` included), so the reference's `state_dict()` loads with strict=True; all arithmetic runs in
csrc/eres2net.hip through the `pf_eres2net` handle:
  * `forward(x [B, T, feat_dim]) -> [B, E]`: the reference's forward on ready features (extract_feature's mean-normalised fbank);
  * `embed_chunks(wav, starts, chunk_len, valid=None)`: chunks of a waveform already in GPU memory straight to embeddings
    (gather, kaldi fbank, mean removal, network) in one library call -- the diarization path of funasr_amd/speaker.py;
  * `inference(data_in, ...)`: the reference's contract -> ([{"spk_embedding": [B, E]}], meta).
Weights come from `pretrained_eres2netv2.ckpt` in the model directory or `init_param` (bare keys, optionally under "state_dict", as
the reference's `_load_pretrained` reads them) or from a `model.pt` with "model."-prefixed keys (AutoModel's strict load).
Built: feat_dim and m_channels in multiples of 8 (8 .. 128, 8 .. 64), any four positive num_blocks, any embedding_size >= 1, with
baseWidth 26, scale 2, expansion 2, TSTP pooling and one embedding layer; everything else is refused by name.
"""
from __future__ import annotations

import logging
import os
from typing import Optional, Sequence

import torch

from . import _lib
from .campplus import _BN, speaker_fbank, speaker_inference
from .hip_module import Holder, HipModule, ParamHolder, _truthy, stream_ptr
from .register import tables

MIN_FRAMES = 9           # fewer leave one frame after the three stride-2 stages


def _aff(channels: int, r: int = 4) -> Holder:
    """AFF's parameter names: local_att = Sequential(Conv2d, BatchNorm2d, SiLU, Conv2d, BatchNorm2d) -> indices 0, 1, 3, 4"""
    inter = channels // r
    a = Holder()
    att = torch.nn.Module()
    att.add_module("0", ParamHolder((inter, 2 * channels, 1, 1), (inter,)))
    att.add_module("1", _BN(inter))
    att.add_module("3", ParamHolder((channels, inter, 1, 1), (channels,)))
    att.add_module("4", _BN(channels))
    a.local_att = att
    return a


def _block(in_planes: int, planes: int, stride: int, fuse: bool) -> Holder:
    width = planes * 26 // 64
    b = Holder()
    b.conv1 = ParamHolder((2 * width, in_planes, 1, 1))
    b.bn1 = _BN(2 * width)
    b.convs = torch.nn.ModuleList([ParamHolder((width, width, 3, 3)) for _ in range(2)])
    b.bns = torch.nn.ModuleList([_BN(width) for _ in range(2)])
    if fuse:
        b.fuse_models = torch.nn.ModuleList([_aff(width)])
    b.conv3 = ParamHolder((2 * planes, 2 * width, 1, 1))
    b.bn3 = _BN(2 * planes)
    if stride != 1 or in_planes != 2 * planes:
        b.shortcut = torch.nn.Sequential(ParamHolder((2 * planes, in_planes, 1, 1)), _BN(2 * planes))
    return b


@tables.register("model_classes", "ERes2NetV2")
@tables.register("model_classes", "iic/speech_eres2netv2_sv_zh-cn_16k-common")
class ERes2NetV2SV(HipModule):
    _prefix = "pf_eres2net"
    _push_buffers = True      # BatchNorm running statistics: the library folds them into the convs

    def __init__(self, feat_dim: int = 80, embedding_size: int = 192, m_channels: int = 64, baseWidth: int = 26, scale: int = 2,
                 expansion: int = 2, num_blocks=(3, 4, 6, 3), pooling_func: str = "TSTP", two_emb_layer: bool = False,
                 max_batch: int = 256, **kwargs):
        super().__init__()
        name = "ERes2NetV2SV(HIP)"
        for opt, val, built in (("baseWidth", baseWidth, 26), ("scale", scale, 2), ("expansion", expansion, 2),
                                ("pooling_func", pooling_func, "TSTP")):
            if val != built:
                raise NotImplementedError(f"{name}: {opt}={val!r} is not built; the published model uses {opt}={built!r}")
        if _truthy(two_emb_layer):
            raise NotImplementedError(f"{name}: two_emb_layer=True (seg_bn_1 + seg_2) is not built; the published model has one "
                                      "embedding layer")
        num_blocks = [int(n) for n in num_blocks]
        if int(feat_dim) % 8 != 0 or not 8 <= int(feat_dim) <= 128:
            raise NotImplementedError(f"{name}: feat_dim={feat_dim!r} is not built; the three stride-2 stages need a multiple of 8 "
                                      "from 8 to 128")
        if int(m_channels) % 8 != 0 or not 8 <= int(m_channels) <= 64:
            raise NotImplementedError(f"{name}: m_channels={m_channels!r} is not built (a multiple of 8 from 8 to 64 is)")
        if len(num_blocks) != 4 or min(num_blocks) < 1:
            raise NotImplementedError(f"{name}: num_blocks={num_blocks!r} is not built (four positive counts are)")
        if int(embedding_size) < 1:
            raise NotImplementedError(f"{name}: embedding_size={embedding_size!r} is not built (>= 1 is)")
        for flag in ("bf16", "fp16"):
            if _truthy(kwargs.get(flag, False)):
                raise NotImplementedError(f"{name}: {flag}=True is not built; the network has one arithmetic, fp32 on the exact-f32 "
                                          "matrix instruction")
        if kwargs.get("precision", "fp32") not in ("fp32", None):
            raise NotImplementedError(f"{name}: precision={kwargs['precision']!r} is not built (fp32 only)")
        self.feat_dim, self.embedding_size, self.m_channels = int(feat_dim), int(embedding_size), int(m_channels)
        self.num_blocks, self.bn_eps, self.max_batch = num_blocks, 1e-5, int(max_batch)
        mc = self.m_channels
        net = Holder()
        net.conv1 = ParamHolder((mc, 1, 3, 3))
        net.bn1 = _BN(mc)
        in_planes = mc
        for i, n in enumerate(num_blocks):
            planes, blocks = mc << i, []
            for b in range(n):
                blocks.append(_block(in_planes, planes, 2 if (b == 0 and i > 0) else 1, fuse=i >= 2))
                in_planes = 2 * planes
            net.add_module(f"layer{i + 1}", torch.nn.Sequential(*blocks))
        net.layer3_ds = ParamHolder((16 * mc, 8 * mc, 3, 3))
        net.fuse34 = _aff(16 * mc)
        self.stats_dim = (self.feat_dim // 8) * mc * 8
        net.seg_1 = ParamHolder((self.embedding_size, self.stats_dim * 2 * 2), (self.embedding_size,))
        self.model = net
        # the reference's constructor (model.py): pretrained_eres2netv2.ckpt of the model directory, or init_param
        init_param, model_path = kwargs.get("init_param"), kwargs.get("model_path")
        if init_param is None and model_path is not None:
            ckpt = os.path.join(model_path, "pretrained_eres2netv2.ckpt")
            if os.path.exists(ckpt):
                init_param = ckpt
        if init_param is not None and os.path.exists(init_param) and not str(init_param).endswith(".arena"):
            self._load_pretrained(init_param)

    def _load_pretrained(self, path: str):
        """a checkpoint in either layout: bare keys ("conv1.weight", the published .ckpt, optionally under "state_dict") or
        "model."-prefixed keys (a saved ERes2NetV2SV.state_dict())"""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
            sd = sd["state_dict"]
        own = self.state_dict()
        if not any(k in own for k in sd):
            sd = {"model." + k: v for k, v in sd.items()}
        missing, _ = self.load_state_dict(sd, strict=False)
        if missing:
            logging.warning("ERes2NetV2 missing keys: %s...", missing[:5])

    # ------------------------------------------------------------------------------------------------ handle
    def _make_config(self):
        return _lib.pf_eres2net_config(self.feat_dim, self.embedding_size, self.m_channels, (_lib.C.c_int32 * 4)(*self.num_blocks),
                                       self.bn_eps)

    def _after_create(self, lib, handle):
        _lib.check(lib.pf_eres2net_set_max_batch(handle, self.max_batch), "pf_eres2net_set_max_batch")

    def set_max_batch(self, n: int):
        """chunks per launch sequence (never changes a result). The workspace is `workspace_bytes(T)` per chunk of a sub-batch
        (about 20 MB per 1.5-s chunk at the default configuration, 5.2 GB for the default 256 chunks): bounded by this for equal-length chunks, but one long
        utterance through forward() needs its whole length at once."""
        self.max_batch = int(n)
        if self._handle is not None:
            _lib.check(_lib.load().pf_eres2net_set_max_batch(self._handle, self.max_batch), "pf_eres2net_set_max_batch")

    def workspace_bytes(self, T: int) -> int:
        lib, h = self._ensure_handle()
        return int(lib.pf_eres2net_workspace_bytes(h, int(T)))

    # ------------------------------------------------------------------------------------------------ compute
    @staticmethod
    def frames_after_strides(T: int) -> int:
        for _ in range(3):
            T = (T - 1) // 2 + 1
        return T

    def _refuse_short(self, T: int, what: str):
        if T < MIN_FRAMES:
            raise ValueError(f"ERes2NetV2SV: {what} {T} frames, fewer than {MIN_FRAMES}: one frame is left after the three stride-2 "
                             "stages and the standard deviation of the stats pool is undefined (the reference returns NaN)")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 3 or x.shape[2] != self.feat_dim:
            raise ValueError(f"ERes2NetV2SV: expected features [B, T, {self.feat_dim}], got {tuple(x.shape)}")
        B, T, _ = x.shape
        self._refuse_short(T, "the input has")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        emb = torch.empty(B, self.embedding_size, device=dev, dtype=torch.float32)
        if B == 0:
            return emb
        with torch.cuda.device(dev):
            _lib.check(lib.pf_eres2net_forward(h, x.data_ptr(), B, T, emb.data_ptr(), stream_ptr()), "pf_eres2net_forward")
        return emb

    def forward_stages(self, x: torch.Tensor) -> dict:
        """forward of one sub-batch that also returns what the network computes on the way (tests): the stem, layer1 .. layer4,
        layer3_ds and fuse34 outputs as channels-last [B, t, f, c], the pooled "stats" [B, 2 S] and "emb" """
        B, T, _ = x.shape
        self._refuse_short(T, "the input has")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        mc, shapes, t, f = self.m_channels, {}, T, self.feat_dim
        shapes["stem"] = (B, t, f, mc)
        for i in range(4):
            if i > 0:
                t, f = (t - 1) // 2 + 1, (f - 1) // 2 + 1
            shapes[f"layer{i + 1}"] = (B, t, f, 2 * (mc << i))
        shapes["layer3_ds"] = shapes["fuse34"] = shapes["layer4"]
        shapes["stats"] = (B, 2 * f * 16 * mc)
        out = {k: torch.empty(s, device=dev, dtype=torch.float32) for k, s in shapes.items()}
        out["emb"] = torch.empty(B, self.embedding_size, device=dev, dtype=torch.float32)
        ptrs = (_lib.C.c_void_p * 8)(*[out[k].data_ptr() for k in ("stem", "layer1", "layer2", "layer3", "layer4", "layer3_ds", "fuse34",
                                                                    "stats")])
        with torch.cuda.device(dev):
            _lib.check(lib.pf_eres2net_forward_stages(h, x.data_ptr(), B, T, out["emb"].data_ptr(), ptrs, stream_ptr()),
                       "pf_eres2net_forward_stages")
        return out

    def debug_poison(self):
        """fill the handle's workspace with NaN bytes (tests: no result may depend on what a buffer held before)"""
        lib, h = self._ensure_handle()
        with torch.cuda.device(self._handle_device):
            _lib.check(lib.pf_eres2net_debug_poison(h), "pf_eres2net_debug_poison")

    def embed_chunks(self, wav: torch.Tensor, starts: Sequence[int], chunk_len: int,
                     valid: Optional[Sequence[int]] = None) -> torch.Tensor:
        """embeddings of chunks of one waveform in GPU memory: chunk i = wav[starts[i] : starts[i] + valid[i]] zero-padded to
        chunk_len samples (sv_chunk's padding of a short segment, campplus/utils.py:76-116) -> [N, E]"""
        lib, h = self._ensure_handle()
        dev = self._handle_device
        w = wav.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        n = len(starts)
        emb = torch.empty(n, self.embedding_size, device=dev, dtype=torch.float32)
        if n == 0:
            return emb
        if int(chunk_len) < 400:
            raise ValueError("ERes2NetV2SV: a chunk must hold at least one 25-ms analysis window")
        self._refuse_short((int(chunk_len) - 400) // 160 + 1, f"chunks of {chunk_len} samples give")
        st = (_lib.C.c_int64 * n)(*[int(s) for s in starts])
        va = None
        if valid is not None:
            if len(valid) != n:
                raise ValueError("ERes2NetV2SV: one valid length per chunk")
            va = (_lib.C.c_int32 * n)(*[int(v) for v in valid])
        with torch.cuda.device(dev):
            _lib.check(lib.pf_eres2net_embed_chunks(h, w.data_ptr(), w.numel(), st, va, n, int(chunk_len), emb.data_ptr(),
                                                    stream_ptr()), "pf_eres2net_embed_chunks")
            torch.cuda.current_stream(dev).synchronize()      # the host arrays above are staged asynchronously
        return emb

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """the reference's ERes2NetV2SV.inference (model.py): CAM++'s extract_feature on every waveform (its own kaldi fbank and
        time-mean removal, zero-padded to the longest), then the network -> ([{"spk_embedding": [B, E]}], meta)"""
        return speaker_inference(self, data_in, **kwargs)

    def fbank(self, wav: torch.Tensor) -> torch.Tensor:
        """extract_feature for one waveform on the device: kaldi fbank (CAM++ options, feat_dim bins) minus its time mean"""
        return speaker_fbank(self, wav)
