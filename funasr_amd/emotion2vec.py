"""emotion2vec speech emotion recognition on gfx950 (funasr/models/emotion2vec/model.py, audio.py, base.py, modules.py).

`Emotion2vec` is registered as model_classes/"Emotion2vec". It holds the reference's parameters under the reference's state_dict
keys (the training-only `modality_encoders.AUDIO.decoder.*` keys are accepted and never uploaded); all arithmetic runs in
csrc/emotion2vec.hip, csrc/attention_alibi.hip and csrc/engine_emotion2vec.hip through the `pf_emotion2vec` handle:
  * `extract_features(source, lengths=None)` -> {"x": [B, T, D] frames (zero past each utterance's frames), "padding_mask"};
  * `inference(data_in, ...)` -> the reference's records {"key", "labels", "scores"[, "feats"]} for the whole batch in one forward.
Precision follows the project's modes: "f16x2" (default; GEMMs on the fp16 MFMA with two-plane operands, fp32-class results) or
"fp32" (exact-f32 MFMA GEMMs). Attention, convs, LayerNorms and softmax are fp32 in both.
"""
from __future__ import annotations

import ast
import os
import time

import numpy as np
import torch

from . import _lib
from .hip_module import Holder, HipModule, ParamHolder, _truthy, stream_ptr
from .register import tables

SAMPLE_RATE = 16000
CONV_DIM = 512
_PRECISIONS = {"fp32": 0, "f16x2": 3}


def parse_feature_encoder_spec(spec) -> list:
    """feature_encoder_spec ('[(512, 10, 5)] + [(512, 3, 2)] * 4 + ...') -> [(dim, kernel, stride), ...] WITHOUT eval: lists,
    tuples, integers, + and * only"""
    if not isinstance(spec, str):
        return [tuple(int(v) for v in layer) for layer in spec]

    def walk(n):
        if isinstance(n, ast.Expression):
            return walk(n.body)
        if isinstance(n, ast.Constant) and isinstance(n.value, int) and not isinstance(n.value, bool):
            return n.value
        if isinstance(n, ast.List):
            return [walk(e) for e in n.elts]
        if isinstance(n, ast.Tuple):
            return tuple(walk(e) for e in n.elts)
        if isinstance(n, ast.BinOp) and isinstance(n.op, (ast.Add, ast.Mult)):
            a, b = walk(n.left), walk(n.right)
            return a + b if isinstance(n.op, ast.Add) else a * b
        raise ValueError(f"feature_encoder_spec: unsupported expression {ast.dump(n)[:60]}")

    out = walk(ast.parse(spec, mode="eval"))
    if not isinstance(out, list) or not all(isinstance(t, tuple) and len(t) == 3 for t in out):
        raise ValueError(f"feature_encoder_spec: expected a list of (dim, kernel, stride) tuples, got {spec!r}")
    return [tuple(int(v) for v in t) for t in out]


def _num(v, kind=float):
    """yaml.safe_load reads `1e-05` as a string where omegaconf reads a float"""
    if isinstance(v, str):
        v = float(v)
    return kind(v)


def get_slopes(n: int) -> list:
    """the ALiBi slopes of base.py get_alibi (interleaved when n is not a power of two)"""
    import math

    def pow2(n):
        start = 2 ** (-(2 ** -(math.log2(n) - 3)))
        return [start * start ** i for i in range(n)]

    if math.log2(n).is_integer():
        return pow2(n)
    cp = 2 ** math.floor(math.log2(n))
    return pow2(cp) + get_slopes(2 * cp)[0::2][: n - cp]


def _block(D: int, ffn: int) -> Holder:
    b = Holder()
    b.norm1 = ParamHolder((D,), (D,))
    attn = Holder()
    attn.qkv = ParamHolder((3 * D, D), (3 * D,))
    attn.proj = ParamHolder((D, D), (D,))
    b.attn = attn
    b.norm2 = ParamHolder((D,), (D,))
    mlp = Holder()
    mlp.fc1 = ParamHolder((ffn, D), (ffn,))
    mlp.fc2 = ParamHolder((D, ffn), (D,))
    b.mlp = mlp
    return b


@tables.register("model_classes", "Emotion2vec")
class Emotion2vec(HipModule):
    _prefix = "pf_emotion2vec"
    _skip_keys = ("modality_encoders.AUDIO.decoder.",)

    def __init__(self, model_conf: dict = None, vocab_size: int = -1, precision: str = None, max_samples: int = 8 << 20, **kwargs):
        super().__init__()
        conf = dict(kwargs)
        conf.update(model_conf or {})                      # the reference's form: Emotion2vec(model_conf=..., vocab_size=...)
        audio = dict((conf.get("modalities") or {}).get("audio") or {})
        if not audio:
            raise ValueError("Emotion2vec: model_conf.modalities.audio is required")
        self.embed_dim = _num(conf.get("embed_dim", 768), int)
        self.num_heads = _num(conf.get("num_heads", 12), int)
        self.depth = _num(conf.get("depth", 8), int)
        self.mlp_ratio = _num(conf.get("mlp_ratio", 4.0))
        self.norm_eps = _num(conf.get("norm_eps", 1e-5))
        self.normalize = _truthy(conf.get("normalize", True))
        self.prenet_depth = _num(audio.get("prenet_depth", 4), int)
        self.num_extra_tokens = _num(audio.get("num_extra_tokens", 0), int)
        self.num_alibi_heads = _num(audio.get("num_alibi_heads", self.num_heads), int)
        self.conv_pos_depth = _num(audio.get("conv_pos_depth", 5), int)
        self.conv_pos_groups = _num(audio.get("conv_pos_groups", 16), int)
        self.conv_pos_kernel = max(3, _num(audio.get("conv_pos_width", 95), int) // self.conv_pos_depth) if self.conv_pos_depth else 3
        self.spec = parse_feature_encoder_spec(audio.get("feature_encoder_spec", "[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512,2,2)] * 2"))
        self.ffn_dim = int(self.embed_dim * self.mlp_ratio)
        self.per_layer = _truthy(audio.get("learned_alibi_scale_per_layer", False))
        self.per_head = _truthy(audio.get("learned_alibi_scale_per_head", False))
        refusals = [
            (_truthy(conf.get("layer_norm_first", False)), "layer_norm_first: true (pre-LN blocks and a final norm)"),
            (str(audio.get("extractor_mode", conf.get("extractor_mode", "layer_norm"))) != "layer_norm",
             "extractor_mode other than 'layer_norm' (the group-norm conv encoder)"),
            (_truthy(audio.get("learned_alibi", False)), "learned_alibi (a learned bias table)"),
            (_truthy(audio.get("conv_pos_pre_ln", False)), "conv_pos_pre_ln"),
            (not _truthy(audio.get("use_alibi_encoder", True)), "use_alibi_encoder: false"),
            (self.embed_dim != 64 * self.num_heads, f"head dim {self.embed_dim / max(self.num_heads, 1):g} (only 64 is built)"),
            (any(d != CONV_DIM for d, _, _ in self.spec), "conv encoder layers of other than 512 channels"),
            (not _truthy(conf.get("norm_affine", True)), "norm_affine: false"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"Emotion2vec(HIP): {why} is not built")
        vocab_size = int(vocab_size) if vocab_size is not None else -1
        self.vocab_size = vocab_size
        self.max_samples = int(max_samples)
        mode = precision or conf.get("precision") or "f16x2"
        if mode not in _PRECISIONS:
            raise NotImplementedError(f"Emotion2vec(HIP): precision {mode!r}: built are {sorted(_PRECISIONS)}")
        self.precision = mode
        self.label_mask = None
        D = self.embed_dim
        enc = Holder()
        enc.extra_tokens = torch.nn.Parameter(torch.zeros(1, self.num_extra_tokens, D), requires_grad=False)
        n_scale = (self.prenet_depth + self.depth) if self.per_layer else 1
        enc.alibi_scale = torch.nn.Parameter(torch.ones(n_scale, 1, self.num_alibi_heads if self.per_head else 1, 1, 1),
                                             requires_grad=False)
        local = Holder()
        convs = torch.nn.ModuleList()
        cin = 1
        for d, k, s in self.spec:
            layer = torch.nn.Module()
            layer.add_module("0", ParamHolder((d, cin, k)))
            ln = torch.nn.Module()
            ln.add_module("1", ParamHolder((d,), (d,)))
            layer.add_module("2", ln)
            convs.append(layer)
            cin = d
        local.conv_layers = convs
        enc.local_encoder = local
        pfm = torch.nn.Module()
        pfm.add_module("1", ParamHolder((CONV_DIM,), (CONV_DIM,)))
        pfm.add_module("2", ParamHolder((D, CONV_DIM), (D,)))
        enc.project_features = pfm
        pos = torch.nn.Module()
        for i in range(self.conv_pos_depth):
            layer = torch.nn.Module()
            layer.add_module("0", ParamHolder((D, D // self.conv_pos_groups, self.conv_pos_kernel), (D,)))
            pos.add_module(str(i + 1), layer)
        enc.relative_positional_encoder = pos
        ctx = Holder()
        ctx.blocks = torch.nn.ModuleList([_block(D, self.ffn_dim) for _ in range(self.prenet_depth)])
        ctx.norm = ParamHolder((D,), (D,))
        enc.context_encoder = ctx
        self.modality_encoders = torch.nn.ModuleDict({"AUDIO": enc})
        self.blocks = torch.nn.ModuleList([_block(D, self.ffn_dim) for _ in range(self.depth)])
        self.proj = ParamHolder((vocab_size, D), (vocab_size,)) if vocab_size > 0 else None

    # ------------------------------------------------------------------------------------------------ state dict
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        skip = prefix + "modality_encoders.AUDIO.decoder."
        unexpected_keys[:] = [k for k in unexpected_keys if not k.startswith(skip)]

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # a checkpoint carries the training-only decoder; it is accepted (and dropped) under strict loading
        sd = {k: v for k, v in state_dict.items() if not k.startswith("modality_encoders.AUDIO.decoder.")}
        return super().load_state_dict(sd, strict=strict)

    # ------------------------------------------------------------------------------------------------ handle
    def _make_config(self):
        c = _lib.pf_emotion2vec_config()
        c.embed_dim, c.num_heads, c.ffn_dim = self.embed_dim, self.num_heads, self.ffn_dim
        c.prenet_depth, c.depth, c.num_extra_tokens, c.num_alibi_heads = self.prenet_depth, self.depth, self.num_extra_tokens, self.num_alibi_heads
        c.alibi_scale_layers = (self.prenet_depth + self.depth) if self.per_layer else 1
        c.alibi_scale_heads = self.num_alibi_heads if self.per_head else 1
        if len(self.spec) > 8:
            raise NotImplementedError("Emotion2vec(HIP): more than 8 conv encoder layers")
        c.n_conv = len(self.spec)
        for i, (_, k, s) in enumerate(self.spec):
            c.conv_kernel[i], c.conv_stride[i] = k, s
        c.conv_pos_depth, c.conv_pos_kernel, c.conv_pos_groups = self.conv_pos_depth, self.conv_pos_kernel, self.conv_pos_groups
        c.vocab_size = max(self.vocab_size, 0)
        c.normalize = int(self.normalize)
        c.precision = _PRECISIONS[self.precision]
        c.norm_eps = self.norm_eps
        return c

    def _after_create(self, lib, handle):
        _lib.check(lib.pf_emotion2vec_set_max_samples(handle, self.max_samples), "pf_emotion2vec_set_max_samples")
        if self.label_mask is not None:
            m = (_lib.C.c_int32 * len(self.label_mask))(*self.label_mask)
            _lib.check(lib.pf_emotion2vec_set_label_mask(handle, m, len(self.label_mask)), "pf_emotion2vec_set_label_mask")

    def set_precision(self, mode: str):
        if mode not in _PRECISIONS:
            raise NotImplementedError(f"Emotion2vec(HIP): precision {mode!r}: built are {sorted(_PRECISIONS)}")
        if mode != self.precision:
            self.precision = mode
            self._free()

    def set_max_samples(self, n: int):
        """samples per launch sequence (never changes a result bit); the workspace is about 1.4 KB per sample of a sub-batch"""
        self.max_samples = int(n)
        if self._handle is not None:
            _lib.check(_lib.load().pf_emotion2vec_set_max_samples(self._handle, self.max_samples), "pf_emotion2vec_set_max_samples")

    def set_labels(self, labels):
        """the token list: classes whose label starts with 'unuse' are excluded from the softmax (model.py:303-305)"""
        mask = [1 if str(lab).startswith("unuse") else 0 for lab in labels]
        if self.vocab_size > 0 and len(mask) != self.vocab_size:
            raise ValueError(f"Emotion2vec: {len(mask)} labels for a {self.vocab_size}-class proj")
        if mask != self.label_mask:
            self.label_mask = mask
            if self._handle is not None and self.vocab_size > 0:
                m = (_lib.C.c_int32 * len(mask))(*mask)
                _lib.check(_lib.load().pf_emotion2vec_set_label_mask(self._handle, m, len(mask)), "pf_emotion2vec_set_label_mask")

    # ------------------------------------------------------------------------------------------------ compute
    def num_frames(self, n_samples: int) -> int:
        L = int(n_samples)
        for _, k, s in self.spec:
            if L < k:
                return 0
            L = (L - k) // s + 1
        return L

    def min_samples(self) -> int:
        n = 1
        while self.num_frames(n) < 1:
            n += 1
        return n

    def forward_packed(self, wav: torch.Tensor, lens, frames: bool = True, pooled: bool = True, probs: bool = True):
        """wav: utterances back to back on the device, lens: their sample counts -> (frames [sum T, D] | None, pooled [B, D] | None,
        probs [B, C] | None)"""
        lens = [int(n) for n in lens]
        for i, n in enumerate(lens):
            if self.num_frames(n) < 1:
                raise ValueError(f"Emotion2vec: utterance {i} has {n} samples; the conv encoder needs at least {self.min_samples()} "
                                 f"({self.min_samples() / SAMPLE_RATE * 1000:.0f} ms at 16 kHz)")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        w = wav.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        if w.numel() != sum(lens):
            raise ValueError("Emotion2vec: the packed waveform must hold sum(lens) samples")
        B, D = len(lens), self.embed_dim
        T = sum(self.num_frames(n) for n in lens)
        f = torch.empty(T, D, device=dev) if frames else None
        p = torch.empty(B, D, device=dev) if pooled else None
        q = torch.empty(B, self.vocab_size, device=dev) if probs and self.vocab_size > 0 else None
        ln = (_lib.C.c_int64 * B)(*lens)
        with torch.cuda.device(dev):
            _lib.check(lib.pf_emotion2vec_forward(h, w.data_ptr(), ln, B, f.data_ptr() if f is not None else None,
                                                  p.data_ptr() if p is not None else None, q.data_ptr() if q is not None else None,
                                                  stream_ptr()), "pf_emotion2vec_forward")
            torch.cuda.current_stream(dev).synchronize()       # the lengths above are staged asynchronously
        return f, p, q

    def extract_features(self, source, lengths=None, padding_mask=None, **kwargs):
        """source [B, N] (or [N]) waveforms, each utterance's first lengths[b] samples (all N by default) -> {"x": [B, T, D] (zero
        past an utterance's frames), "padding_mask": [B, T] bool or None}. The waveform norm is applied when the config says so."""
        src = torch.as_tensor(source)
        if src.dim() == 1:
            src = src[None]
        B, N = src.shape
        lens = [N] * B if lengths is None else [int(v) for v in lengths]
        wav = torch.cat([src[b, : lens[b]] for b in range(B)])
        f, _, _ = self.forward_packed(wav, lens, pooled=False, probs=False)
        T = [self.num_frames(n) for n in lens]
        x = torch.zeros(B, max(T), self.embed_dim, device=f.device)
        mask = torch.zeros(B, max(T), dtype=torch.bool, device=f.device)
        o = 0
        for b in range(B):
            x[b, : T[b]] = f[o: o + T[b]]
            mask[b, T[b]:] = True
            o += T[b]
        return {"x": x, "padding_mask": mask if len(set(T)) > 1 else None}

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        """the reference's Emotion2vec.inference (model.py:234-318) for the whole batch in one forward"""
        from .audio import load_audio_list

        granularity = kwargs.get("granularity", "utterance")
        extract_embedding = kwargs.get("extract_embedding", True) or self.vocab_size <= 0
        meta = {}
        t1 = time.perf_counter()
        if isinstance(data_in, (list, tuple)):
            audio = [torch.as_tensor(np.asarray(d, dtype=np.float32)) if isinstance(d, np.ndarray) and d.dtype.kind == "f"
                     else load_audio_list([d], fs=SAMPLE_RATE, audio_fs=kwargs.get("fs", SAMPLE_RATE))[0] for d in data_in]
        else:
            audio = load_audio_list(data_in, fs=SAMPLE_RATE, audio_fs=kwargs.get("fs", SAMPLE_RATE))
        audio = [torch.as_tensor(a, dtype=torch.float32).reshape(-1) for a in audio]
        t2 = time.perf_counter()
        meta["load_data"] = f"{t2 - t1:0.3f}"
        meta["batch_data_time"] = len(audio[0]) / kwargs.get("fs", SAMPLE_RATE)
        labels = list(tokenizer.token_list) if tokenizer is not None and getattr(tokenizer, "token_list", None) is not None else []
        if self.vocab_size > 0 and labels:
            self.set_labels(labels)
        lens = [int(a.numel()) for a in audio]
        dev = self._device()
        wav = torch.cat(audio).to(dev)
        frames, pooled, probs = self.forward_packed(wav, lens, frames=granularity == "frame", pooled=True, probs=self.vocab_size > 0)
        pooled = pooled.cpu().numpy()
        probs = probs.cpu().numpy() if probs is not None else None
        frames = frames.cpu().numpy() if frames is not None else None
        if key is None:
            key = [f"utt_{i}" for i in range(len(audio))]
        output_dir = kwargs.get("output_dir")
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
        results, o = [], 0
        for i, n in enumerate(lens):
            T = self.num_frames(n)
            feats = frames[o: o + T] if granularity == "frame" else pooled[i]
            o += T
            if output_dir and extract_embedding:
                np.save(os.path.join(output_dir, f"{key[i]}.npy"), feats)
            scores = probs[i].tolist() if probs is not None else []
            keep = [j for j, lab in enumerate(labels) if not str(lab).startswith("unuse")]
            rec = {"key": key[i], "labels": [labels[j] for j in keep], "scores": [scores[j] for j in keep] if scores else []}
            if extract_embedding:
                rec["feats"] = feats
            results.append(rec)
        return results, meta
