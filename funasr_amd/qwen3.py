"""Qwen3 causal LM decoder on gfx950: `Qwen3Decoder`, the LM of `model: FunASRNano` (funasr/models/fun_asr_nano/model.py builds it with
`transformers.AutoModelForCausalLM.from_config`).

One `pf_qwen3` handle (csrc/engine_qwen3.hip, kernels in csrc/qwen3.hip): RMSNorm, a fused q | k | v projection, per-head q/k RMSNorm
+ rotary embedding with the KV-cache write, causal grouped-query attention (one kernel for prefill, a key-split pair for the decode
step), a fused gate | up projection, SwiGLU, and the vocabulary projection with its arg-max. fp32 throughout, greedy search, the
generation loop inside the library.

The module holds the parameters under the upstream state-dict names (`model.embed_tokens.weight`,
`model.layers.N.self_attn.q_proj.weight`, .., `model.norm.weight`, `lm_head.weight`), so a reference checkpoint's `llm.*` keys load key
for key. With `tie_word_embeddings` the vocabulary projection reads `model.embed_tokens.weight`; `lm_head.weight` is then held for the
state dict only.

A batch is 1 .. 16 sequences, each at its own length: there is no left padding, every kernel takes per-row (sequence, position).

Not built (each refused by name): a `model_type` other than qwen3, `attention_bias: true`, a sliding window, a rope type other than
`default`, `hidden_act` other than silu, `head_dim` other than 64 / 128, `hidden_size` / `intermediate_size` off a multiple of 32,
`num_key_value_heads` that does not divide `num_attention_heads`.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import torch
import torch.nn as nn

from . import _lib
from .hip_module import HipModule, Holder, ParamHolder, _truthy, stream_ptr

MAX_BATCH = 16
ROPE_ROWS = 4096          # positions of the first rotary table; doubled on demand


def read_lm_config(path: str) -> dict:
    """the LM's `config.json` below `path` as a dict: through transformers.AutoConfig when that package is importable (it fills the
    defaults of the model type), through json otherwise. Local files only."""
    if not os.path.isdir(path) or not os.path.isfile(os.path.join(path, "config.json")):
        raise FileNotFoundError(f"Qwen3Decoder(HIP): llm_conf.init_param_path {path!r} holds no config.json (a local directory is needed; "
                                "no hub is contacted)")
    try:
        from transformers import AutoConfig
    except ImportError:
        with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
            return json.load(f)
    return AutoConfig.from_pretrained(path, local_files_only=True).to_dict()


def _rope(conf: dict):
    """(theta, type) from wherever this config keeps them: the top level, `rope_parameters` or `rope_scaling`"""
    theta, kind = conf.get("rope_theta"), None
    for key in ("rope_parameters", "rope_scaling"):
        sub = conf.get(key)
        if isinstance(sub, dict):
            theta = sub.get("rope_theta", theta) if theta is None else theta
            kind = kind or sub.get("rope_type") or sub.get("type")
    return float(10000.0 if theta is None else theta), (kind or "default")


def rope_table(head_dim: int, theta: float, positions: int):
    """cos / sin [positions, head_dim / 2] in float32, computed as upstream's rotary embedding computes them"""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))
    freqs = torch.arange(positions, dtype=torch.int64).float()[:, None] * inv_freq[None, :].float()
    return freqs.cos().contiguous(), freqs.sin().contiguous()


def _nobias(out_f, in_f):
    return ParamHolder((out_f, in_f), None)


def _weight(dim):
    return ParamHolder((dim,), None)


class Qwen3Decoder(HipModule):
    _prefix = "pf_qwen3"

    def __init__(self, config: dict):
        super().__init__()
        c = dict(config)
        who = "Qwen3Decoder(HIP)"
        theta, rope_type = _rope(c)
        H, I = int(c.get("hidden_size", 0)), int(c.get("intermediate_size", 0))
        nh = int(c.get("num_attention_heads", 0))
        nkv = int(c.get("num_key_value_heads") or nh)
        hd = int(c.get("head_dim") or (H // max(nh, 1)))
        layer_types = c.get("layer_types") or []
        sliding = (_truthy(c.get("use_sliding_window")) and c.get("sliding_window")) or any(t != "full_attention" for t in layer_types)
        refusals = [
            (c.get("model_type") != "qwen3", f"model_type: {c.get('model_type')} (only qwen3)"),
            (_truthy(c.get("attention_bias", False)), "attention_bias: true"),
            (bool(sliding), "a sliding window (use_sliding_window / layer_types)"),
            (rope_type != "default", f"rope type: {rope_type} (only default)"),
            (c.get("hidden_act", "silu") != "silu", f"hidden_act: {c.get('hidden_act')} (only silu)"),
            (hd not in (64, 128), f"head_dim: {hd} (64 or 128)"),
            (H < 32 or H % 32 != 0, f"hidden_size: {H} (a multiple of 32)"),
            (I < 32 or I % 32 != 0, f"intermediate_size: {I} (a multiple of 32)"),
            (nh < 1 or nkv < 1 or nh % nkv != 0, f"num_key_value_heads: {nkv} with num_attention_heads {nh} (must divide it)"),
            (int(c.get("vocab_size", 0)) < 2 or int(c.get("num_hidden_layers", 0)) < 1, "vocab_size < 2 or num_hidden_layers < 1"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"{who}: {why} is not built")
        self.config = c
        self.vocab_size, self.hidden_size, self.intermediate_size = int(c["vocab_size"]), H, I
        self.num_layers, self.num_heads, self.num_kv_heads, self.head_dim = int(c["num_hidden_layers"]), nh, nkv, hd
        self.rms_eps, self.rope_theta = float(c.get("rms_norm_eps", 1e-6)), theta
        self.tie_word_embeddings = _truthy(c.get("tie_word_embeddings", False))
        eos = c.get("eos_token_id")
        self.eos_token_ids = [] if eos is None else ([int(e) for e in eos] if isinstance(eos, (list, tuple)) else [int(eos)])
        self.pad_token_id = c.get("pad_token_id")
        model = Holder()
        model.embed_tokens = ParamHolder((self.vocab_size, H), None)
        layers = nn.ModuleList()
        for _ in range(self.num_layers):
            l = Holder()
            a = Holder()
            a.q_proj, a.k_proj, a.v_proj, a.o_proj = _nobias(nh * hd, H), _nobias(nkv * hd, H), _nobias(nkv * hd, H), _nobias(H, nh * hd)
            a.q_norm, a.k_norm = _weight(hd), _weight(hd)
            m = Holder()
            m.gate_proj, m.up_proj, m.down_proj = _nobias(I, H), _nobias(I, H), _nobias(H, I)
            l.self_attn, l.mlp, l.input_layernorm, l.post_attention_layernorm = a, m, _weight(H), _weight(H)
            layers.append(l)
        model.layers = layers
        model.norm = _weight(H)
        self.model = model
        self.lm_head = _nobias(self.vocab_size, H)
        if self.tie_word_embeddings:
            self._skip_keys = ("lm_head.weight",)
        for p in self.parameters():
            p.requires_grad_(False)
        self._rope_rows = 0
        self._batch = 0

    @classmethod
    def from_config_dir(cls, path: str) -> "Qwen3Decoder":
        return cls(read_lm_config(path))

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def _make_config(self):
        c = _lib.pf_qwen3_config()
        c.vocab_size, c.hidden_size, c.intermediate_size, c.n_layers = self.vocab_size, self.hidden_size, self.intermediate_size, self.num_layers
        c.n_heads, c.n_kv_heads, c.head_dim = self.num_heads, self.num_kv_heads, self.head_dim
        c.tie_word_embeddings, c.rms_eps = int(self.tie_word_embeddings), self.rms_eps
        return c

    def _after_create(self, lib, handle):
        self._rope_rows = 0

    def _ensure_rope(self, lib, h, positions: int):
        if positions <= self._rope_rows:
            return
        rows = max(ROPE_ROWS, self._rope_rows)
        while rows < positions:
            rows *= 2
        cos, sin = rope_table(self.head_dim, self.rope_theta, rows)
        _lib.check(lib.pf_qwen3_set_rope_table(h, cos.data_ptr(), sin.data_ptr(), rows), "pf_qwen3_set_rope_table")
        self._rope_rows = rows

    # -- the pieces ---------------------------------------------------------------------------------------------------
    def embed(self, ids: torch.Tensor) -> torch.Tensor:
        """model.embed_tokens rows of `ids` (any integer tensor) -> [n, hidden_size] on the device"""
        lib, h = self._ensure_handle()
        dev = self._handle_device
        idv = ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty(idv.numel(), self.hidden_size, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.pf_qwen3_embed(h, idv.data_ptr(), idv.numel(), out.data_ptr(), stream_ptr()), "pf_qwen3_embed")
        return out

    def prefill(self, inputs_embeds, max_new_tokens: int, return_logits: bool = False):
        """inputs_embeds: a list of 1 .. 16 tensors [rows_b, hidden_size]. Starts the batch; returns the first id per sequence (a list)
        and, with return_logits, the logits of every row as a list of [rows_b, vocab_size] tensors."""
        lib, h = self._ensure_handle()
        dev = self._handle_device
        embs = [e.reshape(-1, self.hidden_size) for e in inputs_embeds]
        B = len(embs)
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"Qwen3Decoder: a batch is 1 .. {MAX_BATCH} sequences, got {B}")
        rows = [int(e.shape[0]) for e in embs]
        if min(rows) < 1:
            raise ValueError("Qwen3Decoder: a sequence without rows")
        x = torch.cat(embs, 0).to(device=dev, dtype=torch.float32).contiguous()
        logits = torch.empty(sum(rows), self.vocab_size, device=dev) if return_logits else None
        first = (C.c_int32 * B)()
        with torch.cuda.device(dev):
            self._ensure_rope(lib, h, max(rows) + int(max_new_tokens))
            _lib.check(lib.pf_qwen3_prefill(h, x.data_ptr(), (C.c_int32 * B)(*rows), B, int(max_new_tokens), first,
                                            None if logits is None else logits.data_ptr(), stream_ptr()), "pf_qwen3_prefill")
        self._batch = B
        if return_logits:
            return list(first), list(torch.split(logits, rows, 0))
        return list(first)

    def step(self, ids, return_logits: bool = False):
        """one decode step of every sequence of the batch: ids[b] is appended; returns the next ids (and the logits [B, vocab_size])"""
        lib, h = self._ensure_handle()
        B = self._batch
        if len(ids) != B or B < 1:
            raise ValueError(f"Qwen3Decoder.step: {len(ids)} ids for a batch of {B} sequences")
        dev = self._handle_device
        logits = torch.empty(B, self.vocab_size, device=dev) if return_logits else None
        nxt = (C.c_int32 * B)()
        with torch.cuda.device(dev):
            _lib.check(lib.pf_qwen3_step(h, (C.c_int32 * B)(*[int(i) for i in ids]), nxt, None if logits is None else logits.data_ptr(),
                                         stream_ptr()), "pf_qwen3_step")
        return (list(nxt), logits) if return_logits else list(nxt)

    def greedy(self, max_new_tokens: int, eos_token_ids=None, pad_token_id=None) -> torch.Tensor:
        """the generation loop of the library after prefill(): int64 [B, n] as `generate` returns them for `inputs_embeds` (new tokens
        only; a finished sequence is padded with pad_token_id; n = the step at which the last sequence finished, <= max_new_tokens)"""
        lib, h = self._ensure_handle()
        B, n_max = self._batch, int(max_new_tokens)
        eos = self.eos_token_ids if eos_token_ids is None else [int(e) for e in eos_token_ids]
        pad = pad_token_id if pad_token_id is not None else (self.pad_token_id if self.pad_token_id is not None else (eos[0] if eos else 0))
        out = (C.c_int32 * (B * n_max))()
        n = C.c_int32(0)
        with torch.cuda.device(self._handle_device):
            _lib.check(lib.pf_qwen3_generate(h, n_max, (C.c_int32 * max(1, len(eos)))(*eos), len(eos), int(pad), out, C.byref(n), stream_ptr()),
                       "pf_qwen3_generate")
        return torch.tensor(list(out), dtype=torch.int64).reshape(B, n_max)[:, : n.value]

    def generate(self, inputs_embeds, max_new_tokens: int = 512, eos_token_ids=None, pad_token_id=None) -> list:
        """greedy generation for any number of sequences (slices of 16): a list of id lists, each as the sequence gets alone -- cut
        behind its first eos id, the pad ids of the batch dropped"""
        eos = set(self.eos_token_ids if eos_token_ids is None else [int(e) for e in eos_token_ids])
        out = []
        for i in range(0, len(inputs_embeds), MAX_BATCH):
            self.prefill(inputs_embeds[i:i + MAX_BATCH], max_new_tokens)
            for row in self.greedy(max_new_tokens, eos_token_ids, pad_token_id).tolist():
                cut = next((k + 1 for k, t in enumerate(row) if t in eos), len(row))
                out.append(row[:cut])
        return out

    def debug_poison(self):
        lib, h = self._ensure_handle()
        with torch.cuda.device(self._handle_device):
            _lib.check(lib.pf_qwen3_debug_poison(h), "pf_qwen3_debug_poison")
        self._batch = 0
