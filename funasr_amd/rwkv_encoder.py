"""RWKV encoder on gfx950: `RWKVEncoder` (encoder_classes; funasr/models/rwkv_bat/rwkv_encoder.py), the encoder of the reference's
only Transducer template (funasr/models/rwkv_bat/template.yaml).

The VGG front `RWKVConvInput` at `subsampling_factor: 4` (six 3x3 convs + ReLU, an output linear), `embed_norm`, `num_blocks` blocks of
time mix (token shift, the WKV recurrence, a receptance gate) and channel mix (token shift, a relu^2 feed-forward, a receptance gate),
`final_norm`, then every `time_reduction_factor`-th frame. One `pf_rwkvencoder` handle (csrc/engine_rwkv.hip): the reference walks
frame by frame through every block at inference; here only the WKV recurrence itself keeps that order, as a chunked scan
(csrc/rwkv.hip), and everything else runs over all frames at once. fp32 throughout.

The state dict has the reference's keys and shapes (`time_mix_*` are [1, 1, D]).

Beyond the reference: it handles one clip per call (`rwkv_infer` raises a shape error at B = 2); a batch here is "each clip as the
reference computes it alone", bit for bit what the clip gets in a call of its own.

Not built (each refused by name): `subsampling_factor` other than 4, `kernel` other than 3, `attention_size` different from
`output_size` (the reference allocates its state `output_size` wide, so it cannot run that either), sizes off the ranges below,
`precision` f16x2 / bf16 (the operands of proj_output and proj_value have no a-priori bound). Constructor keys other than the
reference's own are refused: the reference swallows them in **kwargs and silently builds another geometry.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .hip_module import HipModule, Holder, ParamHolder, layer_norm, linear, stream_ptr
from .register import tables

# the reference constructor's own arguments (rwkv_encoder.py:36-51)
CONF_KEYS = ("input_size", "output_size", "context_size", "linear_size", "attention_size", "num_blocks", "att_dropout_rate",
             "ffn_dropout_rate", "dropout_rate", "subsampling_factor", "time_reduction_factor", "kernel")
MAX_D, MAX_LINEAR = 1024, 4096


def foreign_keys(conf) -> list:
    """the keys of an encoder_conf that RWKVEncoder's constructor does not name"""
    return sorted(k for k in (conf or {}) if k not in CONF_KEYS and k != "precision")


def subsampled_length(n: int, time_reduction_factor: int = 1) -> int:
    """output frames of a clip of n feature frames: ceil(ceil(n / 2) / 2) after the front, then floor((. - 1) / r) + 1"""
    t2 = ((int(n) + 1) // 2 + 1) // 2
    return (t2 - 1) // int(time_reduction_factor) + 1


def channels_last_output_weight(weight: torch.Tensor, channels: int) -> torch.Tensor:
    """`embed.output.weight` [D, C F2] with its columns moved from the reference's flattening `transpose(1, 2).view(b, t, c * f)`
    (column c F2 + f) to the channels-last order of the HIP convs (column f C + c). The handle does this once at load
    (csrc/engine_rwkv.hip); this is the same permutation for tests and tools."""
    D, K = weight.shape
    return weight.reshape(D, channels, K // channels).transpose(1, 2).reshape(D, K).contiguous()


class _Vec(nn.Module):
    """time_decay / time_first / time_mix_* under the reference's names; never executed"""

    def __init__(self, names, shape):
        super().__init__()
        for n in names:
            setattr(self, n, nn.Parameter(torch.zeros(*shape), requires_grad=False))


@tables.register("encoder_classes", "RWKVEncoder")
class RWKVEncoder(HipModule):
    _prefix = "pf_rwkvencoder"

    def __init__(self, input_size: int, output_size: int = 512, context_size: int = 1024, linear_size: int = None,
                 attention_size: int = None, num_blocks: int = 4, att_dropout_rate: float = 0.0, ffn_dropout_rate: float = 0.0,
                 dropout_rate: float = 0.0, subsampling_factor: int = 4, time_reduction_factor: int = 1, kernel: int = 3,
                 precision: str = None, **kwargs):
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"RWKVEncoder(HIP): encoder_conf keys {sorted(kwargs)} are not the reference constructor's "
                                      f"({', '.join(CONF_KEYS)}); the reference ignores them and builds another geometry")
        D = int(output_size)
        H = 4 * D if linear_size is None else int(linear_size)
        A = D if attention_size is None else int(attention_size)
        refusals = [
            (int(subsampling_factor) != 4, f"subsampling_factor: {subsampling_factor} (only 4)"),
            (int(kernel) != 3, f"kernel: {kernel} (only 3)"),
            (A != D, f"attention_size: {attention_size} with output_size {output_size} (the reference allocates its WKV state "
                     "output_size wide, so only attention_size == output_size runs there or here)"),
            (D < 32 or D % 32 != 0 or D > MAX_D, f"output_size: {output_size} (a multiple of 32 up to {MAX_D})"),
            (H < 32 or H % 32 != 0 or H > MAX_LINEAR, f"linear_size: {H} (a multiple of 32 up to {MAX_LINEAR})"),
            (not 8 <= int(input_size) <= 256 or int(input_size) % 4 != 0, f"input_size: {input_size} (a multiple of 4 from 8 to 256)"),
            (int(num_blocks) < 1, f"num_blocks: {num_blocks} (at least 1)"),
            (int(time_reduction_factor) < 1, f"time_reduction_factor: {time_reduction_factor} (at least 1)"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"RWKVEncoder(HIP): {why} is not built")
        self.set_precision(precision)
        self.input_size, self._output_size, self.linear_size, self.num_blocks = int(input_size), D, H, int(num_blocks)
        self.context_size, self.subsampling_factor, self.time_reduction_factor = int(context_size), 4, int(time_reduction_factor)
        embed = Holder()
        conv = nn.Module()
        chans = (1, D // 4, D // 4, D // 2, D // 2, D, D)
        for i in range(6):
            conv.add_module(str(2 * i), ParamHolder((chans[i + 1], chans[i], 3, 3), (chans[i + 1],)))
        embed.conv = conv
        embed.output = linear(D, D * (self.input_size // 4))
        self.embed = embed
        blocks = nn.ModuleList()
        for _ in range(self.num_blocks):
            b = Holder()
            b.layer_norm_att, b.layer_norm_ffn = layer_norm(D), layer_norm(D)
            att = _Vec(("time_decay", "time_first"), (D,))
            for n in ("time_mix_key", "time_mix_value", "time_mix_receptance"):
                setattr(att, n, nn.Parameter(torch.zeros(1, 1, D), requires_grad=False))
            att.proj_key, att.proj_value, att.proj_receptance, att.proj_output = linear(D, D), linear(D, D), linear(D, D), linear(D, D)
            ffn = _Vec(("time_mix_key", "time_mix_receptance"), (1, 1, D))
            ffn.proj_key, ffn.proj_value, ffn.proj_receptance = linear(H, D), linear(D, H), linear(D, D)
            b.att, b.ffn = att, ffn
            blocks.append(b)
        self.rwkv_blocks = blocks
        self.embed_norm, self.final_norm = layer_norm(D), layer_norm(D)
        for p in self.parameters():
            p.requires_grad_(False)

    def output_size(self) -> int:
        return self._output_size

    def set_precision(self, mode=None):
        """None or "fp32": the encoder has one arithmetic"""
        if mode not in (None, "fp32"):
            raise NotImplementedError(f"RWKVEncoder(HIP): precision: {mode} is not built (only fp32: the operands of proj_output and "
                                      "proj_value have no a-priori bound for the two-plane fp16 form)")
        self.precision = "fp32"
        return self

    def _make_config(self):
        c = _lib.pf_rwkvencoder_config()
        c.input_dim, c.d_model, c.linear_size, c.n_blocks = self.input_size, self._output_size, self.linear_size, self.num_blocks
        c.time_reduction, c.ln_eps = self.time_reduction_factor, 1e-12
        return c

    def _check_length(self, length: int):
        if length > self.context_size * self.subsampling_factor:      # the reference's assert (rwkv_encoder.py:110-115)
            raise ValueError("Context size is too short for current length: %d versus %d" % (length, self.context_size * self.subsampling_factor))

    def forward(self, xs_pad: torch.Tensor, ilens):
        """xs_pad [B, L, input_size], ilens [B] -> (out [B, T, D], olens [B] int64 on the device, None); every clip at its own length,
        rows at or past olens[b] zero"""
        out, olens, _ = self._run(xs_pad, ilens, False)
        return out, olens, None

    def forward_stages(self, xs_pad: torch.Tensor, ilens):
        """tests: (out, olens, [front, embed_norm, block 0 ..]), the stages [B, T2, D] each as the handle computed them on the way"""
        return self._run(xs_pad, ilens, True)

    def _run(self, xs_pad, ilens, stages: bool):
        lens = [int(v) for v in (ilens.tolist() if isinstance(ilens, torch.Tensor) else ilens)]
        B, L = int(xs_pad.shape[0]), int(xs_pad.shape[1])
        self._check_length(L)
        if len(lens) != B or L < 1 or any(n < 1 or n > L for n in lens):
            raise ValueError(f"RWKVEncoder: lengths {lens} for a batch of {B} clips padded to {L} frames")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = xs_pad.to(device=dev, dtype=torch.float32).contiguous()
        T = subsampled_length(L, self.time_reduction_factor)
        out = torch.empty(B, T, self._output_size, device=dev)
        ln = (_lib.C.c_int32 * B)(*lens)
        ol = (_lib.C.c_int32 * B)()
        taps = None
        with torch.cuda.device(dev):
            if stages:
                taps = [torch.zeros(B, subsampled_length(L), self._output_size, device=dev) for _ in range(self.num_blocks + 2)]
                ptrs = (_lib.C.c_void_p * len(taps))(*[t.data_ptr() for t in taps])
                rc = lib.pf_rwkvencoder_forward_stages(h, x.data_ptr(), ln, B, L, out.data_ptr(), ol, ptrs, stream_ptr())
            else:
                rc = lib.pf_rwkvencoder_forward(h, x.data_ptr(), ln, B, L, out.data_ptr(), ol, stream_ptr())
            _lib.check(rc, "pf_rwkvencoder_forward")
            torch.cuda.current_stream(dev).synchronize()           # the lengths are staged asynchronously
        return out, torch.tensor(list(ol), dtype=torch.int64, device=dev), taps

    def debug_poison(self):
        lib, h = self._ensure_handle()
        with torch.cuda.device(self._handle_device):
            _lib.check(lib.pf_rwkvencoder_debug_poison(h), "pf_rwkvencoder_debug_poison")
