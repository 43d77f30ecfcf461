"""Chunk Conformer encoder on gfx950: `ChunkConformerEncoder` (encoder_classes; funasr/models/conformer/encoder.py:914, class
ConformerChunkEncoder), the encoder of the reference's streaming / unified RNN-T recipes.

A Conformer whose self-attention is chunk-masked (`RelPositionMultiHeadedAttentionChunk` under `make_chunk_mask`), whose convolution
module is causal when one of the two training flags is set (`CausalConvolution`), whose front is `StreamingConvInput` at 1/2, 1/4 or
1/6 subsampling (with a chunk size every chunk is convolved on its own), and which ends in `norm_blocks` and every
`time_reduction_factor`-th frame. One `pf_chunkconformer` handle (csrc/engine_chunk_conformer.hip); the hot kernel is the window
attention of csrc/chunk_conformer.hip, which walks only the key tiles inside a query tile's window. fp32 throughout.

The three forward modes are the reference's (encoder.py:1069-1168), in eval:
  * neither flag:              (x, olens, None), full attention, symmetric conv, un-chunked front;
  * `dynamic_chunk_training`:  (x, olens, None), chunk size `default_chunk_size`: chunked front, chunk mask, causal conv;
  * `unified_model_training`:  (x_utt, x_chunk, olens), both over the chunked front with causal convs, x_utt without the chunk mask.
`simu_chunk_forward` is the chunked path at the call's chunk size. `forward_utt` runs the unified mode's utt branch alone.

The state dict has the reference's keys and shapes, BatchNorm statistics included. The positional table is the repository's "latest"
table (StreamingRelPositionalEncoding builds the same rows), made on the host in float32.

Not built (each refused by name): `embed_vgg_like: true` (fails inside the reference itself), `subsampling_factor: 1`,
`simplified_att_score: true`, a head dim other than 64, `cnn_module_kernel` even or above 31, `linear_units` off a multiple of 32,
activations other than swish, `positionwise_layer_type` other than linear, `normalize_before: false`, `concat_after: true`,
`zero_triu: true`, `use_cnn_module: false`, `pos_enc_layer_type` / `selfattention_layer_type` other than the defaults,
`time_reduction_factor < 1`, `default_chunk_size < 1`, `precision` other than fp32 (the front's GEMMs take the caller's features, for
which no a-priori bound exists, and a second arithmetic for the blocks alone is not offered), constructor keys the reference's
constructor does not name, and a batch padded beyond its longest clip (the reference's masks then disagree in length). The
cache-carrying `chunk_forward` does not exist here.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .conformer import MAX_LEN, _attention, _ffn, latest_rel_pos_table
from .hip_module import HipModule, Holder, ParamHolder, _truthy, layer_norm, linear, stream_ptr
from .register import tables

# the reference constructor's own arguments (conformer/encoder.py:924-960)
CONF_KEYS = ("input_size", "output_size", "attention_heads", "linear_units", "num_blocks", "dropout_rate", "positional_dropout_rate",
             "attention_dropout_rate", "embed_vgg_like", "normalize_before", "concat_after", "positionwise_layer_type",
             "positionwise_conv_kernel_size", "macaron_style", "rel_pos_type", "pos_enc_layer_type", "selfattention_layer_type",
             "activation_type", "use_cnn_module", "zero_triu", "norm_type", "cnn_module_kernel", "conv_mod_norm_eps",
             "conv_mod_norm_momentum", "simplified_att_score", "dynamic_chunk_training", "short_chunk_threshold", "short_chunk_size",
             "left_chunk_size", "time_reduction_factor", "unified_model_training", "default_chunk_size", "jitter_range",
             "subsampling_factor")
_SUB = {2: (3, 1), 4: (3, 2), 6: (5, 3)}                  # sub_factor_to_params: (kernel, stride) of the second conv


def foreign_keys(conf) -> list:
    """the keys of an encoder_conf that ConformerChunkEncoder's constructor does not name"""
    return sorted(k for k in (conf or {}) if k not in CONF_KEYS and k != "precision")


def front_length(n: int, subsampling_factor: int) -> int:
    """encoder frames of n feature frames: the mask rule mask[:, ::2][:, ::s2], which is also the convs' row count"""
    s2 = _SUB[int(subsampling_factor)][1]
    return ((int(n) + 1) // 2 + s2 - 1) // s2


def subsampled_length(n: int, subsampling_factor: int, time_reduction_factor: int = 1) -> int:
    """output frames of a clip of n feature frames: floor((front_length - 1) / r) + 1"""
    return (front_length(n, subsampling_factor) - 1) // int(time_reduction_factor) + 1


def chunk_window(i: int, size: int, chunk_size: int, left_chunk_size: int):
    """the keys [start, end) query i sees under make_chunk_mask(size, chunk_size, left_chunk_size) (nets_utils.py:614); chunk_size 0: all.
    The code decides, not its docstring: left_chunk_size 0 is the own chunk only, a negative one all of the past."""
    if not chunk_size:
        return 0, size
    ci = i // chunk_size
    start = 0 if left_chunk_size < 0 else max((ci - left_chunk_size) * chunk_size, 0)
    return start, min((ci + 1) * chunk_size, size)


@tables.register("encoder_classes", "ChunkConformerEncoder")
class ChunkConformerEncoder(HipModule):
    _prefix = "pf_chunkconformer"
    _push_buffers = True

    def __init__(self, input_size: int, output_size: int = 256, attention_heads: int = 4, linear_units: int = 2048, num_blocks: int = 6,
                 dropout_rate: float = 0.1, positional_dropout_rate: float = 0.1, attention_dropout_rate: float = 0.0,
                 embed_vgg_like: bool = False, normalize_before: bool = True, concat_after: bool = False,
                 positionwise_layer_type: str = "linear", positionwise_conv_kernel_size: int = 3, macaron_style: bool = False,
                 rel_pos_type: str = "legacy", pos_enc_layer_type: str = "rel_pos", selfattention_layer_type: str = "rel_selfattn",
                 activation_type: str = "swish", use_cnn_module: bool = True, zero_triu: bool = False, norm_type: str = "layer_norm",
                 cnn_module_kernel: int = 31, conv_mod_norm_eps: float = 0.00001, conv_mod_norm_momentum: float = 0.1,
                 simplified_att_score: bool = False, dynamic_chunk_training: bool = False, short_chunk_threshold: float = 0.75,
                 short_chunk_size: int = 25, left_chunk_size: int = 0, time_reduction_factor: int = 1,
                 unified_model_training: bool = False, default_chunk_size: int = 16, jitter_range: int = 4, subsampling_factor: int = 1,
                 precision: str = None, **kwargs):
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"ChunkConformerEncoder(HIP): encoder: ChunkConformerEncoder does not take encoder_conf keys "
                                      f"{sorted(kwargs)} (the reference constructor's are {', '.join(CONF_KEYS)}; it raises TypeError)")
        D, H = int(output_size), int(attention_heads)
        refusals = [
            (_truthy(embed_vgg_like), "embed_vgg_like: true (the reference's own forward fails on it)"),
            (int(subsampling_factor) not in _SUB, f"subsampling_factor: {subsampling_factor} (only 2, 4 or 6)"),
            (_truthy(simplified_att_score), "simplified_att_score: true"),
            (pos_enc_layer_type != "rel_pos", f"pos_enc_layer_type: {pos_enc_layer_type} (only rel_pos)"),
            (selfattention_layer_type != "rel_selfattn", f"selfattention_layer_type: {selfattention_layer_type} (only rel_selfattn)"),
            (not _truthy(normalize_before), "normalize_before: false"),
            (_truthy(concat_after), "concat_after: true"),
            (positionwise_layer_type != "linear", f"positionwise_layer_type: {positionwise_layer_type} (only linear)"),
            (activation_type != "swish", f"activation_type: {activation_type} (only swish)"),
            (not _truthy(use_cnn_module), "use_cnn_module: false"),
            (_truthy(zero_triu), "zero_triu: true"),
            (int(cnn_module_kernel) % 2 != 1 or not 1 <= int(cnn_module_kernel) <= 31, f"cnn_module_kernel: {cnn_module_kernel} (odd, at most 31)"),
            (H < 1 or D != 64 * H or D > 2048, f"attention_heads: {attention_heads} with output_size {output_size} (only a head dim of 64 is built, "
                                               "output_size up to 2048)"),
            (int(linear_units) < 32 or int(linear_units) % 32 != 0, f"linear_units: {linear_units} (a multiple of 32)"),
            (not 16 <= int(input_size) <= 256, f"input_size: {input_size} (16 .. 256 features)"),
            (int(num_blocks) < 1, f"num_blocks: {num_blocks} (at least 1)"),
            (int(time_reduction_factor) < 1, f"time_reduction_factor: {time_reduction_factor} (at least 1)"),
            (int(default_chunk_size) < 1, f"default_chunk_size: {default_chunk_size} (at least 1)"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"ChunkConformerEncoder(HIP): {why} is not built")
        self.set_precision(precision)
        self.input_size, self._output_size, self.attention_heads, self.linear_units = int(input_size), D, H, int(linear_units)
        self.num_blocks, self.kernel, self.subsampling_factor = int(num_blocks), int(cnn_module_kernel), int(subsampling_factor)
        self.conv_mod_norm_eps = float(conv_mod_norm_eps)
        self.dynamic_chunk_training, self.unified_model_training = _truthy(dynamic_chunk_training), _truthy(unified_model_training)
        self.left_chunk_size, self.default_chunk_size = int(left_chunk_size), int(default_chunk_size)
        self.time_reduction_factor = int(time_reduction_factor)
        self.short_chunk_threshold, self.short_chunk_size, self.jitter_range = short_chunk_threshold, short_chunk_size, jitter_range
        k2, s2 = _SUB[self.subsampling_factor]
        f2 = ((self.input_size - 1) // 2 - k2) // s2 + 1
        embed = Holder()
        conv = nn.Module()
        conv.add_module("0", ParamHolder((D, 1, 3, 3), (D,)))
        conv.add_module("2", ParamHolder((D, D, k2, k2), (D,)))
        embed.conv = conv
        embed.output = linear(D, D * f2)
        self.embed = embed
        blocks = nn.ModuleList()
        for _ in range(self.num_blocks):
            b = Holder()
            b.self_att = _attention(D, rel=True)
            b.feed_forward = _ffn(D, self.linear_units)
            b.feed_forward_macaron = _ffn(D, self.linear_units)       # always there, whatever macaron_style says
            cm = Holder()
            cm.pointwise_conv1 = ParamHolder((2 * D, D, 1), (2 * D,))
            cm.depthwise_conv = ParamHolder((D, 1, self.kernel), (D,))
            cm.norm = nn.BatchNorm1d(D, eps=self.conv_mod_norm_eps, momentum=conv_mod_norm_momentum)   # a holder: eval-mode statistics
            cm.pointwise_conv2 = ParamHolder((D, D, 1), (D,))
            b.conv_mod = cm
            b.norm_feed_forward, b.norm_self_att = layer_norm(D), layer_norm(D)
            b.norm_macaron, b.norm_conv, b.norm_final = layer_norm(D), layer_norm(D), layer_norm(D)
            blocks.append(b)
        encoders = Holder()
        encoders.blocks = blocks
        encoders.norm_blocks = layer_norm(D)
        self.encoders = encoders
        for p in self.parameters():
            p.requires_grad_(False)
        self.pos_table = latest_rel_pos_table(D)                       # not in the state dict (the reference keeps `pe` as an attribute)

    def output_size(self) -> int:
        return self._output_size

    def _extra_tensors(self):
        return (("pos_table", self.pos_table),)

    def set_precision(self, mode=None):
        """None or "fp32": the encoder has one arithmetic"""
        if mode not in (None, "fp32"):
            raise NotImplementedError(f"ChunkConformerEncoder(HIP): precision: {mode} is not built (only fp32: the front's operands are the "
                                      "caller's features, for which no a-priori bound exists)")
        self.precision = "fp32"
        return self

    def _make_config(self):
        c = _lib.pf_chunkconformer_config()
        c.input_dim, c.d_model, c.n_heads, c.ffn_dim = self.input_size, self._output_size, self.attention_heads, self.linear_units
        c.n_blocks, c.kernel_size, c.subsampling = self.num_blocks, self.kernel, self.subsampling_factor
        c.causal_conv = int(self.dynamic_chunk_training or self.unified_model_training)
        c.left_chunk, c.time_reduction = self.left_chunk_size, self.time_reduction_factor
        c.ln_eps, c.bn_eps = 1e-12, self.conv_mod_norm_eps
        return c

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, xs_pad: torch.Tensor, ilens):
        """xs_pad [B, L, input_size] zero-padded features, ilens [B] -> what the reference returns in the encoder's mode:
        (x, olens, None), or (x_utt, x_chunk, olens) with unified_model_training"""
        if self.unified_model_training:
            (x_utt, x_chunk), olens, _ = self._run(xs_pad, ilens, self.default_chunk_size, 3)
            return x_utt, x_chunk, olens
        if self.dynamic_chunk_training:
            (_, x), olens, _ = self._run(xs_pad, ilens, self.default_chunk_size, 2)
        else:
            (x, _), olens, _ = self._run(xs_pad, ilens, 0, 1)
        return x, olens, None

    def forward_utt(self, xs_pad: torch.Tensor, ilens):
        """what decoding needs: (x, olens) -- in unified mode the utt branch ALONE (x_chunk is not computed), else forward's x"""
        if self.unified_model_training:
            (x, _), olens, _ = self._run(xs_pad, ilens, self.default_chunk_size, 1)
            return x, olens
        x, olens, _ = self.forward(xs_pad, ilens)
        return x, olens

    def simu_chunk_forward(self, xs_pad: torch.Tensor, ilens, chunk_size: int = 16, left_context: int = 32, right_context: int = 0):
        """encoder.py:1207-1255: the chunked front and the chunk mask at the CALL's chunk size (left_chunk_size is the config's; the
        two context arguments are unused there as here) -> x"""
        if int(chunk_size) < 1:
            raise ValueError(f"simu_chunk_forward: chunk_size {chunk_size} must be positive")
        (_, x), _, _ = self._run(xs_pad, ilens, int(chunk_size), 2)
        return x

    def forward_stages(self, xs_pad: torch.Tensor, ilens, chunk_size: int, branch: str):
        """tests: (out, olens, [front, block 0 .., norm_blocks]) of ONE branch ("utt": no chunk mask, "chunk": masked), each stage
        [B, T, D] before the time reduction, as the handle computed it on the way"""
        (u, c), olens, taps = self._run(xs_pad, ilens, int(chunk_size), 1 if branch == "utt" else 2, True)
        return (u if branch == "utt" else c), olens, taps

    def front(self, xs_pad: torch.Tensor, chunk_size: int = 0):
        """tests: the front alone -> [B, front_length(L), D]"""
        B, L = int(xs_pad.shape[0]), int(xs_pad.shape[1])
        self._check_length(L)
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = xs_pad.to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty(B, front_length(L, self.subsampling_factor), self._output_size, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.pf_chunkconformer_front(h, x.data_ptr(), B, L, int(chunk_size), out.data_ptr(), stream_ptr()), "pf_chunkconformer_front")
        return out

    def _check_length(self, L: int):
        # no TooShortUttError: the reference calls subsampling.check_short_utt (an isinstance test of Conv2dSubsampling modules) with
        # the integer factor, which never says "too short"; its convs pad in time, so one frame gives one frame
        if L < 1:
            raise ValueError("ChunkConformerEncoder: an empty batch")
        if front_length(L, self.subsampling_factor) > MAX_LEN:
            raise ValueError(f"ChunkConformerEncoder: {front_length(L, self.subsampling_factor)} encoder frames in one batch; the positional "
                             f"table holds {MAX_LEN}. Split the input")

    def _run(self, xs_pad, ilens, chunk: int, branches: int, stages: bool = False):
        lens = [int(v) for v in (ilens.tolist() if isinstance(ilens, torch.Tensor) else ilens)]
        B, L = int(xs_pad.shape[0]), int(xs_pad.shape[1])
        self._check_length(L)
        if len(lens) != B or any(n < 1 or n > L for n in lens):
            raise ValueError(f"ChunkConformerEncoder: lengths {lens} for a batch of {B} clips padded to {L} frames")
        if max(lens) != L:
            raise NotImplementedError(f"ChunkConformerEncoder(HIP): a batch padded to {L} frames whose longest clip has {max(lens)} is not built "
                                      "(the reference's source mask is then shorter than its rows); pad to the longest clip")
        lib, h = self._ensure_handle()
        dev = self._handle_device
        x = xs_pad.to(device=dev, dtype=torch.float32).contiguous()
        T2 = front_length(L, self.subsampling_factor)
        T = (T2 - 1) // self.time_reduction_factor + 1
        outs = [torch.empty(B, T, self._output_size, device=dev) if branches & bit else None for bit in (1, 2)]
        ln = (_lib.C.c_int32 * B)(*lens)
        ol = (_lib.C.c_int32 * B)()
        taps, ptrs = None, None
        with torch.cuda.device(dev):
            if stages:
                taps = [torch.zeros(B, T2, self._output_size, device=dev) for _ in range(self.num_blocks + 2)]
                ptrs = (_lib.C.c_void_p * len(taps))(*[t.data_ptr() for t in taps])
            rc = lib.pf_chunkconformer_forward(h, x.data_ptr(), ln, B, L, int(chunk), int(branches),
                                               outs[0].data_ptr() if outs[0] is not None else None,
                                               outs[1].data_ptr() if outs[1] is not None else None, ol, ptrs, stream_ptr())
            _lib.check(rc, "pf_chunkconformer_forward")
            torch.cuda.current_stream(dev).synchronize()           # the lengths are staged asynchronously
        return outs, torch.tensor(list(ol), dtype=torch.int64, device=dev), taps

    def debug_poison(self):
        lib, h = self._ensure_handle()
        with torch.cuda.device(self._handle_device):
            _lib.check(lib.pf_chunkconformer_debug_poison(h), "pf_chunkconformer_debug_poison")
