"""Restatement of the reference's ConformerChunkEncoder (funasr/models/conformer/encoder.py:914) in plain torch, in the dtype of its
inputs: the float64 oracle of tests/test_chunk_conformer*.py. State-dict keys are the reference's, below `prefix`. Every function
follows the reference's own order of operations; none of its code is used."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

SUB = {2: (3, 1), 4: (3, 2), 6: (5, 3)}


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def window(i: int, size: int, chunk: int, left: int):
    """keys [start, end) of query i under make_chunk_mask (nets_utils.py:614); chunk 0: all"""
    if not chunk:
        return 0, size
    ci = i // chunk
    return (0 if left < 0 else max((ci - left) * chunk, 0)), min((ci + 1) * chunk, size)


def visible(T: int, klen: int, chunk: int, left: int) -> torch.Tensor:
    """[T, T] bool: query i sees key j"""
    m = torch.zeros(T, T, dtype=torch.bool)
    for i in range(T):
        s, e = window(i, T, chunk, left)
        m[i, s:min(e, klen)] = True
    return m


def front_length(n: int, factor: int) -> int:
    s2 = SUB[factor][1]
    return ((n + 1) // 2 + s2 - 1) // s2


def front(sd, x, factor: int, chunk: int = 0, prefix: str = ""):
    """StreamingConvInput, vgg_like False: x [B, L, F] -> [B, front_length(L), D]"""
    k2, s2 = SUB[factor]
    B, L, Fd = x.shape
    T = front_length(L, factor)
    if chunk:
        piece = chunk * factor
        n = -(-L // piece)
        x = F.pad(x, (0, 0, 0, n * piece - L)).reshape(B * n, piece, Fd)
    y = F.relu(F.conv2d(x[:, None], sd[prefix + "embed.conv.0.weight"], sd[prefix + "embed.conv.0.bias"], stride=2, padding=(1, 0)))
    y = F.relu(F.conv2d(y, sd[prefix + "embed.conv.2.weight"], sd[prefix + "embed.conv.2.bias"], stride=s2, padding=((k2 - 1) // 2, 0)))
    _, c, _, f = y.shape
    y = y.transpose(1, 2).contiguous().view(B, -1, c * f)[:, :T]
    return F.linear(y, sd[prefix + "embed.output.weight"], sd[prefix + "embed.output.bias"])


def pos_rows(D: int, T: int, dtype):
    """the 2 T - 1 rows StreamingRelPositionalEncoding hands a forward over T frames: row k = position T - 1 - k, built in float32"""
    from funasr_amd.conformer import MAX_LEN, latest_rel_pos_table

    return latest_rel_pos_table(D)[MAX_LEN - T: MAX_LEN + T - 1].to(dtype)


def window_attention(qkv, P, u, v, klens, chunk: int, left: int, H: int):
    """qkv [B, T, 3 D], P [2 T - 1, D] (= linear_pos of pos_rows), u, v [H, d] -> [B, T, D] before linear_out. Only visible (query,
    key) pairs are touched, so NaN elsewhere in K / V / P cannot reach the result; rows without a visible key are zeros."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    d = D // H
    out = torch.zeros(B, T, D, dtype=qkv.dtype)
    q, k, val = (qkv[..., j * D:(j + 1) * D].reshape(B, T, H, d) for j in range(3))
    Ph = P.reshape(-1, H, d)
    for b in range(B):
        for i in range(T):
            s, e = window(i, T, chunk, left)
            e = min(e, int(klens[b]))
            if e <= s:
                continue
            ac = torch.einsum("hd,jhd->hj", q[b, i] + u, k[b, s:e])
            bd = torch.einsum("hd,jhd->hj", q[b, i] + v, Ph[T - 1 - i + s: T - 1 - i + e])
            p = torch.softmax((ac + bd) / math.sqrt(d), dim=-1)
            out[b, i] = torch.einsum("hj,jhd->hd", p, val[b, s:e]).reshape(D)
    return out


def glu_dw(g, dw, dw_bias, bn_scale, bn_shift, causal: bool):
    """g [B, T, 2 D] -> GLU, depthwise conv (dw [D, taps]), scale / shift, Swish -> [B, T, D]"""
    D, taps = dw.shape
    x = F.glu(g.transpose(1, 2), dim=1)
    x = F.pad(x, (taps - 1, 0) if causal else (taps // 2, taps // 2))
    z = F.conv1d(x, dw[:, None], dw_bias, groups=D) * bn_scale[:, None] + bn_shift[:, None]
    return (z * torch.sigmoid(z)).transpose(1, 2)


def _ln(sd, p, x):
    return F.layer_norm(x, x.shape[-1:], sd[p + "weight"], sd[p + "bias"], 1e-12)


def _ffn(sd, p, x):
    h = F.linear(x, sd[p + "w_1.weight"], sd[p + "w_1.bias"])
    return F.linear(h * torch.sigmoid(h), sd[p + "w_2.weight"], sd[p + "w_2.bias"])


def block(sd, p, x, pos, klens, chunk, left, H, causal, bn_eps):
    """ChunkEncoderLayer.forward over x [B, T, D]"""
    D = x.shape[-1]
    x = x + 0.5 * _ffn(sd, p + "feed_forward_macaron.", _ln(sd, p + "norm_macaron.", x))
    xn = _ln(sd, p + "norm_self_att.", x)
    a = p + "self_att."
    qkv = torch.cat([F.linear(xn, sd[a + f"linear_{n}.weight"], sd[a + f"linear_{n}.bias"]) for n in "qkv"], dim=-1)
    att = window_attention(qkv, F.linear(pos, sd[a + "linear_pos.weight"]), sd[a + "pos_bias_u"], sd[a + "pos_bias_v"], klens, chunk, left, H)
    x = x + F.linear(att, sd[a + "linear_out.weight"], sd[a + "linear_out.bias"])
    c = p + "conv_mod."
    g = F.linear(_ln(sd, p + "norm_conv.", x), sd[c + "pointwise_conv1.weight"][:, :, 0], sd[c + "pointwise_conv1.bias"])
    scale = sd[c + "norm.weight"] / torch.sqrt(sd[c + "norm.running_var"] + bn_eps)
    shift = sd[c + "norm.bias"] - sd[c + "norm.running_mean"] * scale
    z = glu_dw(g, sd[c + "depthwise_conv.weight"][:, 0], sd[c + "depthwise_conv.bias"], scale, shift, causal)
    x = x + F.linear(z, sd[c + "pointwise_conv2.weight"][:, :, 0], sd[c + "pointwise_conv2.bias"])
    x = x + 0.5 * _ffn(sd, p + "feed_forward.", _ln(sd, p + "norm_feed_forward.", x))
    return _ln(sd, p + "norm_final.", x)


def encoder(sd, x, lens, conf: dict, chunk: int, masked: bool, prefix: str = ""):
    """x [B, L, F], lens -> {"front", "blocks": [...], "norm_blocks", "out", "olens"}: the chunked front when chunk > 0, the chunk mask
    when `masked`; the conv is causal when the conf sets one of the two training flags"""
    factor, r = int(conf["subsampling_factor"]), int(conf.get("time_reduction_factor", 1))
    H, left = int(conf["attention_heads"]), int(conf.get("left_chunk_size", 0))
    causal = bool(conf.get("dynamic_chunk_training", False) or conf.get("unified_model_training", False))
    eps = float(conf.get("conv_mod_norm_eps", 1e-5))
    klens = [front_length(int(n), factor) for n in lens]
    e = front(sd, x, factor, chunk, prefix)
    res = {"front": e, "blocks": []}
    pos = pos_rows(e.shape[-1], e.shape[1], e.dtype)
    y = e
    for i in range(int(conf["num_blocks"])):
        y = block(sd, f"{prefix}encoders.blocks.{i}.", y, pos, klens, chunk if masked else 0, left, H, causal, eps)
        res["blocks"].append(y)
    y = _ln(sd, prefix + "encoders.norm_blocks.", y)
    res["norm_blocks"] = y
    res["out"] = y[:, ::r]
    res["olens"] = [(k - 1) // r + 1 for k in klens]
    return res
