"""Torch restatement of the reference's RWKVEncoder (funasr/models/rwkv_bat) for the tests: parallel in time where the reference
walks frame by frame -- the front through conv2d, the blocks over all frames at once -- with the WKV as the sequential recurrence it
is. Works in any dtype, on any device, for single clips and ragged batches ("each clip as the reference computes it alone").
tests/test_rwkv.py checks it against the reference's own recorded stages (tests/golden/rwkv.npz)."""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn.functional as F

EPS = 1e-12                      # funasr/models/transformer/layer_norm.py LayerNorm
STRIDES = ((1, 1), (2, 2), (1, 1), (2, 2), (1, 1), (1, 1))


def cast(sd: Dict[str, torch.Tensor], dtype, device=None) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype=dtype, device=device) for k, v in sd.items()}


def num_blocks(sd, prefix: str = "") -> int:
    return 1 + max(int(k[len(prefix):].split(".")[1]) for k in sd if k.startswith(prefix + "rwkv_blocks."))


def olens(n: int, r: int = 1) -> int:
    t2 = ((n + 1) // 2 + 1) // 2
    return (t2 - 1) // r + 1


def wkv(k: torch.Tensor, v: torch.Tensor, w: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """the recurrence of rwkv_attention.py:421-462 over k, v [T, D] with w = -exp(time_decay), u = time_first and the initial state
    (0, 0, -1e-30) of rwkv_encoder.py:155"""
    T, D = k.shape
    num, den = torch.zeros(D, dtype=k.dtype, device=k.device), torch.zeros(D, dtype=k.dtype, device=k.device)
    m = torch.full((D,), -1e-30, dtype=k.dtype, device=k.device)
    out = []
    for t in range(T):
        uk = u + k[t]
        mo = torch.maximum(m, uk)
        e1, e2 = torch.exp(m - mo), torch.exp(uk - mo)
        out.append((e1 * num + e2 * v[t]) / (e1 * den + e2))
        ms = torch.maximum(k[t], m + w)
        e1, e2 = torch.exp(m + w - ms), torch.exp(k[t] - ms)
        num, den, m = e1 * num + e2 * v[t], e1 * den + e2, ms
    return torch.stack(out)


def wkv_chunked(k: torch.Tensor, v: torch.Tensor, w: torch.Tensor, u: torch.Tensor, L: int) -> torch.Tensor:
    """the same values by the chunk algebra of csrc/rwkv.hip, in the tensors' dtype: every chunk of L frames summarised from the empty
    state (0, 0, -1e38); chunk c's carry = the summaries 0 .. c - 1 folded in order into the reference's initial state, each fold
    carry <- combine(carry decayed by w L, summary) with the same max trick; then the chunk re-run from its carry"""
    T, D = k.shape
    dt, dev = k.dtype, k.device

    def advance(num, den, m, kk, vv):
        ms = torch.maximum(kk, m + w)
        e1, e2 = torch.exp(m + w - ms), torch.exp(kk - ms)
        return e1 * num + e2 * vv, e1 * den + e2, ms

    sums = []
    for t0 in range(0, T, L):
        if t0 + L >= T:
            break
        num, den, m = torch.zeros(D, dtype=dt, device=dev), torch.zeros(D, dtype=dt, device=dev), torch.full((D,), -1e38, dtype=dt, device=dev)
        for t in range(t0, t0 + L):
            num, den, m = advance(num, den, m, k[t], v[t])
        sums.append((num, den, m))
    out = []
    for c, t0 in enumerate(range(0, T, L)):
        num, den, m = torch.zeros(D, dtype=dt, device=dev), torch.zeros(D, dtype=dt, device=dev), torch.full((D,), -1e-30, dtype=dt, device=dev)
        for a, d, q in sums[:c]:
            md = m + w * L
            mo = torch.maximum(md, q)
            e1, e2 = torch.exp(md - mo), torch.exp(q - mo)
            num, den, m = e1 * num + e2 * a, e1 * den + e2 * d, mo
        for t in range(t0, min(t0 + L, T)):
            uk = u + k[t]
            mo = torch.maximum(m, uk)
            e1, e2 = torch.exp(m - mo), torch.exp(uk - mo)
            out.append((e1 * num + e2 * v[t]) / (e1 * den + e2))
            num, den, m = advance(num, den, m, k[t], v[t])
    return torch.stack(out)


def layer_norm(x, sd, p):
    return F.layer_norm(x, x.shape[-1:], sd[p + "weight"], sd[p + "bias"], EPS)


def shift(y):
    """the previous frame's row, zero at frame 0"""
    return torch.cat([torch.zeros_like(y[:1]), y[:-1]])


def mix(y, mu):
    mu = mu.reshape(-1)
    return y * mu + shift(y) * (1 - mu)


def front(feats: torch.Tensor, sd, p: str = "") -> torch.Tensor:
    """RWKVConvInput at subsampling_factor 4: feats [T, F] -> [T2, D]"""
    x = feats[None, None]
    for i, st in enumerate(STRIDES):
        x = torch.relu(F.conv2d(x, sd[f"{p}embed.conv.{2 * i}.weight"], sd[f"{p}embed.conv.{2 * i}.bias"], stride=st, padding=1))
    _, c, t, f = x.shape
    x = x.transpose(1, 2).contiguous().view(t, c * f)
    return F.linear(x, sd[p + "embed.output.weight"], sd[p + "embed.output.bias"])


def time_mix(y, sd, p):
    k = F.linear(mix(y, sd[p + "time_mix_key"]), sd[p + "proj_key.weight"], sd[p + "proj_key.bias"])
    v = F.linear(mix(y, sd[p + "time_mix_value"]), sd[p + "proj_value.weight"], sd[p + "proj_value.bias"])
    r = torch.sigmoid(F.linear(mix(y, sd[p + "time_mix_receptance"]), sd[p + "proj_receptance.weight"], sd[p + "proj_receptance.bias"]))
    o = wkv(k, v, -torch.exp(sd[p + "time_decay"]), sd[p + "time_first"])
    return F.linear(r * o, sd[p + "proj_output.weight"], sd[p + "proj_output.bias"])


def channel_mix(y, sd, p):
    k = torch.square(torch.relu(F.linear(mix(y, sd[p + "time_mix_key"]), sd[p + "proj_key.weight"], sd[p + "proj_key.bias"])))
    val = F.linear(k, sd[p + "proj_value.weight"], sd[p + "proj_value.bias"])
    r = torch.sigmoid(F.linear(mix(y, sd[p + "time_mix_receptance"]), sd[p + "proj_receptance.weight"], sd[p + "proj_receptance.bias"]))
    return r * val


def encode(feats: torch.Tensor, sd, r: int = 1, p: str = "") -> Dict[str, object]:
    """one clip, feats [T, F] -> {"front", "embed_norm" [T2, D], "blocks": [[T2, D]], "out": [olens, D]}"""
    res = {"front": front(feats, sd, p)}
    x = layer_norm(res["front"], sd, p + "embed_norm.")
    res["embed_norm"] = x
    res["blocks"] = []
    for i in range(num_blocks(sd, p)):
        b = f"{p}rwkv_blocks.{i}."
        x = x + time_mix(layer_norm(x, sd, b + "layer_norm_att."), sd, b + "att.")
        x = x + channel_mix(layer_norm(x, sd, b + "layer_norm_ffn."), sd, b + "ffn.")
        res["blocks"].append(x)
    res["out"] = layer_norm(x, sd, p + "final_norm.")[::r]
    return res


def encode_batch(xs_pad: torch.Tensor, lens: List[int], sd, r: int = 1, p: str = ""):
    """a ragged batch [B, L, F]: every clip alone -> (out [B, olens(L), D] zero past a clip's length, olens list)"""
    outs = [encode(xs_pad[b, :n], sd, r, p)["out"] for b, n in enumerate(lens)]
    T = olens(int(xs_pad.shape[1]), r)
    out = torch.zeros(len(lens), T, outs[0].shape[-1], dtype=outs[0].dtype, device=outs[0].device)
    for b, o in enumerate(outs):
        out[b, : o.shape[0]] = o
    return out, [o.shape[0] for o in outs]
