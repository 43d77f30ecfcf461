"""Float64 / float32 restatement of E-Paraformer's predictor and decoder in plain torch (dtype-generic), written from the formulas:
parallel integrate-and-fire (funasr/models/e_paraformer/pif_predictor.py) and the one-pass SAN decoder (decoder.py ParaformerSANDecoder
with the layers of funasr/models/transformer/decoder.py). The encoder is tests/_conformer_oracle.py's."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as Fn

from ._conformer_oracle import _ffn, _lin, _ln, cast, encoder  # noqa: F401  (re-exported)


def pif_alphas(h, lens, conv_w, conv_b, out_w, out_b, l_order: int, r_order: int, smooth: float = 1.0, noise: float = 0.0):
    """h [B, T, D]; conv_w [D, 1, l + r + 1] -> (alphas [B, T] masked at t >= lens[b], token_num [B]). The depthwise conv is zero-padded
    l / r rows around the T rows of the padded batch and is NOT masked."""
    x = Fn.pad(h.transpose(1, 2), (l_order, r_order))
    y = Fn.conv1d(x, conv_w, conv_b, groups=h.shape[-1]).transpose(1, 2) + h
    z = Fn.linear(torch.relu(y), out_w.reshape(1, -1), out_b.reshape(1))[..., 0]
    a = torch.relu(torch.sigmoid(z) * smooth - noise)
    mask = torch.arange(h.shape[1])[None, :] < torch.as_tensor(lens)[:, None]
    a = a * mask.to(a.dtype)
    return a, a.sum(-1)


def pif_align(a, token_num, counts):
    """-> (normalised alphas, their inclusive prefix sums); a clip with a zero sum or count gets zeros (no division)"""
    n = torch.as_tensor(counts).to(a.dtype)
    ok = (token_num > 0) & (n > 0)
    r = torch.where(ok, n / torch.where(ok, token_num, torch.ones_like(token_num)), torch.zeros_like(token_num))
    an = a * r[:, None]
    return an, torch.cumsum(an, dim=-1)


def pif_embed(align, h, sigma, lens, L: int):
    """embeds [B, L, D]: per sigma head g, softmax over t < lens[b] of -((l + 0.5 - align[b, t]) sigma[g])^2, times the head's channel
    slice of h; zero rows for a clip without frames"""
    B, T, D = h.shape
    H = sigma.numel()
    pos = (torch.arange(L) + 0.5).to(h.dtype)
    s = -((pos[None, None, :, None] - align[:, None, None, :]) * sigma[None, :, None, None]) ** 2        # [B, H, L, T]
    mask = torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]
    s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    w = torch.softmax(s, dim=-1)
    w = torch.where(mask[:, None, None, :], w, torch.zeros_like(w))                                        # (all masked: NaN -> 0)
    hh = torch.where(mask[:, :, None], h, torch.zeros_like(h)).view(B, T, H, D // H).transpose(1, 2)      # rows past the end are never read
    return torch.matmul(w, hh).transpose(1, 2).reshape(B, L, D)


def predictor(sd, conf: dict, h, lens, prefix="predictor."):
    """-> dict(alphas_raw, token_num, counts, alphas, align, embeds): PifPredictor.forward at inference. counts: half-to-even rounding"""
    a, tn = pif_alphas(h, lens, sd[prefix + "cif_conv1d.weight"], sd[prefix + "cif_conv1d.bias"], sd[prefix + "cif_output.weight"],
                       sd[prefix + "cif_output.bias"], conf["l_order"], conf["r_order"], conf.get("smooth_factor", 1.0),
                       conf.get("noise_threshold", 0.0))
    counts = [int(v) for v in tn.round().tolist()]
    an, al = pif_align(a, tn, counts)
    L = max(counts)
    emb = pif_embed(al, h, sd[prefix + "sigma"], lens, L) if L > 0 else h.new_zeros(h.shape[0], 0, h.shape[2])
    return dict(alphas_raw=a, token_num=tn, counts=counts, alphas=an, align=al, embeds=emb)


def _mha(q, k, v, H, klens):
    """q [B, Lq, D], k / v [B, Lk, D]; keys at or past klens[b] masked; a sequence without keys gets zeros"""
    B, Lq, D = q.shape
    Lk, dk = k.shape[1], D // H
    s = torch.einsum("bihd,bjhd->bhij", q.view(B, Lq, H, dk), k.view(B, Lk, H, dk)) / math.sqrt(dk)
    mask = torch.arange(Lk)[None, :] >= torch.as_tensor(klens)[:, None]
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    a = torch.softmax(s, dim=-1)
    a = torch.where(mask[:, None, None, :], torch.zeros_like(a), a)
    a = torch.where(torch.isnan(a), torch.zeros_like(a), a)
    return torch.einsum("bhij,bjhd->bihd", a, v.view(B, Lk, H, dk)).reshape(B, Lq, D)


def decoder(sd, conf: dict, memory, mem_lens, embeds, tok_lens, prefix="decoder.", return_hidden=False):
    """-> log-probabilities [B, L, V] (or the after_norm rows with return_hidden)"""
    H = conf["attention_heads"]
    x = embeds
    for i in range(conf["num_blocks"]):
        p = f"{prefix}decoders.{i}."
        xn = _ln(x, sd, p + "norm1.")
        a = p + "self_attn."
        x = x + _lin(_mha(_lin(xn, sd, a + "linear_q."), _lin(xn, sd, a + "linear_k."), _lin(xn, sd, a + "linear_v."), H, tok_lens), sd, a + "linear_out.")
        xn = _ln(x, sd, p + "norm2.")
        a = p + "src_attn."
        x = x + _lin(_mha(_lin(xn, sd, a + "linear_q."), _lin(memory, sd, a + "linear_k."), _lin(memory, sd, a + "linear_v."), H, mem_lens), sd,
                     a + "linear_out.")
        x = x + _ffn(_ln(x, sd, p + "norm3."), sd, p + "feed_forward.", torch.relu)
    y = _ln(x, sd, prefix + "after_norm.")
    if return_hidden:
        return y
    return torch.log_softmax(_lin(y, sd, prefix + "output_layer."), dim=-1)


def greedy(logp, counts, drop=(0, 1, 2)):
    """per clip: arg-max over its own rows, sos / eos / blank filtered"""
    return [[t for t in logp[b, :n].argmax(-1).tolist() if t not in drop] for b, n in enumerate(counts)]


def model(sd, conf: dict, feats, lens, pos_rows=None):
    """features of the zero-padded batch -> dict(enc, olens, + predictor(...), logp, ids)"""
    enc, olens = encoder(sd, conf["encoder_conf"], feats, lens, pos_rows=pos_rows)
    out = predictor(sd, conf["predictor_conf"], enc, olens)
    out.update(enc=enc, olens=olens)
    if max(out["counts"]) > 0:
        out["logp"] = decoder(sd, conf["decoder_conf"], enc, olens, out["embeds"], out["counts"])
        out["ids"] = greedy(out["logp"], out["counts"])
    else:
        out["logp"], out["ids"] = None, [[] for _ in lens]
    return out
