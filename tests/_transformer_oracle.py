"""Float64 restatement of the reference's Transformer encoder (funasr/models/transformer/{encoder,attention,embedding}.py) in
plain torch, dtype- and device-generic (the bench runs it in float32 on the GPU). Written from the formulas:
    embedding   x sqrt(D) + pe[t]                                   (PositionalEncoding over the subsampled rows)
    attention   softmax_j(q_i . k_j / sqrt(d_k)) over the keys j < klen of the sequence; masked keys get -inf before the softmax
                and 0 after it, so a sequence with no valid key gives zero rows
    block       x += linear_out(attention(LN1 x)); x += w_2(relu(w_1(LN2 x)));   after_norm at the end
The subsampling, the decoder stepper and the CTC pieces are the Conformer oracle's (the two models share them)."""
from __future__ import annotations

import math

import torch

from funasr_amd.conformer import abs_pos_table, subsampled_length

from ._conformer_oracle import (DecoderStepper, _ffn, _lin, _ln, cast, ctc_greedy, ctc_log_softmax, score_prefix, subsample,  # noqa: F401
                                to_np)


def attention(q, k, v, klens):
    """q, k, v [B, T, H, dk]; klens [B] -> [B, T, H * dk]"""
    B, T, H, dk = q.shape
    s = torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(dk)
    mask = torch.arange(T, device=q.device)[None, :] >= torch.as_tensor(klens, device=q.device)[:, None]       # [B, T] True = masked
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    a = torch.softmax(s, dim=-1).masked_fill(mask[:, None, None, :], 0.0)
    return torch.einsum("bhij,bjhd->bihd", a, v).reshape(B, T, H * dk)


def embed_rows(x, pe):
    """x [B, T, D], pe [>= T, D] -> x sqrt(D) + pe[:T]"""
    return x * math.sqrt(x.shape[-1]) + pe[: x.shape[1]].to(device=x.device, dtype=x.dtype)


def encoder(sd, conf: dict, feats, lens, prefix="encoder.", pos_rows=None):
    """conf: the encoder_conf (output_size, attention_heads, num_blocks). feats [B, Tin, F] zero-padded, lens [B] ->
    (out [B, T, D], olens list): every row of the padded batch, as the reference. pos_rows: recorded rows of the reference's
    float32 positional table (for at least T frames) instead of this host's own."""
    D, H = conf["output_size"], conf["attention_heads"]
    dk = D // H
    Tin = feats.shape[1]
    x = subsample(feats, sd, prefix + "embed.")
    B, T, _ = x.shape
    olens = [subsampled_length(int(n), Tin) for n in lens]
    x = embed_rows(x, torch.as_tensor(pos_rows) if pos_rows is not None else abs_pos_table(D)[:T])
    for i in range(conf["num_blocks"]):
        p = f"{prefix}encoders.{i}."
        xn = _ln(x, sd, p + "norm1.")
        a = p + "self_attn."
        q = _lin(xn, sd, a + "linear_q.").view(B, T, H, dk)
        k = _lin(xn, sd, a + "linear_k.").view(B, T, H, dk)
        v = _lin(xn, sd, a + "linear_v.").view(B, T, H, dk)
        x = x + _lin(attention(q, k, v, olens), sd, a + "linear_out.")
        x = x + _ffn(_ln(x, sd, p + "norm2."), sd, p + "feed_forward.", torch.relu)
    return _ln(x, sd, prefix + "after_norm."), olens
