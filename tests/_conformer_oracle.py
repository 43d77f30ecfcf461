"""Float64 restatement of the reference's Conformer (funasr/models/conformer/encoder.py, funasr/models/transformer/{attention,
embedding,decoder}.py, utils/subsampling.py) in plain torch, dtype- and device-generic (the bench runs it in float32 on the GPU).
Written from the formulas, not from the reference's code paths: the positional term of the relative-position attention is taken
element by element,
    latest:  bd[i, j] = qv_i . P[T - 1 - i + j]
    legacy:  bd[i, j] = qv_i . P[T - 1 - i + j] (j <= i), 0 (j == i + 1), qv_{i+1} . P[j - i - 2] (j >= i + 2)
instead of through the pad / reshape trick of `rel_shift`. The positional tables are the float32 tables of the reference (built in
float32, then cast), which is what a float64 copy of the reference model holds."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from funasr_amd.conformer import abs_pos_table, latest_rel_pos_table, legacy_rel_pos_table, subsampled_length

LN_EPS = 1e-12


def _ln(x, sd, p):
    return Fn.layer_norm(x, x.shape[-1:], sd[p + "weight"], sd[p + "bias"], LN_EPS)


def _lin(x, sd, p, bias=True):
    return Fn.linear(x, sd[p + "weight"], sd[p + "bias"] if bias else None)


def cast(sd, dtype=torch.float64, device="cpu"):
    return {k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)) for k, v in sd.items()}


def subsample(x, sd, p="encoder.embed."):
    """Conv2dSubsampling without its positional module: x [B, Tin, F] -> [B, T, D] (before the sqrt(D) scale)"""
    y = Fn.relu(Fn.conv2d(x[:, None], sd[p + "conv.0.weight"], sd[p + "conv.0.bias"], stride=2))
    y = Fn.relu(Fn.conv2d(y, sd[p + "conv.2.weight"], sd[p + "conv.2.bias"], stride=2))
    b, c, t, f = y.shape
    return Fn.linear(y.transpose(1, 2).reshape(b, t, c * f), sd[p + "out.0.weight"], sd[p + "out.0.bias"])


def rel_bd(qv, P, legacy: bool):
    """qv [B, H, T, dk], P [H, nP, dk] -> bd [B, H, T, T] by the per-element formulas"""
    T = qv.shape[2]
    M = torch.einsum("bhid,hnd->bhin", qv, P)                                   # every qv_i . P[n]
    i = torch.arange(T, device=qv.device)[:, None]
    j = torch.arange(T, device=qv.device)[None, :]
    low = (T - 1 - i + j)
    if not legacy:
        return torch.gather(M, 3, low.expand(*M.shape[:2], T, T))
    lower = torch.gather(M, 3, low.clamp(0, T - 1).expand(*M.shape[:2], T, T))
    Mn = torch.cat([M[:, :, 1:], M[:, :, -1:]], dim=2)                          # row i holds qv_{i+1} . P[n]
    upper = torch.gather(Mn, 3, (j - i - 2).clamp(0, T - 1).expand(*M.shape[:2], T, T))
    zero = torch.zeros_like(lower)
    return torch.where(j <= i, lower, torch.where(j == i + 1, zero, upper))


def relpos_attention(q, k, v, P, u, vb, klens, legacy: bool):
    """q, k, v [B, T, H, dk]; P [nP, H, dk]; u, vb [H, dk]; klens [B] -> [B, T, H * dk]"""
    B, T, H, dk = q.shape
    ac = torch.einsum("bihd,bjhd->bhij", q + u, k)
    bd = rel_bd((q + vb).transpose(1, 2), P.transpose(0, 1), legacy)
    s = (ac + bd) / math.sqrt(dk)
    mask = torch.arange(T, device=q.device)[None, :] >= torch.as_tensor(klens, device=q.device)[:, None]       # [B, T] True = masked
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    a = torch.softmax(s, dim=-1).masked_fill(mask[:, None, None, :], 0.0)
    return torch.einsum("bhij,bjhd->bihd", a, v).reshape(B, T, H * dk)


def conv_module(x, sd, p, kernel: int):
    """x [B, T, D] -> [B, T, D]: pointwise-1, GLU, depthwise (zero padding at the batch edges), BatchNorm (eval), Swish, pointwise-2"""
    y = Fn.conv1d(x.transpose(1, 2), sd[p + "pointwise_conv1.weight"], sd[p + "pointwise_conv1.bias"])
    y = Fn.glu(y, dim=1)
    y = Fn.conv1d(y, sd[p + "depthwise_conv.weight"], sd[p + "depthwise_conv.bias"], padding=(kernel - 1) // 2, groups=y.shape[1])
    y = (y - sd[p + "norm.running_mean"][None, :, None]) / torch.sqrt(sd[p + "norm.running_var"][None, :, None] + 1e-5)
    y = y * sd[p + "norm.weight"][None, :, None] + sd[p + "norm.bias"][None, :, None]
    y = y * torch.sigmoid(y)
    return Fn.conv1d(y, sd[p + "pointwise_conv2.weight"], sd[p + "pointwise_conv2.bias"]).transpose(1, 2)


def _ffn(x, sd, p, act):
    return _lin(act(_lin(x, sd, p + "w_1.")), sd, p + "w_2.")


def swish(x):
    return x * torch.sigmoid(x)


def encoder(sd, conf: dict, feats, lens, prefix="encoder.", pos_rows=None):
    """conf: the encoder_conf (output_size, attention_heads, num_blocks, cnn_module_kernel, macaron_style, rel_pos_type).
    feats [B, Tin, F] zero-padded, lens [B] -> (out [B, T, D], olens list): every row of the padded batch, as the reference.
    pos_rows: recorded rows of the reference's float32 positional table (for at least T frames) instead of this host's own."""
    D, H = conf["output_size"], conf["attention_heads"]
    legacy = conf.get("rel_pos_type", "legacy") == "legacy"
    macaron = bool(conf.get("macaron_style", False))
    kernel = conf.get("cnn_module_kernel", 31)
    dk = D // H
    Tin = feats.shape[1]
    x = subsample(feats, sd, prefix + "embed.") * math.sqrt(D)
    B, T, _ = x.shape
    olens = [subsampled_length(int(n), Tin) for n in lens]
    if pos_rows is not None:
        pr = torch.as_tensor(pos_rows)
        c = (pr.shape[0] + 1) // 2
        pos = pr[:T] if legacy else pr[c - T: c + T - 1]
    elif legacy:
        pos = legacy_rel_pos_table(D)[:T]
    else:
        pos = latest_rel_pos_table(D)[5000 - T: 5000 + T - 1]
    pos = pos.to(device=x.device, dtype=x.dtype)
    scale = 0.5 if macaron else 1.0
    for i in range(conf["num_blocks"]):
        p = f"{prefix}encoders.{i}."
        if macaron:
            x = x + scale * _ffn(_ln(x, sd, p + "norm_ff_macaron."), sd, p + "feed_forward_macaron.", swish)
        xn = _ln(x, sd, p + "norm_mha.")
        a = p + "self_attn."
        q = _lin(xn, sd, a + "linear_q.").view(B, T, H, dk)
        k = _lin(xn, sd, a + "linear_k.").view(B, T, H, dk)
        v = _lin(xn, sd, a + "linear_v.").view(B, T, H, dk)
        P = _lin(pos, sd, a + "linear_pos.", bias=False).view(-1, H, dk)
        att = relpos_attention(q, k, v, P, sd[a + "pos_bias_u"], sd[a + "pos_bias_v"], olens, legacy)
        x = x + _lin(att, sd, a + "linear_out.")
        x = x + conv_module(_ln(x, sd, p + "norm_conv."), sd, p + "conv_module.", kernel)
        x = x + scale * _ffn(_ln(x, sd, p + "norm_ff."), sd, p + "feed_forward.", swish)
        x = _ln(x, sd, p + "norm_final.")
    return _ln(x, sd, prefix + "after_norm."), olens


def ctc_log_softmax(sd, enc, prefix="ctc."):
    return torch.log_softmax(_lin(enc, sd, prefix + "ctc_lo."), dim=-1)


def ctc_greedy(logp, n: int, blank: int = 0):
    y = torch.unique_consecutive(logp[:n].argmax(-1))
    return y[y != blank].tolist()


def _mha(xq, K, V, H):
    """xq [n, D] queries (already projected), K / V [n, L, D] or [L, D] -> [n, D]"""
    n, D = xq.shape
    dk = D // H
    if K.dim() == 2:
        K, V = K[None].expand(n, -1, -1), V[None].expand(n, -1, -1)
    s = torch.einsum("nhd,nlhd->nhl", xq.view(n, H, dk), K.reshape(n, -1, H, dk)) / math.sqrt(dk)
    a = torch.softmax(s, dim=-1)
    return torch.einsum("nhl,nlhd->nhd", a, V.reshape(n, -1, H, dk)).reshape(n, D)


class DecoderStepper:
    """The reference's TransformerDecoder.forward_one_step for all running hypotheses at once, as the stepper protocol of
    funasr_amd.transformer_search (begin / step / reorder). Per layer it keeps the self-attention K / V of every position of a
    hypothesis -- algebraically what the reference recomputes from its cache of layer outputs."""

    def __init__(self, sd, conf: dict, memory, prefix="decoder."):
        self.sd, self.p, self.H, self.L = sd, prefix, conf["attention_heads"], conf["num_blocks"]
        self.memory = memory
        self.D = memory.shape[-1]
        self.pe = abs_pos_table(self.D).to(device=memory.device, dtype=memory.dtype)
        self.cross = [(_lin(memory, sd, f"{prefix}decoders.{l}.src_attn.linear_k."), _lin(memory, sd, f"{prefix}decoders.{l}.src_attn.linear_v."))
                      for l in range(self.L)]
        self.K = self.V = None

    def begin(self, max_len, max_hyp):
        self.K = [None] * self.L
        self.V = [None] * self.L

    def reorder(self, parents):
        idx = torch.as_tensor(parents, device=self.memory.device)
        self.K = [k[idx] for k in self.K]
        self.V = [v[idx] for v in self.V]

    def step(self, tokens, pos):
        sd, p = self.sd, self.p
        x = sd[p + "embed.0.weight"][torch.as_tensor(tokens, device=self.memory.device)] * math.sqrt(self.D) + self.pe[pos]
        for l in range(self.L):
            q = f"{p}decoders.{l}."
            xn = _ln(x, sd, q + "norm1.")
            k, v = _lin(xn, sd, q + "self_attn.linear_k.")[:, None], _lin(xn, sd, q + "self_attn.linear_v.")[:, None]
            self.K[l] = k if self.K[l] is None else torch.cat([self.K[l], k], 1)
            self.V[l] = v if self.V[l] is None else torch.cat([self.V[l], v], 1)
            x = x + _lin(_mha(_lin(xn, sd, q + "self_attn.linear_q."), self.K[l], self.V[l], self.H), sd, q + "self_attn.linear_out.")
            xn = _ln(x, sd, q + "norm2.")
            x = x + _lin(_mha(_lin(xn, sd, q + "src_attn.linear_q."), self.cross[l][0], self.cross[l][1], self.H), sd, q + "src_attn.linear_out.")
            x = x + _ffn(_ln(x, sd, q + "norm3."), sd, q + "feed_forward.", torch.relu)
        y = _ln(x, sd, p + "after_norm.")
        return torch.log_softmax(_lin(y, sd, p + "output_layer."), dim=-1)


def score_prefix(stepper, prefix):
    """log-probabilities after the whole prefix (<sos> first), through a fresh run of the stepper"""
    stepper.begin(len(prefix), 1)
    out = None
    for pos, tok in enumerate(prefix):
        out = stepper.step([tok], pos)
    return out[0]


def to_np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
