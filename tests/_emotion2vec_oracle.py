"""Functional restatement of the reference's emotion2vec feature path (funasr/models/emotion2vec: model.py extract_features +
inference head, audio.py, base.py, modules.py) on a state dict, dtype-generic: in float64 it is the CPU oracle the HIP network is
measured against, in float32 on the GPU the eager baseline of tools/bench_emotion2vec.py. Written from the math, one utterance
at a time: waveform norm -> conv encoder (conv, LayerNorm(512), GELU) -> LayerNorm + Linear -> positional conv -> extra tokens ->
context LayerNorm -> post-LN ALiBi blocks -> frames, their mean, proj + softmax."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

A = "modality_encoders.AUDIO."


def slopes(n: int) -> list:
    def pow2(n):
        start = 2 ** (-(2 ** -(math.log2(n) - 3)))
        return [start * start ** i for i in range(n)]

    if math.log2(n).is_integer():
        return pow2(n)
    cp = 2 ** math.floor(math.log2(n))
    return pow2(cp) + slopes(2 * cp)[0::2][: n - cp]


def _ln(x, sd, p, eps, D=None):
    if p is None:
        return F.layer_norm(x, (D,), eps=eps)
    return F.layer_norm(x, (x.shape[-1],), sd[p + "weight"], sd[p + "bias"], eps)


def features(wav: torch.Tensor, sd: dict, cfg: dict, dtype=torch.float64, reference_casts: bool = False) -> torch.Tensor:
    """one utterance [N] -> frames [T, D]. reference_casts: the scores, the float32 ALiBi bias and the softmax in float32 whatever
    dtype, and the conv encoder's LayerNorms in float32, as the reference does (modules.py:414, 423; base.py:284;
    fairseq_modules.py:66-89), to compare with its float64 run. cfg: embed_dim, num_heads, prenet_depth, depth, num_extra_tokens, num_alibi_heads,
    spec [(512, k, s)], conv_pos_depth, conv_pos_kernel, conv_pos_groups, norm_eps, normalize, per_layer"""
    dev = wav.device
    g = {k: v.to(device=dev, dtype=dtype) for k, v in sd.items()}
    eps, D, H = cfg["norm_eps"], cfg["embed_dim"], cfg["num_heads"]
    x = wav.to(dtype).reshape(-1)
    if cfg["normalize"]:
        x = F.layer_norm(x, x.shape)
    x = x[None, None]
    for i, (_, k, s) in enumerate(cfg["spec"]):
        p = A + f"local_encoder.conv_layers.{i}."
        x = F.conv1d(x, g[p + "0.weight"], stride=s)
        xt = x.transpose(1, 2)
        if reference_casts:                       # Fp32LayerNorm (fairseq_modules.py:66-89)
            xt = F.layer_norm(xt.float(), (xt.shape[-1],), g[p + "2.1.weight"].float(), g[p + "2.1.bias"].float(), eps).to(dtype)
        else:
            xt = _ln(xt, g, p + "2.1.", eps)
        x = F.gelu(xt.transpose(1, 2))
    x = x.transpose(1, 2)                                                      # [1, T, 512]
    x = F.linear(_ln(x, g, A + "project_features.1.", eps), g[A + "project_features.2.weight"], g[A + "project_features.2.bias"])
    y = x.transpose(1, 2)
    for i in range(cfg["conv_pos_depth"]):
        p = A + f"relative_positional_encoder.{i + 1}.0."
        y = F.conv1d(y, g[p + "weight"], g[p + "bias"], padding=cfg["conv_pos_kernel"] // 2, groups=cfg["conv_pos_groups"])
        y = F.gelu(F.layer_norm(y.transpose(1, 2), (D,), eps=eps).transpose(1, 2))
    x = x + y.transpose(1, 2)
    T = x.shape[1]
    E = cfg["num_extra_tokens"]
    pos = torch.arange(T, device=dev)
    dist = -(pos[None, :] - pos[:, None]).abs().to(dtype)
    NA = cfg["num_alibi_heads"]
    sl = torch.tensor(slopes(NA), dtype=torch.float32).to(device=dev, dtype=dtype)
    scale = g[A + "alibi_scale"].clamp_min(0)                                   # [L or 1, 1, NA or 1, 1, 1]
    x = torch.cat([g[A + "extra_tokens"], x], dim=1)
    x = _ln(x, g, A + "context_encoder.norm.", eps)
    names = [A + f"context_encoder.blocks.{i}." for i in range(cfg["prenet_depth"])] + [f"blocks.{i}." for i in range(cfg["depth"])]
    for li, p in enumerate(names):
        sc = scale[li if scale.shape[0] > 1 else 0].reshape(-1)
        bias = torch.zeros(H, T + E, T + E, device=dev, dtype=dtype)
        bias[:NA, E:, E:] = sl[:, None, None] * dist[None] * sc[:, None, None]
        qkv = F.linear(x[0], g[p + "attn.qkv.weight"], g[p + "attn.qkv.bias"]).reshape(T + E, 3, H, 64).permute(1, 2, 0, 3)
        q, k, v = qkv[0] * 64 ** -0.5, qkv[1], qkv[2]
        if reference_casts:
            b32 = torch.zeros(H, T + E, T + E, device=dev, dtype=torch.float32)
            b32[:NA, E:, E:] = sl.float()[:, None, None] * dist.float()[None] * sc.float()[:, None, None]
            att = torch.softmax((q @ k.transpose(-1, -2)).float() + b32, dim=-1, dtype=torch.float32).to(dtype)
        else:
            att = torch.softmax(q @ k.transpose(-1, -2) + bias, dim=-1)
        o = (att @ v).transpose(0, 1).reshape(1, T + E, D)
        x = _ln(x + F.linear(o, g[p + "attn.proj.weight"], g[p + "attn.proj.bias"]), g, p + "norm1.", eps)
        h = F.linear(F.gelu(F.linear(x, g[p + "mlp.fc1.weight"], g[p + "mlp.fc1.bias"])), g[p + "mlp.fc2.weight"], g[p + "mlp.fc2.bias"])
        x = _ln(x + h, g, p + "norm2.", eps)
    return x[0, E:]


def head(frames: torch.Tensor, sd: dict, labels, dtype=torch.float64):
    """frames [T, D] -> (pooled [D], probs [C] or None): mean over frames, proj, 'unuse*' classes at -inf, softmax"""
    pooled = frames.mean(0)
    if "proj.weight" not in sd:
        return pooled, None
    logits = F.linear(pooled, sd["proj.weight"].to(pooled), sd["proj.bias"].to(pooled))
    mask = torch.tensor([str(lab).startswith("unuse") for lab in labels], device=logits.device)
    logits = logits.masked_fill(mask, float("-inf"))
    return pooled, torch.softmax(logits, -1)


def records(keys, probs, labels, pooled=None):
    """the reference's inference records (model.py:308-317) from probabilities [B, C]"""
    out = []
    for i, k in enumerate(keys):
        scores = [float(v) for v in probs[i]]
        keep = [j for j, lab in enumerate(labels) if not str(lab).startswith("unuse")]
        rec = {"key": k, "labels": [labels[j] for j in keep], "scores": [scores[j] for j in keep]}
        if pooled is not None:
            rec["feats"] = pooled[i]
        out.append(rec)
    return out


def cfg_of(model) -> dict:
    """the oracle's config from a funasr_amd Emotion2vec module"""
    return dict(embed_dim=model.embed_dim, num_heads=model.num_heads, prenet_depth=model.prenet_depth, depth=model.depth,
                num_extra_tokens=model.num_extra_tokens, num_alibi_heads=model.num_alibi_heads, spec=model.spec,
                conv_pos_depth=model.conv_pos_depth, conv_pos_kernel=model.conv_pos_kernel, conv_pos_groups=model.conv_pos_groups,
                norm_eps=model.norm_eps, normalize=model.normalize)
