"""Functional restatement of the reference's ERes2NetV2 (funasr/models/eres2net/eres2netv2.py, fusion.py, model.py) on a state
dict under the reference's keys, dtype-generic: the CPU oracle the HIP network is measured against. Written from the formulas,
not copied: stem 3x3 + BN + ReLU -> four layers of Res2Net blocks (width = floor(26 planes / 64), two 3x3 branches, the second
fed by the sum -- layers 1, 2 -- or by the attentional fusion AFF -- layers 3, 4 -- of the first branch's output and the second
split; every activation inside a block is clamp(0, 20)) -> AFF(out4, layer3_ds(out3)) -> mean / std over time -> seg_1."""
from __future__ import annotations

import torch
import torch.nn.functional as F

EPS = 1e-5
STAGES = ("stem", "layer1", "layer2", "layer3", "layer4", "layer3_ds", "fuse34", "stats", "emb")


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], False, 0.0, EPS)


def act(x):
    return x.clamp(0.0, 20.0)


def aff(x, y, sd, p):
    """x g + y (2 - g), g = 1 + tanh(BN(conv(SiLU(BN(conv(cat(x, y)))))))"""
    p = p + "local_att."
    a = _bn(F.conv2d(torch.cat([x, y], 1), sd[p + "0.weight"], sd[p + "0.bias"]), sd, p + "1.")
    a = _bn(F.conv2d(F.silu(a), sd[p + "3.weight"], sd[p + "3.bias"]), sd, p + "4.")
    g = 1.0 + torch.tanh(a)
    return x * g + y * (2.0 - g)


def block(x, sd, p, stride, pre=None):
    """one BasicBlockERes2NetV2 / ...AFF (told apart by the fuse_models keys). `pre`: a list that receives the block's output
    before its last clamp"""
    h = act(_bn(F.conv2d(x, sd[p + "conv1.weight"], stride=stride), sd, p + "bn1."))
    w = h.shape[1] // 2
    s0, s1 = h[:, :w], h[:, w:]
    sp = act(_bn(F.conv2d(s0, sd[p + "convs.0.weight"], padding=1), sd, p + "bns.0."))
    mix = aff(sp, s1, sd, p + "fuse_models.0.") if p + "fuse_models.0.local_att.0.weight" in sd else sp + s1
    sp1 = act(_bn(F.conv2d(mix, sd[p + "convs.1.weight"], padding=1), sd, p + "bns.1."))
    out = _bn(F.conv2d(torch.cat([sp, sp1], 1), sd[p + "conv3.weight"]), sd, p + "bn3.")
    if p + "shortcut.0.weight" in sd:
        out = out + _bn(F.conv2d(x, sd[p + "shortcut.0.weight"], stride=stride), sd, p + "shortcut.1.")
    else:
        out = out + x
    if pre is not None:
        pre.append(out)
    return act(out)


def stages(x: torch.Tensor, sd, dtype=torch.float64, pre=None) -> dict:
    """[B, T, F] features -> every stage of STAGES; feature maps as [B, C, F, T] like the reference"""
    sd = {k[len("model."):]: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.startswith("model.")}
    out = {}
    h = F.relu(_bn(F.conv2d(x.to(dtype).permute(0, 2, 1).unsqueeze(1), sd["conv1.weight"], padding=1), sd, "bn1."))
    out["stem"] = h
    for l in (1, 2, 3, 4):
        b = 0
        while f"layer{l}.{b}.conv1.weight" in sd:
            h = block(h, sd, f"layer{l}.{b}.", 2 if (b == 0 and l > 1) else 1, pre)
            b += 1
        out[f"layer{l}"] = h
    out["layer3_ds"] = F.conv2d(out["layer3"], sd["layer3_ds.weight"], stride=2, padding=1)
    out["fuse34"] = aff(out["layer4"], out["layer3_ds"], sd, "fuse34.")
    f = out["fuse34"]
    out["stats"] = torch.cat([f.mean(-1).flatten(1), torch.sqrt(f.var(-1, unbiased=True) + 1e-8).flatten(1)], 1)
    out["emb"] = F.linear(out["stats"], sd["seg_1.weight"], sd["seg_1.bias"])
    return out


def forward(x: torch.Tensor, sd, dtype=torch.float64) -> torch.Tensor:
    """[B, T, F] features -> [B, E] embeddings"""
    return stages(x, sd, dtype)["emb"]


def conv_nhwc(a, w, stride=(1, 1), a2=None, mode=0, w2=None, stride2=(1, 1), bias=None, r=None, act_id=0, xy=None):
    """The single conv of the HIP kernel on channels-last tensors (a [n, T, F, C], w [N, C, kF, kT] over (freq, time) like the
    reference's [O, I, kh, kw], stride (time, freq)): second operand summed (mode 1) or as a 1x1 conv of its own added to the
    product (mode 2: concatenation on K), bias, residual, activation 0 none / 1 ReLU / 2 clamp(0, 20) / 3 SiLU, then the AFF
    combine with xy = (x, y). Returns [n, To, Fo, N]."""
    def nchw(t):
        return t.permute(0, 3, 2, 1)                       # [n, T, F, C] -> [n, C, F, T]
    x = nchw(a) + (nchw(a2) if mode == 1 else 0)
    pad = (w.shape[2] // 2, w.shape[3] // 2)
    v = F.conv2d(x, w, stride=(stride[1], stride[0]), padding=pad)
    if mode == 2:
        v = v + F.conv2d(nchw(a2), w2, stride=(stride2[1], stride2[0]))
    v = v.permute(0, 3, 2, 1)
    if bias is not None:
        v = v + bias
    if r is not None:
        v = v + r
    v = [v, F.relu(v), v.clamp(0.0, 20.0), F.silu(v)][act_id]
    if xy is not None:
        g = 1.0 + torch.tanh(v)
        v = xy[0] * g + xy[1] * (2.0 - g)
    return v
