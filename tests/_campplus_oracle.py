"""Float64 functional restatement of the reference's CAM++ (funasr/models/campplus/model.py, components.py) on a state dict:
the CPU oracle the HIP network is measured against. Written from the module structure, not copied: head (FCM) -> TDNN ->
3 CAM dense-TDNN blocks with transits -> out BN-ReLU -> stats pool -> dense -> affine-free BN."""
from __future__ import annotations

import torch
import torch.nn.functional as F

LAYERS = (12, 24, 16)
DILATION = (1, 2, 2)
EPS = 1e-5


def _bn(x, sd, p, affine=True):
    w = sd[p + "weight"] if affine else None
    b = sd[p + "bias"] if affine else None
    return F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], w, b, False, 0.0, EPS)


def seg_mean(h: torch.Tensor, seg: int = 100) -> torch.Tensor:
    """avg_pool1d(h, seg, seg, ceil_mode=True) broadcast back to every frame: frame t gets the mean of its segment
    [seg * (t // seg), min(seg * (t // seg + 1), T)) -- the last, partial segment divides by its true length"""
    T = h.shape[-1]
    out = torch.empty_like(h)
    for s0 in range(0, T, seg):
        s1 = min(s0 + seg, T)
        out[..., s0:s1] = h[..., s0:s1].mean(-1, keepdim=True)
    return out


def head(x: torch.Tensor, sd) -> torch.Tensor:
    """FCM: [B, T, 80] -> [B, 320, T] (channel index c * 10 + f)"""
    out = F.relu(_bn(F.conv2d(x.permute(0, 2, 1).unsqueeze(1), sd["head.conv1.weight"], padding=1), sd, "head.bn1."))
    for l in (1, 2):
        for b in (0, 1):
            p = f"head.layer{l}.{b}."
            stride = (2, 1) if b == 0 else (1, 1)
            o = F.relu(_bn(F.conv2d(out, sd[p + "conv1.weight"], stride=stride, padding=1), sd, p + "bn1."))
            o = _bn(F.conv2d(o, sd[p + "conv2.weight"], padding=1), sd, p + "bn2.")
            if p + "shortcut.0.weight" in sd:
                sc = _bn(F.conv2d(out, sd[p + "shortcut.0.weight"], stride=stride), sd, p + "shortcut.1.")
            else:
                sc = out
            out = F.relu(o + sc)
    out = F.relu(_bn(F.conv2d(out, sd["head.conv2.weight"], stride=(2, 1), padding=1), sd, "head.bn2."))
    B, C, Fq, T = out.shape
    return out.reshape(B, C * Fq, T)


def dense_layer(x: torch.Tensor, sd, p: str, dil: int) -> torch.Tensor:
    """one CAMDenseTDNNLayer: [B, Cin, T] -> its 32 new channels [B, 32, T]"""
    h = F.conv1d(F.relu(_bn(x, sd, p + "nonlinear1.batchnorm.")), sd[p + "linear1.weight"])
    h = F.relu(_bn(h, sd, p + "nonlinear2.batchnorm."))
    q = p + "cam_layer."
    y = F.conv1d(h, sd[q + "linear_local.weight"], padding=dil, dilation=dil)
    ctx = h.mean(-1, keepdim=True) + seg_mean(h)
    m = torch.sigmoid(F.conv1d(F.relu(F.conv1d(ctx, sd[q + "linear1.weight"], sd[q + "linear1.bias"])),
                               sd[q + "linear2.weight"], sd[q + "linear2.bias"]))
    return y * m


def forward(x: torch.Tensor, sd, dtype=torch.float64) -> torch.Tensor:
    """[B, T, 80] features -> [B, 192] embeddings"""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = head(x.to(dtype), sd)
    x = F.relu(_bn(F.conv1d(x, sd["xvector.tdnn.linear.weight"], stride=2, padding=2), sd, "xvector.tdnn.nonlinear.batchnorm."))
    for i, (n, dil) in enumerate(zip(LAYERS, DILATION)):
        for j in range(n):
            x = torch.cat([x, dense_layer(x, sd, f"xvector.block{i + 1}.tdnnd{j + 1}.", dil)], dim=1)
        p = f"xvector.transit{i + 1}."
        x = F.conv1d(F.relu(_bn(x, sd, p + "nonlinear.batchnorm.")), sd[p + "linear.weight"])
    x = F.relu(_bn(x, sd, "xvector.out_nonlinear.batchnorm."))
    stats = torch.cat([x.mean(-1), x.std(-1, unbiased=True)], dim=-1)
    y = F.conv1d(stats.unsqueeze(-1), sd["xvector.dense.linear.weight"]).squeeze(-1)
    return _bn(y, sd, "xvector.dense.nonlinear.batchnorm.", affine=False)
