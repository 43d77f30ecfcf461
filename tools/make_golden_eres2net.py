"""Writes tests/golden/eres2net.npz: the reference's own ERes2NetV2SV (funasr/models/eres2net/model.py), imported read-only
through oracle.ref_import, in float64 AND float32 on synthetic weights (funasr_amd.synth.eres2net_state_dict(seed, shapes); weights
are never stored), at the tiny configuration m_channels 16, num_blocks [1, 1, 2, 1], feat_dim 16, embedding_size 32:
  * x [3, 37, 16]: three chunks of log-mel-like features;
  * the float64 tensors after the stem, layer1 .. layer4, layer3_ds and fuse34 for chunk 1 (`<stage>_c1`, [C, F, T]), the pooled
    stats and the embedding for all three chunks, and gap_<stage> = max |fp32 - fp64| of the reference over all three chunks;
  * clamp_above / clamp_inside: per block, the share of its output's pre-clamp values (float64 oracle) above 20 / strictly inside
    (0, 20);
  * one ragged inference case at feat_dim 80 (the reference's extract_feature has 80 bins): two synthetic waveforms of unequal
    length, their kaldi fbank (kaldi-native-fbank oracle, CAM++ options) minus the time mean, zero-padded, and the reference's
    float64 embeddings with gap_ragged.
The tool refuses a seed for which (a) the float64 oracle tests/_eres2net_oracle.py differs from the reference by more than 1e-9
relative anywhere, (b) the clamp is not exercised (no block with 1 % .. 50 % of its pre-clamp outputs above 20, or a block with
under 10 % strictly inside (0, 20)), or (c) an embedding has max |.| < 0.05.
And tests/golden/eres2net_state_dict.json: names and shapes of the reference's state dict at the DEFAULT configuration.
Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SEED = 5
TINY = dict(feat_dim=16, embedding_size=32, m_channels=16, num_blocks=[1, 1, 2, 1])
RAGGED = dict(TINY, feat_dim=80)
MODULE_STAGES = ("layer1", "layer2", "layer3", "layer4", "layer3_ds", "fuse34")


def _features(g: torch.Generator, T: int, D: int) -> torch.Tensor:
    """log-mel-like frames: a smooth spectral envelope + noise and a slow modulation, minus the time mean"""
    env = torch.linspace(2.0, -3.0, D)[None] + 0.8 * torch.sin(torch.arange(D)[None] / 3.0 + torch.rand(1, generator=g) * 6)
    f = env + 1.5 * torch.randn(T, D, generator=g) + 0.5 * torch.sin(torch.arange(T)[:, None] / 9.0)
    return f - f.mean(0, keepdim=True)


def _reference_stages(model, x):
    """every stage of one forward of the reference module, by forward hooks (feature maps [B, C, F, T])"""
    import torch.nn.functional as F

    got, hooks = {}, []
    net = model.model
    for name in MODULE_STAGES:
        hooks.append(getattr(net, name).register_forward_hook(lambda m, i, o, name=name: got.__setitem__(name, o.detach().clone())))
    hooks.append(net.pool.register_forward_hook(lambda m, i, o: got.__setitem__("stats", o.detach().clone())))
    hooks.append(net.bn1.register_forward_hook(lambda m, i, o: got.__setitem__("stem", F.relu(o.detach()))))
    with torch.no_grad():
        got["emb"] = model(x.clone())
    for h in hooks:
        h.remove()
    return got


def main():
    from oracle import ref_import
    from funasr_amd import synth
    from make_golden_fbank_options import knf_fbank_opts
    from tests import _eres2net_oracle as O

    ref_import.install()
    from funasr.models.eres2net.model import ERes2NetV2SV

    out = dict(seed=np.int64(SEED))
    # ---- the tiny configuration, three chunks
    model = ERes2NetV2SV(**TINY)
    sd = synth.eres2net_state_dict(SEED, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict(sd, strict=True)
    model.eval()
    g = torch.Generator().manual_seed(SEED)
    x = torch.stack([_features(g, 37, TINY["feat_dim"]) for _ in range(3)]).float()
    r64 = _reference_stages(model.double(), x.double())
    r32 = _reference_stages(model.float(), x)
    pre = []
    o64 = O.stages(x, sd, torch.float64, pre)
    out["x"] = x.numpy()
    for name in O.STAGES:
        ref = r64[name]
        err = (o64[name] - ref).abs().max().item() / ref.abs().max().item()
        assert err <= 1e-9, f"(a) oracle vs reference at {name}: {err}"
        out[f"gap_{name}"] = np.float64((r32[name].double() - ref).abs().max().item())
        if name in ("stats", "emb"):
            out[name] = ref.numpy()
        else:
            out[f"{name}_c1"] = ref[1].numpy()
    above = np.array([(p > 20).double().mean().item() for p in pre])
    inside = np.array([((p > 0) & (p < 20)).double().mean().item() for p in pre])
    assert ((above >= 0.01) & (above <= 0.5)).any(), f"(b) no block with 1 % .. 50 % above 20: {above}"
    assert (inside >= 0.10).all(), f"(b) a block with under 10 % inside (0, 20): {inside}"
    out["clamp_above"], out["clamp_inside"] = above, inside
    assert np.abs(out["emb"]).max(axis=1).min() >= 0.05, "(c) embedding too small"
    # ---- ragged inference at 80 bins
    model = ERes2NetV2SV(**RAGGED)
    sdr = synth.eres2net_state_dict(SEED + 1, {k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict(sdr, strict=True)
    model.eval()
    wavs = [(synth.speech_like(n, seed=60 + i) * 0.4).numpy().astype(np.float32) for i, n in enumerate((7000, 4321))]
    feats = []
    for w in wavs:
        f = torch.from_numpy(knf_fbank_opts(w, "povey", True))
        feats.append(f - f.mean(0, keepdim=True))
    T = max(f.shape[0] for f in feats)
    xr = torch.zeros(2, T, 80)
    for i, f in enumerate(feats):
        xr[i, : f.shape[0]] = f
    with torch.no_grad():
        e64 = model.double()(xr.double().clone())
        e32 = model.float()(xr.clone())
    err = (O.forward(xr, sdr) - e64).abs().max().item() / e64.abs().max().item()
    assert err <= 1e-9, f"(a) oracle vs reference, ragged case: {err}"
    assert e64.abs().max(dim=1).values.min().item() >= 0.05, "(c) ragged embedding too small"
    out.update(ragged_seed=np.int64(SEED + 1), ragged_wav0=wavs[0], ragged_wav1=wavs[1], ragged_x=xr.numpy(), ragged_emb=e64.numpy(),
               gap_ragged=np.float64((e32.double() - e64).abs().max().item()))
    path = os.path.join(ROOT, "tests", "golden", "eres2net.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if k.startswith("gap_"):
            print(k, float(out[k]))
    print("above 20:", above.round(4), "inside:", inside.round(4), "max |emb|:", np.abs(out["emb"]).max(), np.abs(out["ragged_emb"]).max())
    # ---- the default configuration's state-dict layout
    default = ERes2NetV2SV()
    layout = {k: list(v.shape) for k, v in default.state_dict().items()}
    assert len(layout) == 557
    path = os.path.join(ROOT, "tests", "golden", "eres2net_state_dict.json")
    with open(path, "w") as f:
        json.dump(layout, f)
    print(path, os.path.getsize(path), "bytes", len(layout), "tensors", sum(int(np.prod(s)) for s in layout.values()), "elements")


if __name__ == "__main__":
    main()
