"""Writes tests/golden/emotion2vec.npz: the reference's own Emotion2vec (funasr/models/emotion2vec/model.py, imported read-only
through oracle.ref_import) in float32 AND float64 on synthetic weights (funasr_amd.synth.emotion2vec_state_dict; weights are never
stored) at a tiny config (D 256, 4 heads, 1 + 2 blocks, the real 512-channel conv stack, 9 classes with one `unuse` label,
per-head ALiBi scales with one negative entry), three odd-length waveforms (0.4 s, 1.03 s, 2.37 s): frame features, their means,
the proj + softmax probabilities. Also the ALiBi slopes for 4 / 12 / 16 heads, and tests/golden/emotion2vec_state_dict.json: the
template config's state-dict names and shapes. Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 7
LABELS = ["angry", "disgusted", "fearful", "happy", "neutral", "other", "sad", "surprised", "unuse_0"]
LENS = (6400, 16480, 37920)


def _reference():
    from oracle import ref_import

    ref_import.install()
    import omegaconf
    omegaconf.MISSING, omegaconf.II = "???", (lambda s: s)          # the stand-in lacks them; base.py imports both
    from funasr.models.emotion2vec.base import get_alibi
    from funasr.models.emotion2vec.model import Emotion2vec
    return Emotion2vec, get_alibi


def _coerce(conf):
    out = dict(conf)
    out["norm_eps"] = float(out["norm_eps"])
    return out


def main():
    from funasr_amd import synth
    from funasr_amd.emotion2vec import Emotion2vec as Hip

    Ref, get_alibi = _reference()
    conf = synth.emotion2vec_conf()
    hip = Hip(model_conf=conf, vocab_size=len(LABELS))
    sd = synth.emotion2vec_state_dict(SEED, hip)
    ref = Ref(model_conf=_coerce(conf), vocab_size=len(LABELS))
    ref.load_state_dict(sd, strict=False)
    missing = [k for k in ref.state_dict() if k not in sd and not k.startswith("modality_encoders.AUDIO.decoder.")]
    assert not missing, missing
    ref.eval()
    g = torch.Generator().manual_seed(SEED)
    out = {"seed": np.int64(SEED), "lens": np.array(LENS, np.int64), "labels": np.array(LABELS)}
    for i, n in enumerate(LENS):
        t = torch.arange(n, dtype=torch.float64) / 16000
        w = (0.3 * torch.sin(2 * np.pi * (180 + 40 * i) * t) + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()
        out[f"wav_{i}"] = w.numpy()
        for name, dt in (("32", torch.float32), ("64", torch.float64)):
            m = ref.to(dt)
            with torch.no_grad():
                src = torch.nn.functional.layer_norm(w.to(dt), w.shape).view(1, -1)
                x = m.extract_features(src, padding_mask=None)["x"]
                p = x.mean(dim=1)
                logits = m.proj(p)
                logits[:, -1] = -np.inf
                prob = torch.softmax(logits, -1)
            out[f"frames{name}_{i}"] = x[0].numpy()
            out[f"pooled{name}_{i}"] = p[0].numpy()
            out[f"probs{name}_{i}"] = prob[0].numpy()
    for h in (4, 12, 16):
        out[f"slopes_{h}"] = (-get_alibi(2, h)[:, 0, 1]).numpy()
    path = os.path.join(ROOT, "tests", "golden", "emotion2vec.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for i in range(len(LENS)):
        print(i, "fp32 vs fp64 max |d| frames", np.abs(out[f"frames32_{i}"] - out[f"frames64_{i}"]).max(),
              "probs", np.abs(out[f"probs32_{i}"] - out[f"probs64_{i}"]).max())
    with open(os.path.join(ROOT, "funasr_amd", "..", "tests", "golden", "emotion2vec_state_dict.json"), "w") as f:
        import yaml
        tmpl = yaml.safe_load(open(os.path.join(os.environ.get("FUNASR_REFERENCE", "/root/reference"),
                                                "funasr", "models", "emotion2vec", "template.yaml")))["model_conf"]
        big = Ref(model_conf=_coerce(tmpl), vocab_size=9)
        json.dump({k: list(v.shape) for k, v in big.state_dict().items()}, f, indent=0)


if __name__ == "__main__":
    main()
