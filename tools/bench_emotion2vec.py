"""emotion2vec throughput on one MI355X: batch 32 x 10-s clips and 4 x 60-s clips at the base (768, 12 heads, 4 + 8 blocks) and
large (1024, 16 heads, 8 + 16) shapes, the HIP network in its f16x2 and fp32 modes and the torch fp32 eager restatement
(tests/_emotion2vec_oracle.py, one utterance at a time as the reference runs) on the same GPU, on synthetic weights. Prints one
JSON line (audio-s/s and ms per batch) and writes it to profiles/emotion2vec_bench.json (--out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def main():
    from funasr_amd import synth
    from funasr_amd.emotion2vec import Emotion2vec
    from tests import _emotion2vec_oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", default="base,large")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emotion2vec_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    shapes = {"base": synth.emotion2vec_conf(768, 12, 4, 8), "large": synth.emotion2vec_conf(1024, 16, 8, 16)}
    batches = {"32x10s": [160000] * 32, "4x60s": [960000] * 4}
    g = torch.Generator().manual_seed(0)
    out = {"metric": "emotion2vec audio-s/s", "results": {}}
    for sname in a.shapes.split(","):
        conf = shapes[sname]
        m = Emotion2vec(model_conf=conf, vocab_size=9)
        sd = synth.emotion2vec_state_dict(1, m)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        cfg = O.cfg_of(m)
        for bname, lens in batches.items():
            wav = (0.1 * torch.randn(sum(lens), generator=g)).to(dev)
            audio_s = sum(lens) / 16000
            row = {}
            for mode in ("f16x2", "fp32"):
                m.set_precision(mode)
                ms = _time(lambda: m.forward_packed(wav, lens, frames=False), a.warmup, a.iters)
                row[mode] = {"ms_per_batch": round(ms, 2), "audio_s_per_s": round(audio_s / ms * 1e3, 1)}
            if not a.no_eager:
                chunks = torch.split(wav, lens)

                def eager():
                    with torch.no_grad():
                        for w in chunks:
                            O.head(O.features(w, sdd, cfg, torch.float32), sdd, ["x"] * 9)

                ms = _time(eager, min(a.warmup, 1), 1)
                row["torch_fp32_eager"] = {"ms_per_batch": round(ms, 2), "audio_s_per_s": round(audio_s / ms * 1e3, 1)}
                row["f16x2_speedup_vs_eager"] = round(ms / row["f16x2"]["ms_per_batch"], 2)
            out["results"][f"{sname}_{bname}"] = row
            print(sname, bname, json.dumps(row), file=sys.stderr, flush=True)
        del m
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
