"""CAM++ embedding throughput on the GPU: N 1.5-s chunks (148 frames) through the HIP network (CAMPPlus.forward on ready features,
and CAMPPlus.embed_chunks from a device waveform, fbank included), and the same network as a torch fp32 eager restatement
(tests/_campplus_oracle.py in float32: MIOpen convolutions / hipBLAS GEMMs) on the same features for comparison.
One JSON line. bench.py is not involved.

    python tools/bench_campplus.py --chunks 4800 --reps 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GFLOP_PER_CHUNK = 1.67          # per 148-frame chunk, counted over the convolutions of the reference module


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4800)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--eager-chunks", type=int, default=480, help="chunks per eager call (the eager path's memory bound)")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    from funasr_amd import synth
    from funasr_amd.campplus import CAMPPlus
    from tests import _campplus_oracle as O

    dev = torch.device("cuda:0")
    sd = synth.campplus_state_dict(0)
    m = CAMPPlus(max_batch=a.max_batch)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    N, L = a.chunks, 24000
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, 148, 80, generator=g).to(dev)
    wav = (0.1 * torch.randn(N * L // 2 + L, generator=g)).to(dev)
    starts = [i * (L // 2) for i in range(N)]
    res = {"chunks": N, "max_batch": a.max_batch}
    t = _time(lambda: m(x), a.reps)
    res["hip_forward_ms"] = round(1e3 * t, 2)
    res["hip_forward_tflops"] = round(N * GFLOP_PER_CHUNK / t / 1e3, 2)
    t = _time(lambda: m.embed_chunks(wav, starts, L), a.reps)
    res["hip_embed_chunks_ms"] = round(1e3 * t, 2)
    if not a.no_eager:
        sd_dev = {k: v.to(dev) for k, v in sd.items()}
        step = a.eager_chunks

        def eager():
            with torch.no_grad():
                for i in range(0, N, step):
                    O.forward(x[i:i + step], sd_dev, torch.float32)
        t = _time(eager, a.reps)
        res["torch_eager_ms"] = round(1e3 * t, 2)
        res["speedup_vs_eager"] = round(res["torch_eager_ms"] / res["hip_forward_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
