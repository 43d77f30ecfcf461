"""RWKV encoder time on the GPU at the geometry of funasr/models/rwkv_bat/template.yaml (D 512, 18 blocks, linear_size 2048, every
second frame kept, 80 features) on synthetic weights: 1 x 30 s and 16 x 30 s of features through the HIP handle (RWKVEncoder.forward),
the split of one forward over the front's convs / every linear / the WKV scan / the row kernels from the library's HIP events
(pf_prof_*), and the same batch through the fp32 torch restatement (tests/_rwkv_oracle.py in float32: parallel in time, the WKV as
the sequential recurrence) on the same GPU.
FLOPs are counted from the shapes (2 M N K of every conv and linear); the fraction is of the measured fp32 matrix rate.
One JSON line (and --out FILE, default profiles/rwkv_encoder_bench.json). bench.py is not involved.

    python tools/bench_rwkv.py [--reps 5] [--seconds 30] [--no-eager]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MATRIX_PEAK_TFLOPS = 155.0          # measured v_mfma_f32_32x32x2_f32 rate of one MI355X (tools/bench_eres2net.py)


def gflop_per_clip(D: int, H: int, blocks: int, F: int, T: int) -> dict:
    """2 M N K of one clip of T feature frames: the six convs and the output linear (front), the seven linears of every block"""
    ch = (1, D // 4, D // 4, D // 2, D // 2, D, D)
    st = (1, 2, 1, 2, 1, 1)
    t, f, front = T, F, 0.0
    for i in range(6):
        t, f = (t - 1) // st[i] + 1, (f - 1) // st[i] + 1
        front += 2.0 * t * f * ch[i + 1] * 9 * ch[i]
    front += 2.0 * t * D * (f * D)
    per_block = 2.0 * t * (5 * D * D + 2 * D * H)
    return {"front": front / 1e9, "blocks": blocks * per_block / 1e9, "frames_after_front": t}


def timed(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def split_by_tag(lib, fn) -> dict:
    """ms of ONE forward per profiling tag"""
    lib.pf_prof_reset()
    lib.pf_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    cap = 64
    tags, kinds = (C.c_char_p * cap)(), (C.c_int * cap)()
    ms, work, n = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    got = lib.pf_prof_read_tags(cap, tags, kinds, ms, work, n)
    lib.pf_prof_enable(0)
    lib.pf_prof_reset()
    out = {}
    for i in range(max(got, 0)):
        tag = tags[i].decode()
        rec = out.setdefault(tag, {"ms": 0.0, "launches": 0})
        rec["ms"] += float(ms[i])
        rec["launches"] += int(n[i])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rwkv_encoder_bench.json"))
    args = ap.parse_args()

    from funasr_amd import _lib, synth
    from funasr_amd.rwkv_encoder import RWKVEncoder
    from tests import _rwkv_oracle as O

    dev = torch.device("cuda:0")
    conf = synth.rwkv_encoder_conf(linear_size=None, **synth.RWKV_TEMPLATE)
    enc = RWKVEncoder(input_size=80, **conf)
    sd = synth.rwkv_encoder_state_dict(1, enc)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev)
    lib = _lib.load()
    T = int(round(args.seconds * 100))
    D, H, r = enc.output_size(), enc.linear_size, enc.time_reduction_factor
    gf = gflop_per_clip(D, H, enc.num_blocks, 80, T)
    res = {"what": "RWKVEncoder, template geometry, synthetic weights, fp32", "frames_per_clip": T, "chunk_length": int(lib.pf_k_rwkv_chunk()),
           "gflop_per_clip": gf, "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS, "cases": {}}
    sd32 = O.cast(sd, torch.float32, dev)
    for B in (1, 16):
        feats = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(B)).to(dev)
        lens = [T] * B
        ms = timed(lambda: enc(feats, lens), args.reps)
        total = B * (gf["front"] + gf["blocks"])
        case = {"encoder_ms": ms, "tflops": total / ms, "fraction_of_fp32_matrix_peak": total / ms / FP32_MATRIX_PEAK_TFLOPS,
                "audio_seconds_per_second": B * args.seconds / (ms / 1e3), "split_ms": split_by_tag(lib, lambda: enc(feats, lens))}
        wkv = case["split_ms"].get("rwkv.wkv")
        if wkv:
            case["wkv_us_per_block"] = 1e3 * wkv["ms"] / enc.num_blocks
        if not args.no_eager:
            with torch.no_grad():                                   # (clip after clip; one timed pass, warmed by its first clip)
                O.encode_batch(feats[:1], lens[:1], sd32, r)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                O.encode_batch(feats, lens, sd32, r)
                torch.cuda.synchronize()
                case["torch_fp32_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        res["cases"][f"{B}x{int(args.seconds)}s"] = case
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
