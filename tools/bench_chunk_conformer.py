"""Chunk-window attention and ChunkConformerEncoder time on the GPU.

Kernels, ONE run, the variants alternating round by round (device events around `--launches` launches each; per variant the median over
the rounds and the spread (max - min) / median): at H = 8 heads and T = 1500 encoder frames (60 s at 1/4 subsampling), B = 1 and 16
clips, the windowed kernel (pf_k_cc_window_attention) at chunk 16 with left_chunk_size 0, 4 and -1 and without a chunk mask, beside the
full "latest" relative-position kernel (pf_k_relpos_attention) on the same operands. Recorded: the times, the ratios to the full kernel,
the 32-key tiles each workgroup walks (counted from the window rule), and two conditions:
  left 4 is faster than the full kernel (it walks about a tenth of the tiles);
  left -1 (all of the past: half the tiles on average) is not slower than the full kernel by more than the recorded spread.
Encoder: one 30-s clip and sixteen at D 512 / 8 heads / 12 blocks / linear_units 2048 / kernel 15, subsampling 4, dynamic mode (chunk
16, left 4), beside ConformerEncoder at the same size in fp32 and in its default f16x2, from the same run. Recorded only.
One JSON line (and --out FILE, default profiles/chunk_conformer_bench.json). bench.py is not involved.

    python tools/bench_chunk_conformer.py [--rounds 7] [--launches 50] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tiles_walked(T: int, chunk: int, left: int) -> int:
    """32-key tiles the workgroups of one (clip, head) walk: per 128 queries, the tiles meeting [start(first), end(last))"""
    from funasr_amd.chunk_conformer import chunk_window

    n = 0
    for q0 in range(0, T, 128):
        lo, hi = chunk_window(q0, T, chunk, left)[0], chunk_window(min(q0 + 127, T - 1), T, chunk, left)[1]
        n += (hi - 1) // 32 - lo // 32 + 1
    return n


def event_ms(fn, launches: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def timed(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_conformer_bench.json"))
    args = ap.parse_args()

    from funasr_amd import _lib, synth
    from funasr_amd.chunk_conformer import ChunkConformerEncoder
    from funasr_amd.conformer import ConformerEncoder

    assert torch.cuda.is_available(), "this is a GPU measurement"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    H, T, c = 8, args.frames, 16
    D = 64 * H
    s = torch.cuda.current_stream().cuda_stream
    res = {"what": "chunk-window attention against the full relative-position kernel, exact fp32, one run, variants alternating",
           "H": H, "T": T, "chunk": c, "rounds": args.rounds, "launches_per_round": args.launches, "kernels": {}}
    for B in (1, 16):
        g = torch.Generator().manual_seed(B)
        qkv = torch.randn(B * T, 3 * D, generator=g).to(dev)
        P = torch.randn(2 * T - 1, D, generator=g).to(dev)
        u, v = (0.3 * torch.randn(H, 64, generator=g)).to(dev), (0.3 * torch.randn(H, 64, generator=g)).to(dev)
        kl = torch.full((B,), T, dtype=torch.int32, device=dev)
        out = torch.empty(B * T, D, device=dev)

        def full():
            _lib.check(lib.pf_k_relpos_attention(qkv.data_ptr(), P.data_ptr(), u.data_ptr(), v.data_ptr(), kl.data_ptr(), B, T, H, 0, out.data_ptr(), s),
                       "pf_k_relpos_attention")

        def windowed(chunk, left):
            def fn():
                _lib.check(lib.pf_k_cc_window_attention(qkv.data_ptr(), P.data_ptr(), u.data_ptr(), v.data_ptr(), kl.data_ptr(), B, T, H, chunk, left,
                                                        out.data_ptr(), s), "pf_k_cc_window_attention")
            return fn

        variants = {"full": (full, tiles_walked(T, 0, 0)), "window_no_mask": (windowed(0, 0), tiles_walked(T, 0, 0)),
                    "window_left0": (windowed(c, 0), tiles_walked(T, c, 0)), "window_left4": (windowed(c, 4), tiles_walked(T, c, 4)),
                    "window_leftall": (windowed(c, -1), tiles_walked(T, c, -1))}
        for fn, _ in variants.values():                               # warm up every shape of the timed window
            event_ms(fn, 5)
        ms = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, (fn, _) in variants.items():
                ms[k].append(event_ms(fn, args.launches))
        case = {}
        for k, (_, tiles) in variants.items():
            med = statistics.median(ms[k])
            case[k] = {"us": 1e3 * med, "spread": (max(ms[k]) - min(ms[k])) / med, "tiles_per_clip_and_head": tiles}
        base = case["full"]["us"]
        for k in variants:
            case[k]["ratio_to_full"] = case[k]["us"] / base
        spread = max(case["full"]["spread"], case["window_leftall"]["spread"])
        case["conditions"] = {"left4_faster_than_full": case["window_left4"]["us"] < base,
                              "leftall_not_slower_than_full_beyond_spread": case["window_leftall"]["us"] <= base * (1.0 + spread)}
        res["kernels"][f"B{B}"] = case

    size = dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=12, cnn_module_kernel=15)
    cc = ChunkConformerEncoder(input_size=80, **synth.chunk_conformer_conf(mode="dynamic", default_chunk_size=16, left_chunk_size=4,
                                                                           time_reduction_factor=1, **size))
    cc.load_state_dict(synth.conformer_state_dict(1, cc), strict=True)
    cc = cc.to(dev)
    cf_conf = synth.conformer_conf(output_size=512, attention_heads=8, linear_units=2048, enc_blocks=12)["encoder_conf"]
    cf_conf["cnn_module_kernel"] = 15
    cf = ConformerEncoder(input_size=80, **cf_conf)
    cf.load_state_dict(synth.conformer_state_dict(1, cf), strict=True)
    cf = cf.to(dev)
    res["encoder"] = {"what": "D 512 / 8 heads / 12 blocks / linear_units 2048 / kernel 15, 30-s clips of 80 features, synthetic weights; "
                              "ChunkConformerEncoder in dynamic mode (chunk 16, left 4, fp32) beside ConformerEncoder (recorded only)",
                      "conformer_macaron": bool(cf.macaron), "cases": {}}
    for B in (1, 16):
        feats = torch.randn(B, 3000, 80, generator=torch.Generator().manual_seed(B)).to(dev)
        lens = [3000] * B
        case = {"chunk_conformer_dynamic_fp32_ms": timed(lambda: cc(feats, lens), args.reps)}
        for mode in ("fp32", "f16x2"):
            cf.set_precision(mode)
            case[f"conformer_{mode}_ms"] = timed(lambda: cf(feats, lens), args.reps)
        res["encoder"]["cases"][f"{B}x30s"] = case
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
