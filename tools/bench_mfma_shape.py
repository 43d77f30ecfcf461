#!/usr/bin/env python3
"""Does the power wall of the f16x2 three-product chain move with the MFMA shape? (tools/micro/mfma_peak.hip; measurement
infrastructure, not product code.)

    python tools/bench_mfma_shape.py peak [seconds] [rounds]   register-resident chains, v_mfma_f32_32x32x16_f16 (mode 0) and
                                                               v_mfma_f32_16x16x32_f16 (mode 2) alternating on one device, random and
                                                               zero hi / lo planes: TFLOP/s, sampled MHz and W per arm, and the ratio
    python tools/bench_mfma_shape.py bits                      one 16x16x32 over k = 0..31 against two chained 32x32x16 (k = 0..15,
                                                               16..31) on the same fp16 operands and start accumulator: equal bits?
Every section prints JSON lines."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from gpu_telemetry import Sampler  # noqa: E402

dev = torch.device("cuda:0")


def load():
    lib = C.CDLL(os.path.join(ROOT, "tools", "micro", "mfma_peak.so"))
    lib.mfma_peak_run.restype = C.c_float
    lib.mfma_peak_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.mfma_shape_bits.restype = C.c_int
    lib.mfma_shape_bits.argtypes = [C.c_void_p] * 5
    return lib


def planes(tiles, data, seed=3):
    """[4 kinds (A hi, A lo, W hi, W lo)][tiles][64 lanes][8] fp16: the planes a GEMM sees, hi = f16(x 2^8), lo = f16(x 2^8 - hi) of
    N(0, 1) values. The 32x32x16 form reads 4 tiles per kind, the 16x16x32 form 8 (the first 4 of each kind are the same values)."""
    n = tiles * 64 * 8
    if data == "zeros":
        return torch.zeros(4, n, device=dev, dtype=torch.float16)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(2, 8 * 64 * 8, device=dev, generator=g) * 256.0
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return torch.stack([hi[0, :n], lo[0, :n], hi[1, :n], lo[1, :n]]).contiguous()


def peak(seconds=2.0, rounds=3):
    lib = load()
    scratch = torch.zeros(16, device=dev)
    blocks = 256
    # (mode, tiles per kind, iterations, FLOP per iteration and wave): equal FLOP per launch
    arms = {"32x32x16": (0, 4, 2000, 48 * 32768.0), "16x16x32": (2, 8, 1000, 192 * 16384.0)}
    for data in ("random", "zeros"):
        rows = {k: [] for k in arms}
        for rnd in range(rounds if data == "random" else 1):
            for name, (mode, tiles, iters, fl) in arms.items():
                pl = planes(tiles, data)
                flops = blocks * 4 * iters * fl
                lib.mfma_peak_run(pl.data_ptr(), mode, blocks, iters, 3, scratch.data_ptr())     # warm
                smp = Sampler(period_s=0.05).start()
                t0, ms = time.time(), []
                while time.time() - t0 < seconds:
                    ms.append(lib.mfma_peak_run(pl.data_ptr(), mode, blocks, iters, 20, scratch.data_ptr()))
                tel = smp.stop()
                if min(ms) < 0:
                    raise RuntimeError("mfma_peak_run failed")
                tail = ms[len(ms) // 2:]
                m = sum(tail) / len(tail)
                row = {"kernel": "mfma_peak", "shape": name, "mode": mode, "dtype": "f16", "data": data, "round": rnd, "seconds": seconds,
                       "ms_per_launch": round(m, 4), "TFLOPs": round(flops / m / 1e9, 1),
                       "sclk_mhz_mean": tel.get("sclk_mhz_mean"), "power_w_mean": tel.get("power_w_mean"), "telemetry": tel}
                rows[name].append(row["TFLOPs"])
                print(json.dumps(row), flush=True)
        a, b = statistics.median(rows["32x32x16"]), statistics.median(rows["16x16x32"])
        print(json.dumps({"summary": "16x16x32 / 32x32x16", "data": data, "TFLOPs_32x32x16": rows["32x32x16"], "TFLOPs_16x16x32": rows["16x16x32"],
                          "median_ratio": round(b / a, 4), "min_ratio": round(min(rows["16x16x32"]) / max(rows["32x32x16"]), 4)}), flush=True)


def bits():
    lib = load()
    g = torch.Generator(device=dev).manual_seed(5)
    total = {}
    for kind in ("hi_planes", "lo_times_hi", "wide_exponents", "cancelling", "small_ints"):
        diff_runs, diff_elems, worst = 0, 0, 0.0
        for trial in range(64):
            if kind == "small_ints":
                a = torch.randint(-8, 9, (32, 32), device=dev, generator=g).float()
                w = torch.randint(-8, 9, (32, 32), device=dev, generator=g).float()
                c = torch.randint(-64, 65, (32, 32), device=dev, generator=g).float()
            else:
                a = torch.randn(32, 32, device=dev, generator=g) * 256.0
                w = torch.randn(32, 32, device=dev, generator=g) * 4096.0 * 32 ** -0.5
                c = torch.randn(32, 32, device=dev, generator=g) * 2.0 ** 20
                if kind == "lo_times_hi":
                    a = a - a.half().float()
                elif kind == "wide_exponents":
                    a = a * torch.exp2(torch.randint(-10, 5, (32, 32), device=dev, generator=g).float())
                    w = w * torch.exp2(torch.randint(-10, 3, (32, 32), device=dev, generator=g).float())
                elif kind == "cancelling":
                    a[:, 16:] = -a[:, :16]
                    w[:, 16:] = w[:, :16] * (1 + 2.0 ** -9)
                    c = c * 2.0 ** -20
            a, w, c = a.half().contiguous(), w.half().contiguous(), c.contiguous()
            d32, d16 = torch.full((32, 32), float("nan"), device=dev), torch.full((32, 32), float("nan"), device=dev)
            if lib.mfma_shape_bits(a.data_ptr(), w.data_ptr(), c.data_ptr(), d32.data_ptr(), d16.data_ptr()) != 0:
                raise RuntimeError("mfma_shape_bits failed")
            ref = c.double() + a.double() @ w.double().T
            bar = 1e-5 * (c.double().abs() + a.double().abs() @ w.double().abs().T).max()      # fp32 accumulation, far below a wrong map
            assert bool(((d32.double() - ref).abs() <= bar).all()), "32x32x16 lane map of the probe is wrong"
            assert bool(((d16.double() - ref).abs() <= bar).all()), "16x16x32 lane map of the probe is wrong"
            ne = d32.view(torch.int32) != d16.view(torch.int32)
            n = int(ne.sum())
            diff_runs += n > 0
            diff_elems += n
            if n:
                worst = max(worst, float(((d32 - d16).abs() / ref.abs().float().clamp(min=1e-30))[ne].max()))
        total[kind] = diff_elems
        print(json.dumps({"bits": kind, "trials": 64, "trials_with_a_difference": diff_runs, "elements_differing": diff_elems,
                          "of": 64 * 1024, "worst_rel_difference": worst}), flush=True)
    print(json.dumps({"bits_equal": all(v == 0 for v in total.values()), "elements_differing": total}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "peak"
    print(json.dumps({"section": what}), flush=True)
    if what == "bits":
        bits()
    else:
        peak(*( [float(sys.argv[2])] if len(sys.argv) > 2 else []), *([int(sys.argv[3])] if len(sys.argv) > 3 else []))
