"""ERes2NetV2 embedding throughput on the GPU at the default configuration: N 1.5-s chunks (150 frames) through the HIP network
(ERes2NetV2SV.forward on ready features, and ERes2NetV2SV.embed_chunks from a device waveform, fbank included), then the same
network as a torch fp32 eager restatement (tests/_eres2net_oracle.py in float32: MIOpen convolutions) on the same features, in
the process order of tools/bench_campplus.py. Also one 3x3, stride-1, 32 -> 32 channel conv on this network's conv kernel and on
CAM++'s (pf_k_eres_conv_vs_cam_time): the one shape both kernels can run.
FLOPs are counted from the shapes (2 M N K over every conv with its true channel counts, the stem and seg_1 included).
One JSON line (and --out FILE). bench.py is not involved.

    python tools/bench_eres2net.py --chunks 4800 --reps 3 --out profiles/eres2net_bench_4800.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_eres2net.py --chunks 960 --reps 1 --no-eager --no-compare
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP32_MATRIX_PEAK_TFLOPS = 155.0          # measured v_mfma_f32_32x32x2_f32 rate of one MI355X


def gflop_per_chunk(conf: dict, T: int) -> dict:
    """2 M N K of every conv of one chunk of T frames, by group"""
    mc, F = conf["m_channels"], conf["feat_dim"]
    out = {"stem": 2.0 * T * F * mc * 9}
    t, f, cin = T, F, mc
    for i, n in enumerate(conf["num_blocks"]):
        planes = mc << i
        w, O = planes * 26 // 64, 2 * planes
        tot = 0.0
        for b in range(n):
            if b == 0 and i > 0:
                t, f = (t - 1) // 2 + 1, (f - 1) // 2 + 1
            pos = t * f
            tot += 2.0 * pos * (2 * w * cin + 2 * 9 * w * w + O * 2 * w)
            if b == 0:
                tot += 2.0 * pos * O * cin                                  # projection shortcut
            if i >= 2:
                tot += 2.0 * pos * (2 * w * (w // 4) + (w // 4) * w)        # AFF
            cin = O
        out[f"layer{i + 1}"] = tot
    C3, C4 = 8 * mc, 16 * mc
    out["layer3_ds"] = 2.0 * t * f * C4 * 9 * C3
    out["fuse34"] = 2.0 * t * f * (2 * C4 * (C4 // 4) + (C4 // 4) * C4)
    out["seg_1"] = 2.0 * conf["embedding_size"] * 2 * f * C4
    out = {k: v / 1e9 for k, v in out.items()}
    out["total"] = sum(out.values())
    return out


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
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--eager-chunks", type=int, default=96, help="chunks per eager call (the eager path's memory bound)")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-compare", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from funasr_amd import _lib, synth
    from funasr_amd.eres2net import ERes2NetV2SV
    from tests import _eres2net_oracle as O
    from tools.gpu_telemetry import Sampler

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    m = ERes2NetV2SV(max_batch=a.max_batch)
    conf = dict(feat_dim=m.feat_dim, embedding_size=m.embedding_size, m_channels=m.m_channels, num_blocks=m.num_blocks)
    sd = synth.eres2net_state_dict(0, m)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    N, T = a.chunks, a.frames
    L = 400 + (T - 1) * 160
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, T, m.feat_dim, generator=g).to(dev)
    wav = (0.1 * torch.randn(N * L // 2 + L, generator=g)).to(dev)
    starts = [i * (L // 2) for i in range(N)]
    gf = gflop_per_chunk(conf, T)
    res = {"chunks": N, "frames": T, "max_batch": a.max_batch, "gflop_per_chunk": {k: round(v, 3) for k, v in gf.items()},
           "workspace_mb_per_chunk": round(m.workspace_bytes(T) / 2 ** 20, 2)}
    tel = Sampler().start()
    t = _time(lambda: m(x), a.reps)
    res["telemetry_hip_forward"] = tel.stop()
    res["hip_forward_ms"] = round(1e3 * t, 2)
    res["hip_forward_tflops"] = round(N * gf["total"] / t / 1e3, 2)
    res["hip_forward_frac_of_fp32_matrix_peak"] = round(res["hip_forward_tflops"] / FP32_MATRIX_PEAK_TFLOPS, 3)
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
        with torch.no_grad():
            ref = O.forward(x[:8], sd_dev, torch.float32)
        res["max_abs_diff_vs_eager_8_chunks"] = float((m(x[:8].contiguous()) - ref).abs().max())
    if not a.no_compare:
        # CAM++'s head conv shape: 3x3, stride 1, 32 -> 32 channels over [chunks, 148, 80]
        n, Tc, Fc, C = 256, 148, 80, 32
        A = torch.randn(n, Tc, Fc, C, device=dev)
        W = torch.randn(C, 9 * C, device=dev) * 0.06
        out = torch.empty(n * Tc * Fc, C, device=dev)
        ms = (ctypes.c_float * 2)()
        _lib.check(_lib.load().pf_k_eres_conv_vs_cam_time(A.data_ptr(), W.data_ptr(), out.data_ptr(), n, Tc, Fc, C, C, 20, ms,
                                                          torch.cuda.current_stream().cuda_stream), "pf_k_eres_conv_vs_cam_time")
        fl = 2.0 * n * Tc * Fc * C * 9 * C / 1e9
        res["conv3x3_c32"] = {"gflop": round(fl, 2), "eres_conv_ms": round(ms[0], 4), "cam_gemm_ms": round(ms[1], 4),
                              "eres_conv_tflops": round(fl / ms[0], 2), "cam_gemm_tflops": round(fl / ms[1], 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
