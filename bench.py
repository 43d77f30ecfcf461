#!/usr/bin/env python3
"""Headline benchmark: audio-seconds per wall-second (RTF^-1) of the full Paraformer-large hot path on MI355X.

One "step" = one pass of the hot path over one batch of synthetic input that is already resident in HBM:
  [B, 480000] float32 PCM -> fbank/LFR/CMVN -> 50-block SAN-M encoder -> CIF predictor -> 16-block SAN-M decoder
  -> fused vocabulary arg-max -> token ids on the host (one D2H copy), i.e. BASELINE.json configs[1]
  ("Paraformer-large, batch=64 synthetic 30 s 16 kHz clips, 1 x MI355X"), random-initialised weights of the exact
  architecture (funasr_amd/synth.py), 64 DISTINCT clips. Arithmetic is fp32-class: the dense GEMMs and the encoder's
  self-attention run on the fp16 matrix cores with every operand split into two fp16 planes (x 2^e = hi + lo, three
  products, fp32 accumulate: gemm_f16x2.hip / attention_f16x2.hip, mode "f16x2"), everything else on the fp32 kernels;
  this mode meets every fp32 parity bar of tests/test_parity_gpu.py. The timed region carries NO instrumentation; the
  per-kernel numbers (`roofline`, `kernels`) come from a second, hipEvent-instrumented pass over the same steps.

A plain run does only what the headline figure needs: set up, calibrate the output layer, warm up, time K steps, write the
last step's outputs if --dump-outputs DIR is given (DIR/<name>.npy, float64: token counts and token ids per clip, what
Paraformer.collect returns to a caller), print the line. Everything else runs with --full only: the instrumented pass
behind `roofline` / `kernels`, the clock / power telemetry of the timed region, and (N = 1 only) beside `value` the
PCIe-inclusive rate (waveforms start in pinned host memory), the other arithmetic modes, full-configuration parity
evidence against the CPU oracle, the CPU baseline in two thread settings, and the secondary workloads of BASELINE.json
(configs[2] SenseVoiceSmall 128 x 10 s, configs[4] streaming).

Multi-GPU (utterance-level data parallelism, weak scaling): one process per GPU, rank 0 builds the weights and
broadcasts ONE packed arena over RCCL, every rank decodes its own 64 clips, hypotheses are gathered on rank 0
inside the timed region. No collective touches the data path.

Contract: python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]   (N>1: either under
torch.distributed.run with N ranks, or bare -- the script then re-executes itself as N ranks, funasr_amd.dp.ensure_ranks; a
world size other than N is an error) prints ONE JSON line on rank 0 (see README / DESIGN.md for the fields, incl. `roofline`
and `cpu_baseline`, which only --full fills).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_16BIT_MFMA_TFLOPS = 2500.0   # same guide, dense bf16 / fp16 (never the 2:1-sparsity figure)
PRODUCTS = {"bf16x3": 6, "f16x2": 3}   # 16-bit MFMA products per fp32-equivalent product
PEAK_HBM_GBS = 8000.0
MODE_DTYPE = {
    "fp32": "f32",
    "bf16": "bf16 operands / f32 accumulate",
    "bf16x3": "f32 (GEMM operands split into 3 bf16 planes, 6 bf16 MFMA products, f32 accumulate; all else f32)",
    "f16x2": "f32 (GEMM / self-attention operands split into 2 fp16 planes, 3 fp16 MFMA products, f32 accumulate; all else f32)",
}

_T0 = time.perf_counter()


def trace(msg):
    """stage timestamps on stderr (stdout carries only the JSON line)"""
    print(f"[bench +{time.perf_counter() - _T0:7.2f}s] {msg}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64, help="clips per GPU per step")
    ap.add_argument("--seconds", type=float, default=30.0, help="clip length")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-decoder-stream", action="store_true", help="the two-phase loop with both phases on ONE stream (default: batch i's decoder on a "
                    "second HIP stream, beside batch i+1's encoder; one model replica, one set of weights)")
    ap.add_argument("--no-interleave", action="store_true", help="round 5's loop: whole batches enqueued one after the other (the host's wait for "
                    "the CIF token count then sits between a batch's encoder and decoder); default: the two-phase loop (begin(i+1), finish(i), collect(i-1))")
    ap.add_argument("--no-bf16", action="store_true", help="skip the other arithmetic modes (fp32-MFMA, bf16x3, bf16 operands)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary workloads (PCIe-inclusive, SenseVoiceSmall, streaming)")
    ap.add_argument("--precision", default="f16x2", choices=["fp32", "bf16", "bf16x3", "f16x2"], help="mode of the MAIN timed region: "
                    "f16x2 (default) = fp32-class results, GEMM / attention operands as two fp16 planes on the fp16 MFMA (3 products); "
                    "bf16x3 = three bf16 planes (6 products); fp32 = every GEMM on the fp32 MFMA; bf16 = bf16 operands "
                    "(bf16-class error; for profiling the throughput mode)")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL over xGMI) | gloo (dry run of the N>1 code "
                    "path with every rank on cuda:0 of a single-GPU box)")
    ap.add_argument("--cpu-clips", type=int, default=64, help="max clips of the same workload timed on the host oracle")
    ap.add_argument("--cpu-budget", type=float, default=12.0, help="seconds of CPU work per thread setting")
    ap.add_argument("--enc-option", action="append", default=[], metavar="KEY=VALUE", help="A/B runs: encoder schedule options of the "
                    "f16x2 mode (pf_encoder_set_option), e.g. fuse_row=0, attn_variant=1; results are bitwise / fp32-class equal")
    ap.add_argument("--random-output-layer", action="store_true", help="keep the random-init output layer for the headline run "
                    "(default: the calibrated confident layer, synth.confident_output_layer; arithmetic and cost are identical)")
    ap.add_argument("--weights-route", default="arena", choices=["arena", "device"], help="N > 1: how rank 0's weights reach the other ranks -- "
                    "arena: one packed fp32 tensor through torch.distributed (RCCL broadcast), each rank re-uploads into its handles; "
                    "device: the C ABI's pf_dp_broadcast_* straight into the module handles' HBM (funasr_amd.dp.broadcast_model_device; "
                    "falls back to the arena if any rank fails). The arena is the default because no multi-GPU box has ever run either "
                    "route (DESIGN 6) and a first contact that hangs inside a never-exercised communicator would lose the whole line")
    ap.add_argument("--cpu-threads", type=int, default=0, help="cap on host threads for the CPU baseline (0 = all usable)")
    ap.add_argument("--full", action="store_true", help="everything beside the headline figure: the instrumented pass (`roofline`, "
                    "`kernels`), telemetry, and at N = 1 the A/B loops, the secondary workloads, the other modes and the CPU baseline "
                    "(the --no-* switches above select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last step computed "
                    "(rank 0: token counts and token ids per clip) as DIR/<name>.npy in float64")
    return ap.parse_args()


def build_model(cfg, rank, world, device, route="arena"):
    """rank 0 draws the synthetic checkpoint; with world > 1 it is shipped as one packed arena (RCCL broadcast)."""
    from funasr_amd import synth
    from funasr_amd.paraformer import Paraformer

    model = Paraformer.from_config(cfg)
    arena_bytes = 0
    if rank == 0:
        sd = synth.paraformer_state_dict(cfg, seed=0, cif_bias=synth.BENCH_CIF_BIAS)
        model.load_state_dict(sd, strict=False)
    model = model.to(device)
    bcast_s = 0.0
    if world > 1:
        from funasr_amd import dp
        torch.cuda.synchronize()
        tb = time.perf_counter()
        done = False
        if route == "device":
            import torch.distributed as dist
            ok = 1
            try:
                comm = dp.DeviceComm.from_process_group(device)
                arena_bytes = dp.broadcast_model_device(model, comm, src=0)     # grouped in-place broadcasts into the handles
            except Exception as e:                               # noqa: BLE001
                trace(f"rank {rank}: device route failed ({e!r})")
                ok = 0
            flag = torch.tensor([ok], dtype=torch.int32, device=device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            done = bool(flag.item())
            if not done:
                trace(f"rank {rank}: some rank could not take the device route: every rank falls back to the arena")
        if not done:
            arena_bytes = dp.broadcast_model(model, src=0)      # ONE packed fp32 arena over RCCL (~880 MB)
        torch.cuda.synchronize()
        bcast_s = time.perf_counter() - tb
        trace(f"rank {rank}: weights broadcast ({'C ABI, in place' if done else 'packed arena'}), {arena_bytes / 1e6:.0f} MB in {bcast_s:.2f} s")
    return model, arena_bytes, bcast_s


def run_two_replicas(cfg, model, frontend, wav, lens, args, B, device, res_main):
    """A reported variant, never `value`: a SECOND replica of the model (own handles and workspaces, same weights) on its own HIP
    stream, batches dealt round-robin, each replica software-pipelined like the headline loop. One replica's frontend / predictor /
    decoder phases (few rows, launch-bound) then run beside the other's encoder GEMMs (tools/exp_two_streams.py)."""
    from funasr_amd.paraformer import Paraformer
    from funasr_amd.wav_frontend import WavFrontend
    m2 = Paraformer.from_config(cfg)
    m2.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=False)
    m2 = m2.to(device)
    m2.set_precision(args.precision)
    models = [model, m2]
    fes = [frontend, WavFrontend(cmvn=frontend.cmvn, lfr_m=7, lfr_n=6, dither=0.0, device=device)]
    streams = [torch.cuda.Stream(device=device) for _ in models]
    torch.cuda.synchronize()

    def run(k):
        pend, last = [[], []], [None, None]
        for i in range(k):
            r = i % 2
            with torch.cuda.stream(streams[r]):
                f, fl = fes[r](wav, lens)
                pend[r].append(models[r].enqueue_features(f, fl))
                if len(pend[r]) > 1:
                    last[r] = models[r].collect(pend[r].pop(0))
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                for p_ in pend[r]:
                    last[r] = models[r].collect(p_)
        return last

    run(4)
    torch.cuda.synchronize()
    k = max(4, args.steps // 2 * 2)
    t0 = time.perf_counter()
    last = run(k)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    m2.close()                              # the pipeline object owns device buffers (two encoder outputs, embeds, ids)
    del m2
    return {"value": round(B * args.seconds * k / dt, 1), "unit": "audio-s/s", "ms_per_step": round(dt / k * 1e3, 2), "steps": k, "replicas": 2,
            "ids_equal_main": all(r is not None and r["raw_ids"] == res_main["raw_ids"] for r in last),
            "note": "two model replicas on two HIP streams of one process; reported beside `value`, which stays the one-stream rate"}


def hbm_copy_probe(device):
    """State of the box's memory system, outside the clock: device-to-device copies, best of 20 (read + write bytes / time) -- 1 GiB
    (beyond the 256-MB infinity cache: HBM) and 32 MiB (both buffers cache-resident: fabric / infinity cache). Boxes of the pool
    differ: on some the memory-bound kernels of the step run 60 % longer at a HIGHER shader clock and LOWER power than on the
    others (profiles/r05_box_variance.jsonl: linear_out 108 vs 177 us) although the matrix-pipe probe and the 1-GiB copy agree."""
    out = {"kernel": "torch copy_ (d2d)", "best_of": 20}
    try:
        for name, n in (("GBps_read_plus_write", 1 << 28), ("GBps_32MiB_cache_resident", 1 << 23)):
            a = torch.empty(n, dtype=torch.float32, device=device).normal_()
            b = torch.empty_like(a)
            for _ in range(3):
                b.copy_(a)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
            ev[0].record()
            for i in range(20):
                b.copy_(a)
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = min(ev[i].elapsed_time(ev[i + 1]) for i in range(20))
            out[name] = round(2 * 4 * n / ms / 1e6, 0)
            del a, b
        out["bytes"] = 4 * (1 << 28)
    except Exception as e:                              # noqa: BLE001
        out["error"] = repr(e)
    try:
        # own probe kernels (tools/micro/mfma_peak.hip, mem_probe_kernel): streaming read / streaming write of 2 GiB, and 2048
        # workgroups re-reading 1-MiB windows 32 times (L2-resident: the pattern of a GEMM workgroup re-streaming its W panel)
        lib = C.CDLL(os.path.join(ROOT, "tools", "micro", "mfma_peak.so"))
        lib.mem_probe_run.restype = C.c_float
        lib.mem_probe_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        n16 = 1 << 27
        buf = torch.empty(n16 * 4, dtype=torch.int32, device=device).random_(0, 1 << 30)
        sink = torch.zeros(4, dtype=torch.int32, device=device)
        torch.cuda.synchronize()
        for name, mode, blocks, reps, byts in (("own_read_GBps", 0, 8192, 1, 16.0 * n16), ("own_write_GBps", 1, 8192, 1, 16.0 * n16),
                                                ("own_L2_reread_GBps", 2, 2048, 32, 2048 * 32 * float(1 << 20))):
            ms = lib.mem_probe_run(buf.data_ptr(), buf.data_ptr(), n16, mode, blocks, reps, 10, sink.data_ptr())
            out[name] = round(byts / ms / 1e6, 0) if ms > 0 else None
        del buf
    except Exception as e:                              # noqa: BLE001
        out["own_probe_error"] = repr(e)
    return out


def power_limited_peak(seconds=1.5):
    """tools/micro/mfma_peak.so (built by __graft_entry__.build()): 256 workgroups x 4 waves of register-resident
    v_mfma_f32_32x32x16_f16 chains in the f16x2 GEMM's product pattern on random hi / lo planes, for `seconds`; executed TFLOP/s
    of the second half of the run with the sampled clock and power. Falls back to the recorded run (profiles/r05a_w4_first_run.jsonl)."""
    so = os.path.join(ROOT, "tools", "micro", "mfma_peak.so")
    try:
        lib = C.CDLL(so)
        lib.mfma_peak_run.restype = C.c_float
        lib.mfma_peak_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        dev = torch.device("cuda", torch.cuda.current_device())
        g = torch.Generator(device=dev).manual_seed(3)
        x = torch.randn(16 * 64 * 8, device=dev, generator=g) * 256.0
        hi = x.to(torch.float16)
        lo = (x - hi.float()).to(torch.float16)
        q = 4 * 64 * 8
        pl = torch.stack([hi[:q], lo[:q], hi[q:2 * q], lo[q:2 * q]]).contiguous()
        scratch = torch.zeros(16, device=dev)
        iters, blocks = 2000, torch.cuda.get_device_properties(dev).multi_processor_count
        flops = blocks * 4 * iters * 48 * 32768.0
        lib.mfma_peak_run(pl.data_ptr(), 0, blocks, iters, 3, scratch.data_ptr())
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from gpu_telemetry import Sampler
        smp = Sampler(device=torch.cuda.current_device(), period_s=0.05).start()
        t0, ms = time.time(), []
        while time.time() - t0 < seconds:
            ms.append(lib.mfma_peak_run(pl.data_ptr(), 0, blocks, iters, 10, scratch.data_ptr()))
        tel = smp.stop()
        tail = ms[len(ms) // 2:]
        m = sum(tail) / len(tail)
        if m <= 0:
            raise RuntimeError("mfma_peak_run failed")
        return {"TFLOPs": round(flops / m / 1e9, 1), "source": f"tools/micro/mfma_peak.so, live, {seconds:g} s on random planes",
                "sclk_mhz_mean": tel.get("sclk_mhz_mean"), "power_w_mean": tel.get("power_w_mean")}
    except Exception as e:                              # noqa: BLE001  (an auxiliary measurement must not lose the line)
        trace(f"power-limited peak not measured live ({e!r}); the line carries the recorded figure, flagged, and no live fraction")
        return {"TFLOPs": None, "recorded_TFLOPs": 1647.0,
                "source": "NOT measured in this run; recorded: profiles/r05a_w4_first_run.jsonl (1647 TFLOP/s at 1782 MHz, 1237 W on another box)"}


def apply_power_limited_peak(roofline: dict, plp: dict, products: int) -> dict:
    """`roofline` + the power-limited ceiling of the matrix pipe (power_limited_peak()). A figure that was not measured in this run
    never turns into a fraction of this run: `frac_of_power_limited_peak` is then null and the recorded number is labelled as such."""
    live = plp.get("TFLOPs")
    if live:
        roofline.update(power_limited_peak=round(live / products, 1), power_limited_peak_executed_16bit=live,
                        frac_of_power_limited_peak=round(roofline["achieved"] / (live / products), 4), power_limited_peak_source=plp["source"],
                        power_limited_peak_sclk_mhz=plp.get("sclk_mhz_mean"), power_limited_peak_power_w=plp.get("power_w_mean"))
    else:
        roofline.update(power_limited_peak=None, frac_of_power_limited_peak=None, power_limited_peak_source=plp["source"],
                        power_limited_peak_recorded=round(plp["recorded_TFLOPs"] / products, 1))
    return roofline


def assemble_roofline(gemm: dict, kname: str, peak: float, step_ms: float, pmc, products=None) -> dict:
    """The `roofline` object of the line from the instrumented pass's figures for the dominant kernel family: `gemm` =
    {work_per_step (algorithmic flops), ms_per_step (hipEvent time on the launch stream), launches_per_step}."""
    ach = gemm["work_per_step"] / (gemm["ms_per_step"] * 1e-3) / 1e12 if gemm["ms_per_step"] > 0 else 0.0
    roofline = dict(bound="mfma", kernel=("gemm_f16x2_kernel + gemm_f16x2_row_kernel" if kname == "gemm_f16x2_" else kname), achieved=round(ach, 2), peak=round(peak, 1),
                    unit="TFLOP/s", frac=round(ach / peak, 4), traffic=pmc[0] if pmc else None,
                    traffic_unit="HBM bytes per launch (PMC)", traffic_source=pmc[1] if pmc else None,
                    flops_per_launch=gemm["work_per_step"] / max(gemm["launches_per_step"], 1),
                    avg_launch_ms=gemm["ms_per_step"] / max(gemm["launches_per_step"], 1),
                    launches_per_step=gemm["launches_per_step"],
                    share_of_step=round(gemm["ms_per_step"] / step_ms, 3))
    if products:
        roofline.update(peak_note=f"dense 16-bit MFMA peak 2500 TFLOP/s / {products} products per fp32-equivalent product",
                        executed_16bit_tflops=round(ach * products, 1), fp32_mfma_peak_for_comparison=PEAK_F32_MFMA_TFLOPS)
    return roofline


def assemble_line(*, value, dt, steps, warmup, world, dtype, B, seconds, token_num, arena_bytes, n_pad, per_rank_ms, bcast_all, weights_route,
                  host_pin, roofline, kernels, telemetry, output_layer) -> dict:
    """The contract part of the JSON line (what the driver reads) from plain values; tests/test_bench_contract.py checks its schema on
    synthetic inputs. `value` = whole-job audio-seconds per second with the waveforms resident in HBM when the clock starts."""
    return {
        "metric": "audio-seconds/sec (RTF^-1) Paraformer-large 30s@bs64", "value": round(value, 1),
        "unit": "audio-s/s", "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": round(dt / steps * 1e3, 2), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": dtype, "data": "synthetic",
        "config": {"workload": f"Paraformer-large (50 enc + 16 dec blocks, vocab 8404, random-init), "
                               f"{B} x {seconds:g} s distinct 16 kHz clips per GPU, wav in HBM -> token ids on host",
                   "h2d": "excluded (waveforms resident in HBM when the clock starts; the PCIe-inclusive rate is `pcie_inclusive`)",
                   "clips_per_gpu": B, "clip_seconds": seconds, "parallelism": f"utterance-dp{world}",
                   "tokens_per_clip": round(sum(token_num) / len(token_num), 1),
                   "tokens_max": max(token_num), "tokens_min": min(token_num),
                   "rccl_ranks": world, "weight_arena_bytes_broadcast": arena_bytes,
                   "hypothesis_gather_bytes_per_rank_per_step": (B * (n_pad + 1) * 4) if world > 1 else 0,
                   "per_rank_ms_per_step": per_rank_ms, "weight_broadcast_seconds_per_rank": bcast_all if world > 1 else None,
                   "weights_route": weights_route if world > 1 else None, "host_cores_rank0": host_pin,
                   "output_layer": output_layer},
        "roofline": roofline, "kernels": kernels,
        "sclk_mhz_mean": (telemetry or {}).get("sclk_mhz_mean"), "power_w_mean": (telemetry or {}).get("power_w_mean"),
        "telemetry": telemetry,
    }


def read_prof(lib, steps):
    kinds = {0: "gemm_f32_mfma", 1: "attention", 2: "fsmn", 3: "layernorm", 4: "fbank", 5: "gemm_split"}
    prof = {}
    for k, name in kinds.items():
        ms, work, n = C.c_double(0), C.c_double(0), C.c_int64(0)
        lib.pf_prof_read(k, C.byref(ms), C.byref(work), C.byref(n))
        prof[name] = dict(ms_per_step=ms.value / steps, work_per_step=work.value / steps, launches_per_step=n.value / steps)
    return prof


def read_prof_tags(lib, steps, peak_tflops):
    """per call site (ProfScope tags in engine_encoder.hip): ms per launch, fp32-equivalent TFLOP/s and its fraction of the mode's MFMA peak"""
    cap = 32
    tags, kinds = (C.c_char_p * cap)(), (C.c_int * cap)()
    ms, work, n = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    k = lib.pf_prof_read_tags(cap, tags, kinds, ms, work, n)
    rows = []
    for i in range(max(k, 0)):
        if n[i] == 0 or ms[i] <= 0:
            continue
        tf = work[i] / (ms[i] * 1e-3) / 1e12
        rows.append({"site": tags[i].decode(), "launches_per_step": n[i] / steps, "us_per_launch": round(ms[i] / n[i] * 1e3, 1),
                     "ms_per_step": round(ms[i] / steps, 3), "tflops_fp32_equiv": round(tf, 1), "frac": round(tf / peak_tflops, 4)})
    rows.sort(key=lambda r: -r["ms_per_step"])
    return rows


def kernel_figures(lib, steps, precision):
    """`roofline` and `kernels` of the line from the counters of the instrumented pass (pf_prof_*) over `steps` steps."""
    prof = read_prof(lib, steps)
    if precision in PRODUCTS:
        # dominant kernel: the split-operand GEMM. `achieved` = algorithmic (fp32-equivalent) 2MNK flops per second; the
        # kernel executes PRODUCTS 16-bit MFMA flops per algorithmic flop, so its ceiling is the dense 16-bit peak / PRODUCTS
        gemm = prof["gemm_split"]
        # f16x2: the tile kernel and its full-row form (gemm_f16x2_row_kernel: linear_out / w_2 with the fused LayerNorm)
        kname = "gemm_f16x2_" if precision == "f16x2" else "gemm_split3_kernel"
        peak = PEAK_16BIT_MFMA_TFLOPS / PRODUCTS[precision]
    else:
        gemm, kname = prof["gemm_f32_mfma"], "gemm_f32_mfma_kernel"
        peak = PEAK_16BIT_MFMA_TFLOPS if precision == "bf16" else PEAK_F32_MFMA_TFLOPS
    roofline = assemble_roofline(gemm, kname, peak, sum(v["ms_per_step"] for v in prof.values()), pmc_traffic(kname), PRODUCTS.get(precision))
    roofline["measured_in"] = ("instrumented pass on ONE stream (hipEvent pairs on the launch stream); share_of_step = this family's share of the "
                               "instrumented kernel time of a step")
    kernels = {k: dict(ms_per_step=round(v["ms_per_step"], 3), launches=v["launches_per_step"]) for k, v in prof.items()}
    for nm in ("gemm_f32_mfma", "gemm_split", "attention"):
        if prof[nm]["ms_per_step"] > 0:
            kernels[nm]["tflops"] = round(prof[nm]["work_per_step"] / (prof[nm]["ms_per_step"] * 1e-3) / 1e12, 2)
    for nm in ("fsmn", "layernorm", "fbank"):
        if prof[nm]["ms_per_step"] > 0:
            kernels[nm]["GBps"] = round(prof[nm]["work_per_step"] / (prof[nm]["ms_per_step"] * 1e-3) / 1e9, 1)
    inst = sum(v["ms_per_step"] for v in prof.values())
    kernels["by_call_site"] = read_prof_tags(lib, steps, peak)[:8]
    kernels["instrumented_sum_ms"] = round(inst, 2)
    kernels["non_gemm_non_attention_ms"] = round(inst - prof["gemm_f32_mfma"]["ms_per_step"] - prof["gemm_split"]["ms_per_step"]
                                                 - prof["attention"]["ms_per_step"], 2)
    return roofline, kernels


def dump_outputs(res, out_dir) -> list:
    """--dump-outputs: the result of the timed path's last step as a caller receives it (Paraformer.collect) -- the token count
    per clip and the token ids per clip, raw (as the arg-max produced them) and without <s> / </s> / <blank>; rows of ids are
    right-padded with -1. float64 holds every id exactly. Returns the names written."""
    import numpy as np

    def padded(rows):
        a = np.full((len(rows), max((len(r) for r in rows), default=0)), -1.0, dtype=np.float64)
        for i, r in enumerate(rows):
            a[i, :len(r)] = r
        return a

    arrays = {"token_num": np.asarray(res["token_num"], dtype=np.float64), "raw_ids": padded(res["raw_ids"]), "ids": padded(res["ids"])}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    return sorted(arrays)


def main():
    args = parse()
    from funasr_amd.dp import ensure_ranks
    world = ensure_ranks(args.gpus)        # --gpus N > 1 without a launcher: re-executes itself as N ranks; a mismatch is an error
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an AMD GPU: the HIP path is the only implementation")
    if args.dist_backend == "gloo":
        local_rank = 0                                       # dry run: all ranks share the one visible GPU
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "gloo":
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=device)    # backend "nccl" is RCCL on ROCm

    from funasr_amd import _lib, dp, synth
    from funasr_amd.wav_frontend import WavFrontend
    dp.guard_shared_gpu(world, all_on_one=args.dist_backend == "gloo")
    host_pin = dp.pin_rank_to_cores(int(os.environ.get("LOCAL_RANK", "0")), world) if world > 1 else None

    lib = _lib.load()
    cfg = synth.PARAFORMER_LARGE
    trace("library loaded, building model")
    model, arena_bytes, bcast_s = build_model(cfg, rank, world, device, args.weights_route)
    trace("model on device")
    shift, scale = synth.synthetic_cmvn(560)
    frontend = WavFrontend(cmvn=torch.stack([shift, scale]), lfr_m=7, lfr_n=6, dither=0.0, device=device)

    # ---- synthetic workload: B distinct clips, resident in HBM before the clock starts
    B = args.batch
    n_samples = int(args.seconds * 16000)
    clips = [synth.speech_like(n_samples, seed=1000 * rank + i) for i in range(B)]
    wav_host = torch.stack(clips).pin_memory()
    wav = wav_host.to(device)
    lens = [n_samples] * B
    N_PAD = 512
    interleave = not args.no_interleave
    # PF_DEC_STREAM_PRIORITY: measurement switch (-1 = high priority for the decoder stream; profiles/r06ao_ab_stream_priorities.txt)
    dec_stream = (torch.cuda.Stream(device=device, priority=int(os.environ.get("PF_DEC_STREAM_PRIORITY", "0")))
                  if (interleave and not args.no_decoder_stream) else None)
    if os.environ.get("PF_MAIN_STREAM_PRIORITY") is not None:     # measurement switch: the loop's own stream with a HIP priority (same record)
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.Stream(device=device, priority=int(os.environ["PF_MAIN_STREAM_PRIORITY"])))
    if dec_stream is not None:
        lib.pf_set_concurrency_guard(1)        # kernels of two streams may share a CU: the frontend's cross-check on (0.4 % of a step)
    trace("workload resident in HBM")

    def enqueue(src=None):
        feats, flens = frontend(wav if src is None else src, lens)
        return model.enqueue_features(feats, flens)

    def collect(pending):
        if world > 1 and pending["ids"] is not None:
            if pending.get("ready") is not None:
                torch.cuda.current_stream().wait_event(pending["ready"])     # the ids were produced on the decoder stream
            # gather hypotheses on rank 0 (fixed-stride int32 ids + counts packed on the device), the path's only exchange
            dp.gather_packed(dp.pack_hypotheses_device(pending["ids"], pending["tok"], N_PAD), dst=0)
        return model.collect(pending)

    def step():
        return collect(enqueue())

    def begin(src=None):
        feats, flens = frontend(wav if src is None else src, lens)
        return model.begin_features(feats, flens)

    def run_steps_sequential(k):
        """round 5's loop (kept for the A/B figure `interleave.sequential_ms_per_step`): batch i+1 is enqueued whole -- frontend ..
        fused arg-max, with the host's wait for the CIF token count in its middle -- before batch i's ids are collected."""
        pending = enqueue()
        for _ in range(k - 1):
            nxt = enqueue()
            collect(pending)
            pending = nxt
        return collect(pending)

    def run_steps(k, stream="default"):
        """k batches, software-pipelined like a serving loop, in the two phases of the forward (Paraformer.begin_features /
        finish_features = pf_paraformer_begin / _finish): batch i+1's frontend + encoder + CIF scan are enqueued BEFORE the host waits
        for batch i's token counts and launches its decoder, and batch i-1's ids are collected after that -- the stream always holds
        a whole encoder while the host reads a count, so the GPU never waits for the host. Every batch is fully processed
        and collected inside the call. With `dec_stream` the second phase runs on its own HIP stream: batch i's decoder (few rows per
        kernel, launch- and latency-bound) beside batch i+1's encoder GEMMs -- ONE model replica, one set of weights."""
        if not interleave:
            return run_steps_sequential(k)
        stream = dec_stream if stream == "default" else stream
        ticket, pending, out = begin(), None, None
        for _ in range(k - 1):
            nxt = begin()
            fin = model.finish_features(ticket, stream=stream)
            if pending is not None:
                collect(pending)
            pending, ticket = fin, nxt
        fin = model.finish_features(ticket, stream=stream)
        if pending is not None:
            collect(pending)
        return collect(fin)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(x: float) -> float:
        tt = torch.tensor([x], dtype=torch.float64, device="cpu" if args.dist_backend == "gloo" else device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    model.set_precision(args.precision)
    for kv in args.enc_option:
        key, _, val = kv.partition("=")
        model.encoder.set_option(key, int(val))
    # ---- output layer. The checkpoint is random-init; a random 8404-way Linear leaves ~1 position in 10^4 on a top-2 near-tie
    #      that any fp32 summation order flips, so the headline run uses a CONFIDENT output layer (synth.confident_output_layer,
    #      the closed-form stand-in for training, calibrated on this batch's own hidden states; same shape, same kernels, same
    #      cost) and the id-level parity below is strict. The random layer's ids are kept as the stress case.
    gpu_random = None
    confident, conf_stats = None, None
    if not args.random_output_layer:
        feats0, flens0 = frontend(wav, lens)
        if args.full and rank == 0 and not args.no_cpu_baseline:
            gpu_random = model.recognize_features(feats0, flens0)["raw_ids"]
        confident, conf_stats = synth.make_paraformer_confident(model, feats0, flens0)
        del feats0
        trace(f"output layer calibrated: {conf_stats}")
    for i in range(args.warmup):
        res = step()
        torch.cuda.synchronize()
        trace(f"warmup step {i} done")

    # ------------------------------------------------------------------------------- the timed region (no instrumentation)
    sampler = None
    if args.full and rank == 0:                        # host thread polling librocm_smi64 every 20 ms: clock + socket power
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from gpu_telemetry import Sampler
            sampler = Sampler(device=local_rank)
        except Exception as e:                         # noqa: BLE001  (telemetry must never take the bench down)
            trace(f"telemetry unavailable: {e!r}")
    sync()
    if sampler is not None:
        sampler.start()
    t0 = time.perf_counter()
    res = run_steps(args.steps)
    sync()
    dt = time.perf_counter() - t0
    telemetry = sampler.stop() if sampler is not None else None
    trace(f"timed region done: {dt:.3f} s for {args.steps} steps; telemetry {telemetry}")
    per_rank_ms = None
    if world > 1:
        # every rank's own time for the same K steps (the line's `value` uses the maximum): first-contact diagnostics for the
        # 8-GPU run -- a slow rank (clock / power) or a slow broadcast shows up here, not in the aggregate
        cdev = "cpu" if args.dist_backend == "gloo" else device
        mine = torch.tensor([dt / args.steps * 1e3, bcast_s], dtype=torch.float64, device=cdev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_ms = [round(float(t[0]), 2) for t in allr]
        bcast_all = [round(float(t[1]), 3) for t in allr]
        dt = max_over_ranks(dt)
    audio_s = world * B * args.seconds * args.steps
    value = audio_s / dt

    if args.dump_outputs and rank == 0:
        names = dump_outputs(res, args.dump_outputs)
        trace(f"outputs of the last timed step written: {', '.join(names)} under {args.dump_outputs}")

    # ---- per-kernel numbers (--full): the same steps again with a hipEvent pair around every launch of the dominant kernels, on
    #      the launch stream (the events cost ~5 ms per step, which is why this pass is not the timed one). Every rank runs it
    #      (the steps contain the hypothesis gather); only rank 0's numbers are reported
    #      ONE stream here even when the timed loop runs the decoder on a second stream: a kernel's duration beside another stream's
    #      kernels is not the kernel's (w_1 reads 261 us instead of 211 with the decoder next to it) -- the roofline fraction is quoted
    #      for the kernel running alone, as in every earlier round, and tools/profile.sh runs rocprofv3 on the same one-stream loop
    if args.full:
        torch.cuda.synchronize()
        lib.pf_prof_reset()
        lib.pf_prof_enable(1)
        run_steps(args.steps, stream=None)
        sync()
        lib.pf_prof_enable(0)
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return
    roofline, kernels = None, None
    if args.full:
        roofline, kernels = kernel_figures(lib, args.steps, args.precision)
        trace("instrumented pass done")

    line = assemble_line(value=value, dt=dt, steps=args.steps, warmup=args.warmup, world=world, dtype=MODE_DTYPE[args.precision], B=B,
                         seconds=args.seconds, token_num=res["token_num"], arena_bytes=arena_bytes, n_pad=N_PAD, per_rank_ms=per_rank_ms,
                         bcast_all=bcast_all if world > 1 else None, weights_route=args.weights_route, host_pin=host_pin, roofline=roofline,
                         kernels=kernels, telemetry=telemetry,
                         output_layer=("random-init" if confident is None else
                                       {"kind": "confident (synth.confident_output_layer, calibrated on the batch)", **conf_stats}))
    if world > 1 or not args.full:
        print(json.dumps(line), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return

    # ------------------------------------------------------------------- everything below: --full, N = 1 only, outside the timed region
    line["hbm_copy_probe"] = hbm_copy_probe(device)
    if interleave:
        # A/B in the same process: round 5's loop (the host's wait for the CIF count between a batch's encoder and its decoder)
        run_steps_sequential(2)
        torch.cuda.synchronize()
        t0s = time.perf_counter()
        run_steps_sequential(args.steps)
        torch.cuda.synchronize()
        seq_ms = (time.perf_counter() - t0s) / args.steps * 1e3
        line["interleave"] = {"loop": "begin(i+1) -> finish(i) -> collect(i-1) (pf_paraformer_begin / _finish)" +
                                      ("; finish on a second HIP stream (the decoder beside the next encoder)" if dec_stream is not None else ""),
                              "sequential_ms_per_step": round(seq_ms, 2), "gain": round(seq_ms / (dt / args.steps * 1e3), 4)}
        if dec_stream is not None:          # and the two-phase loop with both phases on one stream
            run_steps(2, stream=None)
            torch.cuda.synchronize()
            t0s = time.perf_counter()
            run_steps(args.steps, stream=None)
            torch.cuda.synchronize()
            line["interleave"]["one_stream_ms_per_step"] = round((time.perf_counter() - t0s) / args.steps * 1e3, 2)
    if not args.no_secondary:
        line["pcie_inclusive"] = run_pcie_inclusive(frontend, model, wav_host, wav, lens, args, B, dec_stream)
        # SURVEY 8(d) counts the waveforms' H2D copy; this run's rules make `value` the HBM-resident rate -- both at the top level
        line["value_pcie_inclusive"] = line["pcie_inclusive"]["value"]
        trace(f"PCIe-inclusive: {line['pcie_inclusive']['value']} audio-s/s")
        try:
            line["two_replicas"] = run_two_replicas(cfg, model, frontend, wav, lens, args, B, device, res)
            trace(f"two replicas on two streams: {line['two_replicas']['value']} audio-s/s")
        except Exception as e:                                   # noqa: BLE001  (a secondary leg must not lose the headline line)
            line["two_replicas"] = {"error": repr(e)}

    # other arithmetic modes on the same batch, each with its token agreement against the main result measured, not assumed
    def time_mode(mode, steps):
        from funasr_amd.metrics import micro_error_rate
        model.set_precision(mode)
        for _ in range(2):
            r = step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = run_steps(steps)
        torch.cuda.synchronize()
        dtm = time.perf_counter() - t1
        ter, _, _ = micro_error_rate(res["raw_ids"], r["raw_ids"])
        same = sum(1 for a, b in zip(res["raw_ids"], r["raw_ids"]) if a == b)
        same_n = sum(1 for a, b in zip(res["token_num"], r["token_num"]) if a == b)
        return {"value": round(B * args.seconds * steps / dtm, 1), "unit": "audio-s/s", "ms_per_step": round(dtm / steps * 1e3, 2),
                "dtype": MODE_DTYPE[mode], "clips_with_identical_token_ids_vs_main": f"{same}/{B}",
                "clips_with_identical_token_count_vs_main": f"{same_n}/{B}", "token_error_rate_vs_main": round(ter, 4)}

    if not args.no_bf16:
        try:
            others = {}
            for mode in ("fp32", "bf16x3", "f16x2", "bf16"):
                if mode != args.precision:
                    others[mode] = time_mode(mode, max(2, args.steps // 2))
                    trace(f"mode {mode}: {others[mode]['value']} audio-s/s")
            line["fp32_mfma_mode"] = others.get("fp32")
            line["bf16x3_mode"] = others.get("bf16x3")
            line["f16x2_mode"] = others.get("f16x2")
            line["bf16_mode"] = others.get("bf16")
        finally:
            model.set_precision(args.precision)

    line["cpu_baseline"] = None
    if not args.no_cpu_baseline:
        trace("cpu baseline (oracle on host cores) + full-configuration parity ...")
        feats, flens = frontend(wav, lens)
        gpu_full = model.recognize_features(feats, flens, return_intermediate=True)
        # decoder hidden states (the output layer's input) and the logits themselves, for max |difference| against the CPU path
        tokt = torch.tensor(gpu_full["token_num"])
        gpu_full["hidden"] = model.decoder(gpu_full["enc"], gpu_full["olens"], gpu_full["embeds"], tokt, return_hidden=True)[0].cpu()
        gpu_full["logits_fn"] = lambda i: model.decoder(gpu_full["enc"][i:i + 1], gpu_full["olens"][i:i + 1], gpu_full["embeds"][i:i + 1],
                                                        tokt[i:i + 1])[0][0].cpu()
        line["cpu_baseline"] = run_cpu_baseline(cfg, clips, shift, scale, gpu_full, args, confident, gpu_random)

        trace("cpu baseline done")
    del wav

    if not args.no_secondary:
        try:
            line["generate_wav_files"] = run_generate(model, frontend, cfg, device)
            trace(f"AutoModel.generate over wav files: {line['generate_wav_files']['value']} audio-s/s")
        except Exception as e:                                   # noqa: BLE001
            line["generate_wav_files"] = {"error": repr(e)}
        try:
            line["sensevoice"] = run_sensevoice(device, args)
            trace(f"SenseVoiceSmall: {line['sensevoice']['value']} audio-s/s")
        except Exception as e:                                   # a secondary workload must not lose the headline line
            line["sensevoice"] = {"error": repr(e)}
        try:
            line["streaming"] = run_streaming(device)
            trace("streaming done")
        except Exception as e:
            line["streaming"] = {"error": repr(e)}
    if args.precision == "f16x2":
        # what the matrix pipe sustains for THIS instruction mix on random operand planes under the part's power / clock
        # management (tools/micro/mfma_peak.hip: register-resident three-product chains, no LDS, no memory), measured now -- LAST,
        # so that its 1.5 s at the power limit do not precede (and heat) any timed leg above
        apply_power_limited_peak(line["roofline"], power_limited_peak(), PRODUCTS["f16x2"])
    print(json.dumps(line), flush=True)


def run_generate(model, frontend, cfg, device, clips=2000, batch_size=256):
    """The caller's side of the path (SURVEY 8 f3 / INTEGRATION 1): `AutoModel.generate` over wav FILES -- read, decode, pad, upload,
    features, forward, ids -> text -- with this run's model: the batches overlapped (funasr_amd/auto_model.py) against the reference's
    one-batch-after-the-other loop (funasr/auto/auto_model.py:790-840), records compared. AISHELL-like durations, sorted by length."""
    import shutil
    import tempfile
    import wave
    from funasr_amd import synth
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.tokenizer import CharTokenizer
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from sweep import durations
    work = tempfile.mkdtemp(prefix="pf_bench_generate_")
    threads = torch.get_num_threads()
    torch.set_num_threads(4)      # what AutoModel's constructor does (ncpu = 4, auto_model.py:563-566): with one thread per visible core the
    try:                          # small host-side copies of this loop oversubscribe a container's CPU quota and run 10x slower
        durs = durations(clips)                               # the list stays in this (unsorted) order
        pool = [synth.speech_like(int(14.7 * 16000) + 1, seed=1000 + i) for i in range(16)]
        paths = []
        for i, d in enumerate(durs):
            p = os.path.join(work, f"clip{i:05d}.wav")
            pcm = (pool[i % 16].roll(31 * i)[: int(d * 16000)].clamp(-1, 1) * 32767.0).round().to(torch.int16).numpy()
            with wave.open(p, "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(16000)
                f.writeframes(pcm.tobytes())
            paths.append(p)
        V = cfg["decoder"]["vocab_size"]
        am = AutoModel.__new__(AutoModel)
        am.model, am.vad_model, am.punc_model = model, None, None
        am.kwargs = {"batch_size": batch_size, "device": str(device), "disable_pbar": True, "frontend": frontend,
                     "tokenizer": CharTokenizer(token_list=["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(V - 4)] + ["<unk>"])}
        am._base_kwargs = {k: v for k, v in am.kwargs.items() if k not in ("frontend", "tokenizer")}
        total = float(sum(durs))
        am.generate(input=paths, batch_size_rows=32768)       # warm-up: files in the page cache, buffers at their final sizes
        am.generate(input=paths[: 2 * batch_size], pipeline=False)
        out = {}
        # this package's loop (batches planned by encoder rows from the WAV headers, overlapped) against the reference's (count
        # batches in list order, one after the other)
        for name, kw in (("overlapped", {"batch_size_rows": 32768}), ("plain_loop", {"pipeline": False})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = am.generate(input=paths, **kw)
            torch.cuda.synchronize()
            out[name] = (res, total / (time.perf_counter() - t0))
        same = sum(1 for a, b in zip(out["overlapped"][0], out["plain_loop"][0]) if a["text"] == b["text"])
        one_after_the_other = am.generate(input=paths, batch_size_rows=32768, pipeline=False)      # the SAME plan without the overlap
        same_plan = sum(1 for a, b in zip(out["overlapped"][0], one_after_the_other) if a == b)
        return {"value": round(out["overlapped"][1], 1), "unit": "audio-s/s", "plain_loop": round(out["plain_loop"][1], 1),
                "gain": round(out["overlapped"][1] / out["plain_loop"][1], 3), "records_identical_to_the_same_plan_without_overlap": f"{same_plan}/{clips}",
                "records_with_identical_text_across_the_two_batch_plans": f"{same}/{clips}",
                "workload": f"{clips} wav files, {total / 3600:.2f} h (AISHELL-like durations, unsorted list); value: generate(batch_size_rows=32768), "
                            f"batches overlapped; plain_loop: generate(batch_size={batch_size}, pipeline=False), the reference's loop. File reading, padding, "
                            "H2D, features and text included; the larger corpus: profiles/r06ad_generate_rows_budget.txt"}
    finally:
        torch.set_num_threads(threads)
        shutil.rmtree(work, ignore_errors=True)


def run_pcie_inclusive(frontend, model, wav_host, wav_dev, lens, args, B, dec_stream=None):
    """The same steps with every batch's waveforms starting in PINNED HOST memory: H2D copies on a side stream into two
    device buffers, one batch ahead of the compute stream (an event each way). Never `value` -- reported beside it."""
    copy_stream = torch.cuda.Stream()
    main = torch.cuda.current_stream()
    bufs = [torch.empty_like(wav_dev) for _ in range(2)]
    free_ev = [None, None]

    def h2d(i):
        with torch.cuda.stream(copy_stream):
            if free_ev[i % 2] is not None:
                copy_stream.wait_event(free_ev[i % 2])          # the frontend of batch i-2 has consumed this buffer
            bufs[i % 2].copy_(wav_host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(copy_stream)
        return ev

    def begin(i, ev):
        main.wait_event(ev)
        feats, flens = frontend(bufs[i % 2], lens)
        fe = torch.cuda.Event()
        fe.record(main)
        free_ev[i % 2] = fe
        return model.begin_features(feats, flens)

    def run(k):
        # the two-phase loop of the headline run with batch i + 1's copy issued one batch ahead on the side stream
        ev = h2d(0)
        nxt_ev = h2d(1) if k > 1 else None
        ticket, pending = begin(0, ev), None
        for i in range(1, k):
            ev, nxt_ev = nxt_ev, (h2d(i + 1) if i + 1 < k else None)
            nxt = begin(i, ev)
            fin = model.finish_features(ticket, stream=dec_stream)
            if pending is not None:
                model.collect(pending)
            pending, ticket = fin, nxt
        fin = model.finish_features(ticket, stream=dec_stream)
        if pending is not None:
            model.collect(pending)
        return model.collect(fin)

    run(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"value": round(B * args.seconds * args.steps / dt, 1), "unit": "audio-s/s", "ms_per_step": round(dt / args.steps * 1e3, 2),
            "h2d_bytes_per_step": wav_host.numel() * 4,
            "note": "waveforms in pinned host memory, H2D on a side stream one batch ahead of compute"}


def run_sensevoice(device, args):
    """BASELINE configs[2]: SenseVoiceSmall encoder-only (50 + 20 SAN-M blocks, CTC head 25055), 128 x 10 s clips:
    wav in HBM -> fbank/LFR/CMVN -> 4 query frames + encoder -> CTC GEMM with fused arg-max -> ids on host."""
    from funasr_amd import synth
    from funasr_amd.sense_voice import SenseVoiceSmall
    from funasr_amd.wav_frontend import WavFrontend
    cfg = synth.SENSEVOICE_SMALL
    sd = synth.sensevoice_state_dict(cfg, seed=0)
    model = SenseVoiceSmall.from_config(cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(device)
    sh, sc = synth.synthetic_cmvn(560)
    cmvn = torch.stack([sh, sc])
    fe = WavFrontend(cmvn=cmvn, lfr_m=7, lfr_n=6, dither=0.0, device=device)
    Bs, secs, steps = 128, 10.0, 4
    n = int(secs * 16000)
    clips = [synth.speech_like(n, seed=500 + i) for i in range(Bs)]
    wav = torch.stack(clips).to(device)
    lens = [n] * Bs

    def enqueue():
        feats, flens = fe(wav, lens)
        return model.enqueue_features(feats, flens, "auto", "woitn")

    def run_steps(k):                                       # software-pipelined like the headline loop (run_steps above)
        pending = enqueue()
        for _ in range(k - 1):
            nxt = enqueue()
            model.collect(pending)
            pending = nxt
        return model.collect(pending)

    out = {}
    for mode in (args.precision if args.precision != "bf16" else "f16x2", "fp32"):
        model.set_precision(mode)
        run_steps(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = run_steps(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[mode] = dict(value=round(Bs * secs * steps / dt, 1), ms_per_step=round(dt / steps * 1e3, 2), res=r, mode=mode)
    main, ref32 = list(out.values())
    # roofline of this leg's dominant kernel (the same split-operand GEMMs), from an instrumented pass in the main mode
    roof = None
    try:
        from funasr_amd import _lib
        lib = _lib.load()
        model.set_precision(main["mode"])
        run_steps(1)
        torch.cuda.synchronize()
        lib.pf_prof_reset(); lib.pf_prof_enable(1)
        run_steps(steps)
        torch.cuda.synchronize()
        lib.pf_prof_enable(0)
        prof = read_prof(lib, steps)
        g = prof["gemm_split"] if main["mode"] in PRODUCTS else prof["gemm_f32_mfma"]
        peak = PEAK_16BIT_MFMA_TFLOPS / PRODUCTS[main["mode"]] if main["mode"] in PRODUCTS else PEAK_F32_MFMA_TFLOPS
        ach = g["work_per_step"] / (g["ms_per_step"] * 1e-3) / 1e12 if g["ms_per_step"] > 0 else 0.0
        roof = {"bound": "mfma", "kernel": "gemm_f16x2_kernel + gemm_f16x2_row_kernel", "achieved": round(ach, 1), "peak": round(peak, 1), "unit": "TFLOP/s",
                "frac": round(ach / peak, 4), "launches_per_step": g["launches_per_step"], "gemm_ms_per_step": round(g["ms_per_step"], 2),
                "attention_ms_per_step": round(prof["attention"]["ms_per_step"], 2), "traffic": None,
                "by_call_site": read_prof_tags(lib, steps, peak)[:5]}
    except Exception as e:                                   # noqa: BLE001  (the roofline of a secondary leg must not lose its line)
        roof = {"error": repr(e)}
    ok, ncpu, differing = None, 0, []
    if not args.no_cpu_baseline:
        # every clip of the batch against the CPU oracle (round 4 checked 16 of 128), eight clips per oracle call
        from oracle import paraformer_oracle as O
        ok, ncpu = True, Bs
        with torch.no_grad():
            for i0 in range(0, ncpu, 8):
                f, fl = O.wav_frontend(clips[i0:i0 + 8], cmvn)
                ref = O.sensevoice_greedy(f, fl, sd, cfg)
                for j, ids in enumerate(ref["ids"]):
                    if not (ids == main["res"]["ids"][i0 + j] and ids == ref32["res"]["ids"][i0 + j]):
                        ok = False
                        differing.append(i0 + j)
    same = sum(1 for a, b in zip(main["res"]["ids"], ref32["res"]["ids"]) if a == b)
    return {"metric": "audio-seconds/sec SenseVoiceSmall encoder+CTC, 10 s clips @ bs128", "value": main["value"], "unit": "audio-s/s",
            "ms_per_step": main["ms_per_step"], "dtype": MODE_DTYPE[main["mode"]], "steps": steps,
            "config": {"workload": f"SenseVoiceSmall (70 SAN-M blocks, CTC 25055, random-init), {Bs} x {secs:g} s distinct clips, wav in HBM -> ids on host"},
            "fp32_mfma_mode": {"value": ref32["value"], "ms_per_step": ref32["ms_per_step"],
                               "clips_with_identical_ids_vs_main": f"{same}/{Bs}"},
            "roofline": roof, "ids_equal_cpu_oracle": ok, "cpu_oracle_clips_checked": ncpu, "clips_differing_from_cpu_oracle": differing}


def run_streaming(device):
    """BASELINE configs[4]: Paraformer-large-streaming, 600 ms chunks, hipGraph-captured step, S lock-step streams."""
    import copy
    from funasr_amd import synth
    from funasr_amd.paraformer_streaming import ParaformerStreaming, StreamBatch
    cfg = copy.deepcopy(synth.PARAFORMER_LARGE)
    cfg["decoder"]["sanm_shfit"] = 5
    model = ParaformerStreaming.from_config(cfg)
    model.load_state_dict(synth.paraformer_state_dict(cfg, seed=0, cif_bias=synth.BENCH_CIF_BIAS), strict=False)
    model = model.to(device)
    rows = []
    for S in (1, 64, 256):
        # precision by the stream count (StreamBatch default): the fp32 weight-streaming step for a few streams, the f16x2 step
        # (GEMMs on the fp16 matrix cores, fp32-class results) from StreamBatch.AUTO_F16X2_MIN_STREAMS streams on
        sb = StreamBatch(model, S, [0, 10, 5], 4, 1, use_graph=True, pe_rows=16384)
        g = torch.Generator().manual_seed(S)
        feats = (torch.randn(S, 10, 560, generator=g) * 0.8).to(device)
        for _ in range(5):
            sb.step(feats)
        torch.cuda.synchronize()
        steps, lat = 40, []
        t0 = time.perf_counter()
        for _ in range(steps):
            t1 = time.perf_counter()
            sb.step(feats)
            lat.append(time.perf_counter() - t1)
        dt = time.perf_counter() - t0
        lat.sort()
        row = {"streams": S, "precision": sb.precision, "chunks_per_s": round(S * steps / dt, 1), "audio_s_per_s": round(S * steps * 0.6 / dt, 1),
               "step_ms_p50": round(lat[len(lat) // 2] * 1e3, 3), "step_ms_p99": round(lat[int(len(lat) * 0.99)] * 1e3, 3)}
        # what bounds the step: an eager, hipEvent-instrumented replay of the same step (the graph is bypassed while profiling is
        # on) -- the instrumented kernels' launch count and their summed time against the step: a step of a few streams is a chain of
        # ~600 dependent launches of 4-15 us (latency-bound: `roofline.bound` "launch-latency"), many streams are GEMM-bound
        try:
            from funasr_amd import _lib
            lib = _lib.load()
            lib.pf_prof_reset(); lib.pf_prof_enable(1)
            for _ in range(4):
                sb.step(feats)
            torch.cuda.synchronize()
            lib.pf_prof_enable(0)
            prof = read_prof(lib, 4)
            n = sum(v["launches_per_step"] for v in prof.values())
            kms = sum(v["ms_per_step"] for v in prof.values())
            gm = prof["gemm_split"] if sb.precision == "f16x2" else prof["gemm_f32_mfma"]
            peak = PEAK_16BIT_MFMA_TFLOPS / 3 if sb.precision == "f16x2" else PEAK_F32_MFMA_TFLOPS
            ach = gm["work_per_step"] / (gm["ms_per_step"] * 1e-3) / 1e12 if gm["ms_per_step"] > 0 else 0.0
            row["roofline"] = {"bound": "launch-latency" if kms / max(n, 1) < 0.012 else "mfma", "instrumented_launches_per_step": n,
                               "instrumented_kernel_ms_per_step": round(kms, 3), "us_per_instrumented_launch": round(kms / max(n, 1) * 1e3, 2),
                               "gemm_tflops": round(ach, 1), "gemm_frac_of_mfma_peak": round(ach / peak, 4)}
        except Exception as e:                               # noqa: BLE001
            row["roofline"] = {"error": repr(e)}
        rows.append(row)
        sb.close()
    return {"metric": "streaming step (600 ms chunk, Paraformer-large-online, hipGraph-captured); fp32-class results in both "
                      "precisions (fp32 kernels / f16x2 = two fp16 planes on the fp16 MFMA)", "configs": rows}


def pmc_traffic(kernel: str):
    """HBM bytes per launch of `kernel` from the newest committed PMC summary (profiles/*_traffic.json, written by
    tools/summarize_prof.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command, with
    the guide's gfx950 corrections). null when no summary is present: PMC passes are not run inside the timed bench."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")))
    for f_ in reversed(files):
        try:
            with open(f_) as f:
                t = json.load(f)
            rows = [v for k, v in t["kernels"].items() if k.startswith(kernel)]
            n = sum(r["launches"] for r in rows)
            if n == 0:
                continue
            b = sum((r["read_bytes_per_launch"] + r["write_bytes_per_launch"]) * r["launches"] for r in rows) / n
            return round(b), os.path.basename(f_)
        except (OSError, KeyError, ValueError):
            continue
    return None


def host_cores() -> int:
    """CPU threads this process may really use: min(affinity mask, cgroup quota). os.cpu_count() reports the
    machine's cores even inside a CPU-limited container, and an oversubscribed OpenMP pool is ~100x slower."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def run_cpu_baseline(cfg, clips, shift, scale, gpu, args, confident=None, gpu_random=None):
    """The oracle (CPU port of the reference path: the same ATen CPU kernels the reference's nn.Modules call) timed on the
    host cores on a BOUNDED sample of the same workload, batch_size 1 like AutoModel on device="cpu"
    (funasr/auto/auto_model.py:551-561), in two thread settings: the reference's default (`ncpu` = 4,
    auto_model.py:563-566) and every usable core. Each full-length clip it runs doubles as full-configuration parity
    evidence against the GPU result of the SAME clip: token ids, CIF fire indices (bit-exact bars), the encoder's
    max |difference| (bar 1e-3) and how close the CPU prefix sum of alphas came to an integer (the fire decision margin)."""
    from funasr_amd import synth
    from funasr_amd.metrics import micro_error_rate
    from oracle import paraformer_oracle as O

    all_cores = min(host_cores(), args.cpu_threads) if args.cpu_threads > 0 else host_cores()
    sd = synth.paraformer_state_dict(cfg, seed=0, cif_bias=synth.BENCH_CIF_BIAS)
    rand_w, rand_b = sd["decoder.output_layer.weight"], sd["decoder.output_layer.bias"]
    if confident is not None:
        sd.update(confident)                     # the headline run's output layer (calibrated on the GPU, evaluated here on the CPU)
    cmvn = torch.stack([shift, scale])
    full = clips[0].numel() / 16000.0

    # The reference's OWN nn.Modules where its checkout exists (the build container), the port elsewhere (the GPU box has no
    # /root/reference): profiles/r06_cpu_port_vs_reference.json holds both timed on one host (tools/cpu_port_vs_reference.py)
    kind, ref_note = "port", None
    try:
        from oracle import ref_import
        use_ref = ref_import.available()
    except Exception:                                            # noqa: BLE001
        use_ref = False
    if use_ref:
        from oracle import make_golden_full as MG
        enc_m, pred_m, dec_m = MG.build_reference_modules(cfg, sd)
        kind = "reference"

        def run(w):
            feats, flens = O.wav_frontend([w], cmvn)             # fbank: the knf-pinned restatement (the reference's is torchaudio's)
            r = MG.run_reference(enc_m, pred_m, dec_m, feats, flens)
            n = int(r["token_num"][0])
            r["raw_ids"] = [torch.log_softmax(r["logits"][0, :n], dim=-1).argmax(-1).tolist()]
            return r
    else:
        def run(w):
            feats, flens = O.wav_frontend([w], cmvn)
            return O.paraformer_greedy(feats, flens, sd, cfg)
        try:
            with open(os.path.join(ROOT, "profiles", "r06_cpu_port_vs_reference.json")) as f:
                pr = json.load(f)
            ref_note = {"source": "profiles/r06_cpu_port_vs_reference.json (same host, same clips, build container)",
                        "port_over_reference_rate": [dict(threads=x["threads"], ratio=x["port_over_reference"]) for x in pr["settings"]],
                        "outputs_bit_equal": pr["outputs"]}
        except (OSError, KeyError, ValueError):
            pass

    parity = dict(clips=0, token_ids_equal=True, fire_indices_equal=True, token_counts_equal=True, encoder_max_abs_diff=0.0,
                  alpha_max_abs_diff=0.0, decoder_hidden_max_abs_diff=0.0, decoder_hidden_absmax=0.0, logit_max_abs_diff=0.0,
                  logit_absmax=0.0, logit_clips=0, min_prefix_sum_margin_to_integer=1.0, tokens_compared=0, token_flips=[],
                  cpu_top2_logit_gap_min=float("inf"))
    STRESS_GAP = 1e-4            # a flip of the random-init layer is accepted only where the CPU path's own top-2 logits are closer
    stress = dict(output_layer="random-init (stress case: near-ties of a flat 8404-way logit distribution)", tokens_compared=0,
                  token_flips=[], flip_allowed_below_cpu_top2_gap=STRESS_GAP,
                  passed=True) if (confident is not None and gpu_random is not None) else None
    cpu_ids, gpu_ids = [], []
    g_enc, g_alpha, g_peaks = gpu["enc"].cpu(), gpu["alphas"].cpu(), gpu["peaks"].cpu()

    def check(i, r):
        T = int(r["olens"][0])
        parity["clips"] += 1
        parity["tokens_compared"] += len(r["raw_ids"][0])
        parity["token_ids_equal"] &= r["raw_ids"][0] == gpu["raw_ids"][i]
        parity["token_counts_equal"] &= int(r["token_num"][0]) == gpu["token_num"][i]
        parity["encoder_max_abs_diff"] = max(parity["encoder_max_abs_diff"], float((r["enc"][0, :T] - g_enc[i, :T]).abs().max()))
        a = r["alphas"][0]
        parity["alpha_max_abs_diff"] = max(parity["alpha_max_abs_diff"], float((a - g_alpha[i, : a.numel()]).abs().max()))
        fire_c = torch.floor(r["peaks"][0]) >= 1
        fire_g = torch.floor(g_peaks[i, : fire_c.numel()]) >= 1
        parity["fire_indices_equal"] &= bool(torch.equal(fire_c, fire_g))
        ps = torch.cumsum(a.double(), 0)[: T + 1]
        fr = ps - torch.floor(ps)
        parity["min_prefix_sum_margin_to_integer"] = min(parity["min_prefix_sum_margin_to_integer"],
                                                         float(torch.minimum(fr, 1 - fr)[ps > 0.5].min()))
        cpu_ids.append(r["raw_ids"][0]); gpu_ids.append(gpu["raw_ids"][i])
        n_tok = len(r["raw_ids"][0])
        if r.get("hidden") is not None and gpu.get("hidden") is not None and n_tok and n_tok == gpu["token_num"][i]:
            parity["decoder_hidden_max_abs_diff"] = max(parity["decoder_hidden_max_abs_diff"],
                                                        float((r["hidden"][0, :n_tok] - gpu["hidden"][i, :n_tok]).abs().max()))
            parity["decoder_hidden_absmax"] = max(parity["decoder_hidden_absmax"], float(r["hidden"][0, :n_tok].abs().max()))
            if gpu.get("logits_fn") is not None and parity["logit_clips"] < 8:      # [N, 8404] per clip from the GPU: a few clips suffice
                gl = gpu["logits_fn"](i)
                parity["logit_max_abs_diff"] = max(parity["logit_max_abs_diff"], float((r["logits"][0, :n_tok] - gl[:n_tok]).abs().max()))
                parity["logit_absmax"] = max(parity["logit_absmax"], float(r["logits"][0, :n_tok].abs().max()))
                parity["logit_clips"] += 1
        if r["logits"] is not None and len(r["raw_ids"][0]):
            t2 = torch.topk(r["logits"][0, : len(r["raw_ids"][0])], 2, dim=-1).values
            parity["cpu_top2_logit_gap_min"] = min(parity["cpu_top2_logit_gap_min"], float((t2[:, 0] - t2[:, 1]).min()))
        if stress is not None and r.get("hidden") is not None and len(r["raw_ids"][0]) == len(gpu_random[i]):
            lg = r["hidden"][0, : len(gpu_random[i])] @ rand_w.T + rand_b
            t2 = torch.topk(lg, 2, dim=-1).values
            stress["tokens_compared"] += len(gpu_random[i])
            for pos, (x, y) in enumerate(zip(lg.argmax(-1).tolist(), gpu_random[i])):
                if x != y:
                    gap = float(t2[pos, 0] - t2[pos, 1])
                    stress["token_flips"].append({"clip": i, "pos": pos, "cpu_top2_logit_gap": float(f"{gap:.3e}")})
                    stress["passed"] &= gap < STRESS_GAP
        if r["raw_ids"][0] != gpu["raw_ids"][i] and len(r["raw_ids"][0]) == len(gpu["raw_ids"][i]):
            # a differing token: how close were the CPU path's own top-2 logits there? (random-init weights put many
            # arg-maxes over 8404 classes on near-ties that any fp32 summation order may flip)
            top2 = torch.topk(r["logits"][0], 2, dim=-1).values
            for pos, (x, y) in enumerate(zip(r["raw_ids"][0], gpu["raw_ids"][i])):
                if x != y:
                    parity["token_flips"].append({"clip": i, "pos": pos, "cpu_top2_logit_gap": float(f"{float(top2[pos, 0] - top2[pos, 1]):.3e}")})

    settings = []
    next_clip = 0
    with torch.no_grad():
        for threads in sorted({min(4, all_cores), all_cores}):
            torch.set_num_threads(threads)
            t0 = time.perf_counter()
            run(clips[0][: 3 * 16000])
            probe = time.perf_counter() - t0
            rate = 3.0 / probe                                   # audio-s per wall-s on a short clip (optimistic for 30 s)
            trace(f"cpu probe: 3 s clip in {probe:.2f} s on {threads} threads")
            whole = (args.cpu_budget * rate) // full >= 1
            t0 = time.perf_counter()
            done, secs = 0, 0.0
            if whole:
                while next_clip < min(len(clips), args.cpu_clips):
                    i = next_clip
                    next_clip += 1
                    t1 = time.perf_counter()
                    r = run(clips[i])
                    secs += full
                    done += 1
                    tc = time.perf_counter()
                    check(i, r)
                    t0 += time.perf_counter() - tc                # the parity bookkeeping is not CPU-path time
                    if time.perf_counter() - t0 > args.cpu_budget:
                        break
            else:                                                # host too slow for one whole clip inside the budget
                w = clips[0][: max(16000, int(args.cpu_budget * rate * 0.7) * 16000)]
                run(w)
                secs, done = w.numel() / 16000.0, 1
            dts = time.perf_counter() - t0
            settings.append({"value": round(secs / dts, 2), "unit": "audio-s/s", "cores": threads,
                             "sample": f"{done} x {secs / done:g} s clip(s) of the same batch, batch_size 1, {dts:.1f} s of CPU work"})
    # SURVEY 8(d) setting (ii): every usable core with batch_size 8 (one padded batch like AutoModel(batch_size=8) on a GPU host; the
    # CPU default forces 1, auto_model.py:551-561). Bounded like the others: eight full clips if the all-core rate allows them
    # inside twice the budget, else eight equal slices of a clip long enough to fill the budget.
    try:
        with torch.no_grad():
            torch.set_num_threads(all_cores)
            rate1 = next(s["value"] for s in settings if s["cores"] == all_cores)
            secs8 = full if 8 * full / max(rate1, 1e-9) <= 2 * args.cpu_budget else max(3.0, min(full, args.cpu_budget * rate1 / 8))
            t0 = time.perf_counter()
            nb = 0
            while True:                                      # batches of 8 different clips until the budget is used (>= 1 batch)
                ws = [clips[(8 * nb + i) % len(clips)][: int(secs8 * 16000)] for i in range(8)]
                feats8, flens8 = O.wav_frontend(ws, cmvn)
                if use_ref:
                    MG.run_reference(enc_m, pred_m, dec_m, feats8, flens8)
                else:
                    O.paraformer_greedy(feats8, flens8, sd, cfg)
                nb += 1
                if time.perf_counter() - t0 > args.cpu_budget:
                    break
            dt8 = time.perf_counter() - t0
            settings.append({"value": round(nb * 8 * secs8 / dt8, 2), "unit": "audio-s/s", "cores": all_cores, "batch_size": 8,
                             "sample": f"{nb} batch(es) of 8 x {secs8:g} s clips of the same workload, {dt8:.1f} s of CPU work"})
    except Exception as e:                                  # noqa: BLE001  (the extra setting must not lose the baseline)
        settings.append({"cores": all_cores, "batch_size": 8, "error": repr(e)})
    best = max((s for s in settings if "value" in s), key=lambda s: s["value"])
    ter = round(micro_error_rate(cpu_ids, gpu_ids)[0], 6) if cpu_ids else None
    parity["encoder_max_abs_diff"] = float(f"{parity['encoder_max_abs_diff']:.3e}")
    parity["alpha_max_abs_diff"] = float(f"{parity['alpha_max_abs_diff']:.3e}")
    for k in ("decoder_hidden_max_abs_diff", "decoder_hidden_absmax", "logit_max_abs_diff", "logit_absmax"):
        parity[k] = float(f"{parity[k]:.3e}")
    parity["logit_max_rel_diff"] = float(f"{parity['logit_max_abs_diff'] / parity['logit_absmax']:.3e}") if parity["logit_absmax"] else None
    parity["min_prefix_sum_margin_to_integer"] = float(f"{parity['min_prefix_sum_margin_to_integer']:.3e}")
    parity["cpu_top2_logit_gap_min"] = float(f"{parity['cpu_top2_logit_gap_min']:.3e}") if parity["clips"] else None
    if stress is not None:
        parity["stress_case_random_output_layer"] = stress
    # "CIF fire indices bit-exact" is a statistical statement against ANY other fp32 implementation (a fire flips where two
    # prefix sums straddle an integer): the committed 512-clip, 30-s statistic (GPU alphas from a gpurun box, the oracle on the
    # build host; tools/cif_margin_stats.py --dump / --compare) next to this run's clips
    try:
        with open(os.path.join(ROOT, "profiles", "r06_cif_margins_512x30s_ids.json")) as f:
            cm = json.load(f)
        parity["cif_margin_statistic"] = {k: cm.get(k) for k in (
            "clips", "clip_seconds", "mode", "frames_compared", "tokens", "clips_with_different_fire_indices", "clips_with_different_token_count",
            "alpha_max_abs_diff", "prefix_sum_abs_diff", "margin_to_integer", "frames_with_margin_below_4x_prefix_sum_diff",
            "min_margin_over_diff_ratio", "expected_frames_within_diff_of_an_integer")}
        # round 6: the consequence at token-id level -- both paths decoded, with the random-init output layer and with a confident one
        # calibrated once on the GPU's first batch (clips with different ids, token error rate, and whether they are the clips whose
        # fire indices differ)
        ids = cm.get("token_ids") or {}
        parity["cif_margin_statistic"]["token_ids"] = {
            kind: {k: v.get(k) for k in ("clips_with_different_ids", "token_errors", "ref_tokens", "token_error_rate",
                                         "different_ids_among_fire_mismatch_clips", "different_ids_among_fire_equal_clips")}
            for kind, v in ids.items()}
        parity["cif_margin_statistic"]["source"] = "profiles/r06_cif_margins_512x30s_ids.json (tools/cif_margin_stats.py --ids)"
    except (OSError, ValueError):
        pass
    return {"value": best["value"], "unit": "audio-s/s", "cores": best["cores"], "kind": kind,
            "port_vs_reference_modules": ref_note,
            "sample": best["sample"] + f", fp32, torch {torch.__version__} CPU ATen kernels",
            "thread_settings": settings,
            "token_ids_match_gpu": parity["token_ids_equal"] if parity["clips"] else None,
            "token_error_rate_gpu_vs_cpu_ref": ter,
            "full_config_parity": parity if parity["clips"] else None}


if __name__ == "__main__":
    main()
