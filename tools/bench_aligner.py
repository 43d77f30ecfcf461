"""MonotonicAligner measurements -> one JSON line (and --out, default profiles/aligner_bench.json). Device events, one warm-up,
windows of at least half a second.

(a) kernel: csrc/attention_mid.hip at B 64, H 4, d_k 80, T 500 against the existing d_k = 128 kernel (`ops.attention`) on the same
    data zero-padded to 128 columns per head with the same `scale` (zero columns change neither the scores nor the 80 output
    channels that matter), the two alternated in one process. By operation count the new kernel does (80 + 96) / 256 = 0.69 of the
    padded problem's matrix work.
(b) model: the template geometry (30 blocks, D 320, 4 heads of d_k 80, F 1280) on synthetic weights, 64 clips of 30 s with 100-token
    transcripts: audio seconds per second from waveforms in HBM to records on the host (`MonotonicAligner.inference`).
The shares of attention, GEMMs and the LSTM step launches come from a separate kernel-trace run of `--part model --once`."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funasr_amd import ops, synth  # noqa: E402
from funasr_amd.monotonic_aligner import MonotonicAligner  # noqa: E402
from funasr_amd.tokenizer import CharTokenizer  # noqa: E402
from funasr_amd.wav_frontend import WavFrontend  # noqa: E402

MIN_WINDOW_MS = 500.0


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def window(fn):
    """ms per call over a window of >= MIN_WINDOW_MS (the iteration count is sized by a first short run)"""
    fn()
    torch.cuda.synchronize()
    probe = timed(fn, 3) / 3
    iters = max(3, int(1.1 * MIN_WINDOW_MS / max(probe, 1e-3)) + 1)
    while True:
        ms = timed(fn, iters)
        if ms >= MIN_WINDOW_MS:
            return ms / iters, iters, ms
        iters = int(iters * 1.5) + 1                                   # (the probe ran slower than the steady state)


def bench_kernel(dev, rounds):
    B, H, dk, T = 64, 4, 80, 500
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B, T, 3 * H * dk, generator=g).to(dev)
    D = H * dk
    q, k, v = qkv[:, :, :D], qkv[:, :, D: 2 * D], qkv[:, :, 2 * D:]
    pad = torch.zeros(3, B, T, H, 128, device=dev)
    for j, t in enumerate((q, k, v)):
        pad[j, :, :, :, :dk] = t.reshape(B, T, H, dk)
    qp, kp, vp = (pad[j].reshape(B, T, H * 128) for j in range(3))
    klens = torch.full((B,), T, dtype=torch.int32, device=dev)
    scale = dk ** -0.5
    mid = lambda: ops.attention_mid(q, k, v, klens, H, scale)          # noqa: E731
    big = lambda: ops.attention(qp, kp, vp, klens, H, scale)           # noqa: E731
    diff = float((mid() - big().reshape(B, T, H, 128)[..., :dk].reshape(B, T, D)).abs().max())
    a, b = [], []
    for _ in range(rounds):                                            # alternated
        a.append(window(mid)[0])
        b.append(window(big)[0])
    ma, mb = sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]
    flops = 4.0 * B * T * T * H * dk
    return {"shape": {"B": B, "H": H, "d_k": dk, "T": T}, "attention_mid_ms": ma, "attention_f32_padded_to_128_ms": mb,
            "ratio_mid_over_padded": ma / mb, "attention_mid_all_ms": a, "attention_f32_padded_all_ms": b,
            "attention_mid_tflops_algorithmic": flops / ma / 1e9, "max_abs_difference_between_the_two": diff,
            "matrix_work_ratio_by_operation_count": (80 + 96) / 256}


def bench_model(dev, once):
    conf = synth.aligner_conf()
    model = MonotonicAligner(**conf)
    model.load_state_dict(synth.aligner_state_dict(2, model), strict=True)
    model = model.to(dev).eval()
    B, secs, n_tok = 64, 30.0, 100
    vocab = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + i) for i in range(200)] + ["<unk>"]
    tok = CharTokenizer(token_list=vocab)
    fe = WavFrontend(device=str(dev), fs=16000, window="hamming", n_mels=80, frame_length=25, frame_shift=10, lfr_m=7, lfr_n=6)
    waves = [synth.speech_like(int(16000 * secs), seed=100 + i).to(dev) for i in range(B)]
    texts = [[3 + (i + 7 * j) % 200 for j in range(n_tok)] for i in range(B)]
    batch = list(zip(waves, texts))
    keys = [f"utt{i}" for i in range(B)]

    def run():
        with torch.no_grad():
            return model.inference(batch, key=keys, tokenizer=tok, frontend=fe, data_type=("sound", "text"), device=str(dev))[0]

    recs = run()
    assert all(len(r["timestamp"]) == n_tok for r in recs)
    if once:
        return {"once": True}
    ms, iters, total = window(run)
    return {"shape": {"clips": B, "seconds": secs, "tokens": n_tok, "blocks": 30, "D": 320, "H": 4, "F": 1280}, "ms_per_batch": ms,
            "batches_timed": iters, "window_ms": total, "audio_seconds_per_second": B * secs / (ms / 1e3)}


def trace_shares(path):
    """rocprofv3 --kernel-trace --stats of `--part model --once` (its *_kernel_stats.csv) -> time and launches per kernel family"""
    import csv

    fam = {"gemm": 0.0, "attention": 0.0, "lstm_step": 0.0, "other": 0.0}
    calls = dict.fromkeys(fam, 0)
    with open(path) as f:
        for r in csv.DictReader(f):
            n = r["Name"]
            k = "gemm" if "gemm_" in n else "attention" if "attention_" in n else "lstm_step" if "lstm_step" in n else "other"
            fam[k] += float(r["TotalDurationNs"]) / 1e6
            calls[k] += int(r["Calls"])
    total = sum(fam.values())
    return {"kernel_ms_of_one_batch": total, "ms": fam, "launches": calls, "share": {k: v / total for k, v in fam.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("all", "kernel", "model"), default="all")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="model part: warm-up plus nothing else (for a kernel-trace run)")
    ap.add_argument("--trace-stats", help="a *_kernel_stats.csv of a kernel-trace run of `--part model --once`: add its shares to --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner_bench.json"))
    args = ap.parse_args()
    if args.trace_stats:
        with open(args.out) as f:
            res = json.load(f)
        res["model_kernel_trace"] = trace_shares(args.trace_stats)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["model_kernel_trace"]))
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    if args.part in ("all", "kernel"):
        res["kernel"] = bench_kernel(dev, args.rounds)
    if args.part in ("all", "model"):
        res["model"] = bench_model(dev, args.once)
    print(json.dumps(res), flush=True)
    if not args.once:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
