#!/usr/bin/env python3
"""What `output_timestamp=True` costs SenseVoiceSmall at the project's SenseVoice workload (128 x 10 s clips, 50 + 20 SAN-M blocks, CTC
head 25055, random-init weights of the exact architecture, the 128-piece tokenizer of tests/golden/sv_bpe.model): the time of one
`inference` call (waveforms on the host -> records) with and without the option, alternating, each call ended by a device synchronise;
and, where the package has it, the batched alignment op alone at B = 128, T = 167, L = 80 (device events around back-to-back launches).
Prints one JSON line. `--tree DIR` measures the package of another checkout (the parent commit, for the A/B of
profiles/ctc_align_timestamps.json); the workload is the same seeded one either way."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=4, help="timed calls of each kind")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", default="f16x2")
    ap.add_argument("--tree", default=ROOT, help="checkout whose funasr_amd package is measured")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from funasr_amd import ops, synth
    from funasr_amd.sense_voice import SenseVoiceSmall
    from funasr_amd.tokenizer import SentencepiecesTokenizer
    from funasr_amd.wav_frontend import WavFrontend

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    tok = SentencepiecesTokenizer(os.path.join(ROOT, "tests", "golden", "sv_bpe.model"))
    pieces = 128
    cfg = synth.SENSEVOICE_SMALL
    sd = synth.sensevoice_state_dict(cfg, seed=0)
    sd["ctc.ctc_lo.bias"][pieces:] = float("-inf")              # the greedy path stays inside the small tokenizer's pieces
    model = SenseVoiceSmall.from_config(cfg)
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).set_precision(args.mode)
    sh, sc = synth.synthetic_cmvn(560)
    fe = WavFrontend(cmvn=torch.stack([sh, sc]), lfr_m=7, lfr_n=6, dither=0.0, device=dev)
    n = int(args.seconds * 16000)
    base = [synth.speech_like(n, seed=500 + i) for i in range(8)]
    wav = torch.stack([base[i % 8].roll(97 * (i // 8)) for i in range(args.batch)])           # on the host: the call uploads it

    def call(stamps):
        t0 = time.perf_counter()
        res, _ = model.inference(wav, key=[f"u{i}" for i in range(args.batch)], tokenizer=tok, frontend=fe, device="cuda:0",
                                 language="auto", output_timestamp=stamps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    for _ in range(args.warmup):
        call(False), call(True)
    plain, stamped, res = [], [], None
    for _ in range(args.steps):                                  # alternating: a drift of the box hits both kinds alike
        plain.append(call(False)[0])
        ms, res = call(True)
        stamped.append(ms)
    with_ts = [r for r in res if "timestamp" in r]
    out = {"label": args.label, "mode": args.mode, "workload": f"SenseVoiceSmall {args.batch} x {args.seconds:g} s, waveforms on the host -> records",
           "inference_ms": {"plain": [round(v, 2) for v in plain], "output_timestamp": [round(v, 2) for v in stamped],
                            "plain_median": round(statistics.median(plain), 2), "output_timestamp_median": round(statistics.median(stamped), 2)},
           "added_ms_median": round(statistics.median(stamped) - statistics.median(plain), 2),
           "clips_with_timestamp": len(with_ts), "mean_stamps_per_clip": round(sum(len(r["timestamp"]) for r in with_ts) / max(1, len(with_ts)), 1),
           "op_alone": None}

    if hasattr(ops, "ctc_forced_align"):
        B, T, L, V, iters = 128, 167, 80, 25055, 20
        g = torch.Generator().manual_seed(0)
        logits = torch.randn(B, T + 4, V, device=dev) * 2
        tg = torch.randint(1, V, (B, L), generator=g).to(torch.int32).to(dev)

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            return round(a.elapsed_time(b) / iters, 4)

        lse, pred = ops.log_softmax_stats(logits)
        out["op_alone"] = {"shape": f"B {B}, T {T} (+ 4 query rows), L {L}, V {V}",
                           "log_softmax_stats_ms": timed(lambda: ops.log_softmax_stats(logits)),
                           "ctc_forced_align_ms": timed(lambda: ops.ctc_forced_align(logits, tg, [T] * B, [L] * B, t0=4, pred=pred, lse=lse)),
                           "log_softmax_in_place_ms": timed(lambda: ops.log_softmax(logits, inplace=True))}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
