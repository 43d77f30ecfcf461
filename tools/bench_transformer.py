"""Transformer encoder at AISHELL sizes (12 blocks, D 256, 4 heads, FFN 2048, 4234 tokens; synthetic weights) on one MI355X:
encoder + greedy CTC at 32 x 10 s and 4 x 60 s in f16x2 and fp32 against the float32 torch eager restatement
(tests/_transformer_oracle.py) on the same GPU in the same call. The three are timed in turn (f16x2, fp32, eager; f16x2, ...),
`--reps` rounds of `--calls` back-to-back calls each ending in a device synchronise; reported: the median round's ms per call
and the spread (min, max) of the rounds. Every shape is warmed up in every mode first. The decoder and the beam search are the
Conformer's (tools/bench_conformer.py measures them).
Writes profiles/transformer_bench.json.  Usage: python tools/bench_transformer.py [--reps 3] [--calls 20] [--out ...]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funasr_amd import synth  # noqa: E402
from funasr_amd.transformer import Transformer  # noqa: E402
from tests import _transformer_oracle as O  # noqa: E402


def window(fn, calls):
    """ms per call of `calls` back-to-back calls ending in a synchronise"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transformer: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    conf = synth.transformer_conf(**synth.TRANSFORMER_AISHELL)
    models = {}
    for mode in ("f16x2", "fp32"):                                      # one model per mode: a mode switch re-prepares the handle on the host
        m = Transformer(**conf)
        sd = synth.transformer_state_dict(13, m)
        m.load_state_dict(sd, strict=True)
        models[mode] = m.to(dev).set_precision(mode)
    sd32 = O.cast(sd, torch.float32, dev)
    pe = O.abs_pos_table(conf["encoder_conf"]["output_size"]).to(dev)     # built once, as the reference's module holds it
    res = {"device": torch.cuda.get_device_name(0), "config": synth.TRANSFORMER_AISHELL, "reps": a.reps, "calls_per_rep": a.calls,
           "encoder_ctc_ms": {}}
    for B, frames in ((32, 998), (4, 5998)):
        feats = torch.randn(B, frames, 80, generator=torch.Generator().manual_seed(B)).to(dev)
        lens = [frames] * B

        def hip(mode):
            def run():
                enc, _ = models[mode].encode(feats, lens)
                return models[mode].ctc.argmax(enc)
            return run

        def eager():
            with torch.no_grad():
                enc, _ = O.encoder(sd32, conf["encoder_conf"], feats, lens, pos_rows=pe)
                return O.ctc_log_softmax(sd32, enc).argmax(-1)

        fns = {"f16x2": hip("f16x2"), "fp32": hip("fp32"), "eager_fp32": eager}
        ids = {k: f() for k, f in fns.items()}                          # warm-up of every mode at this shape, and the ids they give
        for f in fns.values():
            f()
        ts = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, f in fns.items():
                ts[k].append(window(f, a.calls))
        row = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in ts.items()}
        row["audio_s_per_s_f16x2"] = B * frames / 100 / (row["f16x2"]["median"] / 1e3)
        row["greedy_frames_equal_to_eager"] = {k: float((ids[k] == ids["eager_fp32"]).float().mean()) for k in ("f16x2", "fp32")}
        res["encoder_ctc_ms"][f"{B}x{round(frames / 100)}s"] = row
        print(B, frames, row, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
