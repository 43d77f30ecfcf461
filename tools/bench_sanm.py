"""SANM decoder step and beam search at the template's sizes (funasr_amd.synth.SANM_TEMPLATE: D 512, 4 heads of 128, FFN 2048, 50
encoder and 16 decoder blocks, kernel 11 with sanm_shfit 0, 8404 tokens, no CTC head; synthetic weights) on one MI355X.
  * ms per `FsmnDecoder.step` with 10 running hypotheses over a memory of 170 rows: `--reps` rounds, each a fresh `begin` and
    `--steps` positions in order, every step behind a `reorder` as the search issues them. A step ends in a stream synchronise
    (the log-probabilities go to the host bookkeeping), so the host clock around it is the time of the step. Reported: the
    median round's mean ms per step and per reorder, and the spread (min, max) of the rounds.
  * the whole beam search (beam 10, maxlenratio 0: up to one position per encoder frame) of a 10 s clip (167 LFR frames), encoder
    excluded, host bookkeeping included; and the encoder alone.
Everything is warmed up first. The number of kernel launches of one step follows from the layer table and is written beside the
times. There is no CPU path to time: without a GPU the tool stops.
Writes profiles/sanm_bench.json.  Usage: python tools/bench_sanm.py [--reps 5] [--steps 40] [--out ...]"""
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
from funasr_amd.sanm import SANM  # noqa: E402

N_HYP, T_MEM = 10, 170


def launches_per_step(att_layers: int, blocks: int) -> int:
    """embedding; per layer norm1, w_1, the hidden LayerNorm, w_2, the fused norm2 / FSMN / norm3 kernel (+ linear_q, attention,
    linear_out with cross-attention); decoders3: norm1, w_1, LayerNorm, w_2; after_norm, output_layer, log_softmax"""
    return 1 + 8 * att_layers + 5 * (blocks - att_layers) + 4 + 3


def spread(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sanm_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sanm: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    conf = synth.sanm_conf(**synth.SANM_TEMPLATE)
    m = SANM(**conf)
    m.load_state_dict(synth.sanm_state_dict(13, m), strict=True)
    m = m.to(dev)
    dec, V = m.decoder, conf["vocab_size"]
    g = torch.Generator().manual_seed(0)
    memory = torch.randn(T_MEM, conf["encoder_conf"]["output_size"], generator=g).to(dev)
    tokens = [torch.randint(3, V, (N_HYP,), generator=g).tolist() for _ in range(a.steps)]
    parents = [torch.randint(0, N_HYP, (N_HYP,), generator=g).tolist() for _ in range(a.steps)]

    def round_():
        dec.set_memory(memory)
        dec.begin(a.steps, N_HYP)
        torch.cuda.synchronize()
        t_step = t_reorder = 0.0
        for pos in range(a.steps):
            if pos > 0:
                t = time.perf_counter()
                dec.reorder(parents[pos])
                t_reorder += time.perf_counter() - t
            t = time.perf_counter()
            dec.step(tokens[pos], pos)
            t_step += time.perf_counter() - t
        return t_step * 1e3 / a.steps, t_reorder * 1e3 / (a.steps - 1)

    round_()
    rounds = [round_() for _ in range(a.reps)]
    res = {"device": torch.cuda.get_device_name(0), "config": synth.SANM_TEMPLATE, "reps": a.reps, "steps_per_rep": a.steps,
           "n_hyp": N_HYP, "memory_rows": T_MEM, "launches_per_step": launches_per_step(dec.att_layer_num, dec.num_blocks),
           "step_ms": spread([r[0] for r in rounds]), "reorder_ms": spread([r[1] for r in rounds])}
    print(res, flush=True)
    feats = torch.randn(1, 167, conf["input_size"], generator=g).to(dev)
    m.init_beam_search(decoding_ctc_weight=0.0, beam_size=N_HYP)

    def encode():
        enc, _ = m.encode(feats, [167])
        torch.cuda.synchronize()
        return enc

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    enc = encode()
    nbest = m.beam_search_features(enc[0])                               # warm-up of the search's shapes
    t_enc, t_search = [], []
    for _ in range(a.reps):
        t_enc.append(timed(encode)[0])
        t_search.append(timed(lambda: m.beam_search_features(enc[0]))[0])
    res["clip_10s"] = {"frames": 167, "beam": N_HYP, "positions": max(len(h.yseq) for h in nbest) - 2 if nbest else None,
                       "encoder_precision": m.encoder._mode(), "encoder_ms": spread(t_enc), "beam_search_ms": spread(t_search)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
