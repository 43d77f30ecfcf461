"""Transducer search at the prediction / joint sizes of funasr/models/rwkv_bat/template.yaml (embed 512, hidden 512, joint 512,
4234 tokens; synthetic weights with planted tokens, funasr_amd.synth.transducer_state_dict) over the AISHELL ConformerEncoder on
one MI355X: one utterance of 1006 feature frames (10 s, 250 encoder frames), beam 2 and beam 10.
  search alone   `Transducer.search` on the encoder output (pf_transducer_search: prediction steps, two launches per joint
                 evaluation, one read-back each) against the float32 torch restatement of the same search
                 (tests/_transducer_oracle.py) on the same GPU in the same call;
  end to end     features -> encoder (f16x2) -> search, and the same with the restatement's search behind the HIP encoder.
The synthetic weights are those of the first seed whose search settles under the default cap at both beams (two planted labels on
one frame alternate without end; a trained model has no such frames) -- the seed is recorded. Timed in turn, `--reps` rounds;
reported: the median round's ms, the spread, the joint-evaluation count and the microseconds per evaluation.
Writes profiles/transducer_bench.json.  Usage: python tools/bench_transducer.py [--reps 5] [--out ...]"""
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
from funasr_amd.transducer import Transducer, TransducerSearchError  # noqa: E402
from tests import _transducer_oracle as O  # noqa: E402

FRAMES, BEAMS = 1006, (2, 10)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def build(seed, dev):
    enc = synth.conformer_conf(**{k: v for k, v in synth.CONFORMER_AISHELL.items() if k != "dec_blocks"})["encoder_conf"]
    conf = synth.transducer_conf(**synth.TRANSDUCER_TEMPLATE)
    conf["encoder_conf"] = enc
    m = Transducer(**conf)
    sd = synth.transducer_state_dict(seed, m, threshold=0.8)
    m.load_state_dict(sd, strict=True)
    return m.to(dev), sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transducer_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transducer: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    feats = torch.randn(1, FRAMES, 80, generator=torch.Generator().manual_seed(1)).to(dev)
    for seed in range(40):
        model, sd = build(seed, dev)
        enc, _ = model.encode(feats, [FRAMES])
        try:
            first = {b: model.search(enc[0], beam_size=b, nbest=1) for b in BEAMS}
            break
        except TransducerSearchError as e:
            print(f"seed {seed}: {e}", flush=True)
    else:
        raise SystemExit("bench_transducer: no seed below 40 gives a search that settles")
    sd32 = O.cast(sd, torch.float32, dev)
    res = {"device": torch.cuda.get_device_name(0), "config": synth.TRANSDUCER_TEMPLATE, "seed": seed, "feature_frames": FRAMES,
           "encoder_frames": int(enc.shape[1]), "reps": a.reps, "beams": {}}
    for beam in BEAMS:
        hyps, info = first[beam]

        def hip():
            return model.search(enc[0], beam_size=beam, nbest=1)

        def eager():
            with torch.no_grad():
                return O.search(sd32, enc[0], beam, nbest=1)

        def hip_e2e():
            e, _ = model.encode(feats, [FRAMES])
            return model.search(e[0], beam_size=beam, nbest=1)

        def eager_e2e():
            e, _ = model.encode(feats, [FRAMES])
            with torch.no_grad():
                return O.search(sd32, e[0], beam, nbest=1)

        fns = {"search_hip": hip, "search_torch_fp32": eager, "end_to_end_hip": hip_e2e, "end_to_end_hip_encoder_torch_search": eager_e2e}
        ref = eager()                                                     # warm-up of the restatement, and what it decodes
        hip_e2e()
        ts = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, f in fns.items():
                ts[k].append(timed(f)[0])
        row = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in ts.items()}
        row.update(info)
        row["tokens"] = len(hyps[0][0]) - 1
        row["us_per_joint_eval_hip"] = row["search_hip"]["median"] * 1e3 / info["joint_evals"]
        row["us_per_joint_eval_torch_fp32"] = row["search_torch_fp32"]["median"] * 1e3 / ref["joint_evals"]
        row["torch_fp32_joint_evals"] = ref["joint_evals"]
        row["same_ids_as_torch_fp32"] = bool(ref["ids"][0] == hyps[0][0])
        res["beams"][str(beam)] = row
        print(beam, row, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
