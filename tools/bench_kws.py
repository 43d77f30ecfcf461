"""Keyword spotting at the two recipe sizes (fsmn_4e_l10r2_250_128_fdim80_t2599, sanm_6e_320_256_fdim40_t2602) on synthetic planted
weights and random feature batches of 256 x 2 s and 16 x 60 s -> profiles/kws_bench.json.

Per (model, shape): this package's `detect` (one encoder pass, one candidate launch, one read-back of 7 words per frame, the host
search) split into its phases, and -- for the FSMN -- the torch fp32 restatement of the same network on the same GPU followed by the
reference-style decode: the softmax of each clip copied to the host, `topk(3)` and `.tolist()` per frame from Python, the prefix
search in Python (tests/_kws_oracle.py). The two must return the same verdicts. Medians of `--rounds` rounds after one warm-up, with
the spread (DESIGN 3.9's method). The SAN-M encoder has no GPU restatement here: its baseline column is left out and says so."""
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

from funasr_amd import synth  # noqa: E402
from funasr_amd.kws import FsmnKWS, SanmKWS  # noqa: E402
from funasr_amd.kws_utils import KwsCtcPrefixDecoder, candidates  # noqa: E402
from tests import _kws_oracle as KO  # noqa: E402

SHAPES = {"256x2s": (256, 2.0), "16x60s": (16, 60.0)}
PLANTED = (5, 9, 21, 30, 44)


def reference_style(logits, lens, idxset, keywords):
    out = []
    for i, n in enumerate(lens):
        probs = torch.softmax(logits[i, :n], dim=-1).cpu()
        ns, ids, ps = [], [], []
        for t in range(n):
            tp, ti = probs[t].topk(3)
            kept = [(p, j) for p, j in zip(tp.tolist(), ti.tolist()) if p > 0.05 and j in idxset]
            ns.append(len(kept))
            ids.append([j for _, j in kept] + [-1] * (3 - len(kept)))
            ps.append([p for p, _ in kept] + [0.0] * (3 - len(kept)))
        out.append(KO.decide(KO.beam_search(ns, ids, ps), keywords)[0])
    return out


def med(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kws_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tokens = ["<blank>"] + [f"t{i}" for i in range(1, 2602)]
    res = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "cases": []}
    for name, cls, conf, frame_s in (("fsmn", FsmnKWS, synth.kws_fsmn_conf(**synth.KWS_FSMN_RECIPE), 0.03),
                                     ("sanm", SanmKWS, synth.kws_sanm_conf(**synth.KWS_SANM_RECIPE), 0.06)):
        V = conf["vocab_size"]
        model = cls(**conf)
        sd = synth.kws_state_dict(7, model, planted=PLANTED, blank=8.0 if name == "fsmn" else 11.0, gain=8.0 if name == "fsmn" else 4.5)
        model.load_state_dict(sd, strict=True)
        model = model.to(dev).eval()
        dec = KwsCtcPrefixDecoder(model.ctc, "t5t9,t21", tokens[:V], None)
        kw = [dec.keywords_token[k]["token_id"] for k in dec.keywords]
        sd_dev = {k: v.to(dev) for k, v in sd.items()}
        for shape, (B, secs) in SHAPES.items():
            T = int(secs / frame_s)
            g = torch.Generator().manual_seed(B)
            feats = torch.randn(B, T, conf["input_size"] if name == "sanm" else conf["encoder_conf"]["input_dim"], generator=g).to(dev)
            lens = [T] * B
            ph = {"network_and_candidates": [], "read_back": [], "host_search": [], "total": []}
            base = []
            mine = theirs = None
            for r in range(args.rounds + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                logits, olens = model._logits(feats, lens)
                cand = candidates(logits.reshape(B * T, -1), dec.mask_on(dev), V)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                host = cand.cpu().numpy().reshape(B, T, 7)
                t2 = time.perf_counter()
                mine = [w for w, _, _ in dec.decode_candidates(host, olens)]
                t3 = time.perf_counter()
                if r:
                    for k, v in zip(ph, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                        ph[k].append(v)
                if name == "fsmn":
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with torch.no_grad():
                        lg = KO.fsmn_logits(sd_dev, conf["encoder_conf"], feats, prefix="encoder.")
                    theirs = reference_style(lg, lens, dec.keywords_idxset, kw)
                    if r:
                        base.append(time.perf_counter() - t0)
            case = {"model": name, "shape": shape, "B": B, "T": T, "V": V, "detected": sum(1 for w in mine if w),
                    "ours": {k: med(v) for k, v in ph.items()}}
            if name == "fsmn":
                case["torch_restatement_with_reference_style_loop"] = med(base)
                case["same_verdicts"] = [bool(w) for w in mine] == [w >= 0 for w in theirs]
                assert case["same_verdicts"], (name, shape)
            else:
                case["torch_restatement_with_reference_style_loop"] = "not measured: no GPU restatement of the SAN-M encoder in this tool"
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
