"""Conformer at AISHELL sizes (12 + 6 blocks, D 256, 4 heads, FFN 2048, kernel 15, 4234 tokens; synthetic weights) on one MI355X:
encoder + greedy CTC at 32 x 10 s and 4 x 60 s in f16x2 and fp32 against the float32 torch eager restatement
(tests/_conformer_oracle.py) on the same GPU in the same call, alternating; and the beam search (beam 10, CTC weight 0.3) on a 10-s
clip: ms per step and per utterance against the same restatement stepping one hypothesis at a time as the reference does.
Writes profiles/conformer_bench.json.  Usage: python tools/bench_conformer.py [--reps 5] [--out profiles/conformer_bench.json]
`--profile MODE` (f16x2 | fp32) runs only the HIP path for a kernel trace (`rocprofv3 --kernel-trace --stats -- python
tools/bench_conformer.py --profile f16x2` -> profiles/conformer_kernel_stats_<mode>.csv): three encoder + CTC passes at 32 x 10 s
in that mode and one beam search, nothing else (`--part encoder | beam` runs one of the two)."""
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
from funasr_amd.conformer import Conformer  # noqa: E402
from funasr_amd.transformer_search import BeamSearchTransformer  # noqa: E402
from tests import _conformer_oracle as O  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return sorted(ts)[len(ts) // 2]


class OneAtATime:
    """the eager restatement driven as the reference drives its decoder: one hypothesis per call"""

    def __init__(self, sd, conf, memory):
        self.sd, self.conf, self.memory, self.steppers, self.calls = sd, conf, memory, [], 0

    def begin(self, max_len, max_hyp):
        self.steppers = [O.DecoderStepper(self.sd, self.conf, self.memory)]
        self.steppers[0].begin(max_len, 1)

    def reorder(self, parents):
        new = []
        for p in parents:
            s = O.DecoderStepper.__new__(O.DecoderStepper)
            s.__dict__.update(self.steppers[p].__dict__)
            s.K, s.V = list(self.steppers[p].K), list(self.steppers[p].V)
            new.append(s)
        self.steppers = new

    def step(self, tokens, pos):
        self.calls += 1
        return torch.cat([s.step([t], pos) for s, t in zip(self.steppers, tokens)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conformer_bench.json"))
    ap.add_argument("--profile", default=None, choices=["f16x2", "fp32"])
    ap.add_argument("--part", default="both", choices=["both", "encoder", "beam"], help="with --profile: what to run")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    conf = synth.conformer_conf(**synth.CONFORMER_AISHELL)
    m = Conformer(**conf)
    sd = synth.conformer_state_dict(13, m)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    if a.profile:
        m.set_precision(a.profile)
        feats = torch.randn(32, 998, 80, generator=torch.Generator().manual_seed(32)).to(dev)
        for _ in range(3 if a.part != "beam" else 1):
            enc, _ = m.encode(feats, [998] * 32)
            m.ctc.argmax(enc)
        if a.part != "encoder":
            m.init_beam_search(beam_size=10, decoding_ctc_weight=0.3)
            m.beam_search_features(enc[0])
        torch.cuda.synchronize()
        return
    sd32 = O.cast(sd, torch.float32, dev)
    res = {"device": torch.cuda.get_device_name(0), "config": synth.CONFORMER_AISHELL, "reps": a.reps, "encoder_ctc_ms": {}}
    for B, frames in ((32, 998), (4, 5998)):
        feats = torch.randn(B, frames, 80, generator=torch.Generator().manual_seed(B)).to(dev)
        lens = [frames] * B

        def hip():
            enc, ol = m.encode(feats, lens)
            return m.ctc.argmax(enc)

        def eager():
            with torch.no_grad():
                enc, _ = O.encoder(sd32, conf["encoder_conf"], feats, lens)
                return O.ctc_log_softmax(sd32, enc).argmax(-1)

        row = {}
        for mode in ("f16x2", "fp32"):
            m.set_precision(mode)
            row[mode] = timed(hip, a.reps)
            row["eager_fp32_after_" + mode] = timed(eager, a.reps)
        res["encoder_ctc_ms"][f"{B}x{round(frames / 100)}s"] = row
        print(B, frames, row, flush=True)
    # beam search on a 10-s clip
    m.set_precision("f16x2")
    feats = torch.randn(1, 998, 80, generator=torch.Generator().manual_seed(77)).to(dev)
    enc, _ = m.encode(feats, [998])
    m.init_beam_search(beam_size=10, decoding_ctc_weight=0.3)
    t = time.perf_counter()
    nb = m.beam_search_features(enc[0])
    torch.cuda.synchronize()
    hip_ms = (time.perf_counter() - t) * 1e3
    steps = max(len(h.yseq) for h in nb) - 1 if nb else 0
    ctc_logp = m.ctc.log_softmax(enc)[0].cpu().numpy()
    bs = BeamSearchTransformer(beam_size=10, vocab_size=m.vocab_size, sos=m.sos, eos=m.eos, ctc_weight=0.3)
    st = OneAtATime(sd32, conf["decoder_conf"], enc[0])
    t = time.perf_counter()
    with torch.no_grad():
        nb2 = bs(st, enc.shape[1], ctc_logp)
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t) * 1e3
    res["beam_search_10s"] = {"beam": 10, "ctc_weight": 0.3, "hip_ms_per_utterance": hip_ms, "eager_ms_per_utterance": eager_ms,
                              "positions": st.calls, "hip_ms_per_step": hip_ms / max(st.calls, 1), "eager_ms_per_step": eager_ms / max(st.calls, 1),
                              "longest_hypothesis": steps, "same_best_ids": bool(nb and nb2 and nb[0].yseq == nb2[0].yseq)}
    print(res["beam_search_10s"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
