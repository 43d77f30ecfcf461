"""Writes tests/golden/conformer_<variant>.npz (variant = {legacy, latest} x {macaron, plain}; one file per variant keeps each
fixture well below 1 MiB) and tests/golden/conformer_state_dict.json. The reference's own `Conformer`
(funasr/models/conformer/model.py, imported read-only through oracle.ref_import) runs in float64 AND float32 on synthetic weights
(funasr_amd.synth.conformer_state_dict; weights are never stored) at a tiny configuration (D 128, 2 heads, FFN 256, kernel 15,
2 + 2 blocks, 60 tokens):
  * three single clips of 101 / 163 / 247 feature frames and the ragged batch of the three (the reference's lengths recorded):
    encoder output, CTC log-probabilities, greedy ids;
  * `forward_one_step` log-probabilities for a few prefixes over clip 1's memory;
  * the beam n-best (ids, scores) of clip 0 for decoding_ctc_weight 0.0 and 0.3 at beam 5, nbest 2;
  * `pos_rows`: the rows of the reference's float32 positional table that these clips read.
Stored: the float64 results and, of the float32 run, only max |fp32 - fp64| per quantity (`gap_*`, also printed). The n-best
scores are ONE quantity (`gap_nbest_score` = the maximum over the stored hypotheses): a single hypothesis' float32 score can land
within 1e-8 of the float64 one by chance (below one float32 ulp of a score of -20), which says nothing about the reference's error.
The generator asserts that greedy ids and n-best ids agree between the float32 and the float64 run for every stored case.
Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 5
LENS = (101, 163, 247)
PREFIXES = ([1], [1, 5], [1, 5, 9, 17], [1, 30, 31, 32, 33, 34])
CTC_WEIGHTS = (0.0, 0.3)
BEAM, NBEST = 5, 2
VARIANTS = {"legacy_macaron": ("legacy", True), "legacy_plain": ("legacy", False), "latest_macaron": ("latest", True),
            "latest_plain": ("latest", False)}
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(56)] + ["<unk>"]


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.conformer.encoder  # noqa: F401  (registers ConformerEncoder)
    import funasr.models.transformer.decoder  # noqa: F401  (registers TransformerDecoder)
    from funasr.models.conformer.model import Conformer
    return Conformer


def features(seed: int = SEED):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, 80, generator=g) for n in LENS]


def run(model, dt, feats):
    """every stored quantity of one precision"""
    m = model.to(dt)
    out = {}
    with torch.no_grad():
        for i, f in enumerate(feats):
            enc, olens = m.encode(f[None].to(dt), torch.tensor([f.shape[0]]))
            out[f"enc_{i}"] = enc[0].numpy()
            lp = m.ctc.log_softmax(enc)[0]
            out[f"ctc_{i}"] = lp.numpy()
            y = torch.unique_consecutive(lp.argmax(-1))
            out[f"greedy_{i}"] = y[y != 0].numpy().astype(np.int64)
        pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True).to(dt)
        enc, olens = m.encode(pad, torch.tensor(LENS))
        out["batch_olens"] = olens.numpy().astype(np.int64)
        lp = m.ctc.log_softmax(enc)
        for i in range(len(feats)):
            n = int(olens[i])
            out[f"batch_enc_{i}"] = enc[i, :n].numpy()
            out[f"batch_ctc_{i}"] = lp[i, :n].numpy()
            y = torch.unique_consecutive(lp[i, :n].argmax(-1))
            out[f"batch_greedy_{i}"] = y[y != 0].numpy().astype(np.int64)
        memory = torch.from_numpy(out["enc_1"])[None]
        for j, pre in enumerate(PREFIXES):
            ys = torch.tensor([pre])
            mask = torch.tril(torch.ones(len(pre), len(pre), dtype=torch.bool))[None]
            logp, _ = m.decoder.forward_one_step(ys, mask, memory, cache=None)
            out[f"step_{j}"] = logp[0].numpy()
        x = torch.from_numpy(out["enc_0"])
        for w in CTC_WEIGHTS:
            m.beam_search = None
            m.init_beam_search(token_list=TOKENS, decoding_ctc_weight=w, beam_size=BEAM)
            hyps = m.beam_search(x=x, maxlenratio=0.0, minlenratio=0.0)[:NBEST]
            assert len(hyps) == NBEST, len(hyps)
            for r, h in enumerate(hyps):
                out[f"nbest_ids_w{w}_{r}"] = np.asarray([int(t) for t in h.yseq], np.int64)
                out[f"nbest_score_w{w}_{r}"] = np.float64(float(h.score))
        m.beam_search = None                                         # (a registered sub-module: keep it out of the state dict)
    return out


def main():
    from funasr_amd import synth

    Ref = _reference()
    feats = features()
    for name, (rel, mac) in VARIANTS.items():
        conf = synth.conformer_conf(macaron=mac, rel_pos_type=rel, vocab=len(TOKENS))
        ref = Ref(**conf)
        sd = synth.conformer_state_dict(SEED, ref)
        ref.load_state_dict(sd, strict=True)
        ref.eval()
        r64 = run(ref, torch.float64, feats)
        ref.load_state_dict(sd, strict=True)                         # the float32 weights again, not the rounded float64 copy
        r32 = run(ref, torch.float32, feats)
        out = {"seed": np.int64(SEED), "lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS),
               "prefixes": np.asarray([",".join(map(str, p)) for p in PREFIXES]), "ctc_weights": np.asarray(CTC_WEIGHTS),
               "beam": np.int64(BEAM), "nbest": np.int64(NBEST)}
        for i, f in enumerate(feats):
            out[f"feats_{i}"] = f.numpy()
        # the rows of the reference's positional table these clips read. The float32 table depends on the CPU's exp() in the last
        # bit of div_term, which moves a sinusoid of position ~5000 by up to 5e-4: a test on another machine pins these rows
        pe = ref.float().encoder.embed.out[1].pe[0]
        tmax = int(r64["batch_enc_2"].shape[0])
        out["pos_rows"] = (pe[:tmax] if rel == "legacy" else pe[pe.shape[0] // 2 - tmax + 1: pe.shape[0] // 2 + tmax]).numpy().astype(np.float32)
        for k, v in r64.items():
            if "greedy" in k or "nbest_ids" in k or k == "batch_olens":
                assert np.array_equal(v, r32[k]), (name, k, v, r32[k])
                out[k] = v
            else:
                out[k] = v
                out["gap_" + k] = np.float64(np.abs(np.asarray(v, np.float64) - np.asarray(r32[k], np.float64)).max())
        out["gap_nbest_score"] = np.float64(max(float(out.pop(k)) for k in list(out) if k.startswith("gap_nbest_score_")))
        path = os.path.join(ROOT, "tests", "golden", f"conformer_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes; olens", out["batch_olens"].tolist(),
              "greedy", [len(out[f"greedy_{i}"]) for i in range(3)], "nbest", [out[f"nbest_ids_w{w}_0"].tolist() for w in CTC_WEIGHTS])
        for k in sorted(out):
            if k.startswith("gap_"):
                print("   ", k, f"{float(out[k]):.3e}")
    import yaml
    tmpl = yaml.safe_load(open(os.path.join(os.environ.get("FUNASR_REFERENCE", "/root/reference"), "examples", "aishell", "conformer", "conf",
                                            "conformer_12e_6d_2048_256.yaml")))
    big = Ref(encoder=tmpl["encoder"], encoder_conf=tmpl["encoder_conf"], decoder=tmpl["decoder"], decoder_conf=tmpl["decoder_conf"],
              vocab_size=4234, input_size=80, **tmpl["model_conf"])
    with open(os.path.join(ROOT, "tests", "golden", "conformer_state_dict.json"), "w") as f:
        json.dump({"encoder_conf": tmpl["encoder_conf"], "decoder_conf": tmpl["decoder_conf"], "model_conf": tmpl["model_conf"],
                   "vocab_size": 4234, "shapes": {k: list(v.shape) for k, v in big.state_dict().items()}}, f, indent=0)


if __name__ == "__main__":
    main()
