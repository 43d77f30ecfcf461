"""Writes tests/golden/sanm.npz and tests/golden/sanm_state_dict.json. The reference's own `SANM` (funasr/models/sanm/model.py,
imported read-only through oracle.ref_import) runs in float64 AND float32 on synthetic weights (funasr_amd.synth.sanm_state_dict;
weights are never stored) at two tiny configurations, so that both properties of its decoder step are on record:
  A  D 128, 2 heads (d_k 64), FFN 64, decoder kernel 11 with the constructor's default sanm_shfit (R = 0: the causal memory),
     att_layer_num 2 of num_blocks 3 (one `decoders2` layer), a CTC head; n-best at decoding_ctc_weight 0.0 and 0.3
  B  D 256, 2 heads (d_k 128), FFN 256, decoder kernel 4 (even) with sanm_shfit 0 (R = 2: NOT the causal memory),
     att_layer_num == num_blocks == 2, ctc_weight 0.0 (no CTC head); n-best at decoding_ctc_weight 0.0
Per configuration (keys prefixed "A_" / "B_"): the encoder output of two clips of 23 / 41 feature frames (SANMEncoder with the true
length), the log-probabilities of `FsmnDecoder.score` -- the call of the beam search, one token at a time with the cache it returns
-- after prefixes of 1, 2, K - 1, K, K + 1 and K + 3 tokens over clip 1's memory, and the beam n-best (ids, scores) of clip 0 at
beam 5, nbest 2. Stored: the float64 results and, of the float32 run, only max |fp32 - fp64| per quantity (`gap_*`, also printed);
the n-best scores are ONE quantity per configuration (`gap_nbest_score`, the maximum over the stored hypotheses). The generator
asserts that greedy ids and n-best ids agree between the two runs: a seed where they do not fails it -- pick another one.
The json holds the shapes of the reference's state dict at funasr/models/sanm/template.yaml (vocabulary 8404, 560 features).
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
LENS = (23, 41)
BEAM, NBEST = 5, 2
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(56)] + ["<unk>"]
CONFIGS = {
    "A": dict(conf=dict(output_size=128, attention_heads=2, linear_units=64, enc_blocks=2, dec_blocks=3, att_layer_num=2, kernel=11,
                        ctc_weight=0.3), ctc_weights=(0.0, 0.3)),
    "B": dict(conf=dict(output_size=256, attention_heads=2, linear_units=256, enc_blocks=2, dec_blocks=2, att_layer_num=2, kernel=4,
                        sanm_shfit=0, ctc_weight=0.0), ctc_weights=(0.0,)),
}


def prefix_lengths(K: int):
    return sorted({1, 2, K - 1, K, K + 1, K + 3})


def prefix(n: int):
    """<sos> and n - 1 tokens off the special ids"""
    return [1] + [3 + (5 + 11 * i) % (len(TOKENS) - 4) for i in range(n - 1)]


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.sanm.decoder  # noqa: F401  (registers FsmnDecoder)
    import funasr.models.sanm.encoder  # noqa: F401  (registers SANMEncoder)
    from funasr.models.sanm.model import SANM
    return SANM


def features(seed: int = SEED):
    g = torch.Generator().manual_seed(2000 + seed)
    return [torch.randn(n, 80, generator=g) for n in LENS]


def run(model, dt, feats, K, ctc_weights):
    """every stored quantity of one precision"""
    m = model.to(dt)
    out = {}
    with torch.no_grad():
        for i, f in enumerate(feats):
            enc, olens = m.encode(f[None].to(dt), torch.tensor([f.shape[0]]))
            assert int(olens[0]) == f.shape[0]
            out[f"enc_{i}"] = enc[0].numpy()
            if m.ctc is not None:
                lp = m.ctc.log_softmax(enc)[0]
                out[f"ctc_{i}"] = lp.numpy()
                y = torch.unique_consecutive(lp.argmax(-1))
                out[f"greedy_{i}"] = y[y != 0].numpy().astype(np.int64)
        memory = torch.from_numpy(out["enc_1"])
        for n in prefix_lengths(K):
            ys, state, logp = torch.tensor(prefix(n)), None, None
            for j in range(1, n + 1):
                logp, state = m.decoder.score(ys[:j], state, memory)
            out[f"step_{n}"] = logp.numpy()
        x = torch.from_numpy(out["enc_0"])
        for w in ctc_weights:
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
    out = {"seed": np.int64(SEED), "lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS), "beam": np.int64(BEAM),
           "nbest": np.int64(NBEST)}
    for i, f in enumerate(feats):
        out[f"feats_{i}"] = f.numpy()
    for name, spec in CONFIGS.items():
        conf = synth.sanm_conf(vocab=len(TOKENS), **spec["conf"])
        K = conf["decoder_conf"]["kernel_size"]
        ref = Ref(**conf)
        sd = synth.sanm_state_dict(SEED, ref)
        ref.load_state_dict(sd, strict=True)
        ref.eval()
        r64 = run(ref, torch.float64, feats, K, spec["ctc_weights"])
        ref.load_state_dict(sd, strict=True)                         # the float32 weights again, not the rounded float64 copy
        r32 = run(ref, torch.float32, feats, K, spec["ctc_weights"])
        out[name + "_ctc_weights"] = np.asarray(spec["ctc_weights"])
        out[name + "_prefix_lengths"] = np.asarray(prefix_lengths(K), np.int64)
        gaps = []
        for k, v in r64.items():
            out[f"{name}_{k}"] = v
            if "greedy" in k or "nbest_ids" in k:
                assert np.array_equal(v, r32[k]), (name, k, v, r32[k])
            elif k.startswith("nbest_score"):
                gaps.append(abs(float(v) - float(r32[k])))
            else:
                out[f"{name}_gap_{k}"] = np.float64(np.abs(np.asarray(v, np.float64) - np.asarray(r32[k], np.float64)).max())
        out[name + "_gap_nbest_score"] = np.float64(max(gaps))
        print(name, "nbest", [out[f"{name}_nbest_ids_w{w}_0"].tolist() for w in spec["ctc_weights"]])
    path = os.path.join(ROOT, "tests", "golden", "sanm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if "_gap_" in k:
            print("   ", k, f"{float(out[k]):.3e}")
    import yaml
    from oracle import ref_import
    tmpl = yaml.safe_load(open(os.path.join(ref_import.REF_ROOT, "funasr", "models", "sanm", "template.yaml")))
    big = Ref(encoder=tmpl["encoder"], encoder_conf=tmpl["encoder_conf"], decoder=tmpl["decoder"], decoder_conf=tmpl["decoder_conf"],
              vocab_size=8404, input_size=560, **tmpl["model_conf"])
    with open(os.path.join(ROOT, "tests", "golden", "sanm_state_dict.json"), "w") as f:
        json.dump({"encoder_conf": tmpl["encoder_conf"], "decoder_conf": tmpl["decoder_conf"], "model_conf": tmpl["model_conf"],
                   "vocab_size": 8404, "input_size": 560, "shapes": {k: list(v.shape) for k, v in big.state_dict().items()}}, f, indent=0)


if __name__ == "__main__":
    main()
