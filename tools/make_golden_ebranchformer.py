"""Writes tests/golden/ebranchformer.npz and tests/golden/ebranchformer_state_dict.json. The reference's own `EBranchformer`
(funasr/models/e_branchformer/model.py over its EBranchformerEncoder, TransformerDecoder and CTC, imported read-only through
oracle.ref_import) runs in float64 AND float32 on synthetic weights (funasr_amd.synth.ebranchformer_state_dict; weights are never
stored) at a tiny configuration (D 128, 2 heads, cgMLP 256, FFN 256, 2 + 2 blocks, 80 features, 40 tokens) in two variants:
  * `latest_macaron`: rel_pos_type latest, use_ffn + macaron_ffn, conv kernels 31 / 31 (the template's layout);
  * `legacy_noffn`:   rel_pos_type legacy, use_ffn false, conv kernels 15 / 3.
Per variant (keys `<variant>/<name>`), as tools/make_golden_conformer.py stores them for the Conformer:
  * two single clips of 163 / 247 feature frames and the ragged batch of both (the reference's lengths recorded): encoder rows, CTC
    log-probabilities, greedy ids;
  * `forward_one_step` log-probabilities for a few prefixes over clip 0's memory;
  * the beam n-best (ids, scores) of clip 0 for decoding_ctc_weight 0.0 and 0.3 at beam 5, nbest 2;
  * `pos_rows`: the rows of the reference's float32 positional table that these clips read;
  * the float64 results and `gap_* = max |fp32 - fp64|` per quantity, with ONE `gap_nbest_score`.
The generator asserts that greedy ids and n-best ids agree between the float32 and the float64 run (a seed that fails is replaced),
and that the shorter clip's batched rows differ from its rows alone by more than 100 x the gap: the reference masks neither depthwise
conv, and a fixture that did not show it would not notice a masked one.
The json holds key -> shape of the reference's state dict at funasr/models/e_branchformer/template.yaml and at the tiny size.
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
LENS = (163, 247)
PREFIXES = ([1], [1, 5], [1, 5, 9, 17], [1, 30, 31, 32, 33, 34])
CTC_WEIGHTS = (0.0, 0.3)
BEAM, NBEST = 5, 2
VARIANTS = {"latest_macaron": dict(rel_pos_type="latest", use_ffn=True, macaron=True, cgmlp_kernel=31, merge_kernel=31),
            "legacy_noffn": dict(rel_pos_type="legacy", use_ffn=False, macaron=False, cgmlp_kernel=15, merge_kernel=3)}
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(36)] + ["<unk>"]


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.e_branchformer.encoder  # noqa: F401  (registers EBranchformerEncoder)
    import funasr.models.transformer.decoder  # noqa: F401  (registers TransformerDecoder)
    from funasr.models.e_branchformer.model import EBranchformer
    return EBranchformer


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
        memory = torch.from_numpy(out["enc_0"])[None]
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
    import yaml

    from funasr_amd import synth
    from oracle import ref_import

    Ref = _reference()
    feats = features()
    out = {"seed": np.int64(SEED), "lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS), "variants": np.asarray(list(VARIANTS)),
           "prefixes": np.asarray([",".join(map(str, p)) for p in PREFIXES]), "ctc_weights": np.asarray(CTC_WEIGHTS),
           "beam": np.int64(BEAM), "nbest": np.int64(NBEST)}
    for i, f in enumerate(feats):
        out[f"feats_{i}"] = f.numpy()
    tiny_shapes = {}
    for name, kw in VARIANTS.items():
        conf = synth.ebranchformer_conf(vocab=len(TOKENS), **kw)
        ref = Ref(**conf)
        sd = synth.ebranchformer_state_dict(SEED, ref)
        ref.load_state_dict(sd, strict=True)
        ref.eval()
        tiny_shapes[name] = {k: list(v.shape) for k, v in ref.state_dict().items()}
        r64 = run(ref, torch.float64, feats)
        ref.load_state_dict(sd, strict=True)                         # the float32 weights again, not the rounded float64 copy
        r32 = run(ref, torch.float32, feats)
        v = {}
        # the rows of the reference's positional table these clips read (its last bits depend on the recording host's float32 exp())
        pe = ref.float().encoder.embed.out[1].pe[0]
        tmax = int(r64["batch_enc_1"].shape[0])
        legacy = kw["rel_pos_type"] == "legacy"
        v["pos_rows"] = (pe[:tmax] if legacy else pe[pe.shape[0] // 2 - tmax + 1: pe.shape[0] // 2 + tmax]).numpy().astype(np.float32)
        for k, a in r64.items():
            v[k] = a
            if "greedy" in k or "nbest_ids" in k or k == "batch_olens":
                assert np.array_equal(a, r32[k]), (name, k, a, r32[k])
            else:
                v["gap_" + k] = np.float64(np.abs(np.asarray(a, np.float64) - np.asarray(r32[k], np.float64)).max())
        v["gap_nbest_score"] = np.float64(max(float(v.pop(k)) for k in list(v) if k.startswith("gap_nbest_score_")))
        n = min(v["enc_0"].shape[0], v["batch_enc_0"].shape[0])
        apart = float(np.abs(v["enc_0"][:n] - v["batch_enc_0"][:n]).max())
        assert apart > 100 * float(v["gap_batch_enc_0"]), (name, apart, float(v["gap_batch_enc_0"]))
        print(name, "olens", v["batch_olens"].tolist(), "frames alone", [v[f"enc_{i}"].shape[0] for i in range(len(LENS))], "greedy",
              [len(v[f"greedy_{i}"]) for i in range(len(LENS))], "nbest", [v[f"nbest_ids_w{w}_0"].tolist() for w in CTC_WEIGHTS],
              f"clip 0 batched vs alone {apart:.3e}")
        for k in sorted(v):
            if k.startswith("gap_"):
                print("   ", k, f"{float(v[k]):.3e}")
        out.update({f"{name}/{k}": a for k, a in v.items()})
    path = os.path.join(ROOT, "tests", "golden", "ebranchformer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)
    tmpl = yaml.safe_load(open(os.path.join(ref_import.REF_ROOT, "funasr", "models", "e_branchformer", "template.yaml")))
    big = Ref(encoder=tmpl["encoder"], encoder_conf=tmpl["encoder_conf"], decoder=tmpl["decoder"], decoder_conf=tmpl["decoder_conf"],
              vocab_size=4234, input_size=80, **tmpl["model_conf"])
    with open(os.path.join(ROOT, "tests", "golden", "ebranchformer_state_dict.json"), "w") as f:
        json.dump({"model": tmpl["model"], "encoder": tmpl["encoder"], "encoder_conf": tmpl["encoder_conf"], "decoder": tmpl["decoder"],
                   "decoder_conf": tmpl["decoder_conf"], "model_conf": tmpl["model_conf"], "vocab_size": 4234,
                   "shapes": {k: list(v.shape) for k, v in big.state_dict().items()}, "tiny_shapes": tiny_shapes}, f, indent=0)


if __name__ == "__main__":
    main()
