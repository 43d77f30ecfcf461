"""Writes tests/golden/transformer.npz and tests/golden/transformer_state_dict.json. The reference's own `Transformer`
(funasr/models/transformer/model.py, imported read-only through oracle.ref_import) runs in float64 AND float32 on synthetic weights
(funasr_amd.synth.transformer_state_dict; weights are never stored) at a tiny configuration (D 128, 2 heads, FFN 256, 2 + 2 blocks,
60 tokens, 80 features). Contents, stored quantities and the float32 / float64 agreement asserts are those of
tools/make_golden_conformer.py (whose `run` this calls): three single clips of 101 / 163 / 247 frames and the ragged batch of the
three, `forward_one_step` for a few prefixes, the beam n-best of clip 0 at decoding_ctc_weight 0.0 and 0.3 (beam 5, nbest 2),
`pos_rows`, the float64 results and `gap_* = max |fp32 - fp64|` per quantity with ONE `gap_nbest_score`. A seed whose greedy ids
or n-best ids differ between the two runs fails the generator: pick another one.
The json holds the shapes of the reference's state dict at examples/aishell/transformer/conf/transformer_12e_6d_2048_256.yaml.
Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.make_golden_conformer import BEAM, CTC_WEIGHTS, LENS, NBEST, PREFIXES, TOKENS, features, run  # noqa: E402

SEED = 5


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.transformer.decoder  # noqa: F401  (registers TransformerDecoder)
    import funasr.models.transformer.encoder  # noqa: F401  (registers TransformerEncoder)
    from funasr.models.transformer.model import Transformer
    return Transformer


def main():
    from funasr_amd import synth

    Ref = _reference()
    feats = features(SEED)
    conf = synth.transformer_conf(vocab=len(TOKENS))
    ref = Ref(**conf)
    sd = synth.transformer_state_dict(SEED, ref)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    r64 = run(ref, torch.float64, feats)
    ref.load_state_dict(sd, strict=True)                             # the float32 weights again, not the rounded float64 copy
    r32 = run(ref, torch.float32, feats)
    out = {"seed": np.int64(SEED), "lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS),
           "prefixes": np.asarray([",".join(map(str, p)) for p in PREFIXES]), "ctc_weights": np.asarray(CTC_WEIGHTS),
           "beam": np.int64(BEAM), "nbest": np.int64(NBEST)}
    for i, f in enumerate(feats):
        out[f"feats_{i}"] = f.numpy()
    # the rows of the reference's positional table these clips read (its last bits depend on the recording host's float32 exp())
    pe = ref.float().encoder.embed.out[1].pe[0]
    out["pos_rows"] = pe[: int(r64["batch_enc_2"].shape[0])].numpy().astype(np.float32)
    for k, v in r64.items():
        out[k] = v
        if "greedy" in k or "nbest_ids" in k or k == "batch_olens":
            assert np.array_equal(v, r32[k]), (k, v, r32[k])
        else:
            out["gap_" + k] = np.float64(np.abs(np.asarray(v, np.float64) - np.asarray(r32[k], np.float64)).max())
    out["gap_nbest_score"] = np.float64(max(float(out.pop(k)) for k in list(out) if k.startswith("gap_nbest_score_")))
    path = os.path.join(ROOT, "tests", "golden", "transformer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; olens", out["batch_olens"].tolist(), "frames alone", [out[f"enc_{i}"].shape[0] for i in range(3)],
          "greedy", [len(out[f"greedy_{i}"]) for i in range(3)], "nbest", [out[f"nbest_ids_w{w}_0"].tolist() for w in CTC_WEIGHTS])
    for k in sorted(out):
        if k.startswith("gap_"):
            print("   ", k, f"{float(out[k]):.3e}")
    import yaml
    from oracle import ref_import
    tmpl = yaml.safe_load(open(os.path.join(ref_import.REF_ROOT, "examples", "aishell", "transformer", "conf", "transformer_12e_6d_2048_256.yaml")))
    big = Ref(encoder=tmpl["encoder"], encoder_conf=tmpl["encoder_conf"], decoder=tmpl["decoder"], decoder_conf=tmpl["decoder_conf"],
              vocab_size=4234, input_size=80, **tmpl["model_conf"])
    with open(os.path.join(ROOT, "tests", "golden", "transformer_state_dict.json"), "w") as f:
        json.dump({"encoder_conf": tmpl["encoder_conf"], "decoder_conf": tmpl["decoder_conf"], "model_conf": tmpl["model_conf"],
                   "vocab_size": 4234, "shapes": {k: list(v.shape) for k, v in big.state_dict().items()}}, f, indent=0)


if __name__ == "__main__":
    main()
