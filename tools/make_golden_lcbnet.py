"""Writes tests/golden/lcbnet.npz and tests/golden/lcbnet_state_dict.json. The reference's own `LCBNet`
(funasr/models/lcbnet/model.py, imported read-only through oracle.ref_import) runs in float64 AND float32 on synthetic weights
(funasr_amd.synth.lcbnet_state_dict; weights are never stored) at a tiny configuration (D 128, 2 heads, FFN 256, 2 + 2 audio blocks,
2 text blocks, the one fusion layer, ctc_weight 0.3, 300 tokens -- the default ids of a decode without text need 296 --, 80 features).

How the reference is driven: its `inference` cannot run here. The sound route needs waveforms and the reference's frontend (kaldi
fbank through torchaudio, which oracle.ref_import only stubs), and its `data_type="fbank"` route raises UnboundLocalError
(`ocr_sample_list` is unbound, model.py:481-487). So the four calls of model.py:516-533 are composed exactly as `inference` composes
them, on the reference's own objects: `encode`, the id shift (+1 for every id but 0) and `text_encoder(ocr, ocr_lengths)` with the full
length, `fusion_encoder(encoder_out, None, ocr, None)`, `encoder_out + fusion_out`, `init_beam_search` / `beam_search(x=encoder_out[0])`.

Contents: one clip of 163 feature frames and one of 247, each with OCR texts of 1, 2 (the reference's default ids [294, 0]), 6, 33 and
120 ids:
  * `enc_<c>`: the audio encoder's rows; `text_<j>`: the text encoder's rows (they do not depend on the clip);
  * `fusion_<c>_<j>`: the fusion layer's output. The fused memory `encoder_out + fusion_out` is NOT stored as an array: in float64 it is
    bitwise `enc_<c> + fusion_<c>_<j>` (the same float64 addition of the same two stored arrays), and storing it again would take the
    file past the size limit of a committed fixture; tests/test_lcbnet.py `load_golden` forms it. Its `gap_fused_<c>_<j>` is stored;
  * `greedy_<c>_<j>`: the greedy CTC ids of the fused memory; `nbest_ids_w<w>_<c>_<j>_<r>` / `nbest_score_...`: the n-best at
    decoding_ctc_weight 0.0 and 0.3 (beam 5, nbest 2);
  * `pos_rows`: the rows of the reference's float32 positional table that these clips and texts read (both encoders build the same one);
  * `gap_* = max |fp32 - fp64|` per quantity, with ONE `gap_nbest_score` as in tools/make_golden_conformer.py.
The generator asserts that greedy ids and n-best ids agree between the float32 and the float64 run (a seed that fails is replaced),
and that for each clip at least two of the texts give different n-best ids: otherwise the fixture would not notice a fusion layer that
does nothing.
The json holds the shapes of the reference's state dict at a zoo-like size (D 256, 4 heads, FFN 2048, 12 + 6 blocks, 6 text blocks,
5000 tokens) and at the tiny size of the npz. Build container only (needs the reference tree)."""
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
TEXT_LENS = (1, 2, 6, 33, 120)
CTC_WEIGHTS = (0.0, 0.3)
BEAM, NBEST = 5, 2
VOCAB = 300
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(VOCAB - 4)] + ["<unk>"]


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.lcbnet.encoder  # noqa: F401  (registers TransformerTextEncoder / FusionSANEncoder / ConvBiasPredictor)
    import funasr.models.transformer.decoder  # noqa: F401  (registers TransformerDecoder)
    import funasr.models.transformer.encoder  # noqa: F401  (registers TransformerEncoder)
    from funasr.models.lcbnet.model import LCBNet
    return LCBNet


def features(seed: int = SEED):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, 80, generator=g) for n in LENS]


def texts(seed: int = SEED):
    """the raw ids (before the shift) of the five texts; text 1 is the reference's default. The others hold id 0 (never shifted) and
    the largest id the shift leaves inside the vocabulary"""
    g = torch.Generator().manual_seed(2000 + seed)
    out = []
    for n in TEXT_LENS:
        ids = torch.randint(1, VOCAB - 1, (n,), generator=g).tolist()
        if n >= 6:
            ids[2], ids[-1] = 0, VOCAB - 2
        out.append(ids)
    out[1] = [294, 0]
    return out


def run(model, dt, feats, ocrs):
    """every stored quantity of one precision: the calls of LCBNet.inference (model.py:516-533) composed as it composes them"""
    m = model.to(dt)
    out = {}
    with torch.no_grad():
        for j, raw in enumerate(ocrs):
            shifted = [t + 1 if t else 0 for t in raw]                  # every id but 0 moves up by one; the length is the full one
            text, _, _ = m.text_encoder(torch.tensor([shifted]), torch.tensor([len(shifted)]))
            out[f"text_{j}"] = text[0].numpy()
        for c, f in enumerate(feats):
            enc, _ = m.encode(f[None].to(dt), torch.tensor([f.shape[0]]))
            out[f"enc_{c}"] = enc[0].numpy()
            for j in range(len(ocrs)):
                text = torch.from_numpy(out[f"text_{j}"])[None]
                fusion, _, _, _ = m.fusion_encoder(enc, None, text, None)
                fused = enc + fusion
                out[f"fusion_{c}_{j}"] = fusion[0].numpy()
                out[f"fused_{c}_{j}"] = fused[0].numpy()
                y = torch.unique_consecutive(m.ctc.log_softmax(fused)[0].argmax(-1))
                out[f"greedy_{c}_{j}"] = y[y != 0].numpy().astype(np.int64)
                for w in CTC_WEIGHTS:
                    m.beam_search = None
                    m.init_beam_search(token_list=TOKENS, decoding_ctc_weight=w, beam_size=BEAM)
                    hyps = m.beam_search(x=fused[0], maxlenratio=0.0, minlenratio=0.0)[:NBEST]
                    assert len(hyps) == NBEST, len(hyps)
                    for r, h in enumerate(hyps):
                        out[f"nbest_ids_w{w}_{c}_{j}_{r}"] = np.asarray([int(t) for t in h.yseq], np.int64)
                        out[f"nbest_score_w{w}_{c}_{j}_{r}"] = np.float64(float(h.score))
        m.beam_search = None                                         # (a registered sub-module: keep it out of the state dict)
    return out


def main():
    from funasr_amd import synth

    Ref = _reference()
    feats, ocrs = features(), texts()
    conf = synth.lcbnet_conf(vocab=VOCAB)
    ref = Ref(**conf)
    assert ref.sos == ref.eos == VOCAB - 1
    sd = synth.lcbnet_state_dict(SEED, ref)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    r64 = run(ref, torch.float64, feats, ocrs)
    ref.load_state_dict(sd, strict=True)                             # the float32 weights again, not the rounded float64 copy
    r32 = run(ref, torch.float32, feats, ocrs)
    out = {"seed": np.int64(SEED), "lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS), "ctc_weights": np.asarray(CTC_WEIGHTS),
           "beam": np.int64(BEAM), "nbest": np.int64(NBEST)}
    for c, f in enumerate(feats):
        out[f"feats_{c}"] = f.numpy()
    for j, raw in enumerate(ocrs):
        out[f"ocr_{j}"] = np.asarray(raw, np.int64)
    pe = ref.float().encoder.embed.out[1].pe[0]
    pe_text = ref.text_encoder.embed[1].pe[0]
    rows = max(max(TEXT_LENS), max(int(r64[f"enc_{c}"].shape[0]) for c in range(len(feats))))
    assert torch.equal(pe[:rows], pe_text[:rows].float())
    out["pos_rows"] = pe[:rows].numpy().astype(np.float32)
    for k, v in r64.items():
        if "greedy" in k or "nbest_ids" in k:
            assert np.array_equal(v, r32[k]), (k, v, r32[k])
            out[k] = v
            continue
        out["gap_" + k] = np.float64(np.abs(np.asarray(v, np.float64) - np.asarray(r32[k], np.float64)).max())
        if k.startswith("fused_"):                                   # bitwise enc + fusion in float64: formed by the reader
            c, j = k.split("_")[1:]
            assert np.array_equal(v, r64[f"enc_{c}"] + r64[f"fusion_{c}_{j}"])
            continue
        out[k] = v
    out["gap_nbest_score"] = np.float64(max(float(out.pop(k)) for k in list(out) if k.startswith("gap_nbest_score_")))
    for c in range(len(feats)):
        for w in CTC_WEIGHTS:
            seen = {tuple(out[f"nbest_ids_w{w}_{c}_{j}_0"].tolist()) for j in range(len(ocrs))}
            print(f"clip {c} w {w}: {len(seen)} distinct best hypotheses over {len(ocrs)} texts, lengths",
                  [len(out[f"nbest_ids_w{w}_{c}_{j}_0"]) for j in range(len(ocrs))])
        assert len({tuple(tuple(out[f"nbest_ids_w{w}_{c}_{j}_{r}"].tolist()) for w in CTC_WEIGHTS for r in range(NBEST))
                    for j in range(len(ocrs))}) >= 2, f"clip {c}: every text gives the same n-best"
        print(f"clip {c} greedy", [out[f"greedy_{c}_{j}"].tolist() for j in range(len(ocrs))])
        print(f"clip {c} best at 0.3", [out[f"nbest_ids_w0.3_{c}_{j}_0"].tolist() for j in range(len(ocrs))],
              [float(out[f"nbest_score_w0.3_{c}_{j}_0"]) for j in range(len(ocrs))])
        print(f"clip {c} best at 0.0", [out[f"nbest_ids_w0.0_{c}_{j}_0"].tolist() for j in range(len(ocrs))])
    path = os.path.join(ROOT, "tests", "golden", "lcbnet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; frames", [out[f"enc_{c}"].shape[0] for c in range(len(feats))])
    for k in sorted(out):
        if k.startswith("gap_"):
            print("   ", k, f"{float(out[k]):.3e}")
    big = Ref(**synth.lcbnet_conf(**synth.LCBNET_ZOO_LIKE))
    with open(os.path.join(ROOT, "tests", "golden", "lcbnet_state_dict.json"), "w") as f:
        json.dump({"conf": synth.lcbnet_conf(**synth.LCBNET_ZOO_LIKE), "shapes": {k: list(v.shape) for k, v in big.state_dict().items()},
                   "tiny_conf": conf, "tiny_shapes": {k: list(v.shape) for k, v in ref.state_dict().items()}}, f, indent=0)


if __name__ == "__main__":
    main()
