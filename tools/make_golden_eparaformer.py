"""Writes tests/golden/eparaformer.npz and tests/golden/eparaformer_state_dict.json. The reference's own `EParaformer`
(funasr/models/e_paraformer/model.py over ConformerEncoder, PifPredictor and ParaformerSANDecoder, imported read-only through
oracle.ref_import) runs in float64 AND float32, everything under torch.no_grad(), on synthetic weights
(funasr_amd.synth.eparaformer_state_dict; only the calibrated output layer is stored) at a tiny recipe-shaped configuration (D 128,
2 heads, 2 + 2 blocks, 256 units, 80 features, 40 tokens, 4 sigma heads). Inputs, keys `<run>/<name>`:
  * `s0`, `s1`: two single clips of 163 / 247 feature frames; `b`: the ragged batch of both; `z`: clip 1 beside a 3-frame clip that
    gets ZERO tokens.
Per run: the encoder rows of the whole padded batch, the pre-normalisation `token_num`, the normalised `alphas`, `align`, `embeds`
(all Lmax rows), the decoder log-probabilities, the rounded counts, the greedy ids, the `inference` records (text with the
reference's CharTokenizer, and `token_int` without a tokenizer), and `gap_* = max |fp32 - fp64|` per float quantity.
A random output layer gives one repeated id (the embeddings of neighbouring fire positions are close), so the output layer is
calibrated with synth.confident_output_layer on the float64 after_norm rows of the token positions, as make_paraformer_confident does.
The generator asserts, and takes the next seed if one fails: every token_num at least 0.05 away from a half-integer; fp32 and fp64
agree on counts and ids; each normal clip's greedy ids hold at least 5 distinct tokens; the shorter clip's batched embeds differ from
its rows alone by more than 100 x the gap (the unmasked conv and the batch-wide Lmax); the short clip of `z` really has n == 0; and no
`gap_token_num` lies under half an fp32 ulp of the sum (B numbers can agree by chance to a fraction of an ulp, and a bar of 4 x that
would lie below the spacing of fp32 itself).
The json holds key -> shape of the reference's state dict at the recipe and at the tiny size.
Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEEDS = tuple(range(5, 40))
LENS = (163, 247)
ZLEN = 3
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(36)] + ["<unk>"]
RECIPE = "examples/aishell/e_paraformer/conf/e_paraformer_conformer_12e_6d_2048_256.yaml"
FLOATS = ("enc", "token_num", "alphas", "align", "embeds", "logp")


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.conformer.encoder  # noqa: F401  (registers ConformerEncoder)
    import funasr.models.e_paraformer.decoder  # noqa: F401  (registers ParaformerSANDecoder)
    import funasr.models.e_paraformer.pif_predictor  # noqa: F401  (registers PifPredictor)
    from funasr.models.e_paraformer.model import EParaformer
    from funasr.tokenizer.char_tokenizer import CharTokenizer
    return EParaformer, CharTokenizer


def batches(seed: int):
    g = torch.Generator().manual_seed(1000 + seed)
    f0, f1 = [torch.randn(n, 80, generator=g) for n in LENS]
    fz = torch.randn(ZLEN, 80, generator=g)
    pad = torch.nn.utils.rnn.pad_sequence
    return {"s0": (f0[None], [LENS[0]]), "s1": (f1[None], [LENS[1]]), "b": (pad([f0, f1], batch_first=True), list(LENS)),
            "z": (pad([f1, fz], batch_first=True), [LENS[1], ZLEN])}


def run(m, dt, feats, lens, tokenizer, hidden=None):
    """every stored quantity of one batch in one precision; `hidden` (a list) collects the after_norm rows of the token positions"""
    out = {}
    with torch.no_grad():
        enc, olens = m.encode(feats.to(dt), torch.tensor(lens))
        emb, tn, alphas, _ = m.calc_predictor(enc, olens)
        counts = tn.round().long()
        out.update(enc=enc.numpy(), olens=olens.numpy().astype(np.int64), token_num=tn.numpy(), alphas=alphas.numpy(),
                   align=torch.cumsum(alphas, dim=-1).numpy(), embeds=emb.numpy(), counts=counts.numpy().astype(np.int64))
        grabbed = []
        hook = m.decoder.after_norm.register_forward_hook(lambda mod, i, o: grabbed.append(o))
        logp, _ = m.cal_decoder_with_predictor(enc, olens, emb, counts)
        hook.remove()
        if hidden is not None:
            hidden.extend(grabbed[0][b, : int(n)] for b, n in enumerate(counts))
        out["logp"] = logp.numpy()
        for b, n in enumerate(counts.tolist()):
            out[f"ids_{b}"] = logp[b, :n].argmax(-1).numpy().astype(np.int64)
        keys = [f"utt{b}" for b in range(len(lens))]
        kw = dict(data_lengths=torch.tensor(lens)[:, None], key=keys, frontend=None, data_type="fbank", device="cpu")
        res, _ = m.inference(feats.to(dt), tokenizer=tokenizer, **kw)
        out["texts"] = np.asarray([r["text"] for r in res])
        res, _ = m.inference(feats.to(dt), tokenizer=None, **kw)
        for b, r in enumerate(res):
            out[f"token_int_{b}"] = np.asarray(r["token_int"], np.int64)
        assert [r["key"] for r in res] == keys
    return out


def attempt(seed: int, Ref, tokenizer):
    from funasr_amd import synth

    conf = synth.eparaformer_conf(vocab=len(TOKENS))
    ref = Ref(**conf)
    ref.eval()
    sd = synth.eparaformer_state_dict(seed, ref)
    ref.load_state_dict(sd, strict=True)
    bs = batches(seed)
    hidden = []
    ref.double()
    for name in ("s0", "s1", "b"):
        run(ref, torch.float64, *bs[name], tokenizer, hidden)
    W, b, stats = synth.confident_output_layer(sd["decoder.output_layer.weight"], sd["decoder.output_layer.bias"], torch.cat(hidden).float())
    sd["decoder.output_layer.weight"], sd["decoder.output_layer.bias"] = W, b
    out = {"seed": np.int64(seed), "output_layer_weight": W.numpy(), "output_layer_bias": b.numpy()}
    res = {}
    for dt in (torch.float64, torch.float32):
        ref.float()
        ref.load_state_dict(sd, strict=True)                         # the float32 weights again, not a rounded float64 copy
        ref.to(dt)
        res[dt] = {name: run(ref, dt, *bs[name], tokenizer) for name in bs}
    for name, (feats, lens) in bs.items():
        r64, r32 = res[torch.float64][name], res[torch.float32][name]
        out[f"{name}/feats"], out[f"{name}/lens"] = feats.numpy(), np.asarray(lens, np.int64)
        for k, a in r64.items():
            out[f"{name}/{k}"] = a
            if k in FLOATS:
                out[f"{name}/gap_{k}"] = np.float64(np.abs(np.asarray(a, np.float64) - np.asarray(r32[k], np.float64)).max())
            else:
                assert np.array_equal(a, r32[k]), (seed, name, k, a, r32[k])
        frac = np.abs(r64["token_num"] - np.floor(r64["token_num"]) - 0.5)
        assert float(frac.min()) >= 0.05, (seed, name, r64["token_num"])
        # token_num is B numbers, not thousands: its fp32 run can land within a fraction of an ulp of the fp64 one by chance, and 4 x such
        # a gap is a bar below the spacing of fp32 itself. A gap under half an ulp of the largest sum measures luck, not fp32.
        half_ulp = 0.5 * float(np.spacing(np.float32(np.abs(r64["token_num"]).max())))
        assert float(out[f"{name}/gap_token_num"]) >= half_ulp, (seed, name, "token_num gap below half an fp32 ulp", float(out[f"{name}/gap_token_num"]))
    for name, clips in (("s0", [0]), ("s1", [0]), ("b", [0, 1]), ("z", [0])):
        for c in clips:
            ids = [t for t in out[f"{name}/ids_{c}"].tolist() if t not in (0, 1, 2)]
            assert len(set(ids)) >= 5, (seed, name, c, ids)
    assert out["z/counts"].tolist()[1] == 0 and out["z/counts"].tolist()[0] > 0, (seed, out["z/counts"])
    n0 = int(out["s0/counts"][0])
    assert int(out["b/counts"][0]) == n0
    apart = float(np.abs(out["b/embeds"][0, :n0] - out["s0/embeds"][0, :n0]).max())
    assert apart > 100 * float(out["b/gap_embeds"]), (seed, apart, float(out["b/gap_embeds"]))
    # the rows of the reference's float32 positional table these clips read (legacy: the first T rows)
    pe = ref.float().encoder.embed.out[1].pe[0]
    out["pos_rows"] = pe[: out["b/enc"].shape[1]].numpy().astype(np.float32)
    print("seed", seed, "counts", {n: out[f"{n}/counts"].tolist() for n in bs}, "token_num", {n: out[f"{n}/token_num"].round(3).tolist() for n in bs},
          f"clip 0 batched vs alone {apart:.3e}", stats)
    for k in sorted(out):
        if "/gap_" in k:
            print("   ", k, f"{float(out[k]):.3e}")
    return out, {k: list(v.shape) for k, v in ref.state_dict().items()}


def main():
    import yaml

    from oracle import ref_import

    Ref, CharTokenizer = _reference()
    tokenizer = CharTokenizer(token_list=TOKENS, unk_symbol="<unk>", split_with_space=True)
    out = None
    for seed in SEEDS:
        try:
            out, tiny_shapes = attempt(seed, Ref, tokenizer)
            break
        except AssertionError as e:
            print("seed", seed, "fails:", str(e)[:300])
    assert out is not None, "no seed passed"
    out["tokens"] = np.asarray(TOKENS)
    path = os.path.join(ROOT, "tests", "golden", "eparaformer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000
    y = yaml.safe_load(open(os.path.join(ref_import.REF_ROOT, RECIPE)))
    big = Ref(encoder=y["encoder"], encoder_conf=y["encoder_conf"], decoder=y["decoder"], decoder_conf=y["decoder_conf"], predictor=y["predictor"],
              predictor_conf=y["predictor_conf"], vocab_size=4234, input_size=80, **y["model_conf"])
    with open(os.path.join(ROOT, "tests", "golden", "eparaformer_state_dict.json"), "w") as f:
        json.dump({"model": y["model"], "encoder": y["encoder"], "encoder_conf": y["encoder_conf"], "decoder": y["decoder"],
                   "decoder_conf": y["decoder_conf"], "predictor": y["predictor"], "predictor_conf": y["predictor_conf"],
                   "model_conf": y["model_conf"], "vocab_size": 4234, "shapes": {k: list(v.shape) for k, v in big.state_dict().items()},
                   "tiny_shapes": tiny_shapes}, f, indent=0)


if __name__ == "__main__":
    main()
