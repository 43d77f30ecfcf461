"""Writes tests/golden/rwkv.npz and tests/golden/rwkv_state_dict.json. The reference's own `RWKVEncoder` and `Transducer`
(funasr/models/rwkv_bat/rwkv_encoder.py, funasr/models/transducer/model.py with BeamSearchTransducer, imported read-only through
oracle.ref_import) run ONE CLIP PER CALL -- the reference's rwkv_infer handles no other batch -- in float64 AND float32 on synthetic
weights (funasr_amd.synth.transducer_state_dict with the RWKV drawing rule; weights are never stored) at a tiny configuration:
RWKVEncoder D 64 / linear_size 160 / 3 blocks / time_reduction_factor 2, 80 features, and the prediction / joint sizes of
tools/make_golden_transducer.py (61 tokens, embed 48, hidden 64, 2 LSTM layers, joint 96). Per quantity the float64 result and
`gap_* = max |fp32 - fp64|` of the reference itself:
  feats_i                       five clips of 1 / 5 / 39 / 55 / 87 frames
  front_i, embed_norm_i         the front's output and embed_norm's [T2, D]
  block_i_j                     block j's output, collected from the reference's own frame-by-frame walk
  enc_i                         the encoder output [olens, D] (asserted equal to what `model.encode` returns)
  gap_logp                      over the joint log-probabilities of the (clip 3 frame, prefix) pairs PAIRS, each precision from its OWN
                                encoder output (the values themselves are not stored: the searches cover them)
  search_c{i}_b{beam}_*         for the three longer clips the complete searches (nbest = beam) at beam 1, 2, 5, each precision from
                                its OWN encoder output: ids_r, scores, and the counts by tests/_transducer_oracle.py
  olens_r{r}                    the reference's output lengths for T = 1 .. 40 at time_reduction_factor r = 1, 2, 3
  gap_logp, gap_score, min_margin
Conditions (a)-(d) are those of tools/make_golden_transducer.py, enforced by seed probing (`--probe N`); the only change is that
gap_logp includes the encoder's float32 error.
The json holds the reference's state-dict shapes at funasr/models/rwkv_bat/template.yaml (D 512, 18 blocks) with 4234 tokens, and
under "template" every setting of that yaml (what the AutoModel test writes as a model directory's config.yaml).
Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _transducer_oracle as TO  # noqa: E402

SEED = 12019
LENS = (1, 5, 39, 55, 87)
SEARCH_CLIPS = (2, 3, 4)
BEAMS = (1, 2, 5)
PREFIXES = ([0], [0, 5], [0, 60, 1, 17], [0, 30, 31, 32, 33, 34])
PAIRS = ((0, 0), (2, 1), (4, 2), (6, 3))                         # (frame of clip 3, index into PREFIXES)
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(57)] + ["<unk>"]
TINY = dict(encoder="RWKVEncoder", output_size=64, linear_units=160, enc_blocks=3)
PLANT = dict(n_planted=7, threshold=0.8)                          # few planted labels: the clips have 5, 7 and 11 encoder frames


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.rwkv_bat.rwkv_encoder  # noqa: F401  (registers RWKVEncoder)
    import funasr.models.transducer.joint_network  # noqa: F401
    import funasr.models.transducer.rnnt_decoder  # noqa: F401
    from funasr.models.transducer.beam_search_transducer import BeamSearchTransducer
    from funasr.models.transducer.model import Transducer
    return Transducer, BeamSearchTransducer


def features(seed: int):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, 80, generator=g) for n in LENS]


def stages(enc, x):
    """the reference encoder's own forward on one clip x [1, T, F], with forward hooks keeping what its modules pass along:
    (front [T2, D], embed_norm [T2, D], [block outputs [T2, D]], out [olens, D]).
    One thing is changed around the call: the reference allocates its recurrent state with dtype=torch.float32 whatever the module's
    dtype, which would round every frame's state of the float64 run to float32; while it runs, an explicit float32 request to
    torch.zeros is served in the clip's dtype. The float32 run is therefore the reference untouched."""
    kept = {"blocks": [[] for _ in enc.rwkv_blocks]}
    hooks = [enc.embed.register_forward_hook(lambda m, a, o: kept.__setitem__("front", o[0])),
             enc.embed_norm.register_forward_hook(lambda m, a, o: kept.__setitem__("embed_norm", o))]
    for idx, block in enumerate(enc.rwkv_blocks):
        hooks.append(block.register_forward_hook(lambda m, a, o, idx=idx: kept["blocks"][idx].append(o[0])))
    zeros = torch.zeros

    def zeros_in_run_dtype(*a, **k):
        if k.get("dtype") is torch.float32:
            k["dtype"] = x.dtype
        return zeros(*a, **k)

    torch.zeros = zeros_in_run_dtype
    try:
        out, olens, _ = enc(x, torch.tensor([x.shape[1]]))
    finally:
        torch.zeros = zeros
        for h in hooks:
            h.remove()
    assert int(olens[0]) == out.shape[1]
    return kept["front"][0], kept["embed_norm"][0], [torch.cat(rows, dim=1)[0] for rows in kept["blocks"]], out[0]


def searches(enc):
    """(name, encoder rows, beam) of every recorded search"""
    return [(f"c{i}_b{b}", enc[i], b) for i in SEARCH_CLIPS for b in BEAMS]


def run(model, Search, dt, feats):
    """every stored quantity of one precision, by the reference"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dt)                                      # RNNTDecoder.init_state builds default-dtype zeros
    try:
        m = model.to(dt)
        out = {}
        with torch.no_grad():
            enc = {}
            for i, f in enumerate(feats):
                front, en, blocks, o = stages(m.encoder, f[None].to(dt))
                e, el = m.encode(f[None].to(dt), torch.tensor([f.shape[0]]))
                assert int(el[0]) == o.shape[0] and e[0].shape == o.shape, (i, e.shape, o.shape)
                if dt == torch.float32:
                    assert torch.equal(e[0], o), i
                elif torch.isfinite(o).all():                        # (its float32 state leaves `encode` at float32 accuracy)
                    assert float((e[0] - o).abs().max()) < 1e-3, i
                out[f"front_{i}"], out[f"embed_norm_{i}"], out[f"enc_{i}"] = front.numpy(), en.numpy(), o.numpy()
                for j, b in enumerate(blocks):
                    out[f"block_{i}_{j}"] = b.numpy()
                enc[i] = o
            dec_outs = []
            for pre in PREFIXES:
                state = m.decoder.init_state(1)
                for lab in pre:
                    d, state = m.decoder.rnn_forward(m.decoder.embed(torch.full((1, 1), lab, dtype=torch.long)), state)
                dec_outs.append(d[0])
            for n, (t, j) in enumerate(PAIRS):
                out[f"logp_{n}"] = torch.log_softmax(m.joint_network(enc[3][t: t + 1], dec_outs[j]), dim=-1)[0].numpy()
            for name, x, beam in searches(enc):
                bs = Search(m.decoder, m.joint_network, beam, nbest=beam)
                hyps = bs(x, is_final=True)
                out[f"search_{name}_n"] = np.int64(len(hyps))
                out[f"search_{name}_scores"] = np.asarray([float(h.score) for h in hyps], np.float64)
                for r, h in enumerate(hyps):
                    out[f"search_{name}_ids_{r}"] = np.asarray([int(v) for v in h.yseq], np.int64)
    finally:
        torch.set_default_dtype(prev)
    return out


def length_table(Ref):
    """the reference encoder's olens for T = 1 .. 40 at r = 1, 2, 3 (a small encoder: lengths do not depend on the weights)"""
    import funasr.models.rwkv_bat.rwkv_encoder as R

    table = {}
    for r in (1, 2, 3):
        enc = R.RWKVEncoder(input_size=8, output_size=32, linear_size=32, num_blocks=2, time_reduction_factor=r).eval()
        with torch.no_grad():
            table[f"olens_r{r}"] = np.asarray([int(enc(torch.zeros(1, T, 8), torch.tensor([T]))[1][0]) for T in range(1, 41)], np.int64)
    return table


def build(seed: int):
    """-> (npz contents, None) or (None, why the seed fails)"""
    from funasr_amd import synth

    Ref, Search = _reference()
    feats = features(seed)
    conf = synth.transducer_conf(vocab=len(TOKENS), **TINY)
    ref = Ref(**conf)
    sd = synth.transducer_state_dict(seed, ref, **PLANT)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    r64 = run(ref, Search, torch.float64, feats)
    ref.load_state_dict(sd, strict=True)                             # the float32 weights again, not the rounded float64 copy
    r32 = run(ref, Search, torch.float32, feats)
    out = {"seed": np.int64(seed), "lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS), "beams": np.asarray(BEAMS, np.int64),
           "search_clips": np.asarray(SEARCH_CLIPS, np.int64), "pairs": np.asarray(PAIRS, np.int64),
           "n_planted": np.int64(PLANT["n_planted"]), "threshold": np.float64(PLANT["threshold"])}
    for i, f in enumerate(feats):
        out[f"feats_{i}"] = f.numpy()
    gap_logp, gap_score = 0.0, 0.0
    for k, v in r64.items():
        if "_ids_" in k or k.endswith("_n"):
            out[k] = v
            if not np.array_equal(v, r32[k]):
                return None, f"(a) {k}: float64 {np.asarray(v).tolist()} float32 {np.asarray(r32[k]).tolist()}"
            continue
        if not np.isfinite(np.asarray(v)).all():
            return None, f"{k} is not finite"
        gap = float(np.abs(np.asarray(v, np.float64) - np.asarray(r32[k], np.float64)).max())
        if k.endswith("_scores"):
            out[k] = v
            gap_score = max(gap_score, gap)
        elif k.startswith("logp_"):
            gap_logp = max(gap_logp, gap)                            # (the values themselves are not stored: the searches cover them)
        else:
            out[k] = v
            out["gap_" + k] = np.float64(gap)
    out["gap_logp"], out["gap_score"] = np.float64(gap_logp), np.float64(gap_score)
    sd64 = TO.cast(sd, torch.float64)
    min_margin = float("inf")
    enc = {i: torch.from_numpy(r64[f"enc_{i}"]) for i in SEARCH_CLIPS}
    for name, x, beam in searches(enc):
        res = TO.search(sd64, x, beam, nbest=beam, margins=True)
        ref_ids = [r64[f"search_{name}_ids_{r}"].tolist() for r in range(int(r64[f"search_{name}_n"]))]
        assert res["ids"] == ref_ids, (name, res["ids"], ref_ids)
        assert np.allclose(res["scores"], r64[f"search_{name}_scores"], rtol=0, atol=1e-9), name
        for c in ("joint_evals", "pred_steps", "max_frame_evals"):
            out[f"search_{name}_{c}"] = np.int64(res[c])
        min_margin = min(min_margin, res["min_margin"])
        n_tok = len([v for v in ref_ids[0] if v != 0])
        if not 3 <= n_tok < x.shape[0]:
            return None, f"(c) {name}: the 1-best has {n_tok} tokens over {x.shape[0]} frames"
        if res["max_frame_evals"] > 64 * beam // 4:
            return None, f"(d) {name}: {res['max_frame_evals']} evaluations in one frame, a quarter of the cap is {64 * beam // 4}"
    out["min_margin"] = np.float64(min_margin)
    if min_margin < 1000 * gap_logp:
        return None, f"(b) min_margin {min_margin:.3e} < 1000 x gap_logp {gap_logp:.3e}"
    out.update(length_table(Ref))
    return out, None


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--probe":
        for seed in range(SEED, SEED + int(sys.argv[2])):
            out, why = build(seed)
            print(seed, "ok" if out is not None else why, flush=True)
        return
    out, why = build(SEED)
    assert out is not None, f"seed {SEED} fails condition {why}: pick another"
    path = os.path.join(ROOT, "tests", "golden", "rwkv.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; frames", [out[f"enc_{i}"].shape[0] for i in range(len(LENS))], "min_margin", float(out["min_margin"]))
    for name, _, beam in searches({i: out[f"enc_{i}"] for i in SEARCH_CLIPS}):
        print("   ", name, "1-best", out[f"search_{name}_ids_0"].tolist(), "evals", int(out[f"search_{name}_joint_evals"]))
    for k in sorted(out):
        if k.startswith("gap_"):
            print("   ", k, f"{float(out[k]):.3e}")
    import yaml
    from oracle import ref_import
    Ref, _ = _reference()
    tmpl = yaml.safe_load(open(os.path.join(ref_import.REF_ROOT, "funasr", "models", "rwkv_bat", "template.yaml")))
    big = Ref(encoder=tmpl["encoder"], encoder_conf=tmpl["encoder_conf"], decoder=tmpl["decoder"], decoder_conf=tmpl["decoder_conf"],
              joint_network=tmpl["joint_network"], joint_network_conf=tmpl["joint_network_conf"], vocab_size=4234, input_size=80,
              **tmpl["model_conf"])
    with open(os.path.join(ROOT, "tests", "golden", "rwkv_state_dict.json"), "w") as f:
        json.dump({"encoder": tmpl["encoder"], "encoder_conf": tmpl["encoder_conf"], "decoder_conf": tmpl["decoder_conf"],
                   "joint_network_conf": tmpl["joint_network_conf"], "model_conf": tmpl["model_conf"], "vocab_size": 4234,
                   "template": tmpl, "shapes": {k: list(v.shape) for k, v in big.state_dict().items()}}, f, indent=0)


if __name__ == "__main__":
    main()
