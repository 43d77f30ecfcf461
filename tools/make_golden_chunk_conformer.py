"""Writes tests/golden/chunk_conformer.npz and tests/golden/chunk_conformer_state_dict.json. The reference's own
`ConformerChunkEncoder` (funasr/models/conformer/encoder.py:914), imported read-only through oracle.ref_import, runs in float64 AND float32 on synthetic weights (funasr_amd.synth; never stored) at a tiny size: linear_units 128,
2 blocks, cnn_module_kernel 15, 80 features; D 64 with 1 head ("a") and D 128 with 2 heads ("b"). Per quantity the float64 value and
`gap_* = max |fp32 - fp64|` of the reference itself:
  feats_i                          clips of 7 / 19 / 39 / 67 / 87 frames
  {mode}_{i}_{stage}               size "a", default_chunk_size 4, left_chunk_size 1, time_reduction_factor 2, subsampling 4; mode full /
                                   dynamic / unified (the utt branch; its chunk branch is asserted equal to dynamic's: same weights);
                                   stage front / block_j / norm_blocks / out, kept by forward hooks. unified shares dynamic's front.
  front_f{2,6}_{whole,chunk}       size "b": the front alone on clip 3 (67 frames: no multiple of chunk * factor), chunk 4
  simu_out                         size "b", dynamic conf: simu_chunk_forward(clip 3, chunk_size 3)
  left0_out, leftall_out           size "b", dynamic conf with left_chunk_size 0 / -1 on clip 3
  batch_{mode}_{x,olens}           size "b": clips 4 and 2 as one zero-padded batch
  olens_f{factor}_r{r}, short_f{factor}  the reference's output lengths for T = 1 .. 48 (0 where it raises TooShortUttError) and
                                   whether it raises; lengths depend on neither weights nor size
  mask_c{c}_l{left}_n{n}           ~make_chunk_mask(n, c, left) (True: visible), n in 1, 5, 13, 20, c in 1, 3, 4, 16, left in -1, 0, 1, 2
  search_{mode}_c{i}_b{beam}_*     complete searches (nbest = beam) of the reference's Transducer + BeamSearchTransducer at beam 1, 2, 5 for
                                   the three longer clips in the dynamic and unified modes, each precision from its OWN encoder output:
                                   n, ids_r, scores, the counts by tests/_transducer_oracle.py; `search_names` lists what is recorded,
                                   `search_excluded` what is not and why. Conditions (a)-(d) and the seed probing (`--probe N`) are
                                   tools/make_golden_transducer.py's (gap_logp: the search networks' own float32 error on the float64 encoder rows); see REQUIRED_CLIPS below for (c)
The json holds the reference Transducer's state-dict shapes at D 512 / 8 heads / 12 blocks / linear_units 2048 / 4234 tokens and the settings used.
Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 14777
LENS = (7, 19, 39, 67, 87)
MODES = ("full", "dynamic", "unified")
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(57)] + ["<unk>"]
SIZE_A = dict(output_size=64, attention_heads=1)
SIZE_B = dict(output_size=128, attention_heads=2)
BIG = dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=12, cnn_module_kernel=15)


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.conformer.encoder as E
    import funasr.models.transducer.joint_network  # noqa: F401
    import funasr.models.transducer.rnnt_decoder  # noqa: F401
    from funasr.models.transducer.model import Transducer
    return E, Transducer


def features(seed: int):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, 80, generator=g) for n in LENS]


def stages(enc, call):
    """run `call()` on the reference encoder with forward hooks keeping what its modules pass along (the LAST call of each module:
    in unified mode the chunk branch runs second, so `call` selects the branch by what it keeps)"""
    kept = {"blocks": [[] for _ in enc.encoders.blocks], "norm_blocks": []}
    hooks = [enc.embed.register_forward_hook(lambda m, a, o: kept.__setitem__("front", o[0]))]
    for idx, b in enumerate(enc.encoders.blocks):
        hooks.append(b.register_forward_hook(lambda m, a, o, idx=idx: kept["blocks"][idx].append(o[0])))
    hooks.append(enc.encoders.norm_blocks.register_forward_hook(lambda m, a, o: kept["norm_blocks"].append(o)))
    try:
        out = call()
    finally:
        for h in hooks:
            h.remove()
    return kept, out


def encoder_of(E, seed, size, mode, **more):
    from funasr_amd import synth

    conf = synth.chunk_conformer_conf(mode=mode, **size, **more)
    enc = E.ConformerChunkEncoder(input_size=80, **conf).eval()
    sd = synth.conformer_state_dict(seed, enc)
    enc.load_state_dict(sd, strict=True)
    return enc, sd


def run_encoder(E, seed, dt, feats):
    """every encoder quantity of one precision, by the reference"""
    out = {}
    with torch.no_grad():
        finals = {}
        for mode in MODES:
            enc, sd = encoder_of(E, seed, SIZE_A, mode)
            enc = enc.to(dt)
            for i, f in enumerate(feats):
                kept, res = stages(enc, lambda: enc(f[None].to(dt), torch.tensor([f.shape[0]])))
                pick = 0                                             # unified: the utt branch is each module's FIRST call
                x, olens = (res[0], res[2]) if mode == "unified" else (res[0], res[1])
                assert int(olens[0]) == x.shape[1], (mode, i)
                if mode != "unified":
                    out[f"{mode}_{i}_front"] = kept["front"][0].numpy()
                for j, rows in enumerate(kept["blocks"]):
                    out[f"{mode}_{i}_block_{j}"] = rows[pick][0].numpy()
                out[f"{mode}_{i}_norm_blocks"] = kept["norm_blocks"][pick][0].numpy()
                out[f"{mode}_{i}_out"] = x[0].numpy()
                finals[(mode, i)] = res
            if mode == "unified":
                for i in range(len(feats)):                          # same weights (same shapes, same draw): the chunk branch IS dynamic's
                    assert torch.equal(finals[("unified", i)][1], finals[("dynamic", i)][0]), i
        f3 = feats[3][None].to(dt)
        for factor in (2, 6):
            enc, _ = encoder_of(E, seed, SIZE_B, "dynamic", subsampling_factor=factor)
            enc = enc.to(dt)
            mask = torch.zeros(1, f3.shape[1], dtype=torch.bool)
            out[f"front_f{factor}_whole"] = enc.embed(f3, mask, None)[0][0].numpy()
            out[f"front_f{factor}_chunk"] = enc.embed(f3, mask, 4)[0][0].numpy()
        enc, _ = encoder_of(E, seed, SIZE_B, "dynamic")
        enc = enc.to(dt)
        out["simu_out"] = enc.simu_chunk_forward(f3, torch.tensor([f3.shape[1]]), chunk_size=3)[0].numpy()
        for name, left in (("left0", 0), ("leftall", -1)):
            enc, _ = encoder_of(E, seed, SIZE_B, "dynamic", left_chunk_size=left)
            out[f"{name}_out"] = enc.to(dt)(f3, torch.tensor([f3.shape[1]]))[0][0].numpy()
        xb = torch.zeros(2, LENS[4], 80, dtype=dt)
        xb[0], xb[1, :LENS[2]] = feats[4].to(dt), feats[2].to(dt)
        for mode in MODES:
            enc, _ = encoder_of(E, seed, SIZE_B, mode)
            res = enc.to(dt)(xb, torch.tensor([LENS[4], LENS[2]]))
            out[f"batch_{mode}_x"] = res[0].numpy()
            out[f"batch_{mode}_olens"] = (res[2] if mode == "unified" else res[1]).numpy().astype(np.int64)
    return out


def tables(E):
    """lengths, too-short refusals and chunk masks: what the reference's own code gives"""
    from funasr.models.transformer.utils.nets_utils import make_chunk_mask
    from funasr.models.transformer.utils.subsampling import TooShortUttError

    t = {}
    for factor in (2, 4, 6):
        short = []
        for r in (1, 2, 3):
            enc = E.ConformerChunkEncoder(input_size=80, output_size=64, attention_heads=1, linear_units=32, num_blocks=1, cnn_module_kernel=3,
                                          subsampling_factor=factor, time_reduction_factor=r).eval()
            lens, raised = [], []
            for T in range(1, 49):
                try:
                    with torch.no_grad():
                        lens.append(int(enc(torch.zeros(1, T, 80), torch.tensor([T]))[1][0]))
                    raised.append(0)
                except TooShortUttError as err:
                    lens.append(0)
                    raised.append(int(err.limit))
            t[f"olens_f{factor}_r{r}"] = np.asarray(lens, np.int64)
            short.append(raised)
        assert short[0] == short[1] == short[2]
        t[f"short_f{factor}"] = np.asarray(short[0], np.int64)           # 0: runs; else the limit the error reports
    for c in (1, 3, 4, 16):
        for left in (-1, 0, 1, 2):
            for n in (1, 5, 13, 20):                                      # sizes inside a chunk and across several
                t[f"mask_c{c}_l{left}_n{n}"] = (~make_chunk_mask(n, c, left)).numpy()
    return t


SEARCH_CLIPS = (2, 3, 4)
BEAMS = (1, 2, 5)
SEARCH_MODES = ("dynamic", "unified")
PLANT = dict(n_planted=7, threshold=0.3)                          # few planted labels: the clips have 5, 9 and 11 encoder frames
# Condition (c) of tools/make_golden_transducer.py asks 3 <= tokens < frames of every 1-best. Clip 2 has 39 feature frames = 5 encoder
# frames at subsampling 4 and time_reduction_factor 2, which leaves 3 or 4 tokens in both modes at once: of 54 seeds probed at
# threshold 0.8 none met it. A seed must therefore meet (c) on clips 3 and 4; clip 2's searches are recorded where IT meets (c) in a
# mode too, and left out (with the reason printed and kept in `search_excluded`) where it does not. (a), (b), (d) hold for every
# recorded search.
REQUIRED_CLIPS = (3, 4)
PREFIXES = ([0], [0, 5], [0, 60, 1, 17], [0, 30, 31, 32, 33, 34])
PAIRS = ((0, 0), (2, 1), (4, 2), (6, 3))                         # (frame of clip 3, index into PREFIXES): where gap_logp is taken


def transducer_of(Ref, seed, mode):
    from funasr_amd import synth

    conf = synth.transducer_conf(encoder="ChunkConformerEncoder", vocab=len(TOKENS), linear_units=128, **SIZE_A)
    conf["encoder_conf"] = synth.chunk_conformer_conf(mode=mode, **SIZE_A)
    ref = Ref(**conf)
    sd = synth.transducer_state_dict(seed, ref, **PLANT)
    ref.load_state_dict(sd, strict=True)
    return ref.eval(), sd


def run_search(Ref, Search, seed, dt, feats, logp_from=None):
    """every search of one precision by the reference, each from its OWN encoder output. `logp_from`: the results of another run whose
    encoder rows (cast to dt) feed the joint log-probabilities of PAIRS -- the float32 run takes the float64 run's, so that gap_logp
    is the search networks' own float32 error, as tools/make_golden_transducer.py defines it; the encoder's float32 error is what
    condition (a) and the stages' gaps cover"""
    models = {mode: transducer_of(Ref, seed, mode)[0] for mode in SEARCH_MODES}      # drawn under the float32 default
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dt)                                      # RNNTDecoder.init_state builds default-dtype zeros
    out = {}
    try:
        with torch.no_grad():
            for mode in SEARCH_MODES:
                m = models[mode].to(dt)
                for i in SEARCH_CLIPS:
                    e, _ = m.encode(feats[i][None].to(dt), torch.tensor([feats[i].shape[0]]))
                    out[f"senc_{mode}_{i}"] = e[0].numpy()
                    if i == 3:                                       # joint log-probabilities of a few (frame, prefix) pairs, for gap_logp
                        for n, (t, j) in enumerate(PAIRS):
                            state = m.decoder.init_state(1)
                            for lab in PREFIXES[j]:
                                d, state = m.decoder.rnn_forward(m.decoder.embed(torch.full((1, 1), lab, dtype=torch.long)), state)
                            rows = e[0] if logp_from is None else torch.from_numpy(logp_from[f"senc_{mode}_{i}"]).to(dt)
                            out[f"logp_{mode}_{n}"] = torch.log_softmax(m.joint_network(rows[t: t + 1], d[0]), dim=-1)[0].numpy()
                    for beam in BEAMS:
                        name = f"{mode}_c{i}_b{beam}"
                        hyps = Search(m.decoder, m.joint_network, beam, nbest=beam)(e[0], is_final=True)
                        out[f"search_{name}_n"] = np.int64(len(hyps))
                        out[f"search_{name}_scores"] = np.asarray([float(h.score) for h in hyps], np.float64)
                        for r, h in enumerate(hyps):
                            out[f"search_{name}_ids_{r}"] = np.asarray([int(v) for v in h.yseq], np.int64)
    finally:
        torch.set_default_dtype(prev)
    return out


def build_searches(seed: int, feats):
    """-> (npz entries, None) or (None, why the seed fails)"""
    from funasr.models.transducer.beam_search_transducer import BeamSearchTransducer as Search
    from tests import _transducer_oracle as TO

    _, Ref = _reference()
    for mode in SEARCH_MODES:                                        # the cheap part of (c) and (d) first: beam 1 by the oracle alone
        m, sd = transducer_of(Ref, seed, mode)
        sd64 = TO.cast(sd, torch.float64)
        m = m.double()
        with torch.no_grad():
            for i in REQUIRED_CLIPS:
                e, _ = m.encode(feats[i][None].double(), torch.tensor([feats[i].shape[0]]))
                res = TO.search(sd64, e[0], 1, nbest=1, margins=True)
                n_tok = len([v for v in res["ids"][0] if v != 0])
                if not 3 <= n_tok < e.shape[1]:
                    return None, f"(c) {mode}_c{i}_b1: the 1-best has {n_tok} tokens over {e.shape[1]} frames"
                if res["max_frame_evals"] > 16:
                    return None, f"(d) {mode}_c{i}_b1: {res['max_frame_evals']} evaluations in one frame, a quarter of the cap is 16"
    s64 = run_search(Ref, Search, seed, torch.float64, feats)
    s32 = run_search(Ref, Search, seed, torch.float32, feats, logp_from=s64)
    out, names, excluded = {}, [], []
    gap_logp = max(float(np.abs(v.astype(np.float64) - s32[k].astype(np.float64)).max()) for k, v in s64.items() if k.startswith("logp_"))
    gap_score, min_margin = 0.0, float("inf")
    for mode in SEARCH_MODES:
        _, sd = transducer_of(Ref, seed, mode)
        sd64 = TO.cast(sd, torch.float64)
        for i in SEARCH_CLIPS:
            x = torch.from_numpy(s64[f"senc_{mode}_{i}"])
            rec, why = {}, None
            for beam in BEAMS:
                name = f"{mode}_c{i}_b{beam}"
                n = int(s64[f"search_{name}_n"])
                keys = [f"search_{name}_n", f"search_{name}_scores"] + [f"search_{name}_ids_{r}" for r in range(n)]
                ref_ids = [s64[f"search_{name}_ids_{r}"].tolist() for r in range(n)]
                n_tok = len([v for v in ref_ids[0] if v != 0])
                if not 3 <= n_tok < x.shape[0]:
                    why = f"(c) {name}: the 1-best has {n_tok} tokens over {x.shape[0]} frames"
                    break
                if any(k not in s32 or not np.array_equal(s64[k], s32[k]) for k in keys if not k.endswith("_scores")):
                    return None, f"(a) {name}: float64 {ref_ids} differs from float32"
                res = TO.search(sd64, x, beam, nbest=beam, margins=True)
                assert res["ids"] == ref_ids, (name, res["ids"], ref_ids)
                assert np.allclose(res["scores"], s64[f"search_{name}_scores"], rtol=0, atol=1e-9), name
                if res["max_frame_evals"] > 64 * beam // 4:
                    return None, f"(d) {name}: {res['max_frame_evals']} evaluations in one frame, a quarter of the cap is {64 * beam // 4}"
                for k in keys:
                    rec[k] = s64[k]
                for c in ("joint_evals", "pred_steps", "max_frame_evals"):
                    rec[f"search_{name}_{c}"] = np.int64(res[c])
                rec["#gap"] = max(rec.get("#gap", 0.0), float(np.abs(s64[f"search_{name}_scores"] - s32[f"search_{name}_scores"]).max()))
                rec["#margin"] = min(rec.get("#margin", float("inf")), res["min_margin"])
            if why is not None:
                if i in REQUIRED_CLIPS:
                    return None, why
                excluded.append(why)
                continue
            gap_score, min_margin = max(gap_score, rec.pop("#gap")), min(min_margin, rec.pop("#margin"))
            out.update(rec)
            names += [f"{mode}_c{i}_b{beam}" for beam in BEAMS]
    if min_margin < 1000 * gap_logp:
        return None, f"(b) min_margin {min_margin:.3e} < 1000 x gap_logp {gap_logp:.3e}"
    out.update({"gap_logp": np.float64(gap_logp), "gap_score": np.float64(gap_score), "min_margin": np.float64(min_margin), "search_names": np.asarray(names),
                "search_excluded": np.asarray(excluded if excluded else ["none"]), "n_planted": np.int64(PLANT["n_planted"]),
                "threshold": np.float64(PLANT["threshold"])})
    return out, None


def build(seed: int, searches_only: bool = False):
    """-> (npz contents, None) or (None, why the seed fails)"""
    E, _ = _reference()
    feats = features(seed)
    out = {"seed": np.int64(seed), "lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS)}
    found, why = build_searches(seed, feats)
    if found is None or searches_only:
        return found, why
    out.update(found)
    for i, f in enumerate(feats):
        out[f"feats_{i}"] = f.numpy()
    e64, e32 = run_encoder(E, seed, torch.float64, feats), run_encoder(E, seed, torch.float32, feats)
    for k, v in e64.items():
        if k.endswith("_olens"):
            assert np.array_equal(v, e32[k]), k
            out[k] = v
            continue
        if not np.isfinite(v).all():
            return None, f"{k} is not finite"
        out[k] = v
        out["gap_" + k] = np.float64(np.abs(v.astype(np.float64) - e32[k].astype(np.float64)).max())
    out.update(tables(E))
    return out, None


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--probe":               # --probe N [START]: the first seed that meets the conditions
        start = int(sys.argv[3]) if len(sys.argv) > 3 else SEED
        for seed in range(start, start + int(sys.argv[2])):
            found, why = build(seed, searches_only=True)
            print(seed, "ok: " + " ".join(found["search_names"].tolist()) + " | excluded: " + "; ".join(found["search_excluded"].tolist())
                  if found is not None else why, flush=True)
            if found is not None:
                break
        return
    out, why = build(SEED)
    assert out is not None, f"seed {SEED} fails condition {why}: pick another (--probe N)"
    path = os.path.join(ROOT, "tests", "golden", "chunk_conformer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; min_margin", float(out["min_margin"]), "gap_score", float(out["gap_score"]))
    print("    searches:", " ".join(out["search_names"].tolist()))
    print("    excluded:", "; ".join(out["search_excluded"].tolist()))
    for k in sorted(out):
        if k.startswith("gap_"):
            print("   ", k, f"{float(out[k]):.3e}")
    from funasr_amd import synth
    _, Ref = _reference()
    conf = synth.transducer_conf(encoder="ChunkConformerEncoder", **synth.TRANSDUCER_TEMPLATE)
    conf["encoder_conf"] = synth.chunk_conformer_conf(mode="unified", default_chunk_size=16, left_chunk_size=4, **BIG)
    big = Ref(**conf)
    tiny = {m: synth.chunk_conformer_conf(mode=m, **SIZE_A) for m in MODES}
    with open(os.path.join(ROOT, "tests", "golden", "chunk_conformer_state_dict.json"), "w") as f:
        json.dump({"conf": conf, "tiny_encoder_conf": tiny, "size_a": SIZE_A, "size_b": SIZE_B, "plant": PLANT,
                   "shapes": {k: list(v.shape) for k, v in big.state_dict().items()}}, f, indent=0)


if __name__ == "__main__":
    main()
