"""Writes tests/golden/kws.npz and tests/golden/kws.json. The reference's own `FsmnKWS`, `SanmKWS` and `KwsCtcPrefixDecoder`
(funasr/models/fsmn_kws/model.py, sanm_kws/model.py, utils/kws_utils.py, imported read-only through oracle.ref_import) run in
float64 AND float32 on synthetic planted weights (funasr_amd.synth.kws_state_dict; weights are never stored) at tiny configurations:
  fsmn    40 features, affine 24, 2 layers, linear 32, proj 16, lorder 4, rorder 2, strides 1, 67 tokens, no ctc_lo
  fsmn2   the same with lstride = rstride = 2
  sanm    SANMEncoder D 128 / 2 heads / 2 blocks / ffn 64, 40 features, ctc_lo to 67 tokens
Per model a ragged zero-padded batch of four clips (LENS frames), decoded as a batch and -- the FSMN gets no lengths, so the two
differ -- for the two FSMN models each clip alone:
  {m}_feats                    [B, T, 40] the zero-padded batch (keywords `model_keywords`: two of two tokens; the search-only clips
                               below use `keywords`, one of three tokens and one of two)
  {m}_logits, {m}_alone{i}_logits     float64 logits of the batch / of clip i alone; gap_* = max |fp32 - fp64| of the reference itself
  {m}_cand, {m}_alone{i}_cand  per-frame candidates [.., 7] = n, ids[3], probs[3] (float64 columns)
  {m}_c{i}_* / {m}_alone{i}_*  per clip: the n-best in final order (prefixes padded with -1, scores, per node token / frame / prob),
                               hit (keyword index or -1), offset, score
Search-only clips `search{j}`: logits of our own making (log of a hand-written posterior) that the reference's softmax, beam_search
and _decode_inside are run on; they carry the coverage of condition (c). gap_prob, gap_score, gap_logits_{m}, margins.
Conditions enforced here -- every model has a seed of its own; a seed that misses a condition fails, pick another (`--probe N` lists how the next N seeds of each model fare):
  (a) the float32 and float64 runs agree on every kept candidate set, every final hypothesis list in order (prefixes, node tokens
      and frames) and every verdict;
  (b) every decision has a margin of at least 1000 x the matching gap: p against 0.05 (gap_prob), third against fourth logit where
      the third is above 0.05 (gap_logits), ps against the node's prob (gap_prob), and -- relative to the larger of the two, path
      scores span many decades -- neighbours in each prune and pb / pnb against 1e-6 (gap_path_rel = the largest relative fp32
      error of a path score). Exact ties and exact zeros are excepted: they are the same in every precision;
  (c) coverage across the clips: a hit at offset 0; a hit of the SECOND keyword at offset > 0 inside a longer prefix; a rejection
      with non-empty hypotheses; a clip without any kept candidate; more than 20 hypotheses before a prune; a hypothesis that takes
      both `s == last` sub-branches; a non-keyword token in the top 3 that leaves a keyword token above 0.05 at rank 4; a clip on
      which the deep-copy variant of tests/_kws_oracle.py returns another hit score or node frame; and in every model's batch at
      least one detection, in the FSMN batches also a rejection (clips are scaled by AMPS: the last one is near silence; the SAN-M
      encoder's LayerNorm undoes the scale);
  (d) the repository's restatement (tests/_kws_oracle.py, float64) reproduces the reference's hypotheses and verdicts exactly.
The json holds the tiny models' settings (MODELS, PLANTED: what the tests rebuild the weights from), the reference's state-dict shapes for the two recipe yamls (fsmn_4e_l10r2_250_128_fdim80_t2599,
sanm_6e_320_256_fdim40_t2602) and the outputs of the reference's split_mixed_label / query_token_set for keyword strings of our own.
Build container only (needs the reference tree)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _kws_oracle as KO  # noqa: E402

SEEDS = {"fsmn": 25, "fsmn2": 25, "sanm": 62}             # one per model, each passing its own conditions (--probe)
LENS = (20, 28, 45, 22)
AMPS = (1.0, 1.0, 1.0, 0.02)                          # per-clip feature scale: the last clip is near silence (for the FSMN: a rejection)
TOKENS = ["<blank>", "<s>", "</s>"] + [chr(0x4E00 + 7 * i) for i in range(57)] + ["hello", "ni", "hao", "a", "b", "sil", "<unk>"]
KW1, KW2 = (5, 9, 13), (21, 30)
KEYWORDS = "".join(TOKENS[i] for i in KW1) + ", " + "".join(TOKENS[i] for i in KW2)
MODEL_KW = ((5, 9), (21,))                            # the networks' keywords: short, so that random planted weights hit some
MODEL_KEYWORDS = ",".join("".join(TOKENS[i] for i in kw) for kw in MODEL_KW)
PLANTED = MODEL_KW[0] + MODEL_KW[1] + (30,)            # (30: a planted token outside the keyword set)
MODELS = {"fsmn": dict(kind="fsmn", conf={}, plant=dict(blank=8.0, gain=8.0)),
          "fsmn2": dict(kind="fsmn", conf=dict(lstride=2, rstride=2), plant=dict(blank=8.0, gain=8.0)),
          "sanm": dict(kind="sanm", conf={}, plant=dict(blank=11.0, gain=4.5))}
PARSE_SEG_DICT = {"world": "a b", "云": TOKENS[7]}
PARSE_STRINGS = [TOKENS[5] + TOKENS[9], "hello" + TOKENS[5], "HELLO ni hao", "!sil" + TOKENS[9], "<blank>" + TOKENS[4], "(noise)a",
                 "xyz" + TOKENS[6], "world", "云" + TOKENS[8], "a?b", TOKENS[5] + "，" + TOKENS[9], "hello", "<sil>b", "q"]
NOKW = 40                                             # a token outside the keyword set


def _reference():
    from oracle import ref_import

    ref_import.install()
    import funasr.models.fsmn_vad_streaming.encoder  # noqa: F401  (registers FSMN)
    import funasr.models.sanm.encoder  # noqa: F401  (registers SANMEncoder)
    from funasr.models.fsmn_kws.model import FsmnKWS
    from funasr.models.sanm_kws.model import SanmKWS
    from funasr.utils import kws_utils
    return FsmnKWS, SanmKWS, kws_utils


def posterior_logits(frames):
    """hand-written posteriors -> float64 logits [T, V]: each frame names some tokens' probabilities, the rest of the mass goes to
    the other tokens in slightly unequal shares"""
    V = len(TOKENS)
    out = torch.zeros(len(frames), V, dtype=torch.float64)
    for t, named in enumerate(frames):
        rest = [v for v in range(V) if v not in named]
        w = torch.tensor([1.0 + 0.01 * ((7 * v + 3 * t) % 11) for v in rest], dtype=torch.float64)
        p = torch.zeros(V, dtype=torch.float64)
        p[rest] = (1.0 - sum(named.values())) * w / w.sum()
        for v, q in named.items():
            p[v] = q
        out[t] = p.log()
    return out


def search_clips():
    a, b, c = KW1
    d, e = KW2
    quiet = {0: 0.93}
    return [
        # 0: a hit of the first keyword at offset 0
        [quiet, {a: 0.81, 0: 0.12}, {a: 0.62, 0: 0.31}, {0: 0.9}, {b: 0.71, 0: 0.2}, {c: 0.88, 0: 0.07}, {0: 0.91}],
        # 1: the second keyword at offset 1 inside a longer prefix
        [{a: 0.72, 0: 0.2}, {0: 0.92}, {d: 0.83, 0: 0.1}, {e: 0.76, 0: 0.15}, {0: 0.89}, {b: 0.63, 0: 0.3}],
        # 2: a rejection with hypotheses
        [{b: 0.61, 0: 0.3}, {0: 0.9}, {a: 0.52, 0: 0.4}],
        # 3: no kept candidate at all: a token outside the set takes every frame
        [{NOKW: 0.9}, {NOKW: 0.88}, {NOKW: 0.91}, {NOKW + 1: 0.86}],
        # 4: three keyword tokens a frame: 27 hypotheses before the third prune and more after
        [{a: 0.413, b: 0.307, c: 0.197}, {d: 0.389, e: 0.303, a: 0.219}, {b: 0.421, c: 0.293, d: 0.207}, {e: 0.377, a: 0.323, b: 0.191},
         {c: 0.403, d: 0.277, 0: 0.231}],
        # 5: the same token three frames running beside blank: the third frame takes both s == last sub-branches
        [{a: 0.5, 0: 0.4}, {a: 0.46, 0: 0.42}, {a: 0.44, 0: 0.41}, {b: 0.7, 0: 0.2}, {c: 0.66, 0: 0.25}],
        # 6: a token outside the set at rank 2 leaves keyword token b (0.1) at rank 4
        [{0: 0.4, NOKW: 0.3, a: 0.15, b: 0.1}, {b: 0.6, 0: 0.3}, {c: 0.7, 0: 0.2}],
        # 7: node sharing: frame 2 raises the first node of prefix (a) -- and with it the first node of (a, b), which a deep copy misses
        [{a: 0.5, 0: 0.4}, {b: 0.41, a: 0.3, 0: 0.24}, {a: 0.8, 0: 0.15}, {c: 0.6, 0: 0.33}],
    ]


def pack_nbest(hyps):
    H = len(hyps)
    L = max([len(h[0]) for h in hyps] + [1])
    pre = np.full((H, L), -1, np.int64)
    tok, frm = np.full((H, L), -1, np.int64), np.full((H, L), -1, np.int64)
    prob = np.zeros((H, L), np.float64)
    for j, (prefix, _, nodes) in enumerate(hyps):
        assert len(prefix) == len(nodes)
        pre[j, : len(prefix)] = prefix
        for k, nd in enumerate(nodes):
            tok[j, k], frm[j, k], prob[j, k] = nd["token"], nd["frame"], nd["prob"]
    return {"nbest_len": np.asarray([len(h[0]) for h in hyps], np.int64), "nbest_prefix": pre,
            "nbest_score": np.asarray([h[1] for h in hyps], np.float64), "node_token": tok, "node_frame": frm, "node_prob": prob}


def decode_clip(dec, logits, dt):
    """the reference on the logits [T, V] of one clip, in dtype dt -> (probs, hyps, verdict)"""
    import torch.nn.functional as F
    probs = F.softmax(logits.to(dt)[None], dim=2)[0]
    hyps = dec.beam_search(probs, None, dec.keywords_idxset)
    hit = dec._decode_inside(probs, torch.tensor([probs.shape[0]]))
    return probs, hyps, hit


def record_clip(out, name, dec, logits64, state):
    """runs one clip in both precisions, checks (a), (b), (d), stores under `name`; returns why it fails or None"""
    keywords = [dec.keywords_token[k]["token_id"] for k in dec.keywords_token]
    names = list(dec.keywords_token)
    p64, h64, v64 = decode_clip(dec, logits64, torch.float64)
    p32, h32, v32 = decode_clip(dec, logits64.to(torch.float32), torch.float32)   # (the fp32 run reads the fp32 logits of ITS network: see build)
    n64, i64, c64, mp, mx = KO.candidates(logits64, dec.keywords_idxset, margins=True)
    n32, i32, c32 = KO.candidates(logits64.to(torch.float32), dec.keywords_idxset)
    if not (torch.equal(n64, n32) and torch.equal(i64, i32)):
        return f"(a) {name}: candidate sets differ"
    # candidates by the reference's own rule (softmax, topk(3)) agree with the restatement's
    for t in range(p64.shape[0]):
        tp, ti = p64[t].topk(3)
        kept = [int(i) for p, i in zip(tp.tolist(), ti.tolist()) if p > 0.05 and i in dec.keywords_idxset]
        if kept != [int(v) for v in i64[t, : int(n64[t])]]:
            return f"(d) {name}: frame {t}: reference keeps {kept}, restatement {i64[t].tolist()}"
    state["gap_prob"] = max(state["gap_prob"], float((c64 - c32.double()).abs().max()) if len(n64) else 0.0)
    if [(h[0], [(nd["token"], nd["frame"]) for nd in h[2]]) for h in h64] != [(h[0], [(nd["token"], nd["frame"]) for nd in h[2]]) for h in h32]:
        return f"(a) {name}: hypothesis lists differ"
    if v64[:2] != v32[:2]:
        return f"(a) {name}: verdicts differ {v64} {v32}"
    state["gap_path_rel"] = max([state["gap_path_rel"]] + [abs(a[1] - b[1]) / abs(a[1]) for a, b in zip(h64, h32) if a[1] != 0.0])
    if v64[0]:
        state["gap_score"] = max(state["gap_score"], abs(v64[2] - v32[2]))
    info = {}
    mine = KO.beam_search(n64, i64, c64, info=info)
    if [(h[0], h[1], h[2]) for h in mine] != [(h[0], h[1], h[2]) for h in h64]:
        return f"(d) {name}: the restatement's hypotheses differ from the reference's"
    w, off, score = KO.decide(mine, keywords)
    if (w >= 0) != v64[0] or (w >= 0 and (names[w] != v64[1] or score != v64[2])):
        return f"(d) {name}: the restatement's verdict differs"
    deep = KO.beam_search(n64, i64, c64, deep_copy=True)
    wd, offd, scored = KO.decide(deep, keywords)
    deep_differs = (wd, offd) != (w, off) or scored != score or \
        [[nd["frame"] for nd in h[2]] for h in deep] != [[nd["frame"] for nd in h[2]] for h in mine]
    state["margin_p"] = min(state["margin_p"], mp)
    state["margin_x"] = min(state["margin_x"], mx)
    state["margin_s"] = min(state["margin_s"], info["min_margin"])
    state["margin_r"] = min(state["margin_r"], info["min_margin_rel"])
    out[f"{name}_cand"] = torch.cat([n64[:, None].double(), i64.double(), c64.detach()], dim=1).numpy()
    for k, v in pack_nbest(h64).items():
        out[f"{name}_{k}"] = v
    out[f"{name}_hit"], out[f"{name}_offset"] = np.int64(w), np.int64(off)
    out[f"{name}_score"] = np.float64(score if w >= 0 else 0.0)
    out[f"{name}_deep_differs"] = np.int64(deep_differs)
    out[f"{name}_max_hyps"], out[f"{name}_both_branches"] = np.int64(info["max_hyps"]), np.int64(info["both_branches"])
    rank4 = False
    for t in range(logits64.shape[0]):
        order = torch.sort(logits64[t], descending=True, stable=True)[1][:4].tolist()
        if order[3] in dec.keywords_idxset and float(p64[t, order[3]]) > 0.05 and any(o not in dec.keywords_idxset for o in order[:3]):
            rank4 = True
    hit_len = next((len(h[0]) for h in mine if any(KO.is_sublist(h[0], lab) != -1 for lab in keywords)), 0)
    state["cover"].append(dict(name=name, hit=w, off=off, n_hyps=len(mine), prefix_len=len(mine[0][0]) if mine else 0,
                               kept=int(n64.sum()), max_hyps=info["max_hyps"], both=info["both_branches"], rank4=rank4, deep=deep_differs,
                               hit_len=hit_len))
    return None


def fresh_state():
    return dict(gap_prob=0.0, gap_score=0.0, gap_path_rel=0.0, gap_logits=0.0, margin_r=float("inf"), margin_p=float("inf"),
                margin_x=float("inf"), margin_s=float("inf"), cover=[])


def check_margins(st):
    if st["margin_p"] < 1000 * st["gap_prob"]:
        return f"(b) p against 0.05: margin {st['margin_p']:.3e} < 1000 x gap_prob {st['gap_prob']:.3e}"
    if st["margin_x"] < 1000 * st["gap_logits"]:
        return f"(b) third against fourth logit: margin {st['margin_x']:.3e} < 1000 x gap_logits {st['gap_logits']:.3e}"
    if st["margin_s"] < 1000 * st["gap_prob"]:
        return f"(b) ps against the node's prob: margin {st['margin_s']:.3e} < 1000 x gap_prob {st['gap_prob']:.3e}"
    if st["margin_r"] < 1000 * st["gap_path_rel"]:
        return f"(b) prune / 1e-6: relative margin {st['margin_r']:.3e} < 1000 x gap_path_rel {st['gap_path_rel']:.3e}"
    return None


def build_model(m: str, seed: int):
    """one model's batch (and, for the FSMN, every clip alone) at `seed` -> (npz contents, state) or (None, why the seed fails)"""
    from funasr_amd import synth

    FsmnKWS, SanmKWS, ku = _reference()
    spec = MODELS[m]
    out, state = {f"{m}_seed": np.int64(seed)}, fresh_state()
    B, T = len(LENS), max(LENS)
    conf = (synth.kws_fsmn_conf if spec["kind"] == "fsmn" else synth.kws_sanm_conf)(vocab=len(TOKENS), **spec["conf"])
    ref = (FsmnKWS if spec["kind"] == "fsmn" else SanmKWS)(**conf).eval()
    sd = synth.kws_state_dict(seed, ref, planted=PLANTED, **spec["plant"])
    g = torch.Generator().manual_seed(1000 + seed)
    feats = torch.randn(B, T, 40, generator=g)
    for b, n in enumerate(LENS):
        feats[b] *= AMPS[b]
        feats[b, n:] = 0
    out[f"{m}_feats"] = feats.numpy()
    dec = ku.KwsCtcPrefixDecoder(ctc=ref.ctc, keywords=MODEL_KEYWORDS, token_list=TOKENS, seg_dict={})
    runs = [("", feats, list(LENS))]
    if spec["kind"] == "fsmn":                                          # (the SAN-M encoder masks by length: alone is the batch)
        runs += [(f"alone{i}", feats[i: i + 1, :n], [n]) for i, n in enumerate(LENS)]
    for tag, x, lens in runs:
        lg = {}
        for dt in (torch.float64, torch.float32):
            ref.load_state_dict(sd, strict=True)
            mm = ref.to(dt)
            with torch.no_grad():
                enc, _ = mm.encode(x.to(dt), torch.tensor(lens))
                lg[dt] = enc if mm.ctc.ctc_lo is None else mm.ctc.ctc_lo(enc)
        ref.to(torch.float32)
        state["gap_logits"] = max(state["gap_logits"], float((lg[torch.float64] - lg[torch.float32].double()).abs().max()))
        out[f"{m}_{tag}_logits".replace("__", "_")] = lg[torch.float64].numpy() if tag == "" else lg[torch.float64][0].numpy()
        if spec["kind"] == "fsmn":                                      # (d) the restatement's FSMN against the reference's
            mine = KO.fsmn_logits(KO.cast(sd, torch.float64), conf["encoder_conf"], x.double(), prefix="encoder.")
            assert float((mine - lg[torch.float64]).abs().max()) < 1e-12, m
        for i, n in enumerate(lens):
            name = f"{m}_c{i}" if tag == "" else f"{m}_{tag}"
            # the fp32 run of (a) is the reference's fp32 NETWORK too: its logits, not the rounded float64 ones
            p32, h32, v32 = decode_clip(dec, lg[torch.float32][i, :n], torch.float32)
            p64, h64, v64 = decode_clip(dec, lg[torch.float64][i, :n], torch.float64)
            if [h[0] for h in h64] != [h[0] for h in h32] or v64[:2] != v32[:2]:
                return None, f"(a) {name}: the fp32 network's hypotheses / verdict differ"
            state["gap_path_rel"] = max([state["gap_path_rel"]] + [abs(a[1] - b[1]) / abs(a[1]) for a, b in zip(h64, h32) if a[1] != 0.0])
            if v64[0]:
                state["gap_score"] = max(state["gap_score"], abs(v64[2] - v32[2]))
            why = record_clip(out, name, dec, lg[torch.float64][i, :n], state)
            if why:
                return None, why
    out[f"gap_logits_{m}"] = np.float64(state["gap_logits"])
    hits = [c["hit"] for c in state["cover"] if c["name"].startswith(m + "_c")]
    if spec["kind"] == "fsmn" and not (any(h >= 0 for h in hits) and any(h < 0 for h in hits)):
        return None, f"(c) {m}: the batch needs a detection and a rejection, hits {hits}"
    if not any(h >= 0 for h in hits):
        return None, f"(c) {m}: the batch needs a detection, hits {hits}"
    why = check_margins(state)
    return (None, why) if why else (out, state)


def build_search():
    """the search-only clips -> (npz contents, state)"""
    from funasr_amd import synth

    FsmnKWS, SanmKWS, ku = _reference()
    out, state = {}, fresh_state()
    ref = FsmnKWS(**synth.kws_fsmn_conf(vocab=len(TOKENS))).eval()
    dec = ku.KwsCtcPrefixDecoder(ctc=ref.ctc, keywords=KEYWORDS, token_list=TOKENS, seg_dict={})
    clips = search_clips()
    out["n_search"] = np.int64(len(clips))
    for j, frames in enumerate(clips):
        lg = posterior_logits(frames)
        out[f"search{j}_logits"] = lg.numpy()
        why = record_clip(out, f"search{j}", dec, lg, state)
        assert why is None, why
    return out, state


def build(seeds: dict):
    """{model: seed} -> (npz contents, None) or (None, why it fails)"""
    out = {"lens": np.asarray(LENS, np.int64), "tokens": np.asarray(TOKENS), "keywords": np.asarray(KEYWORDS),
           "model_keywords": np.asarray(MODEL_KEYWORDS), "models": np.asarray(list(MODELS))}
    total = fresh_state()
    parts = [build_model(m, seeds[m]) for m in MODELS] + [build_search()]
    for part, st in parts:
        if part is None:
            return None, st
        out.update(part)
        for k in ("gap_prob", "gap_score", "gap_path_rel", "gap_logits"):
            total[k] = max(total[k], st[k])
        for k in ("margin_p", "margin_x", "margin_s", "margin_r"):
            total[k] = min(total[k], st[k])
        total["cover"] += st["cover"]
    for k in ("gap_prob", "gap_score", "gap_path_rel", "margin_p", "margin_x", "margin_s", "margin_r"):
        out[k] = np.float64(total[k])
    # (b) holds PER PART, each against its own gaps: a model's gaps include its network's fp32 error (the fp32 run of (a) is the fp32
    # network), which the search-only clips do not have; the totals above are what the tests scale their tolerances with
    names = list(MODELS) + ["search"]
    out["parts"] = np.asarray(names)
    for k in ("gap_prob", "gap_path_rel", "gap_logits", "margin_p", "margin_x", "margin_s", "margin_r"):
        out["part_" + k] = np.asarray([st[k] for _, st in parts], np.float64)
    for name, (_, st) in zip(names, parts):
        why = check_margins(st)
        if why:
            return None, f"{name}: {why}"
    cv = total["cover"]
    need = {"hit at offset 0": any(c["hit"] == 0 and c["off"] == 0 for c in cv),
            "second keyword at offset > 0 in a longer prefix": any(c["hit"] == 1 and c["off"] > 0 and c["hit_len"] > len(KW2) for c in cv),
            "rejection with hypotheses": any(c["hit"] < 0 and c["prefix_len"] > 0 for c in cv),
            "no kept candidate": any(c["kept"] == 0 for c in cv),
            "more than 20 hypotheses": any(c["max_hyps"] > 20 for c in cv),
            "both s == last sub-branches": any(c["both"] for c in cv),
            "keyword token at rank 4": any(c["rank4"] for c in cv),
            "deep copy differs": any(c["deep"] for c in cv)}
    missing = [k for k, v in need.items() if not v]
    if missing:
        return None, f"(c) not covered: {missing}"
    return out, None


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--probe":
        for m in MODELS:
            for seed in range(SEEDS[m], SEEDS[m] + int(sys.argv[2])):
                out, why = build_model(m, seed)
                print(m, seed, "ok" if out is not None else why, flush=True)
        return
    out, why = build(SEEDS)
    assert out is not None, f"seeds {SEEDS} fail condition {why}: pick others"
    path = os.path.join(ROOT, "tests", "golden", "kws.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if k.startswith("gap_") or k.startswith("margin_"):
            print("   ", k, f"{float(out[k]):.3e}")
    for k in sorted(out):
        if k.endswith("_hit"):
            print("   ", k, int(out[k]), int(out[k.replace("_hit", "_offset")]), float(out[k.replace("_hit", "_score")]),
                  "hyps", len(out[k.replace("_hit", "_nbest_len")]), "deep differs", int(out[k.replace("_hit", "_deep_differs")]))
    # the json: state-dict shapes of the two recipes, keyword parsing by the reference's functions
    import yaml
    from oracle import ref_import
    FsmnKWS, SanmKWS, ku = _reference()
    ex = os.path.join(ref_import.REF_ROOT, "examples", "industrial_data_pretraining")
    shapes = {}
    for name, cls, rel, vocab, extra in (("fsmn_4e_l10r2_250_128_fdim80_t2599", FsmnKWS, "fsmn_kws", 2599, {}),
                                         ("sanm_6e_320_256_fdim40_t2602", SanmKWS, "sanm_kws", 2602, {"input_size": 280})):
        y = yaml.safe_load(open(os.path.join(ex, rel, "conf", name + ".yaml")))
        big = cls(encoder=y["encoder"], encoder_conf=y["encoder_conf"], ctc_conf=y["ctc_conf"], vocab_size=vocab, **y["model_conf"], **extra)
        shapes[name] = {"model": y["model"], "encoder": y["encoder"], "encoder_conf": y["encoder_conf"], "ctc_conf": y["ctc_conf"],
                        "model_conf": y["model_conf"], "vocab_size": vocab, **extra,
                        "shapes": {k: list(v.shape) for k, v in big.state_dict().items()}}
    table = {t: i for i, t in enumerate(TOKENS)}
    parse = []
    for s in PARSE_STRINGS:
        strs, idx = ku.query_token_set(s, table, PARSE_SEG_DICT)
        parse.append({"txt": s, "split": ku.split_mixed_label(s), "tokens_str": list(strs), "tokens_idx": [int(i) for i in idx]})
    dec = ku.KwsCtcPrefixDecoder(ctc=None, keywords=" hello ni, " + TOKENS[5] + TOKENS[9] + ",hello ni ,world", token_list=TOKENS, seg_dict=PARSE_SEG_DICT)
    with open(os.path.join(ROOT, "tests", "golden", "kws.json"), "w", encoding="utf-8") as f:
        json.dump({"recipes": shapes, "tokens": TOKENS, "models": MODELS, "planted": list(PLANTED), "seg_dict": PARSE_SEG_DICT, "parse": parse,
                   "decoder": {"keywords": dec.keywords_str, "idxset": sorted(int(i) for i in dec.keywords_idxset),
                               "table": {k: [int(i) for i in v["token_id"]] for k, v in dec.keywords_token.items()}}},
                  f, ensure_ascii=False, indent=0)


if __name__ == "__main__":
    main()
