"""Inputs, oracle sessions and runners shared by tests/test_streaming_batch_gpu.py (the fp32 step) and the batch cases of
tests/_stream_f16x2_cases.py (the f16x2 step): S lock-step streams with OWN features each, at a predictor bias low enough that
many steps fire NO token on some streams while others decode -- every per-stream gate, offset and counter of the step
(n_fired, dec_wp, dec_valid, the rings, the decoder's FSMN state, the CIF carry) then differs between the streams of one batch.

The reference side: the streaming oracle (oracle/streaming_oracle.py), pinned to the reference's own sparse sessions by
tests/test_oracle_streaming.py (tests/golden/streaming_sparse.npz). One oracle session per (geometry, stream), computed once and
shared read-only. The feature seeds were fixed with the oracle alone, before any GPU run; check_inputs() holds them to the
conditions they were chosen by, so that nobody swaps in seeds that dodge a failure."""
import functools
import json
import os

import numpy as np
import torch

from funasr_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIRE_MARGIN = 2e-4          # distance of every integrate-and-fire decision from the threshold (the aligner goldens' margin)
TOP2_MARGIN = 1e-3          # top-two log-probabilities of every decoded row

# chunk, look-backs, predictor bias, steps, frames of the last (final) step, whether a tail chunk ends the session, feature seeds
GEOMETRIES = {
    # sparse_a: six sequences; the four-stream tests take the first four, the 66-stream case all six
    "sparse_a": dict(chunk=[0, 10, 5], enc_lb=4, dec_lb=1, cif_bias=-3.0, steps=8, last=12, tail=False, sparse=True,
                     seeds=[0, 1, 2, 3, 4, 5]),
    # the first-chunk-untrimmed encoder ring and a decoder ring that wraps (15-row windows into 20 rows); ends with a tail chunk
    "sparse_b": dict(chunk=[5, 10, 5], enc_lb=1, dec_lb=2, cif_bias=-3.0, steps=8, last=0, tail=True, sparse=True,
                     seeds=[0, 1, 2, 4]),
    "sparse_c": dict(chunk=[6, 4, 2], enc_lb=1, dec_lb=1, cif_bias=-2.5, steps=10, last=5, tail=False, sparse=True,
                     seeds=[0, 1, 2, 6]),
    # the decoder ring of 20 rows takes 15-row windows: the only geometry here whose ring is NOT rewritten whole by every append, i.e.
    # where a stream's own write pointer decides which cached rows survive (elsewhere it only rotates the order of the keys)
    "sparse_d": dict(chunk=[0, 10, 5], enc_lb=4, dec_lb=2, cif_bias=-3.0, steps=8, last=12, tail=False, sparse=True,
                     seeds=[0, 1, 2, 3]),
    # 49 token rows per step: the 96-row instance of the decoder's FSMN kernel (every step fires, so only (d) and (e) apply)
    "rows96": dict(chunk=[0, 40, 8], enc_lb=1, dec_lb=1, cif_bias=0.6, steps=6, last=42, tail=False, sparse=False,
                   seeds=[0, 3]),
}


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(GOLD, "streaming.npz"), allow_pickle=False)
    return json.loads(bytes(g["config"]).decode()), int(g["seed"])


@functools.lru_cache(maxsize=None)
def state_dict(cif_bias):
    cfg, seed = golden()
    return synth.paraformer_state_dict(cfg, seed=seed, cif_bias=cif_bias)


_models = {}


def model_for(cif_bias, dev):
    from funasr_amd.paraformer_streaming import ParaformerStreaming
    key = (cif_bias, str(dev))
    if key not in _models:
        m = ParaformerStreaming.from_config(golden()[0])
        m.load_state_dict(state_dict(cif_bias), strict=False)
        _models[key] = m.to(dev)
    return _models[key]


def steps_of(name):
    """[(frames, is_final, tail)] of the session"""
    g = GEOMETRIES[name]
    n = g["steps"]
    if g["tail"]:
        return [(g["chunk"][1], False, False)] * (n - 1) + [(0, True, True)]
    return [(g["chunk"][1], False, False)] * (n - 1) + [(g["last"], True, False)]


@functools.lru_cache(maxsize=None)
def features(name, seed):
    """randn * 0.7 per step, from a generator seeded per (geometry, stream); None for a tail chunk"""
    gen = torch.Generator().manual_seed(100 * sorted(GEOMETRIES).index(name) + seed)
    return tuple(None if tail else torch.randn(1, n, 560, generator=gen) * 0.7 for n, _, tail in steps_of(name))


def _fire_margin(alphas, thr=1.0):
    """the oracle's float32 integrate-and-fire loop over the weights it used: min |alpha + integrate - threshold|"""
    integ, worst = torch.tensor(0.0), float("inf")
    thr = torch.tensor(float(thr))
    for a in alphas:
        s = a + integ
        worst = min(worst, abs(float(s) - float(thr)))
        integ = s if s < thr else s - thr
    return worst


@functools.lru_cache(maxsize=None)
def oracle_session(name, seed):
    """one record per step: enc [1, W, D], n, ids (sos / eos / blank dropped), carried CIF state, the two margins"""
    from oracle import streaming_oracle as S
    g = GEOMETRIES[name]
    cfg, _ = golden()
    sd = state_dict(g["cif_bias"])
    st = S.model_init(cfg, tuple(g["chunk"]), g["enc_lb"], g["dec_lb"])
    out = []
    for f, (_, fin, tail) in zip(features(name, seed), steps_of(name)):
        if tail:
            st["tail_chunk"] = True
            f = st["feats"]
        trace = []
        with torch.no_grad():
            ids = S.generate_chunk(f.clone(), st, sd, cfg, fin, trace)
        r = trace[0]
        top2 = float("inf")
        if r["n"] >= 1:
            t = r["logp"].topk(2, dim=-1).values
            top2 = float((t[:, 0] - t[:, 1]).min())
        out.append(dict(enc=r["enc"], n=r["n"], ids=ids, cif_alpha=float(st["cif_alphas"]), cif_hidden=st["cif_hidden"].reshape(-1).clone(),
                        start_idx=st["start_idx"], fire_margin=_fire_margin(r["alphas"], cfg["predictor"]["threshold"]), top2=top2))
    return out


def stream_ok(name, seed):
    """the conditions on ONE stream: (b) a zero-fire step followed by a firing one (sparse geometries), (d), (e)"""
    o = oracle_session(name, seed)
    ns = [r["n"] for r in o]
    b = any(x == 0 and y >= 1 for x, y in zip(ns, ns[1:])) or not GEOMETRIES[name]["sparse"]
    return b and min(r["fire_margin"] for r in o) >= FIRE_MARGIN and min(r["top2"] for r in o) >= TOP2_MARGIN


def batch_ok(name, seeds):
    """the conditions across the streams of a batch: (a) at least two steps in which one stream fires nothing while another decodes,
    (c) after the third step (and after the fourth: where reset() is tested) two streams differ in how many decoder calls they made"""
    ns = [[r["n"] for r in oracle_session(name, s)] for s in seeds]
    steps = list(zip(*ns))
    a = sum(1 for col in steps if min(col) == 0 and max(col) >= 1) >= 2
    c = all(len({sum(1 for x in row[:k] if x >= 1) for row in ns}) >= 2 for k in (3, 4))
    return a and c


def check_inputs(name, seeds=None):
    """conditions (a) - (e) as assertions, on the CPU; returns the number of zero-fire (stream, step) pairs of the batch"""
    g = GEOMETRIES[name]
    seeds = list(seeds if seeds is not None else g["seeds"])
    assert len(set(seeds)) == len(seeds) and all(0 <= s < 50 for s in seeds), seeds
    for s in seeds:
        o = oracle_session(name, s)
        ns = [r["n"] for r in o]
        assert min(r["fire_margin"] for r in o) >= FIRE_MARGIN, (name, s, "(d)", [r["fire_margin"] for r in o])
        assert min(r["top2"] for r in o) >= TOP2_MARGIN, (name, s, "(e)", [r["top2"] for r in o])
        if g["sparse"]:
            assert any(x == 0 and y >= 1 for x, y in zip(ns, ns[1:])), (name, s, "(b)", ns)
    if g["sparse"]:
        assert batch_ok(name, seeds), (name, "(a) / (c)", [[r["n"] for r in oracle_session(name, s)] for s in seeds])
    return sum(1 for s in seeds for r in oracle_session(name, s) if r["n"] == 0)


def token_rows(sb, name):
    """token rows per stream of the session's largest step: min(W + 1 + final, max_tokens), engine_stream.hip stream_token_rows()"""
    return max(min(sb.keep + n + 1 + int(fin), sb.max_tokens) for n, fin, tail in steps_of(name) if not tail)


def run_batch(dev, name, seeds, precision, opts=None, graph=True, reset_after=None):
    """the session on a StreamBatch of len(seeds) streams -> per step (ids per stream, enc [S, W, D] on the host, peek());
    reset_after = k: k steps, reset(), then the whole session"""
    from funasr_amd.paraformer_streaming import StreamBatch
    g = GEOMETRIES[name]
    sb = StreamBatch(model_for(g["cif_bias"], dev), len(seeds), g["chunk"], g["enc_lb"], g["dec_lb"], use_graph=graph, precision=precision)
    for k, v in (opts or {}).items():
        sb.set_option(k, v)
    per_stream = [features(name, s) for s in seeds]
    plan = list(enumerate(steps_of(name)))
    if reset_after is not None:
        plan = plan[:reset_after] + [None] + plan
    out = []
    for item in plan:
        if item is None:
            sb.reset()
            out = []
            continue
        i, (n, fin, tail) = item
        feats = None if tail else torch.cat([f[i] for f in per_stream], 0).to(dev)
        ids, enc = sb.step(feats, is_final=fin, tail_chunk=tail, return_enc=True)
        out.append((ids, enc.cpu(), sb.peek()))
    rows = token_rows(sb, name)
    sb.close()
    return out, rows


def check_vs_oracle(out, name, seeds, what=""):
    """every stream and step against the stream's own oracle session: ids (sos / eos / blank dropped) and counts equal, position counter
    equal, encoder window within 1e-3, carried CIF weight within 1e-4 and frame within 1e-3 (the bars of
    test_stream_steps_match_reference_given_reference_features). Returns (worst encoder window difference, zero-fire steps run)."""
    worst, zeros = 0.0, 0
    for k, s in enumerate(seeds):
        o = oracle_session(name, s)
        assert len(o) == len(out)
        for i, (r, (ids, enc, st)) in enumerate(zip(o, out)):
            at = (what, name, "stream", k, "step", i)
            assert [t for t in ids[k] if t not in (0, 1, 2)] == r["ids"], (at, ids[k], r["ids"])
            assert len(ids[k]) == r["n"], (at, len(ids[k]), r["n"])
            assert st["start_idx"] == r["start_idx"], at
            assert tuple(enc[k:k + 1].shape) == tuple(r["enc"].shape), at
            d = (enc[k:k + 1] - r["enc"]).abs().max().item()
            worst = max(worst, d)
            assert d < 1e-3, (at, d)
            assert abs(st["cif_alphas"][k] - r["cif_alpha"]) < 1e-4, (at, st["cif_alphas"][k], r["cif_alpha"])
            assert (st["cif_hidden"][k] - r["cif_hidden"]).abs().max().item() < 1e-3, at
            zeros += r["n"] == 0
    return worst, zeros


def assert_same(a, b, what, streams_b=None, enc_tol=None):
    """two runs step by step: ids equal; encoder windows and carried CIF state bitwise (enc_tol None) or the windows within enc_tol.
    streams_b[k] = the stream of run b that stream k of run a is compared with (default: the same). Returns the worst window difference."""
    assert len(a) == len(b), what
    S = len(a[0][0])
    idx = list(streams_b) if streams_b is not None else list(range(S))
    worst = 0.0
    for i, ((ia, ea, pa), (ib, eb, pb)) in enumerate(zip(a, b)):
        for k, j in enumerate(idx):
            at = (what, "stream", k, "step", i)
            assert ia[k] == ib[j], (at, ia[k], ib[j])
            if enc_tol is None:
                assert torch.equal(ea[k], eb[j]), (at, (ea[k] - eb[j]).abs().max().item())
                assert pa["cif_alphas"][k] == pb["cif_alphas"][j] and torch.equal(pa["cif_hidden"][k], pb["cif_hidden"][j]), at
            else:
                d = (ea[k] - eb[j]).abs().max().item()
                worst = max(worst, d)
                assert d < enc_tol, (at, d)
    return worst


def reference_sparse_sessions(dev, precision, use_graph):
    """the reference's own ParaformerStreaming sessions with the predictor bias lowered (tests/golden/streaming_sparse.npz,
    oracle/make_golden_streaming.py --sparse): on every chunk, the tail chunk included, token ids, counts and position counter equal,
    encoder window within 1e-3, carried CIF weight within 1e-4 and frame within 1e-3. Returns (worst window difference, zero-fire steps)."""
    from funasr_amd.paraformer_streaming import StreamBatch
    gg = np.load(os.path.join(GOLD, "streaming_sparse.npz"), allow_pickle=False)
    worst, zeros = 0.0, 0
    for si, s in enumerate(json.loads(str(gg["sessions"]))):
        sb = StreamBatch(model_for(s["cif_bias"], dev), 1, s["chunk"], s["enc_lb"], s["dec_lb"], use_graph=use_graph, precision=precision)
        for i in range(s["n_chunks"]):
            fin, tail, start_idx = (int(v) for v in gg[f"s{si}_flags_{i}"])
            feats = None if tail else torch.from_numpy(gg[f"s{si}_feats_{i}"]).to(dev)
            ids, enc = sb.step(feats, is_final=bool(fin), tail_chunk=bool(tail), return_enc=True)
            ref = torch.from_numpy(gg[f"s{si}_enc_{i}"])
            want = gg[f"s{si}_tokens_{i}"].tolist()
            assert tuple(enc.shape) == tuple(ref.shape), (s, i)
            err = (enc.cpu() - ref).abs().max().item()
            worst = max(worst, err)
            assert err < 1e-3, (s, i, err)
            assert [t for t in ids[0] if t not in (0, 1, 2)] == want, (s, i, ids[0], want)
            # the reference returns nothing exactly where it skipped the decoder (the oracle test pins n == 0 there); a decoded row
            # that is sos / eos / blank would show as a longer raw list
            assert len(ids[0]) >= len(want) and (len(want) > 0 or len(ids[0]) == 0), (s, i, ids[0])
            st = sb.peek()
            assert st["start_idx"] == start_idx, (s, i)
            assert abs(st["cif_alphas"][0] - float(gg[f"s{si}_cif_alphas_{i}"][0])) < 1e-4, (s, i)
            assert (st["cif_hidden"][0] - torch.from_numpy(gg[f"s{si}_cif_hidden_{i}"])).abs().max().item() < 1e-3, (s, i)
            zeros += len(ids[0]) == 0
        sb.close()
    assert zeros >= 6
    return worst, zeros
