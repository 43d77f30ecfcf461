"""Cases of tests/test_streaming_f16x2_gpu.py, each run in its OWN process (`python tests/_stream_f16x2_cases.py <case>`): a
GPU fault in a kernel path that has not yet seen hardware must not take the rest of the suite with it. Exit code 0 = passed;
an assertion prints its message and exits 1.

The streaming step in its f16x2 form (StreamBatch(precision="f16x2"), pf_stream_set_option("gemm_mode", 3)): every GEMM of
the step on the fp16 matrix cores with two-plane operands (fp32-class results), everything else as in the default step.
Bars are the default step's: token ids / counts / position counter equal to the REFERENCE's ParaformerStreaming sessions
(tests/golden/streaming.npz, streaming_geometries.npz, streaming_sparse.npz), encoder window and carried CIF state within 1e-3.
The batch_* / sparse_* cases hold EVERY stream of a batch, and steps in which a stream fires no token, to the per-stream oracle and
to the one-stream session (inputs, their preconditions and the bars: tests/_stream_batch_common.py)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from funasr_amd import synth  # noqa: E402


def load():
    g = np.load(os.path.join(GOLD, "streaming.npz"), allow_pickle=False)
    cfg = json.loads(bytes(g["config"]).decode())
    sd = synth.paraformer_state_dict(cfg, seed=int(g["seed"]), cif_bias=float(g["cif_bias"]))
    return g, cfg, sd


def build(cfg, sd, dev):
    from funasr_amd.paraformer_streaming import ParaformerStreaming
    model = ParaformerStreaming.from_config(cfg)
    model.load_state_dict(sd, strict=False)
    return model.to(dev)


def golden_session(dev, use_graph):
    from funasr_amd.paraformer_streaming import StreamBatch
    g, cfg, sd = load()
    model = build(cfg, sd, dev)
    sb = StreamBatch(model, 1, [0, 10, 5], 4, 1, use_graph=use_graph, precision="f16x2")
    for i in range(int(g["n_chunks"])):
        fin, tail, start_idx = (int(v) for v in g[f"flags_{i}"])
        feats = None if tail else torch.from_numpy(g[f"feats_{i}"]).to(dev)
        ids, enc = sb.step(feats, is_final=bool(fin), tail_chunk=bool(tail), return_enc=True)
        ref = torch.from_numpy(g[f"enc_{i}"])
        assert tuple(enc.shape) == tuple(ref.shape), i
        err = (enc.cpu() - ref).abs().max().item()
        assert err < 1e-3, (i, err)
        got = [t for t in ids[0] if t not in (0, 1, 2)]
        assert got == g[f"tokens_{i}"].tolist(), (i, got, g[f"tokens_{i}"].tolist())
        st = sb.peek()
        assert st["start_idx"] == start_idx
        assert abs(st["cif_alphas"][0] - float(g[f"cif_alphas_{i}"][0])) < 1e-4, i
        assert (st["cif_hidden"][0] - torch.from_numpy(g[f"cif_hidden_{i}"])).abs().max().item() < 1e-3, i
    sb.close()


def case_golden_eager(dev):
    golden_session(dev, False)


def case_golden_graph(dev):
    golden_session(dev, True)


def case_geometries(dev):
    """the reference's own sessions at other chunk sizes / look-back settings (tests/golden/streaming_geometries.npz)"""
    from funasr_amd.paraformer_streaming import StreamBatch
    g, cfg, sd = load()
    model = build(cfg, sd, dev)
    gg = np.load(os.path.join(GOLD, "streaming_geometries.npz"), allow_pickle=False)
    for si, s in enumerate(json.loads(str(gg["sessions"]))):
        sb = StreamBatch(model, 1, s["chunk"], s["enc_lb"], s["dec_lb"], use_graph=True, precision="f16x2")
        for i in range(s["n_chunks"]):
            fin, tail, start_idx = (int(v) for v in gg[f"s{si}_flags_{i}"])
            feats = None if tail else torch.from_numpy(gg[f"s{si}_feats_{i}"]).to(dev)
            ids = sb.step(feats, is_final=bool(fin), tail_chunk=bool(tail))
            got = [t for t in ids[0] if t not in (0, 1, 2)]
            assert got == gg[f"s{si}_tokens_{i}"].tolist(), (s, i, got)
            assert sb.peek()["start_idx"] == start_idx
        sb.close()


def _session(model, dev, S, precision, graph, g, seed=5, reps=1):
    from funasr_amd.paraformer_streaming import StreamBatch
    gen = torch.Generator()
    sb = StreamBatch(model, S, [0, 10, 5], 4, 1, use_graph=graph, precision=precision)
    out = []
    for _ in range(reps):
        gen.manual_seed(seed)
        for i in range(int(g["n_chunks"])):
            fin, tail, _ = (int(v) for v in g[f"flags_{i}"])
            feats = None
            if not tail:
                f0 = torch.from_numpy(g[f"feats_{i}"])
                others = [f0 * 0.5 + 0.1 * torch.randn(f0.shape, generator=gen) for _ in range(S - 1)]
                feats = torch.cat([f0] + others, 0).to(dev)
            ids, enc = sb.step(feats, is_final=bool(fin), tail_chunk=bool(tail), return_enc=True)
            out.append((ids, enc.cpu()))
        sb.reset()
    sb.close()
    return out


def case_batch_independence_and_graph(dev):
    """f16x2 step: graph replay == eager bitwise; stream 0 of a 9-stream batch == the 1-stream session bitwise (every GEMM
    block shape gives the same bits, all other ops are per row / per stream); reset() reproduces the session"""
    g, cfg, sd = load()
    model = build(cfg, sd, dev)
    n = int(g["n_chunks"])
    e1 = _session(model, dev, 1, "f16x2", False, g, reps=2)
    g1 = _session(model, dev, 1, "f16x2", True, g)
    g9 = _session(model, dev, 9, "f16x2", True, g)
    for a, b in zip(e1[:n], g1):
        assert a[0] == b[0] and torch.equal(a[1], b[1]), "graph replay differs from eager"
    for a, b in zip(e1[:n], g9):
        assert a[0][0] == b[0][0] and torch.equal(a[1][0], b[1][0]), "stream 0 depends on its batch neighbours"
    for a, b in zip(e1[:n], e1[n:]):
        assert a[0] == b[0] and torch.equal(a[1], b[1]), "reset() does not reproduce the session"


def case_many_streams_vs_fp32_step(dev):
    """9 lock-step streams: the f16x2 step against the default fp32 step on the same features -- token ids and counts equal on
    every stream and chunk, encoder windows within 2e-4 (both are fp32-class; the golden bar vs the reference is 1e-3)"""
    g, cfg, sd = load()
    model = build(cfg, sd, dev)
    a = _session(model, dev, 9, "fp32", True, g)
    b = _session(model, dev, 9, "f16x2", True, g)
    worst = 0.0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0], (i, x[0], y[0])
        worst = max(worst, (x[1] - y[1]).abs().max().item())
    assert worst < 2e-4, worst
    print(f"max |enc f16x2 - enc fp32| = {worst:.3e}")


def case_weight_reload(dev, precision="f16x2"):
    """the prepared planes / exponents (f16x2 step) and the LayerNorm -> GEMM constants (fp32 step, Stream.ln_consts) follow a weight
    reload on the live handles (TensorTable version): a StreamBatch created before load_state_dict gives the results of a model built
    from the new weights"""
    from funasr_amd.paraformer_streaming import StreamBatch
    g, cfg, sd = load()
    sd2 = synth.paraformer_state_dict(cfg, seed=int(g["seed"]) + 1, cif_bias=float(g["cif_bias"]))
    model = build(cfg, sd, dev)
    sb = StreamBatch(model, 2, [0, 10, 5], 4, 1, use_graph=True, precision=precision)
    feats = [torch.from_numpy(g[f"feats_{i}"]).repeat(2, 1, 1).to(dev) for i in range(4)]
    for f in feats:
        sb.step(f)
    model.load_state_dict(sd2, strict=False)
    sb.reset()
    got = [sb.step(f, return_enc=True) for f in feats]
    sb.close()
    fresh = build(cfg, sd2, dev)
    sr = StreamBatch(fresh, 2, [0, 10, 5], 4, 1, use_graph=False, precision=precision)
    ref = [sr.step(f, return_enc=True) for f in feats]
    sr.close()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a[0] == b[0] and torch.equal(a[1], b[1]), i


def case_weight_reload_fp32_step(dev):
    case_weight_reload(dev, "fp32")


def case_shared_encoder_handle(dev):
    """One encoder handle serves an offline forward in fp32 and a gemm_mode 3 session at a time (StreamBatch runs over the model's
    own handles): the planes of each mode carry their own version stamp, so both give BITWISE what handles that serve only one of
    the two give -- before and after a weight reload on the live model"""
    from funasr_amd.paraformer_streaming import StreamBatch
    g, cfg, sd = load()
    sd2 = synth.paraformer_state_dict(cfg, seed=int(g["seed"]) + 1, cif_bias=float(g["cif_bias"]))
    feats = torch.from_numpy(g["feats_0"]).repeat(2, 1, 1).to(dev)
    xs = (torch.randn(2, 40, 560, generator=torch.Generator().manual_seed(6)) * 0.7).to(dev)
    xs[1, 33:] = 0

    def offline(model):
        return model.encoder.set_precision("fp32")(xs, [40, 33])[0].cpu()

    def one_step(model, sb=None):
        own = sb or StreamBatch(model, 2, [0, 10, 5], 4, 1, use_graph=False, precision="f16x2")
        ids, enc = own.step(feats, return_enc=True)
        if sb is None:
            own.close()
        return ids, enc.cpu()

    model = build(cfg, sd, dev)
    sb = StreamBatch(model, 2, [0, 10, 5], 4, 1, use_graph=True, precision="f16x2")
    got = [(offline(model), one_step(model, sb))]
    model.load_state_dict(sd2, strict=False)
    sb.reset()
    got.append((offline(model), one_step(model, sb)))
    sb.close()
    for (off, (ids, enc)), weights in zip(got, (sd, sd2)):
        assert torch.equal(off, offline(build(cfg, weights, dev))), "offline fp32 forward on the shared handle"
        rids, renc = one_step(build(cfg, weights, dev))
        assert ids == rids and torch.equal(enc, renc), "gemm_mode 3 step on the shared handle"
    assert not torch.equal(got[0][0], got[1][0])


def case_oracle_geometry_many_tokens(dev):
    """chunk_size [0, 20, 10] (up to 42 fires per step) against the reference-pinned streaming oracle"""
    from funasr_amd.paraformer_streaming import StreamBatch
    from oracle import streaming_oracle as S
    g, cfg, sd = load()
    model = build(cfg, sd, dev)
    chunk, enc_lb, dec_lb = [0, 20, 10], 2, 1
    sb = StreamBatch(model, 1, chunk, enc_lb, dec_lb, precision="f16x2")
    st = S.model_init(cfg, tuple(chunk), enc_lb, dec_lb)
    gen = torch.Generator().manual_seed(chunk[1] * 10 + enc_lb)
    for i in range(6):
        fin = i == 5
        n = chunk[1] if not fin else chunk[1] + 2
        feats = torch.randn(1, n, 560, generator=gen) * 0.7
        trace = []
        with torch.no_grad():
            oids = S.generate_chunk(feats.clone(), st, sd, cfg, fin, trace)
        ids, enc = sb.step(feats.to(dev), is_final=fin, return_enc=True)
        assert (enc.cpu() - trace[0]["enc"]).abs().max().item() < 1e-3, i
        assert [t for t in ids[0] if t not in (0, 1, 2)] == oids, (i, ids[0], oids)
        assert len(ids[0]) == trace[0]["n"], i
    sb.close()


# ---- every stream of a batch, and steps that fire no token (tests/_stream_batch_common.py; the fp32 step: tests/test_streaming_batch_gpu.py)
def case_sparse_reference_eager(dev):
    from tests import _stream_batch_common as B
    worst, zeros = B.reference_sparse_sessions(dev, "f16x2", False)
    print(f"f16x2 eager: max |enc - reference| = {worst:.3e}, zero-fire steps = {zeros}")


def case_sparse_reference_graph(dev):
    from tests import _stream_batch_common as B
    worst, zeros = B.reference_sparse_sessions(dev, "f16x2", True)
    print(f"f16x2 graph: max |enc - reference| = {worst:.3e}, zero-fire steps = {zeros}")


def _batch_vs_oracle(dev, name, S):
    from tests import _stream_batch_common as B
    seeds = B.GEOMETRIES[name]["seeds"][:S]
    assert len(seeds) == S
    B.check_inputs(name, seeds)
    out, rows = B.run_batch(dev, name, seeds, "f16x2")
    if name == "rows96":
        assert rows > 48, rows                      # the 96-row instance of dec_fsmn_chunk_kernel
    worst, zeros = B.check_vs_oracle(out, name, seeds, "f16x2")
    assert zeros > 0 or not B.GEOMETRIES[name]["sparse"]
    print(f"f16x2 {name} S={S}: max |enc - oracle| = {worst:.3e}, zero-fire (stream, step) pairs = {zeros}, token rows = {rows}")


def case_batch_vs_oracle_sparse_a(dev):
    _batch_vs_oracle(dev, "sparse_a", 4)


def case_batch_vs_oracle_sparse_b(dev):
    _batch_vs_oracle(dev, "sparse_b", 4)


def case_batch_vs_oracle_sparse_c(dev):
    _batch_vs_oracle(dev, "sparse_c", 4)


def case_batch_vs_oracle_sparse_d(dev):
    _batch_vs_oracle(dev, "sparse_d", 4)


def case_batch_vs_oracle_rows96(dev):
    _batch_vs_oracle(dev, "rows96", 2)


def case_batch_streams_equal_their_one_stream_sessions(dev):
    """stream k of a 4-stream batch == the 1-stream session on stream k's features, bitwise (ids, encoder window, carried CIF state);
    the batch with its streams reversed gives the reversed results -- under the default options too: the f16x2 GEMMs give the same bits
    at every block shape"""
    from tests import _stream_batch_common as B
    for name, options in (("sparse_a", ({"ln_carry": 0}, {"ln_carry": 2}, None)), ("sparse_d", (None,))):
        seeds = B.GEOMETRIES[name]["seeds"][:4]
        B.check_inputs(name, seeds)
        for opts in options:
            batch, _ = B.run_batch(dev, name, seeds, "f16x2", opts)
            for k, s in enumerate(seeds):
                one, _ = B.run_batch(dev, name, [s], "f16x2", opts)
                B.assert_same(one, batch, f"{name} {opts}: stream {k} alone / in the batch", streams_b=[k])
            rev, _ = B.run_batch(dev, name, seeds[::-1], "f16x2", opts)
            B.assert_same(batch, rev, f"{name} {opts}: streams reversed", streams_b=[3, 2, 1, 0])


def case_batch_gate_forms_agree(dev):
    """"kv_batched" 1 (one GEMM over the concatenated K | V weights, one gated append) / 0 (per layer, the append gated inside the
    cross-attention or its fallback launch) and "ln_folded" 0 / 1: bitwise on every stream of the sparse session"""
    from tests import _stream_batch_common as B
    for name in ("sparse_a", "sparse_d"):
        seeds = B.GEOMETRIES[name]["seeds"][:4]
        zeros = B.check_inputs(name, seeds)
        assert zeros >= 8
        plain, _ = B.run_batch(dev, name, seeds, "f16x2", {"ln_folded": 0, "kv_batched": 0, "short_k": 0})
        B.check_vs_oracle(plain, name, seeds, "plain launches")
        for folded, kv in ((0, 1), (1, 0), (1, 1)):
            other, _ = B.run_batch(dev, name, seeds, "f16x2", {"ln_folded": folded, "kv_batched": kv, "short_k": 0})
            B.assert_same(plain, other, f"{name} ln_folded {folded} kv_batched {kv}")
        print(f"f16x2 {name}: zero-fire (stream, step) pairs = {zeros}")


def case_batch_graph_and_reset_with_diverged_streams(dev):
    from tests import _stream_batch_common as B
    name, seeds = "sparse_a", B.GEOMETRIES["sparse_a"]["seeds"][:4]
    B.check_inputs(name, seeds)
    eager, _ = B.run_batch(dev, name, seeds, "f16x2", graph=False)
    graph, _ = B.run_batch(dev, name, seeds, "f16x2", graph=True)
    B.assert_same(eager, graph, "graph replay / eager")
    again, _ = B.run_batch(dev, name, seeds, "f16x2", graph=True, reset_after=4)
    B.assert_same(graph, again, "after reset() / fresh")


def case_batch_66_streams(dev):
    """66 streams (the precision such a batch gets by default; the second block of stream_advance_dec_kernel): six sparse feature
    sequences, each eleven times in a shuffled order -- every stream bitwise equal to the 1-stream session on its sequence, and those
    six sessions against the oracle"""
    from funasr_amd.paraformer_streaming import StreamBatch
    from tests import _stream_batch_common as B
    name, six = "sparse_a", B.GEOMETRIES["sparse_a"]["seeds"]
    assert len(six) == 6 and 66 >= StreamBatch.AUTO_F16X2_MIN_STREAMS
    zeros = B.check_inputs(name, six)
    order = torch.randperm(66, generator=torch.Generator().manual_seed(66)).tolist()
    which = [i % 6 for i in order]                               # stream k carries sequence which[k]
    assert sorted(which) == sorted(list(range(6)) * 11) and which[:6] != list(range(6))
    ones = []
    for s in six:
        one, _ = B.run_batch(dev, name, [s], "f16x2")
        B.check_vs_oracle(one, name, [s], "f16x2, one stream")
        ones.append(one)
    batch, _ = B.run_batch(dev, name, [six[w] for w in which], "f16x2")
    for k, w in enumerate(which):
        for i, ((ia, ea, pa), (ib, eb, pb)) in enumerate(zip(ones[w], batch)):
            at = ("stream", k, "sequence", w, "step", i)
            assert ia[0] == ib[k], (at, ia[0], ib[k])
            assert torch.equal(ea[0], eb[k]), (at, (ea[0] - eb[k]).abs().max().item())
            assert pa["cif_alphas"][0] == pb["cif_alphas"][k] and torch.equal(pa["cif_hidden"][0], pb["cif_hidden"][k]), at
    print(f"f16x2 S=66: zero-fire (stream, step) pairs = {zeros * 11}")


CASES = {k[5:]: v for k, v in globals().items() if k.startswith("case_")}

if __name__ == "__main__":
    name = sys.argv[1]
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    CASES[name](torch.device("cuda:0"))
    print(f"case {name}: ok")
