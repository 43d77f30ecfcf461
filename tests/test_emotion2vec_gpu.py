"""emotion2vec on the MI355X: the conv-as-GEMM strided view, the HIP network against the reference's recorded outputs and the
float64 oracle (both precision modes), batch invariance and determinism (bitwise), and AutoModel end to end."""
import os

import numpy as np
import pytest
import torch

from funasr_amd import _lib, synth
from funasr_amd.emotion2vec import Emotion2vec

from . import _emotion2vec_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emotion2vec.npz")
LABELS = ["angry", "disgusted", "fearful", "happy", "neutral", "other", "sad", "surprised", "unuse_0"]


def _model(cuda, conf, seed, vocab=9, precision="f16x2", max_samples=8 << 20):
    m = Emotion2vec(model_conf=conf, vocab_size=vocab, precision=precision, max_samples=max_samples)
    sd = synth.emotion2vec_state_dict(seed, m)
    m.load_state_dict(sd, strict=True)
    if vocab > 0:
        m.set_labels(LABELS[:vocab])
    return m.to(cuda), sd


def _wav(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 16000
    return (0.3 * torch.sin(2 * np.pi * (150 + 10 * seed) * t) * torch.sin(2 * np.pi * 3 * t)
            + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float()


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_conv_gemm_strided_view_equals_im2col(cuda, k, s):
    """output row t of a (k, s) conv = the contiguous K = k * 512 run at row s * t: lda = s * 512 < K reads overlapping rows; the
    product must be bitwise that over an explicit im2col copy, fp32 MFMA and f16x2"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(k)
    Min, N = 999, 512
    M = (Min - k) // s + 1
    x = torch.randn(Min + 8, 512, generator=g).to(cuda)
    w = (torch.randn(N, k * 512, generator=g) / 40).to(cuda)
    col = torch.stack([x[s * t: s * t + k].reshape(-1) for t in range(M)]).contiguous()
    strm = torch.cuda.current_stream().cuda_stream
    outs = []
    for A, lda in ((x, s * 512), (col, k * 512)):
        c = torch.empty(M, N, device=cuda)
        _lib.check(lib.pf_k_gemm_f32(A.data_ptr(), lda, w.data_ptr(), k * 512, None, None, 0, None, 0, c.data_ptr(), N, M, N, k * 512, 0,
                                     strm), "gemm_f32")
        outs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref = col.double() @ w.double().t()
    assert (outs[0].double() - ref).abs().max().item() < 1e-3
    # f16x2: planes of x * 2^10 (the whole buffer; viewed with lda = s * 512) and of the im2col copy
    w2 = torch.empty(2, N, k * 512, dtype=torch.float16, device=cuda)
    _lib.check(lib.pf_k_split2(w.data_ptr(), k * 512, w2.data_ptr(), k * 512, N * k * 512, N, k * 512, 2.0 ** 12, strm), "split2")
    outs2 = []
    for A, rows, width, lda in ((x, Min + 8, 512, s * 512), (col, M, k * 512, k * 512)):
        a2 = torch.empty(2, rows, width, dtype=torch.float16, device=cuda)
        _lib.check(lib.pf_k_split2(A.data_ptr(), width, a2.data_ptr(), width, rows * width, rows, width, 2.0 ** 10, strm), "split2")
        c = torch.empty(M, N, device=cuda)
        _lib.check(lib.pf_k_gemm_f16x2(a2.data_ptr(), lda, rows * width, w2.data_ptr(), k * 512, N * k * 512, 2.0 ** -22, None, None, 0,
                                       None, 0, c.data_ptr(), N, None, 0, 0, 1.0, M, N, k * 512, 0, 0, 0, None, strm), "gemm_f16x2")
        outs2.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs2[0], outs2[1])
    assert (outs2[0].double() - ref).abs().max().item() < 1e-3


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("precision,factor", [("fp32", 4), ("f16x2", 8)])
def test_against_reference_golden(cuda, golden, precision, factor):
    m, _ = _model(cuda, synth.emotion2vec_conf(), int(golden["seed"]), precision=precision)
    n = len(golden["lens"])
    wav = torch.cat([torch.from_numpy(golden[f"wav_{i}"]) for i in range(n)])
    fr, pooled, probs = m.forward_packed(wav, [int(v) for v in golden["lens"]])
    fr, pooled, probs = fr.cpu().double().numpy(), pooled.cpu().double().numpy(), probs.cpu().double().numpy()
    o = 0
    for i in range(n):
        r64 = golden[f"frames64_{i}"]
        T = r64.shape[0]
        for name, got in (("frames", fr[o: o + T]), ("pooled", pooled[i]), ("probs", probs[i])):
            r32, r64 = golden[f"{name}32_{i}"], golden[f"{name}64_{i}"]
            bar = factor * np.abs(r32 - r64).max() + 1e-6
            err = np.abs(got - r64).max()
            assert err <= bar, (precision, name, i, err, bar)
        o += T


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_against_float64_oracle_base_and_large(cuda, precision):
    """base shape (768, 12 heads, 4 + 8 blocks; 8 ALiBi heads of 12) on 1, 10 and 17.3 s; large (1024, 16 heads, 8 + 16) on 5 s. Bars from
    the float32 oracle's own gap on the same input; labels equal wherever the float64 top-2 gap exceeds 1e-4."""
    cases = [(synth.emotion2vec_conf(768, 12, 4, 8, num_alibi_heads=8), (16000, 160000, 276800)),
             (synth.emotion2vec_conf(1024, 16, 8, 16), (80000,))]
    for conf, lens in cases:
        m, sd = _model(cuda, conf, 3, precision=precision)
        cfg = O.cfg_of(m)
        waves = [_wav(n, i) for i, n in enumerate(lens)]
        fr, pooled, probs = m.forward_packed(torch.cat(waves), lens)
        o = 0
        for i, w in enumerate(waves):
            sdd = {k: v.to(cuda) for k, v in sd.items()}
            r64 = O.features(w.to(cuda), sdd, cfg, torch.float64)
            r32 = O.features(w.to(cuda), sdd, cfg, torch.float32).double()
            T = r64.shape[0]
            p64, q64 = O.head(r64, sdd, LABELS)
            p32, q32 = O.head(r32, sdd, LABELS)
            factor = 4 if precision == "fp32" else 8
            for name, got, a, b in (("frames", fr[o: o + T], r64, r32), ("pooled", pooled[i], p64, p32), ("probs", probs[i], q64, q32)):
                bar = factor * (b - a).abs().max().item() + 1e-6
                err = (got.double() - a).abs().max().item()
                assert err <= bar, (precision, conf["embed_dim"], lens[i], name, err, bar)
            top = torch.topk(q64, 2).values
            if (top[0] - top[1]).item() > 1e-4:
                assert int(probs[i].argmax()) == int(q64.argmax())
            o += T


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_batch_invariance_and_determinism(cuda, precision):
    m, _ = _model(cuda, synth.emotion2vec_conf(), 5, precision=precision)
    lens = [24000, 960000, 6400, 17000, 400, 81234, 48000, 33333]
    waves = [_wav(n, i) for i, n in enumerate(lens)]
    fr, pooled, probs = m.forward_packed(torch.cat(waves), lens)
    fr2, pooled2, probs2 = m.forward_packed(torch.cat(waves), lens)
    assert torch.equal(fr, fr2) and torch.equal(pooled, pooled2) and torch.equal(probs, probs2)
    T = [m.num_frames(n) for n in lens]
    o = sum(T[:3])
    f1, p1, q1 = m.forward_packed(waves[3], [lens[3]])
    assert torch.equal(f1, fr[o: o + T[3]]) and torch.equal(p1[0], pooled[3]) and torch.equal(q1[0], probs[3])
    m.set_max_samples(100000)                                   # sub-batches; the 60-s clip alone
    fr3, pooled3, probs3 = m.forward_packed(torch.cat(waves), lens)
    assert torch.equal(fr, fr3) and torch.equal(pooled, pooled3) and torch.equal(probs, probs3)


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_weights_replaced_on_a_live_handle(cuda, precision):
    """a second state dict loaded into a module that already ran: the positional conv weights, ALiBi scales, plane caches and
    exponents derived from the first one are all replaced -- the outputs are a fresh model's, bit for bit"""
    conf = synth.emotion2vec_conf(prenet_depth=1, depth=1)
    lens = [400, 6400]
    wav = torch.cat([_wav(n, i) for i, n in enumerate(lens)])
    m, _ = _model(cuda, conf, 5, precision=precision)
    m.forward_packed(wav, lens)
    m.load_state_dict(synth.emotion2vec_state_dict(6, m), strict=True)
    got = m.forward_packed(wav, lens)
    fresh, _ = _model(cuda, conf, 6, precision=precision)
    want = fresh.forward_packed(wav, lens)
    for x, y in zip(got, want):
        assert torch.equal(x, y)


def test_automodel_end_to_end(cuda, tmp_path):
    import yaml
    from funasr_amd.auto_model import AutoModel

    conf = synth.emotion2vec_conf()
    m = Emotion2vec(model_conf=conf, vocab_size=9)
    sd = synth.emotion2vec_state_dict(9, m)
    d = tmp_path / "e2v"
    d.mkdir()
    with open(d / "config.yaml", "w") as f:
        yaml.safe_dump({"model": "Emotion2vec", "model_conf": conf, "tokenizer": "CharTokenizer",
                        "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}, f)
    torch.save(sd, d / "model.pt")
    (d / "tokens.txt").write_text("\n".join(LABELS) + "\n")
    am = AutoModel(model=str(d), device="cuda:0", disable_update=True)
    lens = [16000, 7000, 40000, 12345, 20000]
    waves = [_wav(n, i).numpy() for i, n in enumerate(lens)]
    res = am.generate(waves, batch_size=4, granularity="utterance", key=[f"k{i}" for i in range(5)])
    assert len(res) == 5
    cfg = O.cfg_of(am.model)
    for i, r in enumerate(res):
        assert r["labels"] == LABELS[:-1] and len(r["scores"]) == 8 and abs(sum(r["scores"]) - 1) < 1e-5
        fr = O.features(torch.from_numpy(waves[i]), sd, cfg)
        p, q = O.head(fr, sd, LABELS)
        assert np.abs(np.array(r["scores"]) - q[:-1].numpy()).max() < 1e-4
        assert r["feats"].shape == (256,) and np.abs(r["feats"] - p.numpy()).max() < 1e-3
    res = am.generate(waves[:2], granularity="frame", extract_embedding=True)
    assert res[0]["feats"].shape == (am.model.num_frames(lens[0]), 256)
    res = am.generate(waves[:2], extract_embedding=False, output_dir=str(tmp_path / "out"))
    assert "feats" not in res[0]
    res = am.generate(waves[:1], output_dir=str(tmp_path / "out2"))
    saved = np.load(tmp_path / "out2" / f"{res[0]['key']}.npy")
    assert np.array_equal(saved, res[0]["feats"])
    with pytest.raises(ValueError, match="at least 400"):
        am.generate([np.zeros(300, np.float32)])
