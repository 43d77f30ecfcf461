"""ERes2NetV2 speaker embedding on the MI355X: the implicit-GEMM conv kernel one launch at a time against the float64 oracle conv,
the network against the reference's recorded tensors, batch invariance and determinism (bitwise), the edges, the waveform-chunk
path, inference, and the speaker branch of AutoModel.

Bars (the project's fp32 rules, DESIGN 3.4 / tests/test_transducer_gpu.py):
  * against recorded reference tensors: max |d| <= 4 x gap_<name> + 1e-6 (gap = the reference's own fp32 - fp64 distance on the same
    inputs, recorded in the golden) and cosine >= 1 - 1e-6 per embedding;
  * random-input kernel tests: 4 x max |oracle fp32 - oracle fp64| on the same inputs, floor 1e-7;
  * the network against the oracle where nothing is recorded (T = 9): 4 x max |oracle fp32 - oracle fp64| + 1e-6, CAM++'s rule."""
import os
import random

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import _lib, synth
from funasr_amd.auto_model import AutoModel
from funasr_amd.eres2net import ERes2NetV2SV

from . import _eres2net_oracle as O
from .test_vad_pipeline import _FakeASR, _FakePunc, _FakeVAD, _auto

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eres2net.npz")
TINY = synth.eres2net_conf()
NAN = float("nan")


def pad4(c):
    return (c + 3) // 4 * 4


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _model(cuda, seed, conf=TINY, **kw):
    m = ERes2NetV2SV(**conf, **kw)
    m.load_state_dict(synth.eres2net_state_dict(seed, m), strict=True)
    return m.to(cuda)


# ------------------------------------------------------------------------------------------------ one launch of the conv kernel
def _slice_buffer(data, col, extra, dev):
    """data [n, T, F, C] as the columns [col, col + C) of a buffer of row stride pad4(C) + col + extra whose every other float --
    the pad channels behind the slice included -- is NaN"""
    n, T, F, C = data.shape
    ld = col + pad4(C) + extra
    buf = torch.full((n, T, F, ld), NAN, dtype=torch.float32)
    buf[..., col:col + C] = data
    return buf.to(dev), ld


def _pack_w(w, w2=None):
    """[N, C, kF, kT] (+ the 1x1 [N, C2, 1, 1] of a K-concatenated operand) -> [N, K] tap-major, channels padded to 4 with zeros"""
    N, C, kF, kT = w.shape
    p = torch.zeros(N, kF * kT, pad4(C))
    p[:, :, :C] = w.permute(0, 2, 3, 1).reshape(N, kF * kT, C)
    p = p.reshape(N, -1)
    if w2 is not None:
        q = torch.zeros(N, pad4(w2.shape[1]))
        q[:, : w2.shape[1]] = w2[:, :, 0, 0]
        p = torch.cat([p, q], 1)
    return p.contiguous()


def _run_conv(dev, a, w, stride=(1, 1), a_col=0, c_col=0, c_extra=0, a2=None, mode=0, w2=None, stride2=(1, 1), a2_col=0, bias=None, r=None,
              act=0, xy=None):
    """one pf_k_eres_conv launch; returns (C slice [n, To, Fo, N], the whole C buffer)"""
    n, T, F, C = a.shape
    N, taps = w.shape[0], w.shape[2] * w.shape[3]
    To, Fo = (T - 1) // stride[0] + 1, (F - 1) // stride[1] + 1
    A, lda = _slice_buffer(a, a_col, 4, dev)
    W = _pack_w(w, w2).to(dev)
    ldc = c_col + N + c_extra
    Cb = torch.full((n, To, Fo, ldc), NAN, dtype=torch.float32, device=dev)
    A2, lda2, cin2, t2, f2 = None, 0, 0, 0, 0
    if a2 is not None:
        A2, lda2 = _slice_buffer(a2, a2_col, 0, dev)
        cin2, t2, f2 = a2.shape[3], a2.shape[1], a2.shape[2]
    dv = lambda t: None if t is None else t.to(dev).contiguous()                       # noqa: E731
    B, R = dv(bias), dv(r)
    X, Y = (dv(xy[0]), dv(xy[1])) if xy is not None else (None, None)
    ptr = lambda t: 0 if t is None else t.data_ptr()                                  # noqa: E731
    rc = _lib.load().pf_k_eres_conv(A.data_ptr(), lda, a_col, C, ptr(A2), lda2, a2_col, cin2, mode, t2, f2, stride2[0], stride2[1],
                                    W.data_ptr(), W.shape[1], ptr(B), ptr(R), N, ptr(X), N, ptr(Y), N, Cb.data_ptr(), ldc, c_col, n, T, F,
                                    taps, stride[0], stride[1], N, act, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "pf_k_eres_conv")
    torch.cuda.synchronize()
    full = Cb.cpu()
    return full[..., c_col:c_col + N], full


def _check(got, args, kwargs, what=""):
    """per chunk: against the float64 oracle conv of that chunk ALONE, within 4 x the oracle's own fp32 - fp64 distance (floor 1e-7)"""
    def one(i, dtype):
        a, w = args
        kw = dict(kwargs)
        for k in ("a2", "r"):                                    # per-chunk operands
            if kw.get(k) is not None:
                kw[k] = kw[k][i:i + 1].to(dtype)
        if kw.get("xy") is not None:
            kw["xy"] = tuple(u[i:i + 1].to(dtype) for u in kw["xy"])
        for k in ("w2", "bias"):                                 # weights
            if kw.get(k) is not None:
                kw[k] = kw[k].to(dtype)
        return O.conv_nhwc(a[i:i + 1].to(dtype), w.to(dtype), **kw)[0]
    for i in range(got.shape[0]):
        r64, r32 = one(i, torch.float64), one(i, torch.float32)
        bar = max(4 * (r32.double() - r64).abs().max().item(), 1e-7)
        err = (got[i].double() - r64).abs().max().item()
        print(f"{what} chunk {i}: err {err:.3e} bar {bar:.3e} max |ref| {r64.abs().max().item():.3e}")
        assert torch.isfinite(got[i]).all(), (what, i)
        assert err <= bar, (what, i, err, bar)


def _cases():
    """a covering set of 40: every value of every axis at least eight times, the pairings drawn by a fixed shuffle"""
    rnd = random.Random(7)
    axes = dict(taps=[1, 9], stride=[(1, 1), (2, 2)], cin=[1, 6, 13, 26, 52], N=[6, 13, 33, 130], ft=[(1, 1), (2, 3), (5, 9), (16, 37)],
                chunks=[1, 3])
    cols = {}
    for k, vals in axes.items():
        col = (vals * 40)[:40]
        rnd.shuffle(col)
        cols[k] = col
    return [tuple(cols[k][i] for k in axes) for i in range(40)]


@pytest.mark.parametrize("taps, stride, cin, N, ft, chunks", _cases())
def test_conv_kernel_against_float64_oracle(cuda, taps, stride, cin, N, ft, chunks):
    """M and N off every tile multiple (128 rows; 32 / 64 / 128 columns), K off the 32-wide K tile, A and C as column slices of
    wider buffers whose other columns hold NaN (and come back untouched), NaN pad channels, and with three chunks the neighbours
    1e3 times larger: every chunk must equal the oracle run on that chunk alone"""
    F, T = ft
    g = torch.Generator().manual_seed(1000 * cin + 10 * N + T + taps)
    a = torch.randn(chunks, T, F, cin, generator=g)
    if chunks == 3:
        a[0] *= 1e3
        a[2] *= 1e3
    k = 3 if taps == 9 else 1
    w = torch.randn(N, cin, k, k, generator=g) * (1.0 / (cin * taps)) ** 0.5
    a_col, c_col = 4 * (N % 3), N % 5
    got, full = _run_conv(cuda, a, w, stride=stride, a_col=a_col, c_col=c_col, c_extra=3)
    _check(got, (a, w), dict(stride=stride), f"taps {taps} stride {stride} cin {cin} N {N} FT {ft}")
    other = torch.ones(full.shape[-1], dtype=torch.bool)
    other[c_col:c_col + N] = False
    assert torch.isnan(full[..., other]).all()                   # the columns beside the C slice are untouched


def _inputs(seed, cin=13, N=33, F=5, T=9, n=2):
    g = torch.Generator().manual_seed(seed)
    return g, torch.randn(n, T, F, cin, generator=g), torch.randn(N, cin, 3, 3, generator=g) * (1.0 / (9 * cin)) ** 0.5


def test_epilogue_bias_and_residual(cuda):
    g, a, w = _inputs(1)
    bias = torch.randn(33, generator=g)
    r = torch.randn(2, 9, 5, 33, generator=g)
    got, _ = _run_conv(cuda, a, w, bias=bias)
    _check(got, (a, w), dict(bias=bias), "bias")
    got, _ = _run_conv(cuda, a, w, r=r)
    _check(got, (a, w), dict(r=r), "residual")
    got, _ = _run_conv(cuda, a, w, bias=bias, r=r)
    _check(got, (a, w), dict(bias=bias, r=r), "bias + residual")


@pytest.mark.parametrize("act", [1, 2, 3])
def test_epilogue_activations(cuda, act):
    """inputs scaled so that the pre-activation values land below 0, inside (0, 20) and above 20"""
    g, a, w = _inputs(2)
    a = a * 25.0
    pre = O.conv_nhwc(a.double(), w.double())
    assert (pre < 0).float().mean() > 0.2 and ((pre > 0) & (pre < 20)).float().mean() > 0.2 and (pre > 20).float().mean() > 0.05
    got, _ = _run_conv(cuda, a, w, act=act)
    _check(got, (a, w), dict(act_id=act), f"act {act}")
    if act == 2:
        assert got.max().item() == 20.0 and got.min().item() == 0.0


def test_summed_second_operand(cuda):
    g, a, w = _inputs(3)
    a2 = torch.randn(a.shape, generator=g)
    got, _ = _run_conv(cuda, a, w, a2=a2, mode=1, a2_col=8)
    _check(got, (a, w), dict(a2=a2, mode=1), "sum")


def test_concatenated_second_operand(cuda):
    """cat(x, y) of AFF's first conv (1x1 on both), and the stride-2 projection shortcut of a larger map inside a 3x3 product"""
    g, a, w = _inputs(4)
    w1 = torch.randn(33, 13, 1, 1, generator=g) * 13 ** -0.5
    y = torch.randn(2, 9, 5, 6, generator=g)
    w2 = torch.randn(33, 6, 1, 1, generator=g) * 6 ** -0.5
    got, _ = _run_conv(cuda, a, w1, a2=y, mode=2, w2=w2, a2_col=4)
    _check(got, (a, w1), dict(a2=y, mode=2, w2=w2), "concat 1x1")
    big = torch.randn(2, 17, 10, 26, generator=g)
    w3 = torch.randn(33, 26, 1, 1, generator=g) * 26 ** -0.5
    got, _ = _run_conv(cuda, a, w, a2=big, mode=2, w2=w3, stride2=(2, 2), act=2)
    _check(got, (a, w), dict(a2=big, mode=2, w2=w3, stride2=(2, 2), act_id=2), "concat stride-2 shortcut")


def test_aff_combine(cuda):
    g, a, w = _inputs(5)
    bias = torch.randn(33, generator=g)
    x, y = torch.randn(2, 9, 5, 33, generator=g) * 5, torch.randn(2, 9, 5, 33, generator=g) * 5
    got, _ = _run_conv(cuda, a * 2, w, bias=bias, xy=(x, y))
    _check(got, (a * 2, w), dict(bias=bias, xy=(x, y)), "AFF combine")


# ------------------------------------------------------------------------------------------------ the network
def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def test_network_against_reference_golden(cuda, golden):
    """every recorded stage of chunk 1 inside the batch of 3, the pooled statistics and the embeddings of all three"""
    m = _model(cuda, int(golden["seed"]))
    got = m.forward_stages(torch.from_numpy(golden["x"]).to(cuda))
    for name in O.STAGES:
        if name in ("stats", "emb"):
            out, ref = got[name].cpu().double().numpy(), golden[name]
            if name == "stats":                                  # the layout's (f, c) column order -> the reference's (c, f)
                B, C, F4 = out.shape[0], 16 * TINY["m_channels"], TINY["feat_dim"] // 8
                out = out.reshape(B, 2, F4, C).transpose(0, 1, 3, 2).reshape(B, -1)
        else:
            out, ref = got[name][1].permute(2, 1, 0).cpu().double().numpy(), golden[f"{name}_c1"]      # [t, f, c] -> [c, f, t]
        assert out.shape == ref.shape, name
        bar = 4 * float(golden[f"gap_{name}"]) + 1e-6
        err = np.abs(out - ref).max()
        print(f"{name}: err {err:.3e} bar {bar:.3e} max |ref| {np.abs(ref).max():.3e}")
        assert err <= bar, (name, err, bar)
    assert _cos(got["emb"].cpu().double().numpy(), golden["emb"]).min() >= 1 - 1e-6
    assert torch.equal(m(torch.from_numpy(golden["x"]).to(cuda)), got["emb"])


def test_determinism_and_sub_batching(cuda, golden):
    m = _model(cuda, 4)
    x = torch.from_numpy(golden["x"]).to(cuda)
    full = m(x)
    assert torch.equal(m(x[1:2].contiguous()), full[1:2])       # chunk 1 alone = chunk 1 inside the batch of 3
    m.set_max_batch(1)
    one = m(x)
    m.set_max_batch(256)
    assert torch.equal(one, full) and torch.equal(m(x), full)
    m.debug_poison()                                             # NaN in every workspace buffer between two forwards
    assert torch.equal(m(x), full)
    assert torch.isfinite(full).all()


def test_weights_replaced_on_a_live_handle(cuda, golden):
    x = torch.from_numpy(golden["x"]).to(cuda)
    m = _model(cuda, 4)
    m(x)
    m.load_state_dict(synth.eres2net_state_dict(1, m), strict=True)
    assert torch.equal(m(x), _model(cuda, 1)(x))


def test_smallest_input_and_refusals(cuda):
    sd = synth.eres2net_state_dict(6, ERes2NetV2SV(**TINY))
    m = _model(cuda, 6)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 9, TINY["feat_dim"], generator=g) * 2
    out = m(x.to(cuda)).cpu().double()
    ref, ref32 = O.forward(x, sd), O.forward(x, sd, torch.float32).double()
    bar = 4 * (ref32 - ref).abs().max().item() + 1e-6
    assert (out - ref).abs().max().item() <= bar
    assert torch.nn.functional.cosine_similarity(out, ref, dim=-1).min().item() >= 1 - 1e-6
    with pytest.raises(ValueError, match="standard deviation"):
        m(torch.zeros(1, 8, TINY["feat_dim"], device=cuda))
    with pytest.raises(ValueError, match="standard deviation"):
        m.embed_chunks(torch.zeros(16000, device=cuda), [0], 400 + 7 * 160)
    with pytest.raises(ValueError, match="25-ms"):
        m.embed_chunks(torch.zeros(16000, device=cuda), [0], 399)
    with pytest.raises(ValueError, match="25-ms"):
        m.fbank(torch.zeros(399, device=cuda))
    assert tuple(m.embed_chunks(torch.zeros(16000, device=cuda), [], 2400).shape) == (0, TINY["embedding_size"])
    lib, h = m._ensure_handle()
    assert lib.pf_eres2net_forward(h, x.to(cuda).data_ptr(), 1, 8, out.data_ptr(), 0) != 0       # the library refuses it too
    assert "T >= 9" in _lib.last_error()


def test_embed_chunks_equals_fbank_then_forward(cuda):
    """chunks of 2400 samples (13 frames), overlapping starts, a last chunk shorter than the window. NOT bitwise: the library removes
    the time mean with one running sum per bin, `fbank` with torch's mean, so the features differ by a rounding of the mean (1e-7
    relative) before the network; CAM++'s bar for the same comparison, 1e-4 of the largest embedding value, holds here. A chunk
    alone and inside the batch IS bitwise the same."""
    m = _model(cuda, 6)
    wav = synth.speech_like(16000, seed=3).to(cuda) * 0.3
    L = 2400
    starts = [0, 1200, 2000, 7000, 13000]
    valid = [L, L, L, L, 1100]
    emb = m.embed_chunks(wav, starts, L, valid)
    chunks = []
    for s, v in zip(starts, valid):
        c = torch.zeros(L, device=cuda)
        c[:v] = wav[s:s + v]
        chunks.append(c)
    feats = torch.stack([m.fbank(c) for c in chunks])
    assert feats.shape[1] == 13
    ref = m(feats)
    err, top = (emb - ref).abs().max().item(), ref.abs().max().item()
    print(f"embed_chunks vs fbank -> forward: {err:.3e} of {top:.3e}")
    assert err <= 1e-4 * top
    assert torch.equal(m.embed_chunks(wav, starts[4:5], L, valid[4:5]), emb[4:5])


def test_inference_on_the_ragged_pair(cuda, golden):
    """two waveforms of unequal length at 80 bins. The network on the RECORDED features meets the recorded-tensor bar; the module's own
    features meet the fbank kernel's documented distance to kaldi-native-fbank (2e-3, tests/test_campplus_gpu.py); inference()
    equals the float64 oracle on the module's own features within the same network bar, and the recorded embeddings by cosine."""
    conf = dict(TINY, feat_dim=80)
    seed = int(golden["ragged_seed"])
    m = _model(cuda, seed, conf)
    ref, gap = golden["ragged_emb"], float(golden["gap_ragged"])
    out = m(torch.from_numpy(golden["ragged_x"]).to(cuda)).cpu().double().numpy()
    assert np.abs(out - ref).max() <= 4 * gap + 1e-6
    assert _cos(out, ref).min() >= 1 - 1e-6
    wavs = [golden["ragged_wav0"], golden["ragged_wav1"]]
    res, meta = m.inference(wavs)
    emb = res[0]["spk_embedding"]
    assert tuple(emb.shape) == (2, conf["embedding_size"]) and "batch_data_time" in meta
    feats = [m.fbank(torch.from_numpy(w).to(cuda)).cpu() for w in wavs]
    x = torch.zeros(2, max(f.shape[0] for f in feats), 80)
    for i, f in enumerate(feats):
        x[i, : f.shape[0]] = f
    assert x.shape == golden["ragged_x"].shape
    assert (x - torch.from_numpy(golden["ragged_x"])).abs().max().item() < 2e-3
    own = O.forward(x, synth.eres2net_state_dict(seed, m)).numpy()
    err = np.abs(emb.cpu().double().numpy() - own).max()
    print(f"inference vs oracle on own features: {err:.3e}; vs recorded: {np.abs(emb.cpu().double().numpy() - ref).max():.3e}")
    assert err <= 4 * gap + 1e-6
    assert _cos(emb.cpu().double().numpy(), ref).min() >= 1 - 1e-6        # and the recorded embeddings, by the project's cosine bar


# ------------------------------------------------------------------------------------------------ AutoModel
SEGS = [[500, 4200], [4600, 5300], [5800, 11500], [12100, 13000], [13500, 21000], [21300, 27900]]
VOICE = [0, 1, 1, 0, 1, 0]


@pytest.fixture(scope="module")
def spk_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("eres2netv2"))
    with open(os.path.join(d, "config.yaml"), "w") as f:
        yaml.safe_dump({"model": "ERes2NetV2", "model_conf": dict(TINY)}, f)
    torch.save(synth.eres2net_state_dict(12, ERes2NetV2SV(**TINY)), os.path.join(d, "model.pt"))
    return d


def test_auto_model_generate_returns_the_embedding(cuda, spk_dir):
    am = AutoModel(model=spk_dir, device="cuda:0")
    wav = synth.speech_like(16000, seed=5) * 0.3
    out = am.generate(wav)[0]
    assert tuple(out["spk_embedding"].shape) == (1, TINY["embedding_size"])
    ref = am.model(am.model.fbank(wav.to(cuda))[None])
    assert torch.equal(out["spk_embedding"].to(cuda), ref)


def test_long_form_recipe_with_spk_model_directory(cuda, spk_dir):
    """AutoModel(..., spk_model=<dir>) builds the module; the VAD + ASR + punctuation + speaker recipe (the synthetic VAD, ASR and
    punctuation models of the existing pipeline tests) labels every sentence with an integer speaker"""
    am = AutoModel(model=spk_dir, spk_model=spk_dir, device="cuda:0")
    assert isinstance(am.spk_model, ERes2NetV2SV) and am.spk_model is not am.model
    spk_model, spk_kwargs = am.spk_model, am.spk_kwargs
    am = _auto(_FakeVAD([SEGS]), _FakeASR(), batch_size_s=300)
    am.punc_model, am.punc_kwargs = _FakePunc(), {}
    am.spk_model, am.spk_kwargs, am.cb_kwargs, am.spk_mode = spk_model, spk_kwargs, {}, "punc_segment"
    wav = torch.zeros(29 * 16000)
    for (b, e), v in zip(SEGS, VOICE):
        s0, s1 = b * 16, e * 16
        x = synth.speech_like(s1 - s0, seed=100 + v)
        wav[s0:s1] = x * (0.3 if v == 0 else 0.08) * (1 + v * torch.sin(torch.arange(s1 - s0) / 3.0))
    out = am.generate(wav, preset_spk_num=2)[0]
    info = out["sentence_info"]
    assert info and all(isinstance(s["spk"], int) for s in info)
    assert {s["spk"] for s in info} <= {0, 1}
