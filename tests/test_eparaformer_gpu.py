"""E-Paraformer on the MI355X through the C ABI: the three predictor kernels against the float64 oracle on random inputs at their
edges, the one-pass decoder handle, the model against the reference's recorded float64 outputs in both precision modes (single clips,
the ragged batch, the batch with a zero-token clip), the `inference` records, bitwise repeats, the live handle, AutoModel end to end
and the recipe's size.

Bars: 4 x (fp32) / 8 x (f16x2) the reference's own fp32 - fp64 gap stored beside the recorded outputs; where no recorded gap exists
(random-input kernel tests, the recipe-size run) 4 x (8 x) max |oracle fp32 - oracle fp64| on the same input -- another valid fp32
summation order may be that far off."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import _lib, synth
from funasr_amd.e_paraformer import EParaformer

from . import _eparaformer_oracle as O
from ._model_dir import write_wav
from .test_eparaformer import RUNS, golden_model, load_golden, pin_positional_rows

pytestmark = pytest.mark.gpu
FACTOR = {"fp32": 4.0, "f16x2": 8.0}
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _maxd(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _check(tag, got, want64, gap, factor):
    d = _maxd(got, want64)
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / max(gap, 1e-30):.2f} (bar {factor:g})")
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), tag
    assert d <= factor * gap, (tag, d, gap)


def _sum_gap(t32, t64):
    """the gap of a per-clip SUM (B numbers): max |oracle fp32 - oracle fp64|, but no less than one fp32 ulp of the largest sum. A handful
    of numbers can agree with their float64 values to a fraction of an ulp by chance (the oracle's fp32 sum happens to be the correctly
    rounded one), and 4 x such a gap is a bar below the spacing of the format the result is stored in."""
    return max(_maxd(t32, t64), float(np.spacing(np.float32(float(torch.as_tensor(t64).abs().max())))))


def _i32(cuda, vals):
    return torch.tensor([int(v) for v in vals], dtype=torch.int32, device=cuda)


# ------------------------------------------------------------------------------------------------ pif_alphas
def _alpha_params(D, lo, ro, seed):
    g = torch.Generator().manual_seed(seed)
    taps = lo + ro + 1
    return [torch.randn(D, 1, taps, generator=g) / taps ** 0.5, 0.1 * torch.randn(D, generator=g), torch.randn(D, generator=g) / D ** 0.5,
            torch.tensor([-0.5])]


def _alphas(cuda, h, lens, p, lo, ro):
    B, T, D = h.shape
    dev = [t.contiguous().to(cuda) for t in p]
    a = torch.full((B, T), NAN, device=cuda)
    tn = torch.full((B,), NAN, device=cuda)
    hd, ld = h.contiguous().to(cuda), _i32(cuda, lens)             # (named: a temporary's block would be reused by the next allocation)
    _lib.check(_lib.load().pf_k_pif_alphas(hd.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                           ld.data_ptr(), B, T, D, lo, ro, 1.0, 0.0, a.data_ptr(), tn.data_ptr(), _stream()), "pf_k_pif_alphas")
    torch.cuda.synchronize()
    return a.cpu(), tn.cpu()


@pytest.mark.parametrize("lo,ro", [(0, 0), (1, 1), (3, 0), (0, 15)])
@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("T", [1, 2, 61, 64, 65, 300])
def test_pif_alphas_against_the_oracle(cuda, T, D, lo, ro):
    """T shorter than the halo, around the 64-lane and 256-thread strides of the two launches; three clips of lengths T, T / 2 and 0;
    masked frames are exactly 0; the sums repeat bit for bit"""
    lens = [T, T // 2, 0]
    h = torch.randn(3, T, D, generator=torch.Generator().manual_seed(100 * T + D + lo))
    p = _alpha_params(D, lo, ro, T + ro)
    a, tn = _alphas(cuda, h, lens, p, lo, ro)
    a64, t64 = O.pif_alphas(h.double(), lens, *[t.double() for t in p], lo, ro)
    a32, t32 = O.pif_alphas(h, lens, *p, lo, ro)
    _check(f"alphas T={T} D={D} orders ({lo}, {ro})", a, a64, _maxd(a32, a64), 4.0)
    _check(f"token_num T={T} D={D} orders ({lo}, {ro})", tn, t64, _sum_gap(t32, t64), 4.0)
    for b, n in enumerate(lens):
        assert bool((a[b, n:] == 0).all()), b
    assert float(tn[2]) == 0.0
    a2, tn2 = _alphas(cuda, h, lens, p, lo, ro)
    assert torch.equal(a, a2) and torch.equal(tn, tn2)


@pytest.mark.parametrize("T,lo,ro", [(5, 0, 15), (33, 3, 0), (64, 1, 1)])
def test_pif_alphas_do_not_read_across_the_clip_boundary(cuda, T, lo, ro):
    """clip 0 keeps its bits whether its neighbours hold 1e6 or noise: the conv's halo rows are the clip's own padded rows or zeros"""
    D = 128
    g = torch.Generator().manual_seed(T)
    h = torch.randn(3, T, D, generator=g)
    p = _alpha_params(D, lo, ro, 7)
    lens = [T, T, T]
    a, tn = _alphas(cuda, h, lens, p, lo, ro)
    big = h.clone()
    big[0], big[2] = 1e6, -1e6
    b_, tb = _alphas(cuda, big, lens, p, lo, ro)
    assert torch.equal(a[1], b_[1]) and torch.equal(tn[1], tb[1])
    alone, ta = _alphas(cuda, h[1:2], [T], p, lo, ro)
    assert torch.equal(a[1], alone[0]) and torch.equal(tn[1], ta[0])


# ------------------------------------------------------------------------------------------------ pif_align
@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000, 5000])
def test_pif_align_prefix_sums(cuda, T):
    """counts 0, 1 and 200 and a clip whose alphas are all zero; the prefix sums against the float64 cumsum"""
    g = torch.Generator().manual_seed(T)
    a = 0.4 * torch.rand(4, T, generator=g)
    a[3] = 0
    tn = a.sum(-1)
    counts = [200, 1, 0, 5]
    ad, td, cd = a.to(cuda), tn.to(cuda), _i32(cuda, counts)
    an = torch.full((4, T), NAN, device=cuda)
    al = torch.full((4, T), NAN, device=cuda)
    _lib.check(_lib.load().pf_k_pif_align(ad.data_ptr(), td.data_ptr(), cd.data_ptr(), 4, T, an.data_ptr(), al.data_ptr(), _stream()),
               "pf_k_pif_align")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(an).all()) and bool(torch.isfinite(al).all())
    n64, c64 = O.pif_align(a.double(), tn.double(), counts)
    n32, c32 = O.pif_align(a, tn, counts)
    _check(f"normalised alphas T={T}", an, n64, _maxd(n32, n64), 4.0)
    _check(f"align T={T}", al, c64, _maxd(c32, c64), 4.0)
    for b in (2, 3):                                               # count 0, and token_num == 0 with a count: all zeros, no division
        assert float(an[b].abs().max()) == 0.0 and float(al[b].abs().max()) == 0.0
    # in place gives the same bits
    _lib.check(_lib.load().pf_k_pif_align(ad.data_ptr(), td.data_ptr(), cd.data_ptr(), 4, T, ad.data_ptr(), al.data_ptr(), _stream()),
               "pf_k_pif_align")
    torch.cuda.synchronize()
    assert torch.equal(ad, an)


# ------------------------------------------------------------------------------------------------ pif_embed
def _embed_case(T, L, D, H, seed, flip=False):
    g = torch.Generator().manual_seed(seed)
    lens = [T, max(T // 2, 1), 0]
    counts = [L, max(L // 2, 1), 0]
    h = torch.randn(3, T, D, generator=g)
    a = 0.05 + 0.4 * torch.rand(3, T, generator=g)
    a = a * (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])
    _, align = O.pif_align(a, a.sum(-1), counts)
    sigma = torch.linspace(0.05, 4.0, H) if H > 1 else torch.tensor([4.0 if flip else 0.05])
    if flip:
        sigma = sigma.flip(0)
    return h, align, sigma.contiguous(), lens


def _embed(cuda, h, align, sigma, lens, L, H):
    B, T, D = h.shape
    out = torch.full((B, L, D), NAN, device=cuda)
    ad, hd, sd, ld = align.contiguous().to(cuda), h.contiguous().to(cuda), sigma.to(cuda), _i32(cuda, lens)
    _lib.check(_lib.load().pf_k_pif_embed(ad.data_ptr(), hd.data_ptr(), sd.data_ptr(), ld.data_ptr(), B, T, L, D, H, out.data_ptr(), _stream()),
               "pf_k_pif_embed")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("D,H", [(256, 1), (256, 2), (256, 4), (256, 8), (128, 4)])
@pytest.mark.parametrize("T,L", [(1, 1), (7, 1), (61, 18), (65, 33), (300, 64)])
def test_pif_embed_against_the_oracle(cuda, T, L, D, H, flip):
    """one frame, fewer frames than a chunk, around the 64-frame chunk and the 16-position tile, several chunks; head widths 256 .. 32;
    sigmas from 0.05 (nearly uniform weights) to 4.0 (one-frame-sharp: far scores underflow to 0); a clip without frames gives zero
    rows; the rows at or past a clip's own count are the oracle's too (every clip gets all L rows); the padding rows of h hold NaN in a
    second run and nothing changes"""
    h, align, sigma, lens = _embed_case(T, L, D, H, 31 * T + L + H, flip)
    got = _embed(cuda, h, align, sigma, lens, L, H)
    assert bool(torch.isfinite(got).all())
    e64 = O.pif_embed(align.double(), h.double(), sigma.double(), lens, L)
    e32 = O.pif_embed(align, h, sigma, lens, L)
    _check(f"embed T={T} L={L} D={D} H={H} flip {flip}", got, e64, _maxd(e32, e64), 4.0)
    assert float(got[2].abs().max()) == 0.0
    poisoned, pal = h.clone(), align.clone()
    for b, n in enumerate(lens):
        poisoned[b, n:] = NAN
        pal[b, n:] = NAN
    assert torch.equal(_embed(cuda, poisoned, pal, sigma, lens, L, H), got)


def test_pif_kernels_refuse_out_of_range_arguments(cuda):
    lib = _lib.load()
    t = torch.zeros(1 << 16, device=cuda)
    i = torch.ones(4, dtype=torch.int32, device=cuda)
    p, q = t.data_ptr(), i.data_ptr()
    assert lib.pf_k_pif_embed(p, p, p, q, 1, 4, 2, 96, 2, p, _stream()) != 0 and "pif_embed" in _lib.last_error()        # D / H = 48
    assert lib.pf_k_pif_embed(p, p, p, q, 1, 4, 2, 288, 9, p, _stream()) != 0                                            # 9 heads
    assert lib.pf_k_pif_embed(p, p, p, q, 1, 4, 2049, 128, 4, p, _stream()) != 0
    assert lib.pf_k_pif_embed(p, p, p, q, 1, 5001, 2, 128, 4, p, _stream()) != 0
    assert lib.pf_k_pif_alphas(p, p, p, p, p, q, 1, 4, 128, 16, 0, 1.0, 0.0, p, p, _stream()) != 0 and "pif_alphas" in _lib.last_error()
    assert lib.pf_k_pif_alphas(p, p, p, p, p, q, 1, 4, 128, 0, 16, 1.0, 0.0, p, p, _stream()) != 0
    assert lib.pf_k_pif_alphas(p, p, p, p, p, q, 1, 4, 1056, 1, 1, 1.0, 0.0, p, p, _stream()) != 0
    assert lib.pf_k_pif_align(p, p, q, 1, 5001, p, p, _stream()) != 0 and "pif_align" in _lib.last_error()
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0                                                                                   # nothing was launched
    for cfg in ((96, 1, 1, 2), (288, 1, 1, 9), (128, 16, 1, 4), (128, 1, 16, 4)):
        c = _lib.pf_pif_config(*cfg, 1.0, 1.0, 0.0)
        assert not lib.pf_pif_create(_lib.C.byref(c)) and "pif: unsupported config" in _lib.last_error()
    c = _lib.pf_sandecoder_config(128, 4, 256, 2, 40, 3, 1e-12)                                                          # head dim 32
    assert not lib.pf_sandecoder_create(_lib.C.byref(c)) and "sandecoder: unsupported config" in _lib.last_error()
    c = _lib.pf_sandecoder_config(128, 2, 256, 2, 40, 1, 1e-12)                                                          # a bf16 mode
    assert not lib.pf_sandecoder_create(_lib.C.byref(c))


# ------------------------------------------------------------------------------------------------ the model's fixtures
@pytest.fixture(scope="module")
def model(cuda):
    m, sd, conf = golden_model()
    if pin_positional_rows(m, load_golden()):
        print("this host's float32 exp() builds another positional table than the recording's: recorded rows pinned")
    return m.to(cuda), sd, conf


# ------------------------------------------------------------------------------------------------ pf_sandecoder
@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_sandecoder_against_the_oracle_and_a_zero_token_clip_beside_the_others(cuda, model, mode):
    """B = 3, token lengths [18, 12, 0], memory lengths [61, 41, 5]: the valid rows against the float64 oracle; the clip without tokens
    (no self-attention key) leaves finite rows and does not move the others by a bit"""
    m, sd, conf = model
    m.set_precision(mode)
    g = torch.Generator().manual_seed(9)
    mem, emb = torch.randn(3, 61, 128, generator=g), 0.7 * torch.randn(3, 18, 128, generator=g)
    tl, ml = [18, 12, 0], [61, 41, 5]
    logp, ids, best = m.decoder.decode(mem.to(cuda), ml, emb.to(cuda), tl)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logp).all()) and bool(torch.isfinite(best).all())
    l64 = O.decoder(O.cast(sd), conf["decoder_conf"], mem.double(), ml, emb.double(), tl)
    l32 = O.decoder(O.cast(sd, torch.float32), conf["decoder_conf"], mem, ml, emb, tl)
    for b, n in enumerate(tl[:2]):
        _check(f"sandecoder {mode} clip {b}", logp[b, :n], l64[b, :n], _maxd(l32[b, :n], l64[b, :n]), FACTOR[mode])
        assert ids[b, :n].tolist() == l64[b, :n].argmax(-1).tolist()
    assert torch.equal(ids.long(), logp.argmax(-1)) and torch.equal(best, logp.max(-1).values)
    two, ids2, _ = m.decoder.decode(mem[:2].to(cuda), ml[:2], emb[:2].to(cuda), tl[:2])
    assert torch.equal(two, logp[:2]) and torch.equal(ids2, ids[:2])
    _, ids3, best3 = m.decoder.decode(mem.to(cuda), ml, emb.to(cuda), tl, want_logp=False)
    assert torch.equal(ids3, ids) and torch.equal(best3, best)


# ------------------------------------------------------------------------------------------------ model against the golden
def _run_model(m, g, cuda):
    feats, lens = torch.from_numpy(g["feats"]).to(cuda), g["lens"].tolist()
    enc, olens = m.encode(feats, lens)
    emb, tn, alphas, peak, align = m.predictor(enc, lengths=olens, return_align=True)
    counts = [int(v) for v in tn.cpu().round().tolist()]
    logp = m.cal_decoder_with_predictor(enc, olens, emb, counts)[0] if max(counts) > 0 else None
    return dict(enc=enc, olens=olens.tolist(), embeds=emb, token_num=tn, alphas=alphas, align=align, counts=counts, logp=logp, peak=peak)


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("run", RUNS)
def test_model_against_the_references_recorded_outputs(cuda, model, run, mode):
    """single clips, the ragged batch (the shorter clip gets the reference's BATCHED rows: unmasked conv, batch-wide Lmax) and the batch
    with a zero-token clip. token_num, alphas, align, embeds (all Lmax rows) and the log-probabilities of every clip's own rows within
    the bars; counts and greedy ids equal."""
    m, sd, conf = model
    m.set_precision(mode)
    g = load_golden(run)
    r = _run_model(m, g, cuda)
    assert r["olens"] == g["olens"].tolist() and r["counts"] == g["counts"].tolist() and r["peak"] is None
    f = FACTOR[mode]
    for k in ("enc", "token_num", "alphas", "align", "embeds"):
        _check(f"{run} {mode} {k}", r[k], g[k], float(g["gap_" + k]), f)
    for b, n in enumerate(r["counts"]):
        if n > 0:
            _check(f"{run} {mode} logp clip {b}", r["logp"][b, :n], g["logp"][b, :n], float(g["gap_logp"]), f)
        assert r["logp"][b, :n].argmax(-1).tolist() == g[f"ids_{b}"].tolist()
        assert bool((r["alphas"][b, r["olens"][b]:] == 0).all())
    if run == "b":
        n0 = int(load_golden("s0")["counts"][0])
        assert _maxd(r["embeds"][0, :n0], load_golden("s0")["embeds"][0, :n0]) > 100 * float(g["gap_embeds"])    # ... not the clip's rows alone


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_inference_records_equal_the_references(cuda, model, mode, tmp_path):
    """text with a CharTokenizer, token_int without a tokenizer; the zero-token clip of `z` gets its empty record"""
    from funasr_amd.tokenizer import CharTokenizer

    m, sd, conf = model
    m.set_precision(mode)
    tok = CharTokenizer(token_list=load_golden()["tokens"].tolist(), unk_symbol="<unk>", split_with_space=True)
    for run in RUNS:
        g = load_golden(run)
        feats, lens = torch.from_numpy(g["feats"]), g["lens"].tolist()
        keys = [f"utt{b}" for b in range(len(lens))]
        res, _ = m.inference(feats, data_lengths=lens, key=keys, tokenizer=tok, data_type="fbank", device="cuda")
        assert res == [{"key": k, "text": t} for k, t in zip(keys, g["texts"].tolist())], run
        res, _ = m.inference(feats, data_lengths=lens, key=keys, tokenizer=None, data_type="fbank", device="cuda")
        assert res == [{"key": k, "token_int": g[f"token_int_{b}"].tolist()} for b, k in enumerate(keys)], run
    g = load_golden("b")
    m.__dict__.pop("writer", None)               # (the writer is made once per model, as the reference's: not this test's directory then)
    res, _ = m.inference(torch.from_numpy(g["feats"]), data_lengths=g["lens"].tolist(), key=["u0", "u1"], tokenizer=tok, data_type="fbank",
                         device="cuda", output_dir=str(tmp_path))
    lines = open(os.path.join(str(tmp_path), "1best_recog", "text"), encoding="utf-8").read().splitlines()
    assert lines == [f"{r['key']} {r['text']}" for r in res] and [r["text"] for r in res] == g["texts"].tolist()


def test_a_batch_without_any_token_returns_one_empty_record_per_key(cuda, model):
    from funasr_amd.tokenizer import CharTokenizer

    m, sd, conf = model
    tok = CharTokenizer(token_list=load_golden()["tokens"].tolist(), unk_symbol="<unk>", split_with_space=True)
    feats = torch.zeros(2, 9, 80)
    feats[:, :3] = torch.from_numpy(load_golden("z")["feats"])[1, :3]
    res, _ = m.inference(feats, data_lengths=[3, 3], key=["a", "b"], tokenizer=tok, data_type="fbank", device="cuda")
    assert res == [{"key": "a", "text": ""}, {"key": "b", "text": ""}]
    emb, tn, alphas, peak = m.calc_predictor(*m.encode(feats.to(cuda), [3, 3]))
    assert emb.shape == (2, 0, 128) and float(alphas.abs().max()) == 0.0 and float(tn.max()) < 0.5 and peak is None


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_bitwise_repeat_and_equal_length_batch(cuda, model, mode):
    m, sd, conf = model
    m.set_precision(mode)
    clips = torch.randn(2, 141, 80, generator=torch.Generator().manual_seed(4))
    clips = torch.stack([clips[0], clips[0]]).to(cuda)
    g = {"feats": clips.cpu().numpy(), "lens": np.asarray([141, 141])}
    a, b = _run_model(m, g, cuda), _run_model(m, g, cuda)
    solo = _run_model(m, {"feats": clips[:1].cpu().numpy(), "lens": np.asarray([141])}, cuda)
    assert a["counts"] == b["counts"] and a["counts"][0] == a["counts"][1] == solo["counts"][0] > 0
    for k in ("enc", "token_num", "alphas", "align", "embeds", "logp"):
        assert torch.equal(a[k], b[k]), k
        for i in range(2):
            assert torch.equal(a[k][i], solo[k][0]), (k, i)


def test_weights_and_precision_replaced_on_a_live_handle(cuda):
    """one model through load_state_dict and set_precision: every result equals a fresh model's with the same weights and mode"""
    conf = synth.eparaformer_conf(enc_blocks=1, dec_blocks=1)
    feats = torch.randn(1, 123, 80, generator=torch.Generator().manual_seed(0)).to(cuda)

    def fresh(seed, mode):
        m = EParaformer(**conf)
        m.load_state_dict(synth.eparaformer_state_dict(seed, m), strict=True)
        return m.to(cuda).set_precision(mode)

    def out(m):
        r = _run_model(m, {"feats": feats.cpu().numpy(), "lens": np.asarray([123])}, cuda)
        assert r["counts"][0] > 0
        return r

    a = fresh(1, "f16x2")
    out(a)
    a.load_state_dict(synth.eparaformer_state_dict(2, a), strict=True)
    want_x2, want_32 = out(fresh(2, "f16x2")), out(fresh(2, "fp32"))
    got = out(a)
    assert all(torch.equal(got[k], want_x2[k]) for k in ("embeds", "alphas", "logp"))
    got = out(a.set_precision("fp32"))
    assert all(torch.equal(got[k], want_32[k]) for k in ("embeds", "alphas", "logp")) and not torch.equal(want_32["logp"], want_x2["logp"])
    got = out(a.set_precision("f16x2"))
    assert torch.equal(got["logp"], want_x2["logp"])
    lib = _lib.load()
    one = torch.zeros(1, device=cuda)
    assert lib.pf_sandecoder_set_tensor(a.decoder._handle, b"embed.0.weight", one.data_ptr(), 1) != 0 and "unknown tensor name" in _lib.last_error()
    assert lib.pf_pif_set_tensor(a.predictor._handle, b"cif_conv1d.weight", one.data_ptr(), 1) != 0           # wrong element count
    assert lib.pf_sandecoder_missing(a.decoder._handle) == 0 and lib.pf_pif_missing(a.predictor._handle) == 0
    assert torch.equal(out(a)["logp"], want_x2["logp"])


# ------------------------------------------------------------------------------------------------ AutoModel
def _model_dir(path, seed=31):
    os.makedirs(path, exist_ok=True)
    tokens = load_golden()["tokens"].tolist()
    c = synth.eparaformer_conf(vocab=len(tokens))
    conf = {"model": "EParaformer", "model_conf": {k: c[k] for k in ("ctc_weight", "lsm_weight", "length_normalized_loss", "predictor_weight",
                                                                     "predictor_bias", "sampling_ratio", "use_1st_decoder_loss")},
            "encoder": c["encoder"], "encoder_conf": c["encoder_conf"], "decoder": c["decoder"], "decoder_conf": c["decoder_conf"],
            "predictor": c["predictor"], "predictor_conf": c["predictor_conf"],
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "specaug": "SpecAug", "specaug_conf": {"apply_time_warp": True},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    sd = synth.eparaformer_state_dict(seed, EParaformer(**c))
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return sd, c, tokens


def test_automodel_end_to_end(cuda, tmp_path):
    """a written model directory over three wav files of equal length: batch_size 3 and batch_size 1 give the same text per key (no
    padding: a clip's result is what it is alone), and the text is what the float64 oracle decodes from the same features"""
    from funasr_amd.audio import batch_to_features
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.tokenizer import sentence_postprocess

    sd, c, tokens = _model_dir(str(tmp_path / "eparaformer"))
    wavs = []
    for i in range(3):
        p = str(tmp_path / f"utt{i}.wav")
        write_wav(p, synth.speech_like(24000, seed=20 + i))
        wavs.append(p)
    am = AutoModel(model=str(tmp_path / "eparaformer"), device="cuda", disable_update=True)
    assert isinstance(am.model, EParaformer)
    res3 = am.generate(input=wavs, batch_size=3)
    res1 = am.generate(input=wavs, batch_size=1)
    assert [r["key"] for r in res3] == ["utt0", "utt1", "utt2"] and all(set(r) == {"key", "text"} for r in res3)
    assert res1 == res3
    speech, lens, _ = batch_to_features(wavs, None, am.kwargs["frontend"], dict(am.kwargs, device="cuda"))
    lens = [int(v) for v in lens.tolist()]
    want = O.model(O.cast(sd), c, speech.double().cpu(), lens)
    tn = want["token_num"]
    if float((tn - tn.floor() - 0.5).abs().min()) >= 0.01:          # (a sum at a half-integer may round either way: README)
        for b, r in enumerate(res3):
            text, _ = sentence_postprocess([tokens[t] for t in want["ids"][b]])
            assert r["text"] == text, b
    with pytest.raises(NotImplementedError, match="bf16"):
        AutoModel(model=str(tmp_path / "eparaformer"), device="cuda", disable_update=True, bf16=True)
    with pytest.raises(NotImplementedError, match="pred_timestamp"):
        am.generate(input=wavs[0], pred_timestamp=True)


# ------------------------------------------------------------------------------------------------ the recipe's size
def test_recipe_size_30_seconds_against_the_oracle(cuda):
    """D 256, 4 heads, 12 + 6 blocks, 2048 units, vocabulary 4234, one 30 s clip: finite, deterministic, and within the bars against the
    float64 oracle (gaps: the oracle's own fp32 run on the same input)"""
    conf = synth.eparaformer_conf(**synth.EPARAFORMER_TEMPLATE)
    m = EParaformer(**conf)
    sd = synth.eparaformer_state_dict(14, m)
    m.load_state_dict(sd, strict=True)
    m = m.to(cuda)
    feats = torch.randn(1, 2999, 80, generator=torch.Generator().manual_seed(2))
    w64 = O.model(O.cast(sd), conf, feats.double(), [2999])
    w32 = O.model(O.cast(sd, torch.float32), conf, feats, [2999])
    tn = w64["token_num"]
    assert w64["olens"] == [749] and w64["counts"] == w32["counts"] and float((tn - tn.floor() - 0.5).abs().min()) >= 0.02
    n = w64["counts"][0]
    assert 50 <= n <= 400
    g = {"feats": feats.numpy(), "lens": np.asarray([2999])}
    for mode in ("fp32", "f16x2"):
        m.set_precision(mode)
        r = _run_model(m, g, cuda)
        assert r["counts"] == w64["counts"] and torch.equal(r["logp"], _run_model(m, g, cuda)["logp"])
        for k in ("enc", "token_num", "alphas", "align", "embeds"):
            gap = _sum_gap(w32[k], w64[k]) if k == "token_num" else _maxd(w32[k], w64[k])
            _check(f"recipe 30 s {mode} {k}", r[k], w64[k], gap, FACTOR[mode])
        _check(f"recipe 30 s {mode} logp", r["logp"][0, :n], w64["logp"][0, :n], _maxd(w32["logp"][0, :n], w64["logp"][0, :n]), FACTOR[mode])
