"""E-Branchformer on the MI355X through the C ABI: the gating-unit, merge and GELU kernels against the float64 oracle on random inputs
(NaN guard rows around every input buffer), the model against the reference's recorded float64 outputs in both variants and both
precision modes (singles and the ragged batch, whose shorter clip must give the reference's BATCHED rows), greedy ids and n-best,
bitwise repeats, the live handle, AutoModel end to end, and the template's size.

Bars are those of tests/test_conformer_gpu.py: 4 x (fp32) / 8 x (f16x2) the reference's own fp32 - fp64 gap stored beside the recorded
outputs; where no recorded gap exists (random-input kernel tests, the template-size run) 4 x max |oracle fp32 - oracle fp64| --
another valid fp32 summation order may be that far off."""
import json
import os

import pytest
import torch
import yaml

from funasr_amd import _lib, synth
from funasr_amd.conformer import TooShortUttError, subsampled_length
from funasr_amd.ebranchformer import EBranchformer

from . import _ebranchformer_oracle as O
from ._model_dir import write_wav
from .test_ebranchformer import VARIANTS, golden_model, load_golden, pin_positional_rows

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
    assert d <= factor * gap, (tag, d, gap)


def _guarded(cuda, rows):
    """rows [M, W] on the device between one row of NaN before the first and one behind the last; returns (buffer, view of the rows)"""
    buf = torch.cat([torch.full((1, rows.shape[1]), NAN), rows, torch.full((1, rows.shape[1]), NAN)]).contiguous().to(cuda)
    return buf, buf[1:-1]


# ------------------------------------------------------------------------------------------------ kernels
def _csgu(cuda, B, T, C, taps, scales=None):
    lib = _lib.load()
    g = torch.Generator().manual_seed(1000 * taps + T)
    h = torch.randn(B, T, 2 * C, generator=g)
    if scales is not None:
        h = h * torch.tensor(scales)[:, None, None]
    p = [1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), torch.randn(C, 1, taps, generator=g) / taps ** 0.5,
         0.1 * torch.randn(C, generator=g)]
    buf, hd = _guarded(cuda, h.reshape(B * T, 2 * C))
    dev = [t.contiguous().to(cuda) for t in p]
    stats = torch.empty(B * T, 2, device=cuda)
    y = torch.full((B, T, C), NAN, device=cuda)
    _lib.check(lib.pf_k_eb_csgu(hd.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), 1e-12, dev[2].data_ptr(), dev[3].data_ptr(), B, T, C, taps,
                                stats.data_ptr(), y.data_ptr(), _stream()), "pf_k_eb_csgu")
    torch.cuda.synchronize()
    r64 = O.csgu(h.double(), *[t.double() for t in p])
    r32 = O.csgu(h, *p)
    _check(f"csgu B={B} T={T} C={C} taps {taps}", y, r64, _maxd(r32, r64), 4.0)
    for b in range(B if scales is not None else 0):                # sequences of unlike size: the small one keeps its own (small) bar
        _check(f"csgu B={B} T={T} C={C} taps {taps} seq {b}", y[b], r64[b], _maxd(r32[b], r64[b]), 4.0)


@pytest.mark.parametrize("taps", [1, 3, 15, 31])
@pytest.mark.parametrize("C", [32, 96, 512])
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 37])
def test_gating_unit_against_the_oracle(cuda, T, C, taps):
    """T shorter than the halo (1, 2), on and around the 32-row tile; 32 gate channels (half a channel block), 96 (one and a half) and
    the template's 512; one tap (no halo) to 31; three sequences. The input sits between two NaN rows: a conv that read the row before
    sequence 0 or behind sequence 2 instead of zero padding gives NaN."""
    _csgu(cuda, 3, T, C, taps)


@pytest.mark.parametrize("T,taps", [(5, 31), (33, 15)])
def test_gating_unit_does_not_read_across_the_sequence_boundary(cuda, T, taps):
    """sequence 1's rows are 1000 x sequence 0's: x_r scales with them, and so does what a conv reading sequence 1's first rows for
    sequence 0's last outputs would multiply into them"""
    _csgu(cuda, 2, T, 96, taps, scales=[1.0, 1000.0])


def _merge(cuda, B, T, D, taps, scales=None):
    lib = _lib.load()
    g = torch.Generator().manual_seed(2000 * taps + T)
    x1, x2 = torch.randn(B, T, D, generator=g), torch.randn(B, T, D, generator=g)
    if scales is not None:
        x1, x2 = x1 * torch.tensor(scales)[:, None, None], x2 * torch.tensor(scales)[:, None, None]
    w, b_ = torch.randn(2 * D, 1, taps, generator=g) / taps ** 0.5, 0.1 * torch.randn(2 * D, generator=g)
    buf1, d1 = _guarded(cuda, x1.reshape(B * T, D))               # two allocations, each with its own guard rows
    buf2, d2 = _guarded(cuda, x2.reshape(B * T, D))
    wd, bd = w.contiguous().to(cuda), b_.to(cuda)
    y = torch.full((B, T, 2 * D), NAN, device=cuda)
    _lib.check(lib.pf_k_eb_merge(d1.data_ptr(), d2.data_ptr(), wd.data_ptr(), bd.data_ptr(), B, T, D, taps, y.data_ptr(), _stream()),
               "pf_k_eb_merge")
    torch.cuda.synchronize()
    r64 = O.merge(x1.double(), x2.double(), w.double(), b_.double())
    r32 = O.merge(x1, x2, w, b_)
    _check(f"merge B={B} T={T} D={D} taps {taps}", y, r64, _maxd(r32, r64), 4.0)
    for b in range(B if scales is not None else 0):
        _check(f"merge B={B} T={T} D={D} taps {taps} seq {b}", y[b], r64[b], _maxd(r32[b], r64[b]), 4.0)


@pytest.mark.parametrize("taps", [1, 3, 15, 31])
@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("T", [1, 2, 31, 32, 33, 37])
def test_merge_against_the_oracle(cuda, T, D, taps):
    """the same T and tap grid; D 64 (x1 and x2 one channel block each) and 192; x1 and x2 in separate allocations between NaN rows"""
    _merge(cuda, 3, T, D, taps)


def test_merge_with_a_channel_block_across_both_inputs_and_a_large_neighbour_sequence(cuda):
    """D 96: the channel block 64 .. 127 takes 32 columns of x1 and 32 of x2; sequence 1 is 1000 x sequence 0"""
    _merge(cuda, 2, 33, 96, 15, scales=[1.0, 1000.0])
    _merge(cuda, 3, 5, 96, 31)


def test_gelu_is_the_exact_erf_form(cuda):
    """against torch.nn.functional.gelu in float64: a grid over [-10, 10] (the left tail, where 1 + erf cancels), random values, +-0"""
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.linspace(-10, 10, 4001), 3 * torch.randn(4091, generator=g), torch.tensor([0.0, -0.0, 10.0, -10.0])])
    assert x.numel() % 4 == 0
    xd = x.to(cuda)
    _lib.check(_lib.load().pf_k_eb_gelu(xd.data_ptr(), x.numel(), _stream()), "pf_k_eb_gelu")
    torch.cuda.synchronize()
    r64 = torch.nn.functional.gelu(x.double())
    _check("gelu", xd, r64, _maxd(torch.nn.functional.gelu(x), r64), 4.0)
    got = xd.cpu()
    assert float(got[-4]) == 0.0 and not bool(torch.signbit(got[-4])) and float(got[-3]) == 0.0 and bool(torch.signbit(got[-3]))
    assert float(got[-2]) == 10.0 and abs(float(got[-1])) < 1e-20
    # the tanh approximation is 4.7e-4 away at its worst: this is not it
    assert _maxd(xd, torch.nn.functional.gelu(x.double(), approximate="tanh")) > 1e-4


def test_kernels_refuse_other_channel_counts_and_kernels(cuda):
    lib = _lib.load()
    t = torch.zeros(4096, device=cuda)
    p = t.data_ptr()
    assert lib.pf_k_eb_csgu(p, p, p, 1e-12, p, p, 1, 4, 48, 3, p, p, _stream()) != 0 and "eb_csgu" in _lib.last_error()
    assert lib.pf_k_eb_csgu(p, p, p, 1e-12, p, p, 1, 4, 32, 4, p, p, _stream()) != 0
    assert lib.pf_k_eb_csgu(p, p, p, 1e-12, p, p, 1, 4, 32, 33, p, p, _stream()) != 0
    assert lib.pf_k_eb_merge(p, p, p, p, 1, 4, 48, 3, p, _stream()) != 0 and "eb_merge" in _lib.last_error()
    assert lib.pf_k_eb_merge(p, p, p, p, 1, 4, 32, 2, p, _stream()) != 0
    assert lib.pf_k_eb_gelu(p, 6, _stream()) != 0
    c = _lib.pf_ebranchformer_config(80, 128, 2, 256, 1, 224, 31, 31, 1, 1, 0, 0, 1e-12)            # cgmlp_units 224: 112 gate channels
    assert not lib.pf_ebranchformer_create(_lib.C.byref(c)) and "ebranchformer: unsupported config" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ the handle
def _encoder_model(cuda, conf, seed, mode):
    m = EBranchformer(**conf)
    sd = synth.ebranchformer_state_dict(seed, m)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda).set_precision(mode), sd


@pytest.fixture(scope="module")
def live(cuda):
    """model A after an encode with seed 1 and a load_state_dict of seed 2 on the live handle; B is a fresh model with seed 2"""
    conf = synth.ebranchformer_conf(enc_blocks=1)
    g = torch.Generator().manual_seed(0)
    lens = [23, 17]
    feats = torch.randn(2, 23, 80, generator=g)
    feats[1, 17:] = 0
    feats = feats.to(cuda)
    a, _ = _encoder_model(cuda, conf, 1, "f16x2")
    a.encode(feats, lens)                                                     # primes the handle with seed 1
    a.load_state_dict(synth.ebranchformer_state_dict(2, a), strict=True)
    b, _ = _encoder_model(cuda, conf, 2, "f16x2")
    return conf, a, b.encode(feats, lens)[0], feats, lens


def test_weights_and_precision_replaced_on_a_live_handle(cuda, live):
    """One handle through load_state_dict and set_precision: every encode equals a fresh model's with the same weights and mode, so
    nothing derived at load time (conv taps, output linear, halved macaron w_2, plane caches and exponents) outlives the weights or
    the mode it was made for: the prepared state follows the version of the tensor table."""
    conf, a, want_x2, feats, lens = live
    assert torch.equal(a.encode(feats, lens)[0], want_x2)
    a.set_precision("fp32")
    c, _ = _encoder_model(cuda, conf, 2, "fp32")
    want_32 = c.encode(feats, lens)[0]
    assert torch.equal(a.encode(feats, lens)[0], want_32) and not torch.equal(want_32, want_x2)
    a.set_precision("f16x2")
    assert torch.equal(a.encode(feats, lens)[0], want_x2)


def test_derived_tensor_names_are_not_writable(cuda, live):
    _, a, want_x2, feats, lens = live
    before = a.encode(feats, lens)[0]
    lib, h = _lib.load(), a.encoder._handle
    one = torch.zeros(1, device=cuda)
    for name in (b"#embed.out", b"#conv1.tap0", b"encoders.0.feed_forward.w_2.weight#half", b"encoders.0.feed_forward_macaron.w_2.bias#half"):
        assert lib.pf_ebranchformer_set_tensor(h, name, one.data_ptr(), 1) != 0, name
        assert "unknown tensor name" in _lib.last_error(), (name, _lib.last_error())
    assert lib.pf_ebranchformer_missing(h) == 0
    assert torch.equal(a.encode(feats, lens)[0], before)


def test_num_frames_short_batches_and_a_clip_without_encoder_frames(cuda, live):
    conf, a, _, _, _ = live
    lib, h = a.encoder._ensure_handle()
    for padded in (7, 101, 247):
        for n in (1, 3, padded // 2, padded):
            assert lib.pf_ebranchformer_num_frames(h, n, padded) == subsampled_length(n, padded)
    assert lib.pf_ebranchformer_num_frames(h, 5, 6) == -1
    with pytest.raises(TooShortUttError, match="has 6 frames and is too short for subsampling"):
        a.encode(torch.zeros(1, 6, 80, device=cuda), [6])
    x, out = torch.zeros(1, 6, 80, device=cuda), torch.zeros(1, 1, 128, device=cuda)
    assert lib.pf_ebranchformer_forward(h, x.data_ptr(), (_lib.C.c_int32 * 1)(6), 1, 6, out.data_ptr(), None, _stream()) != 0
    assert "ebranchformer: has 6 frames and is too short for subsampling (it needs more than 7 frames)" in _lib.last_error()
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 50, 80, generator=g)
    feats[1] = 0
    enc, olens = a.encode(feats.to(cuda), [50, 0])
    assert olens.tolist() == [11, 0] and bool(torch.isfinite(enc[0]).all()) and float(enc[0].abs().max()) > 0
    assert torch.equal(enc, a.encode(feats.to(cuda), [50, 0])[0])


# ------------------------------------------------------------------------------------------------ model against the golden
@pytest.fixture(scope="module")
def models(cuda):
    out = {}
    for variant in VARIANTS:
        g = load_golden(variant)
        m, sd, conf = golden_model(g, variant)
        if pin_positional_rows(m, g):
            print("this host's float32 exp() builds another positional table than the recording's: recorded rows pinned")
        out[variant] = (g, m.to(cuda), sd, conf)
    return out


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_model_against_the_references_recorded_outputs(cuda, models, variant, mode):
    """singles and the ragged batch; the shorter clip's batched rows are the reference's BATCHED rows (its unmasked convs read the
    rows behind the clip's end), which differ from its rows alone by more than 100 x the gap. f16x2: `merge_proj` is left in exact
    fp32 (the a-priori bound of its operand compounds past what a two-plane operand resolves); every other block GEMM runs
    from two-plane operands (linear_pos and the subsampling are fp32 in both modes, as in the Conformer)."""
    g, m, sd, conf = models[variant]
    m.set_precision(mode)
    lens = [int(n) for n in g["lens"]]
    feats = [torch.from_numpy(g[f"feats_{i}"]) for i in range(len(lens))]
    for i, f in enumerate(feats):
        enc, olens = m.encode(f[None].to(cuda), [lens[i]])
        assert olens.tolist() == [g[f"enc_{i}"].shape[0]]
        _check(f"{variant} {mode} enc {i}", enc[0], g[f"enc_{i}"], float(g[f"gap_enc_{i}"]), FACTOR[mode])
        _check(f"{variant} {mode} ctc {i}", m.ctc.log_softmax(enc)[0], g[f"ctc_{i}"], float(g[f"gap_ctc_{i}"]), FACTOR[mode])
        assert m.ctc_greedy(enc, olens)[0] == g[f"greedy_{i}"].tolist()
    pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    enc, olens = m.encode(pad.to(cuda), lens)
    assert olens.tolist() == g["batch_olens"].tolist() == [41, 61]            # the reference's lengths exactly
    lp = m.ctc.log_softmax(enc)
    greedy = m.ctc_greedy(enc, olens)
    for i, n in enumerate(olens.tolist()):
        _check(f"{variant} {mode} batch enc {i}", enc[i, :n], g[f"batch_enc_{i}"], float(g[f"gap_batch_enc_{i}"]), FACTOR[mode])
        _check(f"{variant} {mode} batch ctc {i}", lp[i, :n], g[f"batch_ctc_{i}"], float(g[f"gap_batch_ctc_{i}"]), FACTOR[mode])
        assert greedy[i] == g[f"batch_greedy_{i}"].tolist()
    assert _maxd(enc[0, :40], g["enc_0"]) > 100 * float(g["gap_batch_enc_0"])  # ... and not the rows of the clip alone
    dec = m.decoder.set_memory(torch.from_numpy(g["enc_0"]).float().to(cuda))
    for j, pre in enumerate(g["prefixes"]):
        got = O.score_prefix(dec, [int(t) for t in str(pre).split(",")])
        _check(f"{variant} {mode} step {j}", got, g[f"step_{j}"], float(g[f"gap_step_{j}"]), FACTOR[mode])


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_beam_search_nbest_equals_the_references(cuda, models, variant, mode):
    g, m, sd, conf = models[variant]
    m.set_precision(mode)
    f = torch.from_numpy(g["feats_0"])
    enc, _ = m.encode(f[None].to(cuda), [f.shape[0]])
    for w in g["ctc_weights"].tolist():
        m.beam_search = None
        m.init_beam_search(token_list=g["tokens"].tolist(), decoding_ctc_weight=w, beam_size=int(g["beam"]))
        nbest = m.beam_search_features(enc[0])[: int(g["nbest"])]
        assert len(nbest) == int(g["nbest"])
        for r, h in enumerate(nbest):
            assert h.yseq == g[f"nbest_ids_w{w}_{r}"].tolist(), (variant, mode, w, r)
            d = abs(h.score - float(g[f"nbest_score_w{w}_{r}"]))
            print(f"{variant} {mode} w={w} rank {r}: |d score| {d:.3e}, gap {float(g['gap_nbest_score']):.3e}")
            assert d <= 8 * float(g["gap_nbest_score"]), (variant, mode, w, r, d)
    m.beam_search = None


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_bitwise_repeat_and_equal_length_batch(cuda, models, mode):
    g, m, sd, conf = models["latest_macaron"]
    m.set_precision(mode)
    gen = torch.Generator().manual_seed(4)
    clips = torch.randn(3, 141, 80, generator=gen).to(cuda)
    a, _ = m.encode(clips, [141] * 3)
    b, _ = m.encode(clips, [141] * 3)
    assert torch.equal(a, b)
    for i in range(3):
        solo, _ = m.encode(clips[i: i + 1], [141])
        assert torch.equal(solo[0], a[i]), i


# ------------------------------------------------------------------------------------------------ AutoModel
def _model_dir(path, seed=31):
    os.makedirs(path, exist_ok=True)
    tokens = load_golden("latest_macaron")["tokens"].tolist()
    c = synth.ebranchformer_conf(vocab=len(tokens))
    conf = {"model": "Branchformer", "model_conf": {"ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False},
            "encoder": c["encoder"], "encoder_conf": c["encoder_conf"], "decoder": c["decoder"], "decoder_conf": c["decoder_conf"],
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "specaug": "SpecAug", "specaug_conf": {"apply_time_warp": True},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    sd = synth.ebranchformer_state_dict(seed, EBranchformer(**c))
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return sd, c, tokens


def test_automodel_end_to_end(cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.tokenizer import sentence_postprocess

    sd, c, tokens = _model_dir(str(tmp_path / "ebranchformer"))
    wavs = []
    for i, n in enumerate((16000, 27001, 21503)):
        p = str(tmp_path / f"utt{i}.wav")
        write_wav(p, synth.speech_like(n, seed=20 + i))
        wavs.append(p)
    am = AutoModel(model=str(tmp_path / "ebranchformer"), device="cuda", disable_update=True)
    assert isinstance(am.model, EBranchformer)
    res = am.generate(input=wavs[0], batch_size=1, beam_size=5, decoding_ctc_weight=0.3, nbest=2)
    assert len(res) == 2 and set(res[0]) >= {"key", "token", "text"} and res[0]["key"] == "utt0"
    res = am.generate(input=wavs, batch_size=3)
    assert [r["key"] for r in res] == ["utt0", "utt1", "utt2"] and all(set(r) >= {"key", "text"} and "token" not in r for r in res)
    # what the oracle decodes from the same padded feature batch
    from funasr_amd.audio import batch_to_features
    speech, lens, _ = batch_to_features(wavs, None, am.kwargs["frontend"], dict(am.kwargs, device="cuda"))
    lens = [int(v) for v in lens.tolist()]
    speech = speech.float().cpu()
    for b, n in enumerate(lens):
        speech[b, n:] = 0
    sd64 = O.cast(sd)
    enc, olens = O.encoder(sd64, c["encoder_conf"], speech.double(), lens)
    lp = O.ctc_log_softmax(sd64, enc)
    for b, r in enumerate(res):
        want, _ = sentence_postprocess([tokens[t] for t in O.ctc_greedy(lp[b], olens[b])])
        assert r["text"] == want, b


# ------------------------------------------------------------------------------------------------ the template's size
def _template(cuda, seed=13):
    conf = synth.ebranchformer_conf(**synth.EBRANCHFORMER_TEMPLATE)
    m = EBranchformer(**conf)
    sd = synth.ebranchformer_state_dict(seed, m)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda), sd, conf


def test_template_size_30_seconds_against_the_oracle(cuda):
    """D 256, 4 heads, cgMLP 1024, 12 blocks, one 30 s clip against the float64 oracle: fp32, and f16x2 (`merge_proj` in fp32) at its
    own bar, where the a-priori bounds are the widest"""
    m, sd, conf = _template(cuda)
    feats = torch.randn(1, 2999, 80, generator=torch.Generator().manual_seed(2))
    assert subsampled_length(2999, 2999) == 749
    e64, _ = O.encoder(O.cast(sd), conf["encoder_conf"], feats.double(), [2999])
    e32, _ = O.encoder(O.cast(sd, torch.float32), conf["encoder_conf"], feats, [2999])
    gap = _maxd(e32, e64)
    for mode in ("fp32", "f16x2"):
        m.set_precision(mode)
        enc, olens = m.encode(feats.to(cuda), [2999])
        assert olens.tolist() == [749]
        _check(f"template 30 s {mode}", enc, e64, gap, FACTOR[mode])


def test_template_size_8_x_10_seconds_finite_and_deterministic(cuda):
    m, sd, conf = _template(cuda)
    feats = torch.randn(8, 998, 80, generator=torch.Generator().manual_seed(3)).to(cuda)
    a, olens = m.encode(feats, [998] * 8)
    b, _ = m.encode(feats, [998] * 8)
    assert a.shape == (8, 248, 256) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert len(m.ctc_greedy(a, olens)) == 8
