"""Conformer on the MI355X through the C ABI: the new kernels against the float64 oracle on random inputs, the model against the
reference's recorded float64 outputs in both precision modes (bars: 4 x (fp32) / 8 x (f16x2) the reference's own fp32 - fp64 gap
stored beside them), greedy ids and n-best, bitwise determinism and batch invariance for equal lengths, AutoModel end to end, and
one user-scale shape.

Where no recorded gap exists (random-input kernel tests, the AISHELL-size run) the bar is built the same way from the oracle's
own float32 run: 4 x (8 x for f16x2) max |oracle fp32 - oracle fp64| -- another valid fp32 summation order may be that far off."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import _lib, synth
from funasr_amd.conformer import Conformer, subsampled_length
from funasr_amd.transformer_search import BeamSearchTransformer

from . import _conformer_oracle as O
from ._model_dir import write_wav
from .test_conformer import VARIANTS, load_golden, pin_positional_rows, variant_model

pytestmark = pytest.mark.gpu
FACTOR = {"fp32": 4.0, "f16x2": 8.0}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _maxd(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _check(tag, got, want64, gap, factor):
    d = _maxd(got, want64)
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / max(gap, 1e-30):.2f} (bar {factor:g})")
    assert d <= factor * gap, (tag, d, gap)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_conv_subsampling_against_the_oracle(cuda, mode):
    """a zero-block encoder = Conv2dSubsampling (conv0, conv1 as three strided-view GEMMs, the output linear) x sqrt(D) + after_norm"""
    conf = synth.conformer_conf(enc_blocks=0)
    m = Conformer(**conf)
    sd = synth.conformer_state_dict(3, m)
    m.load_state_dict(sd, strict=True)
    m = m.to(cuda).set_precision(mode)
    g = torch.Generator().manual_seed(0)
    lens = [53, 31, 44]
    feats = torch.randn(3, 53, 80, generator=g)
    for b, n in enumerate(lens):
        feats[b, n:] = 0
    out, olens = m.encode(feats.to(cuda), lens)
    e64, ol = O.encoder(O.cast(sd), conf["encoder_conf"], feats.double(), lens)
    e32, _ = O.encoder(O.cast(sd, torch.float32), conf["encoder_conf"], feats, lens)
    assert olens.tolist() == ol
    _check("subsampling " + mode, out, e64, _maxd(e32, e64), FACTOR[mode])


def _encoder_model(cuda, conf, seed, mode):
    m = Conformer(**conf)
    sd = synth.conformer_state_dict(seed, m)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda).set_precision(mode), sd


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("enc_blocks", [0, 1])
@pytest.mark.parametrize("input_size", [7, 83, 256])
def test_subsampling_feature_counts_and_shortest_batches_against_the_oracle(cuda, input_size, enc_blocks, mode):
    """the feature counts at the ends of the accepted range and an odd one (F1 = 3 / 41 / 127 conv0 columns in a pitch of 4 / 42 /
    128, F2 = 1 / 20 / 63 plus the waste column), batches of 7 .. 15 frames (T = 1, 1, 1, 2, 2, 3: the `NE = T + 1` even / odd
    rows and the slack behind them are most of the buffer), ragged lengths down to 1. With one block (31 taps) T = 1 .. 3 also goes
    through the relative-position attention and through the depthwise conv with a 15-row halo on each side. Then the shape order on
    one handle: long, shortest, long."""
    conf = synth.conformer_conf(input_size=input_size, enc_blocks=enc_blocks, kernel=31)
    m, sd = _encoder_model(cuda, conf, 3, mode)
    sd64, sd32 = O.cast(sd), O.cast(sd, torch.float32)
    g = torch.Generator().manual_seed(input_size)
    expect = {7: (1, [1, 1, 1]), 8: (1, [1, 1, 1]), 10: (1, [1, 1, 1]), 11: (2, [2, 2, 1]), 14: (2, [2, 2, 1]), 15: (3, [3, 3, 1])}
    for Tin in (7, 8, 10, 11, 14, 15):
        lens = [Tin, max(1, Tin - 4), 1]
        feats = torch.randn(3, Tin, input_size, generator=g)
        for b, n in enumerate(lens):
            feats[b, n:] = 0
        out, olens = m.encode(feats.to(cuda), lens)
        e64, ol = O.encoder(sd64, conf["encoder_conf"], feats.double(), lens)
        e32, _ = O.encoder(sd32, conf["encoder_conf"], feats, lens)
        assert bool(torch.isfinite(e64).all()) and (e64.shape[1], ol) == expect[Tin]
        assert out.shape == e64.shape and olens.tolist() == ol
        _check(f"subsampling F={input_size} blocks={enc_blocks} {mode} Tin={Tin}", out, e64, _maxd(e32, e64), FACTOR[mode])
    long = torch.randn(3, 141, input_size, generator=g).to(cuda)
    short = torch.randn(1, 7, input_size, generator=g).to(cuda)
    a, _ = m.encode(long, [141] * 3)
    s, _ = m.encode(short, [7])
    b, _ = m.encode(long, [141] * 3)
    assert torch.equal(a, b)
    fresh, _ = _encoder_model(cuda, conf, 3, mode)
    assert torch.equal(s, fresh.encode(short, [7])[0])


@pytest.fixture(scope="module")
def live(cuda):
    """model A after an encode with seed 1 and a load_state_dict of seed 2 on the live handle; B is a fresh model with seed 2"""
    conf = synth.conformer_conf(enc_blocks=1, macaron=True)
    g = torch.Generator().manual_seed(0)
    lens = [23, 17]
    feats = torch.randn(2, 23, 80, generator=g)
    feats[1, 17:] = 0
    feats = feats.to(cuda)
    a, _ = _encoder_model(cuda, conf, 1, "f16x2")
    a.encode(feats, lens)                                                     # primes the handle with seed 1
    a.load_state_dict(synth.conformer_state_dict(2, a), strict=True)
    b, _ = _encoder_model(cuda, conf, 2, "f16x2")
    return conf, a, b.encode(feats, lens)[0], feats, lens


def test_weights_and_precision_replaced_on_a_live_handle(cuda, live):
    """One handle through load_state_dict and set_precision: every encode equals a fresh model's with the same weights and mode, so
    nothing derived at load time (conv taps, output linear, folded BatchNorm, halved macaron w_2, plane caches and exponents) outlives
    the weights or the mode it was made for."""
    conf, a, want_x2, feats, lens = live
    assert torch.equal(a.encode(feats, lens)[0], want_x2)
    a.set_precision("fp32")
    c, _ = _encoder_model(cuda, conf, 2, "fp32")
    assert torch.equal(a.encode(feats, lens)[0], c.encode(feats, lens)[0])
    a.set_precision("f16x2")
    assert torch.equal(a.encode(feats, lens)[0], want_x2)


def test_derived_tensor_names_are_not_writable(cuda, live):
    """what the library derives from the weights is refused by set_tensor like any unknown name -- also once a forward has put the
    names into the table -- and never counts as missing"""
    _, a, want_x2, feats, lens = live
    before = a.encode(feats, lens)[0]
    assert torch.equal(before, want_x2)
    lib, h = _lib.load(), a.encoder._handle
    one = torch.zeros(1, device=cuda)
    for name in (b"#embed.out", b"#conv1.tap0", b"#bn", b"encoders.0.feed_forward.w_2.weight#half"):
        assert lib.pf_conformer_set_tensor(h, name, one.data_ptr(), 1) != 0, name
        assert "unknown tensor name" in _lib.last_error(), (name, _lib.last_error())
    assert lib.pf_conformer_missing(h) == 0
    assert torch.equal(a.encode(feats, lens)[0], before)


def _glu_dw_against_the_oracle(cuda, B, T, D, taps):
    lib = _lib.load()
    g = torch.Generator().manual_seed(taps)
    x = torch.randn(B, T, 2 * D, generator=g)
    sd = {"depthwise_conv.weight": torch.randn(D, 1, taps, generator=g) / taps ** 0.5, "depthwise_conv.bias": 0.1 * torch.randn(D, generator=g),
          "norm.weight": 1 + 0.2 * torch.randn(D, generator=g), "norm.bias": 0.1 * torch.randn(D, generator=g),
          "norm.running_mean": 0.2 * torch.randn(D, generator=g), "norm.running_var": 0.5 + 1.5 * torch.rand(D, generator=g)}

    def ref(dt):
        s = {k: v.to(dt) for k, v in sd.items()}
        y = torch.nn.functional.glu(x.to(dt).transpose(1, 2), dim=1)
        y = torch.nn.functional.conv1d(y, s["depthwise_conv.weight"], s["depthwise_conv.bias"], padding=taps // 2, groups=D)
        y = (y - s["norm.running_mean"][None, :, None]) / torch.sqrt(s["norm.running_var"][None, :, None] + 1e-5)
        y = y * s["norm.weight"][None, :, None] + s["norm.bias"][None, :, None]
        return (y * torch.sigmoid(y)).transpose(1, 2)

    sc = (sd["norm.weight"].double() / torch.sqrt(sd["norm.running_var"].double() + 1e-5))
    sh = sd["norm.bias"].double() - sd["norm.running_mean"].double() * sc
    dev = [t.float().contiguous().to(cuda) for t in (x, sd["depthwise_conv.weight"], sd["depthwise_conv.bias"], sc, sh)]
    y = torch.empty(B, T, D, device=cuda)
    _lib.check(lib.pf_k_conformer_glu_dw(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), B, T, D,
                                         taps, y.data_ptr(), _stream()), "pf_k_conformer_glu_dw")
    torch.cuda.synchronize()
    r64 = ref(torch.float64)
    _check(f"glu_dw B={B} T={T} D={D} taps {taps}", y, r64, _maxd(ref(torch.float32), r64), 4.0)


@pytest.mark.parametrize("taps", [15, 31])
def test_convolution_module_row_kernel_against_the_oracle(cuda, taps):
    _glu_dw_against_the_oracle(cuda, 2, 37, 128, taps)


@pytest.mark.parametrize("taps", [1, 3, 15, 31])
@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("T", [1, 2, 32, 33, 37])
def test_convolution_module_row_kernel_short_rows_tile_edges_and_tap_counts(cuda, T, D, taps):
    """T shorter than the halo (1, 2: every tap but the centre ones reads padding), T on and one past the 32-row workgroup tile,
    one tap (no halo at all) and three, one and three 64-channel column blocks, three sequences; same reference, same bar"""
    _glu_dw_against_the_oracle(cuda, 3, T, D, taps)


def _relpos_against_the_oracle(cuda, legacy, H, T, klens):
    lib = _lib.load()
    g = torch.Generator().manual_seed(T)
    B, dk = len(klens), 64
    D = H * dk
    nP = T if legacy else 2 * T - 1
    qkv = torch.randn(B, T, 3 * D, generator=g)
    P = torch.randn(nP, D, generator=g)
    u, v = 0.3 * torch.randn(H, dk, generator=g), 0.3 * torch.randn(H, dk, generator=g)

    def ref(dt):
        q, k, vv = [t.to(dt).reshape(B, T, H, dk) for t in qkv.split(D, dim=-1)]
        return O.relpos_attention(q, k, vv, P.to(dt).view(nP, H, dk), u.to(dt), v.to(dt), klens, legacy)

    # one row of NaN behind the last sequence: the K / V staging clamps the rows of a partial tile to the last valid key, and a
    # kernel that read one row further instead (a masked row: probability 0) would turn the last sequence's output into NaN
    guard = torch.full((1, 3 * D), float("nan"))
    dev = [t.contiguous().to(cuda) for t in (torch.cat([qkv.reshape(B * T, 3 * D), guard]), P, u, v)]
    kl = torch.tensor(klens, dtype=torch.int32, device=cuda)
    out = torch.empty(B, T, D, device=cuda)
    _lib.check(lib.pf_k_relpos_attention(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), kl.data_ptr(), B, T, H,
                                         int(legacy), out.data_ptr(), _stream()), "pf_k_relpos_attention")
    torch.cuda.synchronize()
    r64 = ref(torch.float64)
    _check(f"relpos legacy={legacy} H={H} T={T} klens={klens}", out, r64, max(_maxd(ref(torch.float32), r64), 1e-7), 4.0)


@pytest.mark.parametrize("legacy", [True, False])
@pytest.mark.parametrize("T,klens", [(1, [1, 1]), (2, [2, 1]), (77, [77, 50]), (129, [129, 128]), (200, [33, 200])])
def test_relpos_attention_against_the_oracle(cuda, legacy, T, klens):
    """T not a multiple of any tile, ragged key lengths, T = 1 and 2 (no wrapped entries there), wave tiles (32 queries) and a
    workgroup tile (128) whose boundary lies on the diagonal"""
    _relpos_against_the_oracle(cuda, legacy, 2, T, klens)


@pytest.mark.parametrize("legacy", [True, False])
@pytest.mark.parametrize("T,klens", [(32, [32, 31, 1]), (33, [33, 32, 1]), (64, [64, 33, 32]), (128, [128, 97, 64]), (160, [160, 129, 128]),
                                      (33, [1, 32, 33])])
def test_relpos_attention_on_the_tile_edges_with_four_heads(cuda, legacy, T, klens):
    """T and key lengths exactly on, one below and one above the 32-key tile, the 32-query wave tile and the 128-query workgroup
    tile; four heads (the head index enters every pointer), three sequences; T = 33 also with the full-length sequence last, so that
    the row behind its one-key second tile is the guard row"""
    _relpos_against_the_oracle(cuda, legacy, 4, T, klens)


def test_relpos_attention_with_every_key_masked_gives_zero_rows(cuda):
    """a clip the mask rule leaves no encoder frame: the reference masks every key and zeroes the probabilities"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    B, T, D = 2, 40, 128
    dev = [t.contiguous().to(cuda) for t in (torch.randn(B, T, 3 * D, generator=g), torch.randn(T, D, generator=g),
                                             torch.randn(2, 64, generator=g), torch.randn(2, 64, generator=g))]
    kl = torch.tensor([0, 40], dtype=torch.int32, device=cuda)
    out = torch.full((B, T, D), 7.0, device=cuda)
    _lib.check(lib.pf_k_relpos_attention(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), kl.data_ptr(), B, T, 2, 1,
                                         out.data_ptr(), _stream()), "pf_k_relpos_attention")
    torch.cuda.synchronize()
    assert bool((out[0] == 0).all()) and bool(torch.isfinite(out[1]).all()) and float(out[1].abs().max()) > 0


def test_num_frames_entry_point_is_the_mask_rule(cuda):
    m = Conformer(**synth.conformer_conf(enc_blocks=0)).to(cuda)
    lib, h = m.encoder._ensure_handle()
    for padded in (7, 101, 247, 998):
        for n in (1, 2, 3, padded // 2, padded):
            assert lib.pf_conformer_num_frames(h, n, padded) == subsampled_length(n, padded)
    assert lib.pf_conformer_num_frames(h, 5, 6) == -1


def test_decoder_step_and_reorder_against_forward_one_step(cuda):
    conf = synth.conformer_conf()
    m = Conformer(**conf)
    sd = synth.conformer_state_dict(9, m)
    m.load_state_dict(sd, strict=True)
    m = m.to(cuda)
    memory = torch.randn(45, 128, generator=torch.Generator().manual_seed(1))
    dec = m.decoder.set_memory(memory.to(cuda))
    st64 = O.DecoderStepper(O.cast(sd), conf["decoder_conf"], memory.double())
    st32 = O.DecoderStepper(O.cast(sd, torch.float32), conf["decoder_conf"], memory)
    # three hypotheses; after position 1 slot 0 is duplicated, slot 1 dropped: parents [0, 0, 2]
    tokens = [[1], [5, 9, 17], [30, 31, 32], [40, 41, 42], [3, 4, 5]]
    parents = [None, [0, 0, 0], [0, 0, 2], [2, 1, 0], [0, 1, 1]]
    for s in (dec, st64, st32):
        s.begin(8, 4)
    for pos, (tok, par) in enumerate(zip(tokens, parents)):
        outs = []
        for s in (dec, st64, st32):
            if par is not None:
                s.reorder(par)
            outs.append(s.step(tok, pos))
        _check(f"decoder step {pos}", outs[0], outs[1], _maxd(outs[2], outs[1]), 4.0)


# ------------------------------------------------------------------------------------------------ model against the golden
@pytest.fixture(scope="module")
def models(cuda):
    out = {}
    for name in VARIANTS:
        g = load_golden(name)
        model, sd, conf = variant_model(name, g)
        if pin_positional_rows(model, g):
            print(f"{name}: this host's float32 exp() builds another positional table than the recording's: recorded rows pinned")
        out[name] = (g, model.to(cuda), sd, conf)
    return out


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_model_against_the_references_recorded_outputs(cuda, models, name, mode):
    g, model, sd, conf = models[name]
    model.set_precision(mode)
    lens = [int(n) for n in g["lens"]]
    feats = [torch.from_numpy(g[f"feats_{i}"]) for i in range(len(lens))]
    for i, f in enumerate(feats):
        enc, olens = model.encode(f[None].to(cuda), [lens[i]])
        assert olens.tolist() == [g[f"enc_{i}"].shape[0]]
        _check(f"{name} {mode} enc {i}", enc[0], g[f"enc_{i}"], float(g[f"gap_enc_{i}"]), FACTOR[mode])
        _check(f"{name} {mode} ctc {i}", model.ctc.log_softmax(enc)[0], g[f"ctc_{i}"], float(g[f"gap_ctc_{i}"]), FACTOR[mode])
        assert model.ctc_greedy(enc, olens)[0] == g[f"greedy_{i}"].tolist()
    pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    enc, olens = model.encode(pad.to(cuda), lens)
    assert olens.tolist() == g["batch_olens"].tolist()                       # the reference's lengths exactly
    lp = model.ctc.log_softmax(enc)
    greedy = model.ctc_greedy(enc, olens)
    for i, n in enumerate(olens.tolist()):
        _check(f"{name} {mode} batch enc {i}", enc[i, :n], g[f"batch_enc_{i}"], float(g[f"gap_batch_enc_{i}"]), FACTOR[mode])
        _check(f"{name} {mode} batch ctc {i}", lp[i, :n], g[f"batch_ctc_{i}"], float(g[f"gap_batch_ctc_{i}"]), FACTOR[mode])
        assert greedy[i] == g[f"batch_greedy_{i}"].tolist()
    # forward_one_step over the recorded memory
    dec = model.decoder.set_memory(torch.from_numpy(g["enc_1"]).float().to(cuda))
    for j, pre in enumerate(g["prefixes"]):
        got = O.score_prefix(dec, [int(t) for t in str(pre).split(",")])
        _check(f"{name} {mode} step {j}", got, g[f"step_{j}"], float(g[f"gap_step_{j}"]), FACTOR[mode])


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_beam_search_nbest_equals_the_references(cuda, models, name, mode):
    g, model, sd, conf = models[name]
    model.set_precision(mode)
    f = torch.from_numpy(g["feats_0"])
    enc, _ = model.encode(f[None].to(cuda), [f.shape[0]])
    for w in g["ctc_weights"].tolist():
        model.beam_search = None
        model.init_beam_search(token_list=g["tokens"].tolist(), decoding_ctc_weight=w, beam_size=int(g["beam"]))
        runs = [model.beam_search_features(enc[0])[: int(g["nbest"])] for _ in range(2)]
        assert [(h.yseq, h.score) for h in runs[0]] == [(h.yseq, h.score) for h in runs[1]]      # begin() resets the caches
        for r, h in enumerate(runs[0]):
            assert h.yseq == g[f"nbest_ids_w{w}_{r}"].tolist(), (name, mode, w, r)
            d = abs(h.score - float(g[f"nbest_score_w{w}_{r}"]))
            print(f"{name} {mode} w={w} rank {r}: |d score| {d:.3e}, gap {float(g['gap_nbest_score']):.3e}")
            assert d <= 8 * float(g["gap_nbest_score"]), (name, mode, w, r, d)
    model.beam_search = None


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_bitwise_repeat_and_equal_length_batch(cuda, models, mode):
    g, model, sd, conf = models["legacy_macaron"]
    model.set_precision(mode)
    gen = torch.Generator().manual_seed(4)
    clips = torch.randn(3, 141, 80, generator=gen).to(cuda)
    a, _ = model.encode(clips, [141] * 3)
    b, _ = model.encode(clips, [141] * 3)
    assert torch.equal(a, b)
    for i in range(3):
        solo, _ = model.encode(clips[i: i + 1], [141])
        assert torch.equal(solo[0], a[i]), i


# ------------------------------------------------------------------------------------------------ AutoModel
def _model_dir(path, seed=31):
    os.makedirs(path, exist_ok=True)
    g = load_golden("legacy_macaron")
    tokens = g["tokens"].tolist()
    c = synth.conformer_conf(vocab=len(tokens))
    conf = {"model": "Conformer", "model_conf": {"ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False},
            "encoder": c["encoder"], "encoder_conf": c["encoder_conf"], "decoder": c["decoder"], "decoder_conf": c["decoder_conf"],
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "specaug": "SpecAug", "specaug_conf": {"apply_time_warp": True},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    sd = synth.conformer_state_dict(seed, Conformer(**c))
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return sd, c, tokens


def test_automodel_end_to_end(cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.tokenizer import sentence_postprocess

    sd, c, tokens = _model_dir(str(tmp_path / "conformer"))
    wavs = []
    for i, n in enumerate((16000, 27001, 21503)):
        p = str(tmp_path / f"utt{i}.wav")
        write_wav(p, synth.speech_like(n, seed=20 + i))
        wavs.append(p)
    am = AutoModel(model=str(tmp_path / "conformer"), device="cuda", disable_update=True)
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


# ------------------------------------------------------------------------------------------------ one user-scale shape
def _aishell(cuda, seed=13):
    conf = synth.conformer_conf(**synth.CONFORMER_AISHELL)
    m = Conformer(**conf)
    sd = synth.conformer_state_dict(seed, m)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda), sd, conf


def test_aishell_size_30_seconds_against_the_oracle(cuda):
    m, sd, conf = _aishell(cuda)
    feats = torch.randn(1, 2999, 80, generator=torch.Generator().manual_seed(2))
    assert subsampled_length(2999, 2999) == 749
    e64, _ = O.encoder(O.cast(sd), conf["encoder_conf"], feats.double(), [2999])
    e32, _ = O.encoder(O.cast(sd, torch.float32), conf["encoder_conf"], feats, [2999])
    gap = _maxd(e32, e64)
    for mode in ("fp32", "f16x2"):
        m.set_precision(mode)
        enc, olens = m.encode(feats.to(cuda), [2999])
        assert olens.tolist() == [749]
        _check(f"AISHELL 30 s {mode}", enc, e64, gap, FACTOR[mode])


def test_aishell_size_32_x_10_seconds_finite_and_deterministic(cuda):
    m, sd, conf = _aishell(cuda)
    feats = torch.randn(32, 998, 80, generator=torch.Generator().manual_seed(3)).to(cuda)
    a, olens = m.encode(feats, [998] * 32)
    b, _ = m.encode(feats, [998] * 32)
    assert a.shape == (32, subsampled_length(998, 998), 256) and a.shape[1] == 248 and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    ids = m.ctc_greedy(a, olens)
    assert len(ids) == 32
