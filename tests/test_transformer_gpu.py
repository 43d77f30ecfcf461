"""Transformer on the MI355X through the C ABI: the plain attention kernel and the embedding rows against the float64 oracle on
random inputs, the model against the reference's recorded float64 outputs in both precision modes, greedy ids and n-best, the
shared subsampling through the new handle, bitwise determinism and batch invariance for equal lengths, AutoModel end to end, and
one user-scale shape.

Bars are those of tests/test_conformer_gpu.py: 4 x (fp32) / 8 x (f16x2) the reference's own fp32 - fp64 gap stored beside the
recorded outputs; where no recorded gap exists (random-input kernel tests, the AISHELL-size run) 4 x / 8 x
max |oracle fp32 - oracle fp64| -- another valid fp32 summation order may be that far off -- with the floor 1e-7 of the
relative-position kernel tests."""
import json
import os

import pytest
import torch
import yaml

from funasr_amd import _lib, synth
from funasr_amd.conformer import subsampled_length
from funasr_amd.transformer import Transformer

from . import _transformer_oracle as O
from ._model_dir import write_wav
from .test_transformer import golden_model, load_golden, pin_positional_rows

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
def _attention_inputs(cuda, H, T, klens):
    g = torch.Generator().manual_seed(T)
    B, D = len(klens), 64 * H
    qkv = torch.randn(B, T, 3 * D, generator=g)
    # one row of NaN behind the last sequence: the K / V staging clamps the rows of a partial tile to the last valid key, and a
    # kernel that read one row further instead (a masked row: probability 0) would turn the last sequence's output into NaN
    guard = torch.full((1, 3 * D), float("nan"))
    dev = torch.cat([qkv.reshape(B * T, 3 * D), guard]).contiguous().to(cuda)
    return qkv, dev, torch.tensor(klens, dtype=torch.int32, device=cuda)


def _attention(cuda, dev, kl, B, T, H, fill=None):
    out = torch.empty(B, T, 64 * H, device=cuda) if fill is None else torch.full((B, T, 64 * H), fill, device=cuda)
    _lib.check(_lib.load().pf_k_tf_attention(dev.data_ptr(), kl.data_ptr(), B, T, H, out.data_ptr(), _stream()), "pf_k_tf_attention")
    torch.cuda.synchronize()
    return out


def _attention_against_the_oracle(cuda, H, T, klens):
    qkv, dev, kl = _attention_inputs(cuda, H, T, klens)
    B, D = len(klens), 64 * H

    def ref(dt):
        q, k, v = [t.to(dt).reshape(B, T, H, 64) for t in qkv.split(D, dim=-1)]
        return O.attention(q, k, v, klens)

    out = _attention(cuda, dev, kl, B, T, H)
    r64 = ref(torch.float64)
    _check(f"tf_attention H={H} T={T} klens={klens}", out, r64, max(_maxd(ref(torch.float32), r64), 1e-7), 4.0)


@pytest.mark.parametrize("T,klens", [(1, [1, 1]), (2, [2, 1]), (77, [77, 50]), (129, [129, 128]), (200, [33, 200])])
def test_attention_against_the_oracle(cuda, T, klens):
    """T not a multiple of any tile, ragged key lengths, T = 1 and 2, one key past the 128-query workgroup tile"""
    _attention_against_the_oracle(cuda, 2, T, klens)


@pytest.mark.parametrize("T,klens", [(32, [32, 31, 1]), (33, [33, 32, 1]), (64, [64, 33, 32]), (128, [128, 97, 64]), (160, [160, 129, 128]),
                                      (33, [1, 32, 33])])
def test_attention_on_the_tile_edges_with_four_heads(cuda, T, klens):
    """T and key lengths exactly on, one below and one above the 32-key tile, the 32-query wave tile and the 128-query workgroup
    tile; four heads (the head index enters every pointer), three sequences; T = 33 also with the full-length sequence last, so that
    the row behind its one-key second tile is the guard row"""
    _attention_against_the_oracle(cuda, 4, T, klens)


def test_attention_with_every_key_masked_gives_zero_rows(cuda):
    """a clip the mask rule leaves no encoder frame: the reference masks every key and zeroes the probabilities"""
    _, dev, kl = _attention_inputs(cuda, 2, 40, [0, 40])
    out = _attention(cuda, dev, kl, 2, 40, 2, fill=7.0)
    assert bool((out[0] == 0).all()) and bool(torch.isfinite(out[1]).all()) and float(out[1].abs().max()) > 0


def test_attention_twice_is_bitwise_equal(cuda):
    _, dev, kl = _attention_inputs(cuda, 4, 160, [160, 129, 7])
    a = _attention(cuda, dev, kl, 3, 160, 4)
    b = _attention(cuda, dev, kl, 3, 160, 4)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("T", [1, 3, 61])
def test_embedding_rows_against_the_oracle(cuda, T):
    """y[b T + t] = x[b NE + t] sqrt(D) + pe[t] out of rows with one waste row per sequence (NE = T + 1)"""
    B, D, NE = 3, 128, T + 1
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B, NE, D, generator=g)
    pe = O.abs_pos_table(D)[:T].contiguous()
    xd, ped = x.to(cuda), pe.to(cuda)
    y = torch.empty(B, T, D, device=cuda)
    _lib.check(_lib.load().pf_k_tf_embed_rows(xd.data_ptr(), NE, ped.data_ptr(), B, T, D, float(D) ** 0.5, y.data_ptr(), _stream()),
               "pf_k_tf_embed_rows")
    torch.cuda.synchronize()
    r64 = O.embed_rows(x[:, :T].double(), pe.double())
    _check(f"embed rows T={T}", y, r64, max(_maxd(O.embed_rows(x[:, :T], pe), r64), 1e-7), 4.0)
    # without the table: the Conformer's call, the scale alone
    _lib.check(_lib.load().pf_k_tf_embed_rows(xd.data_ptr(), NE, None, B, T, D, float(D) ** 0.5, y.data_ptr(), _stream()), "pf_k_tf_embed_rows")
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), x[:, :T] * torch.tensor(float(D) ** 0.5, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ the handle
def _encoder_model(cuda, conf, seed, mode):
    m = Transformer(**conf)
    sd = synth.transformer_state_dict(seed, m)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda).set_precision(mode), sd


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("enc_blocks", [0, 1])
@pytest.mark.parametrize("input_size", [7, 83, 256])
def test_subsampling_feature_counts_and_shortest_batches_against_the_oracle(cuda, input_size, enc_blocks, mode):
    """the shared subsampling through the new handle: the feature counts at the ends of the accepted range and an odd one, batches
    of 7 .. 15 frames (T = 1, 1, 1, 2, 2, 3), ragged lengths down to 1; with one block T = 1 .. 3 also goes through the attention
    kernel. Then the shape order on one handle: long, shortest, long, each bitwise what a fresh handle gives."""
    conf = synth.transformer_conf(input_size=input_size, enc_blocks=enc_blocks)
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
    fresh, _ = _encoder_model(cuda, conf, 3, mode)
    assert torch.equal(a, fresh.encode(long, [141] * 3)[0])


@pytest.fixture(scope="module")
def live(cuda):
    """model A after an encode with seed 1 and a load_state_dict of seed 2 on the live handle; B is a fresh model with seed 2"""
    conf = synth.transformer_conf(enc_blocks=1)
    g = torch.Generator().manual_seed(0)
    lens = [23, 17]
    feats = torch.randn(2, 23, 80, generator=g)
    feats[1, 17:] = 0
    feats = feats.to(cuda)
    a, _ = _encoder_model(cuda, conf, 1, "f16x2")
    a.encode(feats, lens)                                                     # primes the handle with seed 1
    a.load_state_dict(synth.transformer_state_dict(2, a), strict=True)
    b, _ = _encoder_model(cuda, conf, 2, "f16x2")
    return conf, a, b.encode(feats, lens)[0], feats, lens


def test_weights_and_precision_replaced_on_a_live_handle(cuda, live):
    """One handle through load_state_dict and set_precision: every encode equals a fresh model's with the same weights and mode, so
    nothing derived at load time (conv taps, output linear, plane caches and exponents) outlives the weights or the mode it was
    made for: the prepared state carries the version of the tensor table it was made from."""
    conf, a, want_x2, feats, lens = live
    assert torch.equal(a.encode(feats, lens)[0], want_x2)
    a.set_precision("fp32")
    c, _ = _encoder_model(cuda, conf, 2, "fp32")
    want_32 = c.encode(feats, lens)[0]
    assert torch.equal(a.encode(feats, lens)[0], want_32) and not torch.equal(want_32, want_x2)
    a.set_precision("f16x2")
    assert torch.equal(a.encode(feats, lens)[0], want_x2)


def test_num_frames_entry_point_is_the_mask_rule(cuda):
    m = Transformer(**synth.transformer_conf(enc_blocks=0)).to(cuda)
    lib, h = m.encoder._ensure_handle()
    for padded in (7, 101, 247, 998):
        for n in (1, 2, 3, padded // 2, padded):
            assert lib.pf_tfencoder_num_frames(h, n, padded) == subsampled_length(n, padded)
    assert lib.pf_tfencoder_num_frames(h, 5, 6) == -1


# ------------------------------------------------------------------------------------------------ model against the golden
@pytest.fixture(scope="module")
def model(cuda):
    g = load_golden()
    m, sd, conf = golden_model(g)
    if pin_positional_rows(m, g):
        print("this host's float32 exp() builds another positional table than the recording's: recorded rows pinned")
    assert torch.equal(m.encoder.pos_rows(g["pos_rows"].shape[0]), torch.from_numpy(g["pos_rows"]))
    return g, m.to(cuda), sd, conf


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_model_against_the_references_recorded_outputs(cuda, model, mode):
    g, m, sd, conf = model
    m.set_precision(mode)
    lens = [int(n) for n in g["lens"]]
    feats = [torch.from_numpy(g[f"feats_{i}"]) for i in range(len(lens))]
    for i, f in enumerate(feats):
        enc, olens = m.encode(f[None].to(cuda), [lens[i]])
        assert olens.tolist() == [g[f"enc_{i}"].shape[0]]
        _check(f"{mode} enc {i}", enc[0], g[f"enc_{i}"], float(g[f"gap_enc_{i}"]), FACTOR[mode])
        _check(f"{mode} ctc {i}", m.ctc.log_softmax(enc)[0], g[f"ctc_{i}"], float(g[f"gap_ctc_{i}"]), FACTOR[mode])
        assert m.ctc_greedy(enc, olens)[0] == g[f"greedy_{i}"].tolist()
    pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    enc, olens = m.encode(pad.to(cuda), lens)
    assert olens.tolist() == g["batch_olens"].tolist() == [26, 41, 61]       # the reference's lengths exactly
    lp = m.ctc.log_softmax(enc)
    greedy = m.ctc_greedy(enc, olens)
    for i, n in enumerate(olens.tolist()):
        _check(f"{mode} batch enc {i}", enc[i, :n], g[f"batch_enc_{i}"], float(g[f"gap_batch_enc_{i}"]), FACTOR[mode])
        _check(f"{mode} batch ctc {i}", lp[i, :n], g[f"batch_ctc_{i}"], float(g[f"gap_batch_ctc_{i}"]), FACTOR[mode])
        assert greedy[i] == g[f"batch_greedy_{i}"].tolist()
    # forward_one_step over the recorded memory
    dec = m.decoder.set_memory(torch.from_numpy(g["enc_1"]).float().to(cuda))
    for j, pre in enumerate(g["prefixes"]):
        got = O.score_prefix(dec, [int(t) for t in str(pre).split(",")])
        _check(f"{mode} step {j}", got, g[f"step_{j}"], float(g[f"gap_step_{j}"]), FACTOR[mode])


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_beam_search_nbest_equals_the_references(cuda, model, mode):
    g, m, sd, conf = model
    m.set_precision(mode)
    f = torch.from_numpy(g["feats_0"])
    enc, _ = m.encode(f[None].to(cuda), [f.shape[0]])
    for w in g["ctc_weights"].tolist():
        m.beam_search = None
        m.init_beam_search(token_list=g["tokens"].tolist(), decoding_ctc_weight=w, beam_size=int(g["beam"]))
        nbest = m.beam_search_features(enc[0])[: int(g["nbest"])]
        assert len(nbest) == int(g["nbest"])
        for r, h in enumerate(nbest):
            assert h.yseq == g[f"nbest_ids_w{w}_{r}"].tolist(), (mode, w, r)
            d = abs(h.score - float(g[f"nbest_score_w{w}_{r}"]))
            print(f"{mode} w={w} rank {r}: |d score| {d:.3e}, gap {float(g['gap_nbest_score']):.3e}")
            assert d <= 8 * float(g["gap_nbest_score"]), (mode, w, r, d)
    m.beam_search = None


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_bitwise_repeat_and_equal_length_batch(cuda, model, mode):
    g, m, sd, conf = model
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
    tokens = load_golden()["tokens"].tolist()
    c = synth.transformer_conf(vocab=len(tokens))
    conf = {"model": "Transformer", "model_conf": {"ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False},
            "encoder": c["encoder"], "encoder_conf": c["encoder_conf"], "decoder": c["decoder"], "decoder_conf": c["decoder_conf"],
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "specaug": "SpecAug", "specaug_conf": {"apply_time_warp": True},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    sd = synth.transformer_state_dict(seed, Transformer(**c))
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return sd, c, tokens


def test_automodel_end_to_end(cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.tokenizer import sentence_postprocess

    sd, c, tokens = _model_dir(str(tmp_path / "transformer"))
    wavs = []
    for i, n in enumerate((16000, 27001, 21503)):
        p = str(tmp_path / f"utt{i}.wav")
        write_wav(p, synth.speech_like(n, seed=20 + i))
        wavs.append(p)
    am = AutoModel(model=str(tmp_path / "transformer"), device="cuda", disable_update=True)
    assert isinstance(am.model, Transformer)
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
    conf = synth.transformer_conf(**synth.TRANSFORMER_AISHELL)
    m = Transformer(**conf)
    sd = synth.transformer_state_dict(seed, m)
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
