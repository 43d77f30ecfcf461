"""LCB-Net on the MI355X through the C ABI: the audio-text cross-attention and the token rows against the float64 oracle on random
inputs at their tile edges, the text encoder and the fusion handle against the reference's recorded float64 rows for every text length,
ragged batches through the host lengths, weights replaced on live handles, the model's greedy ids and n-best in both precision modes,
and AutoModel end to end.

Bars are those of tests/test_transformer_gpu.py: 4 x for the fp32 handles (the text encoder and the fusion layer run exact-fp32 GEMMs
in every mode) and 8 x where an f16x2 audio encoder feeds them, applied to the reference's own fp32 - fp64 gap stored beside the
recorded outputs; for random-input kernel tests 4 x max |oracle fp32 - oracle fp64| with the floor 1e-7."""
import json
import os

import pytest
import torch
import yaml

from funasr_amd import _lib, synth
from funasr_amd.lcbnet import LCBNet

from . import _lcbnet_oracle as O
from ._model_dir import write_wav
from .test_lcbnet import N_CLIPS, N_TEXTS, golden_model, load_golden, pin_positional_rows

pytestmark = pytest.mark.gpu
FACTOR = {"fp32": 4.0, "f16x2": 8.0}
VOCAB = 300


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _maxd(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _check(tag, got, want64, gap, factor):
    d = _maxd(got, want64)
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / max(gap, 1e-30):.2f} (bar {factor:g})")
    assert d <= factor * gap, (tag, d, gap)


# ------------------------------------------------------------------------------------------------ the cross-attention kernel
def _klens(L):
    return [L, max(1, L - 7)]


def _cross_inputs(cuda, H, Tq, L, klens, ldq=None):
    """q [B, Tq, D] (rows ldq floats apart on the device) and kv [B, L, 2 D]. On the device a row of NaN stands behind every
    sequence's last valid key (where the sequence is shorter than L) and one behind the buffer: the K / V staging clamps the rows
    of a partial tile to the last valid key, and a kernel that read one row further instead (a masked key: probability 0) would
    turn the output into NaN."""
    g = torch.Generator().manual_seed(1000 * Tq + L)
    B, D = len(klens), 64 * H
    ldq = ldq or D
    q = torch.randn(B, Tq, D, generator=g)
    kv = torch.randn(B, L, 2 * D, generator=g)
    qd = torch.full((B * Tq, ldq), float("nan"))
    qd[:, :D] = q.reshape(B * Tq, D)
    kvd = torch.cat([kv.reshape(B * L, 2 * D), torch.full((1, 2 * D), float("nan"))])
    for b, n in enumerate(klens):
        if n < L:
            kvd[b * L + n] = float("nan")
    return q, kv, qd.contiguous().to(cuda), kvd.contiguous().to(cuda), torch.tensor(klens, dtype=torch.int32, device=cuda)


def _cross(cuda, qd, kvd, kl, B, Tq, L, H, out=None):
    out = torch.empty(B, Tq, 64 * H, device=cuda) if out is None else out
    _lib.check(_lib.load().pf_k_tf_cross_attention(qd.data_ptr(), qd.shape[1], kvd.data_ptr(), kl.data_ptr(), B, Tq, L, H, out.data_ptr(),
                                                   _stream()), "pf_k_tf_cross_attention")
    torch.cuda.synchronize()
    return out


def _cross_reference(q, kv, klens, H, dt):
    B, Tq, D = q.shape
    L = kv.shape[1]
    k, v = kv.to(dt).split(D, dim=-1)
    return O.cross_attention(q.to(dt).reshape(B, Tq, H, 64), k.reshape(B, L, H, 64), v.reshape(B, L, H, 64), klens)


# Tq on, below and above the 32-query workgroup and the 128-query tile of the sibling kernel; L = 1, 2 and on, below and above the
# 32-key tile, two tiles and a key, the longest recorded text. Every value of either list stands with several of the other.
SHAPES = [(1, 1), (1, 33), (1, 120), (2, 2), (2, 32), (33, 1), (33, 31), (33, 65), (128, 2), (128, 32), (128, 120), (129, 31), (129, 33),
          (200, 32), (200, 65), (200, 120)]


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("Tq,L", SHAPES)
def test_cross_attention_against_the_oracle_at_the_tile_edges(cuda, Tq, L, H):
    klens = _klens(L)
    q, kv, qd, kvd, kl = _cross_inputs(cuda, H, Tq, L, klens)
    out = _cross(cuda, qd, kvd, kl, 2, Tq, L, H)
    assert bool(torch.isfinite(out).all()), "a row at or past klens[b] was read"
    r64 = _cross_reference(q, kv, klens, H, torch.float64)
    _check(f"tf_cross_attention H={H} Tq={Tq} L={L} klens={klens}", out, r64, max(_maxd(_cross_reference(q, kv, klens, H, torch.float32), r64), 1e-7), 4.0)


def test_cross_attention_reads_queries_at_their_own_row_stride(cuda):
    """the queries out of a wider buffer (the q | k | v layout of the self-attention: ldq = 3 D), NaN in the columns it must not read"""
    H, Tq, L = 4, 70, 45
    klens = [38, 45]                                                   # the full-length sequence last: its guard is the row behind the buffer
    q, kv, qd, kvd, kl = _cross_inputs(cuda, H, Tq, L, klens, ldq=3 * 64 * H)
    out = _cross(cuda, qd, kvd, kl, 2, Tq, L, H)
    r64 = _cross_reference(q, kv, klens, H, torch.float64)
    _check("tf_cross_attention ldq = 3 D", out, r64, max(_maxd(_cross_reference(q, kv, klens, H, torch.float32), r64), 1e-7), 4.0)


def test_cross_attention_with_every_key_masked_gives_zero_rows(cuda):
    L, Tq = 33, 40
    _, _, qd, kvd, kl = _cross_inputs(cuda, 2, Tq, L, [0, L])
    out = _cross(cuda, qd, kvd, kl, 2, Tq, L, 2, out=torch.full((2, Tq, 128), 7.0, device=cuda))
    assert bool((out[0] == 0).all()) and bool(torch.isfinite(out[1]).all()) and float(out[1].abs().max()) > 0


def test_cross_attention_twice_is_bitwise_equal(cuda):
    _, _, qd, kvd, kl = _cross_inputs(cuda, 4, 200, 120, _klens(120))
    a = _cross(cuda, qd, kvd, kl, 2, 200, 120, 4)
    b = _cross(cuda, qd, kvd, kl, 2, 200, 120, 4)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("Tq", [1, 33, 129])
def test_cross_attention_overwrites_its_rows_and_nothing_beyond(cuda, Tq):
    H, L, B, extra = 2, 33, 2, 5
    _, _, qd, kvd, kl = _cross_inputs(cuda, H, Tq, L, _klens(L))
    buf = torch.full((B * Tq + extra, 64 * H), 7.0, device=cuda)
    _cross(cuda, qd, kvd, kl, B, Tq, L, H, out=buf)
    assert bool((buf[: B * Tq] != 7.0).all()) and bool(torch.isfinite(buf[: B * Tq]).all()) and bool((buf[B * Tq:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ token rows
@pytest.mark.parametrize("L", [1, 5, 129])
def test_token_rows_against_the_oracle(cuda, L):
    """y[b, t] = E[ids[b, t]] sqrt(D) + pe[t], ids 0 and vocab - 1 among them"""
    B, D = 2, 128
    g = torch.Generator().manual_seed(L)
    table = torch.randn(VOCAB, D, generator=g)
    ids = torch.randint(0, VOCAB, (B, L), generator=g)
    ids[0, 0], ids[1, -1] = 0, VOCAB - 1
    pe = O.abs_pos_table(D)[:L].contiguous()
    td, idd, ped = table.to(cuda), ids.to(device=cuda, dtype=torch.int32).contiguous(), pe.to(cuda)
    y = torch.empty(B, L, D, device=cuda)
    _lib.check(_lib.load().pf_k_text_embed_rows(td.data_ptr(), idd.data_ptr(), ped.data_ptr(), B, L, D, float(D) ** 0.5, y.data_ptr(), _stream()),
               "pf_k_text_embed_rows")
    torch.cuda.synchronize()
    r64 = O.token_rows(table.double(), ids, pe.double())
    _check(f"token rows L={L}", y, r64, max(_maxd(O.token_rows(table, ids, pe), r64), 1e-7), 4.0)


# ------------------------------------------------------------------------------------------------ the handles
@pytest.fixture(scope="module")
def model(cuda):
    g = load_golden()
    m, sd, conf = golden_model(g)
    if pin_positional_rows(m, g):
        print("this host's float32 exp() builds another positional table than the recording's: recorded rows pinned")
    return g, m.to(cuda), sd, conf


def _ids(g, j):
    return O.shift_ids(g[f"ocr_{j}"].tolist())


def test_textencoder_forward_rejects_bad_ids_and_lengths_without_launching(cuda, model):
    g, m, _, _ = model
    lib, h = m.text_encoder._ensure_handle()
    out = torch.full((1, 3, 128), 7.0, device=cuda)
    C = _lib.C
    for bad in (VOCAB, -1):
        rc = lib.pf_textencoder_forward(h, (C.c_int32 * 3)(5, bad, 7), (C.c_int32 * 1)(3), 1, 3, out.data_ptr(), _stream())
        assert rc != 0 and str(bad) in _lib.last_error() and "vocabulary" in _lib.last_error()
    rc = lib.pf_textencoder_forward(h, (C.c_int32 * 3)(5, 6, 7), (C.c_int32 * 1)(3), 1, 0, out.data_ptr(), _stream())
    assert rc != 0 and "0 tokens" in _lib.last_error()
    rc = lib.pf_textencoder_forward(h, (C.c_int32 * 3)(5, 6, 7), (C.c_int32 * 1)(4), 1, 3, out.data_ptr(), _stream())
    assert rc != 0 and "length" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="300"):
        m.text_encoder([[1, 300]], [2])
    with pytest.raises(ValueError, match="tokens"):
        m.text_encoder(torch.zeros(1, 0, dtype=torch.long), [0])


@pytest.mark.parametrize("j", range(N_TEXTS))
def test_text_encoder_and_fusion_against_the_references_recorded_rows(cuda, model, j):
    """every text length: the text encoder's rows; then, over the RECORDED audio rows of both clips, the fusion output and the fused
    memory (add_input: the sum inside the last GEMM)"""
    g, m, _, _ = model
    ids = _ids(g, j)
    text, olens, _ = m.text_encoder([ids], [len(ids)])
    assert olens.tolist() == [len(ids)]
    _check(f"text {j} (L={len(ids)})", text[0], g[f"text_{j}"], float(g[f"gap_text_{j}"]), 4.0)
    for c in range(N_CLIPS):
        enc = torch.from_numpy(g[f"enc_{c}"]).float()[None].to(cuda)
        fus, _, _, _ = m.fusion_encoder(enc, None, text, None)
        _check(f"fusion clip {c} text {j}", fus[0], g[f"fusion_{c}_{j}"], float(g[f"gap_fusion_{c}_{j}"]), 4.0)
        fused, _, _, _ = m.fusion_encoder(enc, None, text, None, add_input=True)
        _check(f"fused clip {c} text {j}", fused[0], g[f"fused_{c}_{j}"], float(g[f"gap_fused_{c}_{j}"]), 4.0)
        assert torch.equal(fused, enc + fus)                           # the reference's order of the sum: x + (x2 + ffn)


def test_ragged_batches_through_the_host_lengths_equal_each_text_alone(cuda, model):
    g, m, _, _ = model
    a, b = _ids(g, 2), _ids(g, 3)                                       # 6 and 33 ids
    L = len(b)
    both, olens, _ = m.text_encoder([a + [0] * (L - len(a)), b], [len(a), L])
    assert olens.tolist() == [len(a), L]
    ta, _, _ = m.text_encoder([a], [len(a)])
    tb, _, _ = m.text_encoder([b], [L])
    assert torch.equal(both[0, : len(a)], ta[0]) and torch.equal(both[1], tb[0])
    # the fusion layer: two clips of unequal length against memories of unequal length
    ea = torch.from_numpy(g["enc_0"]).float().to(cuda)
    eb = torch.from_numpy(g["enc_1"]).float().to(cuda)
    T = eb.shape[0]
    x = torch.zeros(2, T, 128, device=cuda)
    x[0, : ea.shape[0]], x[1] = ea, eb
    out, _, _, _ = m.fusion_encoder(x, [ea.shape[0], T], both, [len(a), L], add_input=True)
    oa, _, _, _ = m.fusion_encoder(ea[None], None, ta, None, add_input=True)
    ob, _, _, _ = m.fusion_encoder(eb[None], None, tb, None, add_input=True)
    assert torch.equal(out[0, : ea.shape[0]], oa[0]) and torch.equal(out[1], ob[0])


def test_weights_replaced_on_live_handles(cuda):
    """one text encoder and one fusion handle through load_state_dict: every forward equals a fresh model's with the same weights"""
    conf = synth.lcbnet_conf(text_blocks=1)
    ids = [[3, 0, 299, 17, 150]]
    x = torch.randn(1, 37, 128, generator=torch.Generator().manual_seed(0)).to(cuda)

    def make(seed):
        m = LCBNet(**conf)
        m.load_state_dict(synth.lcbnet_state_dict(seed, m), strict=True)
        return m.to(cuda)

    def run(m):
        t, _, _ = m.text_encoder(ids, [5])
        return t, m.fusion_encoder(x, None, t, None)[0]

    a = make(1)
    t1, f1 = run(a)
    a.load_state_dict(synth.lcbnet_state_dict(2, a), strict=True)
    t2, f2 = run(a)
    tb, fb = run(make(2))
    assert torch.equal(t2, tb) and torch.equal(f2, fb) and not torch.equal(t1, t2) and not torch.equal(f1, f2)


# ------------------------------------------------------------------------------------------------ the model against the golden
@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("c", range(N_CLIPS))
def test_model_fused_memory_and_greedy_ids_against_the_recording(cuda, model, mode, c):
    g, m, _, _ = model
    m.set_precision(mode)
    f = torch.from_numpy(g[f"feats_{c}"])
    enc, olens = m.encode(f[None].to(cuda), [f.shape[0]])
    assert olens.tolist() == [g[f"enc_{c}"].shape[0]]
    _check(f"{mode} enc {c}", enc[0], g[f"enc_{c}"], float(g[f"gap_enc_{c}"]), FACTOR[mode])
    greedy = []
    for j in range(N_TEXTS):
        fused = m.fuse(enc, _ids(g, j))
        _check(f"{mode} fused clip {c} text {j}", fused[0], g[f"fused_{c}_{j}"], float(g[f"gap_fused_{c}_{j}"]), FACTOR[mode])
        greedy.append(m.ctc_greedy(fused, olens)[0])
        assert greedy[-1] == g[f"greedy_{c}_{j}"].tolist(), (mode, c, j)
    assert len({tuple(x) for x in greedy}) >= 2                        # the recorded difference between the texts


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("c", range(N_CLIPS))
@pytest.mark.parametrize("j", range(N_TEXTS))
def test_beam_search_nbest_equals_the_references(cuda, model, mode, c, j):
    g, m, _, _ = model
    m.set_precision(mode)
    f = torch.from_numpy(g[f"feats_{c}"])
    enc, _ = m.encode(f[None].to(cuda), [f.shape[0]])
    fused = m.fuse(enc, _ids(g, j))
    for w in g["ctc_weights"].tolist():
        m.beam_search = None
        m.init_beam_search(token_list=g["tokens"].tolist(), decoding_ctc_weight=w, beam_size=int(g["beam"]))
        nbest = m.beam_search_features(fused[0])[: int(g["nbest"])]
        assert len(nbest) == int(g["nbest"])
        for r, h in enumerate(nbest):
            assert h.yseq == g[f"nbest_ids_w{w}_{c}_{j}_{r}"].tolist(), (mode, w, r)
            d = abs(h.score - float(g[f"nbest_score_w{w}_{c}_{j}_{r}"]))
            print(f"{mode} clip {c} text {j} w={w} rank {r}: |d score| {d:.3e}, gap {float(g['gap_nbest_score']):.3e}")
            assert d <= 8 * float(g["gap_nbest_score"]), (mode, w, r, d)
    m.beam_search = None


def test_two_texts_give_the_recorded_different_nbest(cuda, model):
    g, m, _, _ = model
    m.set_precision("f16x2")
    f = torch.from_numpy(g["feats_0"])
    enc, _ = m.encode(f[None].to(cuda), [f.shape[0]])
    m.beam_search = None
    m.init_beam_search(token_list=g["tokens"].tolist(), decoding_ctc_weight=0.3, beam_size=int(g["beam"]))
    best = [m.beam_search_features(m.fuse(enc, _ids(g, j))[0])[0].yseq for j in (1, 2)]
    m.beam_search = None
    assert best[0] != best[1] and best == [g[f"nbest_ids_w0.3_0_{j}_0"].tolist() for j in (1, 2)]


# ------------------------------------------------------------------------------------------------ AutoModel
def _model_dir(path):
    os.makedirs(path, exist_ok=True)
    g = load_golden()
    tokens = g["tokens"].tolist()
    c = synth.lcbnet_conf(vocab=len(tokens))
    conf = {"model": "LCBNet", "model_conf": {"ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False, "select_num": 2,
                                              "select_length": 3, "insert_blank": True},
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "specaug": "SpecAug", "specaug_conf": {"apply_time_warp": True},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    for k in ("encoder", "decoder", "text_encoder", "fusion_encoder", "bias_predictor"):
        conf[k], conf[k + "_conf"] = c[k], c[k + "_conf"]
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    sd = synth.lcbnet_state_dict(int(g["seed"]), LCBNet(**c))
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return g, tokens


def test_automodel_end_to_end(cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel

    g, tokens = _model_dir(str(tmp_path / "lcbnet"))
    wav = str(tmp_path / "utt0.wav")
    write_wav(wav, synth.speech_like(27001, seed=20))
    am = AutoModel(model=str(tmp_path / "lcbnet"), device="cuda", disable_update=True)
    assert isinstance(am.model, LCBNet) and am.model.sos == am.model.eos == len(tokens) - 1
    pin_positional_rows(am.model, g)
    opts = dict(beam_size=5, decoding_ctc_weight=0.3, nbest=2)
    # (the CharTokenizer cuts a text into characters: the texts hold the one-character tokens, ids 3 .. 298)
    raw = {j: [i for i in g[f"ocr_{j}"].tolist() if 3 <= i < len(tokens) - 1] for j in (2, 4)}
    words = [tokens[i] for i in raw[2]]

    def staged(raw_ids):
        """the same decode through the model's own stages over the features the frontend makes of the wav"""
        from funasr_amd.audio import batch_to_features
        m = am.model
        speech, lens, _ = batch_to_features([wav], None, am.kwargs["frontend"], dict(am.kwargs, device="cuda"))
        enc, _ = m.encode(speech.float(), [int(v) for v in lens.tolist()])
        nbest = m.beam_search_features(m.fuse(enc, m.ocr_ids(raw_ids))[0])[:2]
        return [[tokens[t] for t in h.yseq[1:-1] if t not in (0, len(tokens) - 1)] for h in nbest]

    # a pair with the text as a string, and as a text file (a list file, as the reference reads it: `<key> <text>` per line)
    res = am.generate(input=(wav, " ".join(words)), data_type=("sound", "text"), **opts)
    assert len(res) == 2 and all(set(r) >= {"key", "token", "text"} for r in res)
    assert [r["token"] for r in res] == staged(raw[2])
    listing = tmp_path / "ocr.txt"
    listing.write_text("utt0 " + " ".join(words) + "\n", encoding="utf-8")
    out_dir = tmp_path / "out"
    res_file = am.generate(input=(wav, str(listing)), data_type=("sound", "text"), output_dir=str(out_dir), **opts)
    assert [r["key"] for r in res_file] == ["utt0", "utt0"]
    assert [(r["token"], r["text"]) for r in res_file] == [(r["token"], r["text"]) for r in res]
    for n, r in enumerate(res_file):                                   # the writers of AttentionEncoderDecoder.inference
        d = out_dir / f"{n + 1}best_recog"
        assert (d / "token").read_text(encoding="utf-8").strip() == ("utt0 " + " ".join(r["token"])).strip()
        assert (d / "text").read_text(encoding="utf-8").strip() == ("utt0 " + r["text"]).strip()
    # a plain wav decodes with the default ids [294, 0] ...
    plain = am.generate(input=wav, **opts)
    assert [r["token"] for r in plain] == staged(None) and plain[0]["key"] == "utt0"
    other = am.generate(input=(wav, "".join(tokens[i] for i in raw[4])), data_type=("sound", "text"), **opts)
    assert [r["token"] for r in other] == staged(raw[4])
    assert len({tuple(tuple(r["token"]) for r in x) for x in (res, plain, other)}) >= 2       # the text matters end to end
    with pytest.raises(ValueError, match="299"):                       # "<" is no token: <unk> = 299, past the vocabulary after the shift
        am.generate(input=(wav, "<blank>"), data_type=("sound", "text"), **opts)
    # ... and over the recorded features (the route the reference's own inference cannot take) the recorded default-ids n-best
    for c in range(N_CLIPS):
        rec = am.generate(input=torch.from_numpy(g[f"feats_{c}"]), data_type="fbank", **opts)
        assert len(rec) == 2
        for r, hyp in enumerate(rec):
            want = [t for t in g[f"nbest_ids_w0.3_{c}_1_{r}"].tolist()[1:-1] if t not in (0, len(tokens) - 1)]
            assert hyp["token"] == [tokens[t] for t in want], (c, r)
    with pytest.raises(NotImplementedError, match="batch decoding is not implemented"):
        am.generate(input=[wav, wav], batch_size=2, **opts)
