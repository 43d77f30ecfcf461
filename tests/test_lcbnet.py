"""LCB-Net, CPU side: registry, the reference's state-dict names and shapes at both sizes, refused options, the OCR ids (shift, default
ids, errors), sos / eos, the batch refusal, the (sound, text) pair route, and the float64 oracle (tests/_lcbnet_oracle.py) with the host
beam search against the reference's recorded float64 outputs (tests/golden/lcbnet.npz, written by tools/make_golden_lcbnet.py)."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import synth
from funasr_amd.register import tables
from funasr_amd.transformer_search import BeamSearchTransformer

from . import _lcbnet_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_CLIPS, N_TEXTS = 2, 5


def load_golden():
    """the recorded arrays plus `fused_<c>_<j>` = `enc_<c> + fusion_<c>_<j>`: bitwise the reference's float64 `encoder_out +
    fusion_out` (the same float64 addition of the same two arrays), which the generator checks and therefore does not store twice"""
    g = dict(np.load(os.path.join(GOLDEN, "lcbnet.npz"), allow_pickle=False))
    for c in range(N_CLIPS):
        for j in range(N_TEXTS):
            g[f"fused_{c}_{j}"] = g[f"enc_{c}"] + g[f"fusion_{c}_{j}"]
    return g


def golden_model(g):
    from funasr_amd.lcbnet import LCBNet

    conf = synth.lcbnet_conf(vocab=len(g["tokens"]))
    model = LCBNet(**conf)
    sd = synth.lcbnet_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def pin_positional_rows(model, g):
    """as tests/test_transformer.py pin_positional_rows, for the tables of both encoders. Returns True when it had to."""
    rows = torch.from_numpy(g["pos_rows"])
    pinned = False
    for enc in (model.encoder, model.text_encoder):
        own = enc.pos_rows(rows.shape[0])
        assert float((own - rows).abs().max()) <= 1e-3
        if not torch.equal(own, rows):
            own.copy_(rows)
            enc.mark_dirty()
            pinned = True
    return pinned


class _Tok:
    """a stand-in tokenizer: one token per space-separated word"""
    def __init__(self, tokens):
        self.token_list = list(tokens)
        self._ids = {t: i for i, t in enumerate(self.token_list)}

    def encode(self, text):
        return [self._ids[t] for t in text.split()]

    def ids2tokens(self, ids):
        return [self.token_list[i] for i in ids]


# ------------------------------------------------------------------------------------------------ registry, state dict, refusals
def test_registry_keys():
    from funasr_amd.conformer import AttentionEncoderDecoder
    from funasr_amd.install import hip_classes
    from funasr_amd.lcbnet import ConvBiasPredictor, FusionSANEncoder, LCBNet, TransformerTextEncoder

    assert tables.model_classes["LCBNet"] is LCBNet and issubclass(LCBNet, AttentionEncoderDecoder) and LCBNet._encoder == "TransformerEncoder"
    assert tables.encoder_classes["TransformerTextEncoder"] is TransformerTextEncoder
    assert tables.encoder_classes["FusionSANEncoder"] is FusionSANEncoder
    assert tables.encoder_classes["ConvBiasPredictor"] is ConvBiasPredictor
    have = hip_classes()
    for triple in (("model_classes", "LCBNet", LCBNet), ("encoder_classes", "TransformerTextEncoder", TransformerTextEncoder),
                   ("encoder_classes", "FusionSANEncoder", FusionSANEncoder), ("encoder_classes", "ConvBiasPredictor", ConvBiasPredictor)):
        assert triple in have
    import funasr_amd.auto_model  # noqa: F401  (imports the module, as it does for every family)


def test_state_dict_names_and_shapes_are_the_references_at_both_sizes():
    from funasr_amd.lcbnet import LCBNet

    ref = json.load(open(os.path.join(GOLDEN, "lcbnet_state_dict.json")))
    assert ref["conf"] == synth.lcbnet_conf(**synth.LCBNET_ZOO_LIKE)
    m = LCBNet(**ref["conf"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert not any("pe" == k.split(".")[-1] or "pos_table" in k for k in ref["shapes"])
    for k in ("text_encoder.embed.0.weight", "text_encoder.encoders.5.norm2.bias", "fusion_encoder.src_attn.linear_k.weight",
              "fusion_encoder.norm3.weight", "bias_predictor.conv1d.weight", "bias_predictor.output_linear.bias", "bias_predictor.atten.linear_q.bias"):
        assert k in ref["shapes"], k
    sd = {k: torch.randn(shp) for k, shp in ref["shapes"].items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.fusion_encoder.src_attn.linear_v.bias, sd["fusion_encoder.src_attn.linear_v.bias"])
    # the tiny size of tests/golden/lcbnet.npz
    g = load_golden()
    tiny, tsd, conf = golden_model(g)
    assert conf == ref["tiny_conf"]
    assert {k: list(v.shape) for k, v in tiny.state_dict().items()} == ref["tiny_shapes"] and set(tsd) == set(ref["tiny_shapes"])
    assert ref["tiny_shapes"]["text_encoder.embed.0.weight"] == [300, 128] and ref["tiny_shapes"]["bias_predictor.conv1d.weight"] == [128, 1, 7]


@pytest.mark.parametrize("where,conf,word", [
    ("text_encoder", {"attention_heads": 4}, "attention_heads"), ("text_encoder", {"output_size": 192, "attention_heads": 2}, "output_size"),
    ("text_encoder", {"normalize_before": False}, "normalize_before"), ("text_encoder", {"concat_after": True}, "concat_after"),
    ("text_encoder", {"linear_units": 250}, "linear_units"), ("text_encoder", {"pos_enc_class": "ScaledPositionalEncoding"}, "pos_enc_class"),
    ("text_encoder", {"output_size": 256, "attention_heads": 4}, "text_encoder_conf output_size"),
    ("fusion_encoder", {"attention_heads": 4}, "attention_heads"), ("fusion_encoder", {"normalize_before": False}, "normalize_before"),
    ("fusion_encoder", {"concat_after": True}, "concat_after"), ("fusion_encoder", {"attention_dim": 256}, "attention_dim"),
    ("fusion_encoder", {"linear_units": 250}, "linear_units"),
    ("fusion_encoder", {"size": 256, "attention_dim": 256, "attention_heads": 4}, "fusion_encoder_conf size"),
    ("model", {"text_encoder": "SANMEncoder"}, "text_encoder"), ("model", {"fusion_encoder": None}, "fusion_encoder"),
    ("model", {"bias_predictor": "CifPredictorV2"}, "bias_predictor"), ("model", {"encoder": "ConformerEncoder"}, "ConformerEncoder"),
    ("model", {"interctc_weight": 0.3}, "interctc_weight"), ("model", {"ctc_weight": 1.0}, "decoder")])
def test_unsupported_options_raise_and_name_the_option(where, conf, word):
    from funasr_amd.lcbnet import LCBNet

    c = synth.lcbnet_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        LCBNet(**c)


def test_bias_predictor_holds_parameters_and_refuses_to_run():
    from funasr_amd.lcbnet import ConvBiasPredictor

    p = ConvBiasPredictor(size=128, attention_heads=2, linear_units=256)
    assert len(p.state_dict()) == 20
    with pytest.raises(NotImplementedError, match="inference never runs"):
        p(torch.zeros(1, 3, 128), torch.zeros(1, 5, 128))


# ------------------------------------------------------------------------------------------------ ids, sos / eos, the input routes
def test_sos_eos_are_the_last_token_whatever_is_passed_and_the_beam_defaults_are_the_references():
    from funasr_amd.lcbnet import LCBNet

    m = LCBNet(**dict(synth.lcbnet_conf(), sos=1, eos=2))
    assert m.sos == m.eos == 299
    m.init_beam_search(token_list=["t"] * 300)
    b = m.beam_search
    assert (b.beam_size, b.w_ctc, b.w_dec, b.w_len, b.sos, b.eos, b.pre_beam) == (20, 0.3, 0.7, 0.0, 299, 299, True)
    m.init_beam_search(token_list=["t"] * 300, beam_size=5, decoding_ctc_weight=0.0, penalty=0.5)
    assert (m.beam_search.beam_size, m.beam_search.w_ctc, m.beam_search.w_len) == (5, 0.0, 0.5)


def test_ocr_ids_shift_default_and_errors():
    from funasr_amd.lcbnet import LCBNet

    m = LCBNet(**synth.lcbnet_conf())
    assert m.ocr_ids(None) == [295, 0]                                  # the reference's literal [294, 0]
    assert m.ocr_ids([0, 1, 0, 297, 298]) == [0, 2, 0, 298, 299]       # 0 stays, everything else + 1
    assert m.ocr_ids([O.shift_ids([5, 0])[0] - 1, 0]) == O.shift_ids([5, 0])
    with pytest.raises(ValueError, match="299"):
        m.ocr_ids([3, 299])                                             # 300 after the shift: the reference's Embedding raises IndexError
    with pytest.raises(ValueError, match="-1"):
        m.ocr_ids([-1])
    with pytest.raises(ValueError, match="empty"):
        m.ocr_ids([])
    small = LCBNet(**synth.lcbnet_conf(vocab=295))
    with pytest.raises(ValueError, match="294.*296"):
        small.ocr_ids(None)


def test_batch_size_above_one_raises_the_references_message():
    from funasr_amd.lcbnet import LCBNet

    m = LCBNet(**synth.lcbnet_conf())
    with pytest.raises(NotImplementedError) as e:
        m.inference([torch.zeros(16000)] * 2, batch_size=2, tokenizer=_Tok(["t"] * 300))
    assert str(e.value) == "batch decoding is not implemented"


def test_pair_input_goes_through_load_audio_text(monkeypatch, tmp_path):
    """the tuple route: `load_audio_text` gets the pair and the tokenizer, the text (a string, or a file that is read) becomes ids,
    the ids are shifted; plain sound and fbank input take the default ids. Everything up to the first device call, which a CPU
    model refuses in the package's usual words."""
    from funasr_amd import audio
    from funasr_amd.lcbnet import LCBNet

    g = load_golden()
    tokens = g["tokens"].tolist()
    tok = _Tok(tokens)
    m = LCBNet(**synth.lcbnet_conf())
    seen = {}
    real = audio.load_audio_text

    def spy(data_in, **kw):
        out = real(data_in, **kw)
        seen["args"], seen["out"] = (data_in, kw), out
        return out

    monkeypatch.setattr(audio, "load_audio_text", spy)

    def ocr_spy(ids):
        seen["ids"] = ids
        return LCBNet.ocr_ids(m, ids)

    monkeypatch.setattr(m, "ocr_ids", ocr_spy)
    from funasr_amd.wav_frontend import WavFrontend

    def Front():
        return WavFrontend(cmvn=None, lfr_m=1, lfr_n=1, dither=0.0)

    text = " ".join(tokens[i] for i in (7, 0, 298))
    path = tmp_path / "ocr.txt"
    path.write_text(text + "\n", encoding="utf-8")
    wav = torch.zeros(16000)
    for piece in (text, str(path)):
        seen.clear()
        with pytest.raises(RuntimeError, match="no CPU fallback|no GPU visible"):   # (the frontend without a GPU, the encoder with one)
            m.inference([(wav, piece)], data_type=("sound", "text"), tokenizer=tok, frontend=Front(), key=["k"], beam_size=5)
        assert seen["args"][1]["data_type"] == ("sound", "text") and seen["args"][1]["tokenizer"] is tok
        assert seen["out"][1] == [[7, 0, 298]] and seen["ids"] == [7, 0, 298]
    with pytest.raises(NotImplementedError, match="data_type"):
        m.inference([(wav, text)], data_type=("text", "sound"), tokenizer=tok, frontend=Front())
    with pytest.raises(ValueError, match="empty"):
        m.inference([(wav, "")], data_type=("sound", "text"), tokenizer=tok, frontend=Front())
    seen.clear()
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # fbank input: the default ids (the reference raises here)
        m.inference(torch.zeros(1, 50, 80), data_type="fbank", tokenizer=tok)
    assert "args" not in seen and seen["ids"] is None


# ------------------------------------------------------------------------------------------------ the oracle against the recording
def _maxd(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _rel(a, b):
    return _maxd(a, b) / max(float(np.abs(np.asarray(b)).max()), 1e-30)


def _within(tag, got, want, gap):
    """the float64 oracle against the float64 recording: within the stored fp32 - fp64 gap as a matter of course, and in fact at
    float64 rounding"""
    d, r = _maxd(got, want), _rel(got, want)
    print(f"{tag}: max |d| {d:.3e} (gap {gap:.3e}), relative {r:.3e}")
    assert d <= gap and r <= 1e-9, (tag, d, gap, r)


def test_float64_oracle_equals_the_references_float64_run():
    g = load_golden()
    _, sd, conf = golden_model(g)
    sd64 = O.cast(sd)
    assert [g[f"enc_{c}"].shape[0] for c in range(N_CLIPS)] == [40, 61] and [len(g[f"ocr_{j}"]) for j in range(N_TEXTS)] == [1, 2, 6, 33, 120]
    assert g["ocr_1"].tolist() == [294, 0]
    texts = []
    for j in range(N_TEXTS):
        ids = O.shift_ids(g[f"ocr_{j}"].tolist())
        t = O.text_encoder(sd64, conf["text_encoder_conf"], [ids], [len(ids)], pos_rows=g["pos_rows"])
        _within(f"text {j}", t[0], g[f"text_{j}"], float(g[f"gap_text_{j}"]))
        texts.append(t)
    for c in range(N_CLIPS):
        f = torch.from_numpy(g[f"feats_{c}"]).double()
        enc, olens = O.encoder(sd64, conf["encoder_conf"], f[None], [f.shape[0]], pos_rows=g["pos_rows"])
        assert olens == [g[f"enc_{c}"].shape[0]]
        _within(f"enc {c}", enc[0], g[f"enc_{c}"], float(g[f"gap_enc_{c}"]))
        for j in range(N_TEXTS):
            fus = O.fusion(sd64, conf["fusion_encoder_conf"], enc, texts[j])
            _within(f"fusion {c} {j}", fus[0], g[f"fusion_{c}_{j}"], float(g[f"gap_fusion_{c}_{j}"]))
            fused = enc + fus
            _within(f"fused {c} {j}", fused[0], g[f"fused_{c}_{j}"], float(g[f"gap_fused_{c}_{j}"]))
            assert O.ctc_greedy(O.ctc_log_softmax(sd64, fused)[0], olens[0]) == g[f"greedy_{c}_{j}"].tolist(), (c, j)


def test_the_recording_notices_the_text():
    """for each clip at least two texts give different greedy ids and different n-best ids: a fusion layer that does nothing, or a
    text encoder that ignores its ids, cannot reproduce the recording"""
    g = load_golden()
    for c in range(N_CLIPS):
        assert len({tuple(g[f"greedy_{c}_{j}"].tolist()) for j in range(N_TEXTS)}) >= 2
        assert len({tuple(g[f"nbest_ids_w0.3_{c}_{j}_0"].tolist()) for j in range(N_TEXTS)}) >= 2
        assert _maxd(g[f"fusion_{c}_0"], g[f"fusion_{c}_4"]) > 1e-2


@pytest.mark.parametrize("c,j", [(0, 1), (0, 4), (1, 2)])
def test_host_beam_search_with_the_oracle_decoder_returns_the_references_nbest(c, j):
    g = load_golden()
    model, sd, conf = golden_model(g)
    sd64 = O.cast(sd)
    memory = torch.from_numpy(g[f"fused_{c}_{j}"])
    ctc_logp = O.ctc_log_softmax(sd64, memory).numpy()
    for w in g["ctc_weights"].tolist():
        bs = BeamSearchTransformer(beam_size=int(g["beam"]), vocab_size=len(g["tokens"]), sos=model.sos, eos=model.eos, ctc_weight=w)
        nbest = bs(O.DecoderStepper(sd64, conf["decoder_conf"], memory), memory.shape[0], ctc_logp, dtype=torch.float64)[: int(g["nbest"])]
        assert len(nbest) == int(g["nbest"])
        for r, h in enumerate(nbest):
            assert h.yseq == g[f"nbest_ids_w{w}_{c}_{j}_{r}"].tolist(), (w, r)
            d = abs(h.score - float(g[f"nbest_score_w{w}_{c}_{j}_{r}"]))
            print(f"clip {c} text {j} w={w} rank {r}: score {h.score:.6f} |d| {d:.2e} (bar {8 * float(g['gap_nbest_score']):.2e})")
            assert d <= 8 * float(g["gap_nbest_score"]), (w, r, d)
