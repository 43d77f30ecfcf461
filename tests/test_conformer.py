"""Conformer, CPU side: registry, the reference's state-dict names and shapes, refused options, the float64 oracle against the
reference's recorded float64 outputs (tests/golden/conformer_<variant>.npz, written by tools/make_golden_conformer.py), and the
host beam search driven by the oracle's decoder against the reference's recorded n-best."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import synth
from funasr_amd.conformer import Conformer, ConformerEncoder, TransformerDecoder, subsampled_length
from funasr_amd.register import tables
from funasr_amd.transformer_search import BeamSearchTransformer

from . import _conformer_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = {"legacy_macaron": ("legacy", True), "legacy_plain": ("legacy", False), "latest_macaron": ("latest", True),
            "latest_plain": ("latest", False)}


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"conformer_{name}.npz"), allow_pickle=False))


def variant_model(name, g):
    rel, mac = VARIANTS[name]
    conf = synth.conformer_conf(macaron=mac, rel_pos_type=rel, vocab=len(g["tokens"]))
    model = Conformer(**conf)
    sd = synth.conformer_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def test_registry_keys():
    assert tables.model_classes["Conformer"] is Conformer
    assert tables.encoder_classes["ConformerEncoder"] is ConformerEncoder
    assert tables.decoder_classes["TransformerDecoder"] is TransformerDecoder


def test_state_dict_names_and_shapes_are_the_references():
    ref = json.load(open(os.path.join(GOLDEN, "conformer_state_dict.json")))
    m = Conformer(encoder="ConformerEncoder", encoder_conf=ref["encoder_conf"], decoder="TransformerDecoder", decoder_conf=ref["decoder_conf"],
                  vocab_size=ref["vocab_size"], input_size=80, specaug="SpecAug", specaug_conf={"apply_time_warp": True}, **ref["model_conf"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert m.encoder.legacy                                     # rel_pos_type is absent from the AISHELL yaml: "legacy"
    # a reference-shaped state dict loads strictly, BatchNorm buffers included
    sd = {k: torch.full(shp, 3, dtype=torch.long) if k.endswith("num_batches_tracked") else torch.randn(shp) for k, shp in ref["shapes"].items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.encoder.encoders[3].conv_module.norm.running_var, sd["encoder.encoders.3.conv_module.norm.running_var"])
    pushed = {n for n, _ in m.encoder.named_buffers()}
    assert "encoders.0.conv_module.norm.running_mean" in pushed


@pytest.mark.parametrize("where,conf,word", [
    ("encoder", {"input_layer": "conv2d6"}, "input_layer"), ("encoder", {"pos_enc_layer_type": "abs_pos"}, "pos_enc_layer_type"),
    ("encoder", {"selfattention_layer_type": "selfattn"}, "selfattention_layer_type"), ("encoder", {"concat_after": True}, "concat_after"),
    ("encoder", {"zero_triu": True}, "zero_triu"), ("encoder", {"interctc_layer_idx": [1]}, "interctc_layer_idx"),
    ("encoder", {"use_cnn_module": False}, "use_cnn_module"), ("encoder", {"activation_type": "relu"}, "activation_type"),
    ("encoder", {"normalize_before": False}, "normalize_before"), ("encoder", {"positionwise_layer_type": "conv1d"}, "positionwise_layer_type"),
    ("encoder", {"cnn_module_kernel": 33}, "cnn_module_kernel"), ("encoder", {"attention_heads": 4}, "attention_heads"),
    ("decoder", {"input_layer": "linear"}, "input_layer"), ("decoder", {"normalize_before": False}, "normalize_before"),
    ("decoder", {"concat_after": True}, "concat_after"), ("model", {"decoder": None}, "decoder"), ("model", {"ctc_weight": 1.0}, "decoder"),
    ("model", {"encoder": "TransformerEncoder"}, "encoder"), ("model", {"encoder": "BranchformerEncoder"}, "encoder"),
    ("model", {"interctc_weight": 0.3}, "interctc_weight")])
def test_unsupported_options_raise_and_name_the_option(where, conf, word):
    c = synth.conformer_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        Conformer(**c)


def test_cpu_parameters_raise_the_no_cpu_fallback_error():
    m = Conformer(**synth.conformer_conf())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 50, 80), [50])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.decoder.set_memory(torch.zeros(5, 128))


def test_length_rule_is_the_mask_rule():
    for padded in range(7, 300, 13):
        mask = torch.ones(1, 1, padded, dtype=torch.bool)
        assert subsampled_length(padded, padded) == mask[:, :, :-2:2][:, :, :-2:2].shape[-1]
        for n in range(1, padded + 1, 7):
            mask = (torch.arange(padded) < n)[None, None]
            assert subsampled_length(n, padded) == int(mask[:, :, :-2:2][:, :, :-2:2].sum())
    assert subsampled_length(131, 131) == 32 and subsampled_length(131, 203) == 33     # a clip gains a frame beside a longer one


def pin_positional_rows(model, g):
    """The reference's float32 positional table depends on the CPU's exp() in the last bit of div_term (a sinusoid of position
    ~5000 then moves by up to 5e-4), so the table of the machine that recorded the golden is part of the recording: where this
    machine builds other bits, the recorded rows replace the model's own. Returns True when it had to."""
    rows = torch.from_numpy(g["pos_rows"])
    T = rows.shape[0] if model.encoder.legacy else (rows.shape[0] + 1) // 2
    own = model.encoder.pos_rows(T)
    assert float((own - rows).abs().max()) <= 1e-3                      # the same table up to that last bit
    if torch.equal(own, rows):
        return False
    own.copy_(rows)
    model.encoder.mark_dirty()
    return True


def test_host_built_positional_tables_are_the_recorded_ones_up_to_the_hosts_exp():
    """what this host builds against what the recording's host built: the same table up to the last bit of div_term (<= 1e-3 in a
    sinusoid of position ~5000); whether they are bit-equal is reported"""
    for name in VARIANTS:
        g = load_golden(name)
        model, _, _ = variant_model(name, g)
        rows = torch.from_numpy(g["pos_rows"])
        T = rows.shape[0] if model.encoder.legacy else (rows.shape[0] + 1) // 2
        own = model.encoder.pos_rows(T)
        d = float((own - rows).abs().max())
        print(f"{name}: host-built rows vs recorded rows max |d| {d:.3e} (bit-equal: {torch.equal(own, rows)})")
        assert own.shape == rows.shape and d <= 1e-3


def test_short_and_long_batches_raise_before_any_device_work():
    from funasr_amd.conformer import MAX_LEN, TooShortUttError
    m = Conformer(**synth.conformer_conf())
    with pytest.raises(TooShortUttError, match="too short for subsampling") as e:
        m.encode(torch.zeros(2, 6, 80), [6, 3])                 # the check is on the padded batch, not the clip
    assert e.value.actual_size == 6 and e.value.limit == 7
    n = 4 * MAX_LEN + 7                                         # 5001 encoder frames
    assert subsampled_length(n, n) == MAX_LEN + 1 and subsampled_length(n - 4, n - 4) == MAX_LEN
    with pytest.raises(ValueError, match="5000"):
        m.encode(torch.zeros(1, n, 80), [n])


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-30))


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_float64_oracle_equals_the_references_float64_run(name):
    g = load_golden(name)
    _, sd, conf = variant_model(name, g)
    sd64 = O.cast(sd)
    lens = [int(n) for n in g["lens"]]
    feats = [torch.from_numpy(g[f"feats_{i}"]).double() for i in range(len(lens))]
    for i, f in enumerate(feats):
        enc, olens = O.encoder(sd64, conf["encoder_conf"], f[None], [lens[i]], pos_rows=g["pos_rows"])
        lp = O.ctc_log_softmax(sd64, enc)[0]
        assert _rel(enc[0], g[f"enc_{i}"]) <= 1e-9 and _rel(lp, g[f"ctc_{i}"]) <= 1e-9, (name, i)
        assert O.ctc_greedy(lp, olens[0]) == g[f"greedy_{i}"].tolist()
    pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    enc, olens = O.encoder(sd64, conf["encoder_conf"], pad, lens, pos_rows=g["pos_rows"])
    assert olens == g["batch_olens"].tolist()
    lp = O.ctc_log_softmax(sd64, enc)
    for i, n in enumerate(olens):
        assert _rel(enc[i, :n], g[f"batch_enc_{i}"]) <= 1e-9 and _rel(lp[i, :n], g[f"batch_ctc_{i}"]) <= 1e-9, (name, i)
        assert O.ctc_greedy(lp[i], n) == g[f"batch_greedy_{i}"].tolist()
    # the ragged batch is NOT a set of independent clips: clip 0's frames differ from its solo run
    assert np.abs(g["batch_enc_0"][: g["enc_0"].shape[0]] - g["enc_0"][: g["batch_enc_0"].shape[0]]).max() > 1e-3
    st = O.DecoderStepper(sd64, conf["decoder_conf"], torch.from_numpy(g["enc_1"]))
    for j, pre in enumerate(g["prefixes"]):
        got = O.score_prefix(st, [int(t) for t in str(pre).split(",")])
        assert _rel(got, g[f"step_{j}"]) <= 1e-9, (name, j)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_host_beam_search_with_the_oracle_decoder_returns_the_references_nbest(name):
    g = load_golden(name)
    model, sd, conf = variant_model(name, g)
    sd64 = O.cast(sd)
    memory = torch.from_numpy(g["enc_0"])
    ctc_logp = O.ctc_log_softmax(sd64, memory).numpy()
    for w in g["ctc_weights"].tolist():
        bs = BeamSearchTransformer(beam_size=int(g["beam"]), vocab_size=len(g["tokens"]), sos=model.sos, eos=model.eos, ctc_weight=w)
        nbest = bs(O.DecoderStepper(sd64, conf["decoder_conf"], memory), memory.shape[0], ctc_logp, dtype=torch.float64)[: int(g["nbest"])]
        assert len(nbest) == int(g["nbest"])
        for r, h in enumerate(nbest):
            assert h.yseq == g[f"nbest_ids_w{w}_{r}"].tolist(), (name, w, r)
            d = abs(h.score - float(g[f"nbest_score_w{w}_{r}"]))
            print(f"{name} w={w} rank {r}: score {h.score:.6f} |d| {d:.2e} (bar {8 * float(g['gap_nbest_score']):.2e})")
            assert d <= 8 * float(g["gap_nbest_score"]), (name, w, r, d)


# ------------------------------------------------------------------------------------------------ beam 10 on a random utterance
BEAM10_SEED, BEAM10_WEIGHTS, BEAM10_TOP = 21, (0.0, 0.3), 3


@functools.lru_cache(maxsize=None)
def beam10_setup(seed=BEAM10_SEED):
    """conf, weights, the float64 oracle encoder's output of a 383-frame random clip rounded to float32 (95 frames) and the CTC
    log-probabilities of that memory in float64: what every stepper of the beam-10 searches shares, so that only the decoder differs"""
    conf = synth.conformer_conf(vocab=60)
    model = Conformer(**conf)
    sd = synth.conformer_state_dict(seed, model)
    feats = torch.randn(1, 383, 80, generator=torch.Generator().manual_seed(seed))
    sd64 = O.cast(sd)
    enc, olens = O.encoder(sd64, conf["encoder_conf"], feats.double(), [383])
    assert olens == [95]
    memory = enc[0].float()
    ctc_logp = O.ctc_log_softmax(sd64, memory.double()).numpy()
    return conf, sd, memory, ctc_logp, model.sos, model.eos


def beam10_search(stepper, w, dtype, seed=BEAM10_SEED):
    conf, sd, memory, ctc_logp, sos, eos = beam10_setup(seed)
    bs = BeamSearchTransformer(beam_size=10, vocab_size=60, sos=sos, eos=eos, ctc_weight=w)
    return bs(stepper, memory.shape[0], ctc_logp, dtype=dtype)


@functools.lru_cache(maxsize=None)
def beam10_oracle_nbest(seed=BEAM10_SEED):
    """{(w, "f64" | "f32"): n-best of the search driven by the oracle's stepper in that dtype}"""
    conf, sd, memory, ctc_logp, sos, eos = beam10_setup(seed)
    out = {}
    for w in BEAM10_WEIGHTS:
        out[w, "f64"] = beam10_search(O.DecoderStepper(O.cast(sd), conf["decoder_conf"], memory.double()), w, torch.float64, seed)
        out[w, "f32"] = beam10_search(O.DecoderStepper(O.cast(sd, torch.float32), conf["decoder_conf"], memory), w, torch.float32, seed)
    return out


def beam10_reference_agrees_with_itself(seed=BEAM10_SEED):
    """the precondition of the device comparison: the float32 and the float64 oracle searches return the same top-3 ids for both
    weights and no score sits on the CTC scorer's log-zero. Returns max |score32 - score64| over the compared hypotheses."""
    nb = beam10_oracle_nbest(seed)
    gap = 0.0
    for w in BEAM10_WEIGHTS:
        h64, h32 = nb[w, "f64"][:BEAM10_TOP], nb[w, "f32"][:BEAM10_TOP]
        assert len(h64) == BEAM10_TOP and len(h32) == BEAM10_TOP, (w, len(h64), len(h32))
        for r, (a, b) in enumerate(zip(h64, h32)):
            print(f"beam 10 seed {seed} w={w} rank {r}: len {len(a.yseq)}, score64 {a.score:.6f}, |score32 - score64| {abs(a.score - b.score):.3e}")
            assert a.yseq == b.yseq, (w, r)
            assert a.score >= -1e6 and b.score >= -1e6, (w, r, a.score, b.score)
            gap = max(gap, abs(a.score - b.score))
    return gap


def test_beam_10_oracle_searches_agree_in_float32_and_float64():
    """beam 10 over 95 frames with the two oracle steppers only: the reference must agree with itself (same top-3 ids in float32 and
    float64 for CTC weights 0 and 0.3, every score finite-sized) before the device search is compared with it"""
    beam10_reference_agrees_with_itself()
