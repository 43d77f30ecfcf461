"""Transformer, CPU side: registry, the reference's state-dict names and shapes, refused options, the float64 oracle against the
reference's recorded float64 outputs (tests/golden/transformer.npz, written by tools/make_golden_transformer.py), and the host
beam search driven by the oracle's decoder against the reference's recorded n-best."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import synth
from funasr_amd.conformer import Conformer, TransformerDecoder, subsampled_length
from funasr_amd.register import tables
from funasr_amd.transformer_search import BeamSearchTransformer

from . import _transformer_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "transformer.npz"), allow_pickle=False))


def golden_model(g):
    from funasr_amd.transformer import Transformer

    conf = synth.transformer_conf(vocab=len(g["tokens"]))
    model = Transformer(**conf)
    sd = synth.transformer_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def test_registry_keys():
    from funasr_amd.transformer import Transformer, TransformerEncoder

    assert tables.model_classes["Transformer"] is Transformer
    assert tables.encoder_classes["TransformerEncoder"] is TransformerEncoder
    assert tables.decoder_classes["TransformerDecoder"] is TransformerDecoder
    assert tables.model_classes["Conformer"] is Conformer and not issubclass(Conformer, Transformer) and not issubclass(Transformer, Conformer)
    from funasr_amd.install import hip_classes
    assert ("model_classes", "Transformer", Transformer) in hip_classes() and ("encoder_classes", "TransformerEncoder", TransformerEncoder) in hip_classes()


def test_state_dict_names_and_shapes_are_the_references():
    from funasr_amd.transformer import Transformer

    ref = json.load(open(os.path.join(GOLDEN, "transformer_state_dict.json")))
    m = Transformer(encoder="TransformerEncoder", encoder_conf=ref["encoder_conf"], decoder="TransformerDecoder", decoder_conf=ref["decoder_conf"],
                    vocab_size=ref["vocab_size"], input_size=80, specaug="SpecAug", specaug_conf={"apply_time_warp": True}, **ref["model_conf"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert not any("pe" == k.split(".")[-1] or "pos_table" in k for k in ref["shapes"])          # `pe` is a plain attribute there and here
    sd = {k: torch.randn(shp) for k, shp in ref["shapes"].items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.encoder.encoders[11].norm2.bias, sd["encoder.encoders.11.norm2.bias"])
    big = synth.transformer_conf(**synth.TRANSFORMER_AISHELL)
    assert big["encoder_conf"] == ref["encoder_conf"] and big["decoder_conf"] == ref["decoder_conf"] and big["vocab_size"] == ref["vocab_size"]


@pytest.mark.parametrize("where,conf,word", [
    ("encoder", {"input_layer": "conv2d6"}, "input_layer"), ("encoder", {"input_layer": "linear"}, "input_layer"),
    ("encoder", {"normalize_before": False}, "normalize_before"), ("encoder", {"concat_after": True}, "concat_after"),
    ("encoder", {"positionwise_layer_type": "conv1d"}, "positionwise_layer_type"), ("encoder", {"interctc_layer_idx": [1]}, "interctc_layer_idx"),
    ("encoder", {"interctc_use_conditioning": True}, "interctc_use_conditioning"), ("encoder", {"attention_heads": 4}, "attention_heads"),
    ("encoder", {"output_size": 192, "attention_heads": 2}, "output_size"), ("encoder", {"linear_units": 250}, "linear_units"),
    ("model", {"input_size": 6}, "input_size"), ("model", {"input_size": 257}, "input_size"),
    ("decoder", {"input_layer": "linear"}, "input_layer"), ("decoder", {"normalize_before": False}, "normalize_before"),
    ("decoder", {"concat_after": True}, "concat_after"), ("model", {"decoder": None}, "decoder"), ("model", {"ctc_weight": 1.0}, "decoder"),
    ("model", {"decoder": "ParaformerSANMDecoder"}, "decoder"), ("model", {"encoder": "ConformerEncoder"}, "ConformerEncoder"),
    ("model", {"encoder": "BranchformerEncoder"}, "encoder"), ("model", {"interctc_weight": 0.3}, "interctc_weight"),
    ("model", {"share_embedding": True}, "share_embedding")])
def test_unsupported_options_raise_and_name_the_option(where, conf, word):
    from funasr_amd.transformer import Transformer

    c = synth.transformer_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        Transformer(**c)


def test_conformer_keeps_refusing_the_transformer_encoder_with_the_same_words():
    c = synth.conformer_conf()
    c["encoder"] = "TransformerEncoder"
    with pytest.raises(NotImplementedError) as e:
        Conformer(**c)
    assert str(e.value) == ("Conformer(HIP): encoder: TransformerEncoder is not built (only ConformerEncoder; the Transformer / "
                            "Branchformer families are other models)")


def test_cpu_parameters_raise_the_no_cpu_fallback_error():
    from funasr_amd.transformer import Transformer

    m = Transformer(**synth.transformer_conf())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 50, 80), [50])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.decoder.set_memory(torch.zeros(5, 128))


def test_short_and_long_batches_raise_before_any_device_work():
    from funasr_amd.transformer import MAX_LEN, TooShortUttError, Transformer

    m = Transformer(**synth.transformer_conf())
    with pytest.raises(TooShortUttError, match="too short for subsampling") as e:
        m.encode(torch.zeros(2, 6, 80), [6, 3])                 # the check is on the padded batch, not the clip
    assert e.value.actual_size == 6 and e.value.limit == 7
    n = 4 * MAX_LEN + 7                                         # 5001 encoder frames
    assert subsampled_length(n, n) == MAX_LEN + 1 and subsampled_length(n - 4, n - 4) == MAX_LEN
    with pytest.raises(ValueError, match="5000"):
        m.encode(torch.zeros(1, n, 80), [n])


def pin_positional_rows(model, g):
    """as tests/test_conformer.py pin_positional_rows: the recording host's float32 table is part of the recording; where this host
    builds other bits, the recorded rows replace the model's own. Returns True when it had to."""
    rows = torch.from_numpy(g["pos_rows"])
    own = model.encoder.pos_rows(rows.shape[0])
    assert float((own - rows).abs().max()) <= 1e-3
    if torch.equal(own, rows):
        return False
    own.copy_(rows)
    model.encoder.mark_dirty()
    return True


def test_host_built_positional_table_is_the_recorded_one_up_to_the_hosts_exp():
    g = load_golden()
    model, _, _ = golden_model(g)
    rows = torch.from_numpy(g["pos_rows"])
    own = model.encoder.pos_rows(rows.shape[0])
    d = float((own - rows).abs().max())
    print(f"host-built rows vs recorded rows max |d| {d:.3e} (bit-equal: {torch.equal(own, rows)})")
    assert own.shape == rows.shape == (61, 128) and d <= 1e-3


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-30))


def test_float64_oracle_equals_the_references_float64_run():
    g = load_golden()
    _, sd, conf = golden_model(g)
    sd64 = O.cast(sd)
    lens = [int(n) for n in g["lens"]]
    feats = [torch.from_numpy(g[f"feats_{i}"]).double() for i in range(len(lens))]
    assert [g[f"enc_{i}"].shape[0] for i in range(3)] == [24, 40, 61] and g["batch_olens"].tolist() == [26, 41, 61]
    for i, f in enumerate(feats):
        enc, olens = O.encoder(sd64, conf["encoder_conf"], f[None], [lens[i]], pos_rows=g["pos_rows"])
        lp = O.ctc_log_softmax(sd64, enc)[0]
        assert olens == [g[f"enc_{i}"].shape[0]]
        assert _rel(enc[0], g[f"enc_{i}"]) <= 1e-9 and _rel(lp, g[f"ctc_{i}"]) <= 1e-9, i
        assert O.ctc_greedy(lp, olens[0]) == g[f"greedy_{i}"].tolist()
    pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    enc, olens = O.encoder(sd64, conf["encoder_conf"], pad, lens, pos_rows=g["pos_rows"])
    assert olens == g["batch_olens"].tolist()
    lp = O.ctc_log_softmax(sd64, enc)
    for i, n in enumerate(olens):
        assert _rel(enc[i, :n], g[f"batch_enc_{i}"]) <= 1e-9 and _rel(lp[i, :n], g[f"batch_ctc_{i}"]) <= 1e-9, i
        assert O.ctc_greedy(lp[i], n) == g[f"batch_greedy_{i}"].tolist()
    # the ragged batch is NOT a set of independent clips: clip 0's frames differ from its solo run
    assert np.abs(g["batch_enc_0"][: g["enc_0"].shape[0]] - g["enc_0"][: g["batch_enc_0"].shape[0]]).max() > 1e-3
    st = O.DecoderStepper(sd64, conf["decoder_conf"], torch.from_numpy(g["enc_1"]))
    for j, pre in enumerate(g["prefixes"]):
        got = O.score_prefix(st, [int(t) for t in str(pre).split(",")])
        assert _rel(got, g[f"step_{j}"]) <= 1e-9, j


def test_host_beam_search_with_the_oracle_decoder_returns_the_references_nbest():
    g = load_golden()
    model, sd, conf = golden_model(g)
    sd64 = O.cast(sd)
    memory = torch.from_numpy(g["enc_0"])
    ctc_logp = O.ctc_log_softmax(sd64, memory).numpy()
    for w in g["ctc_weights"].tolist():
        bs = BeamSearchTransformer(beam_size=int(g["beam"]), vocab_size=len(g["tokens"]), sos=model.sos, eos=model.eos, ctc_weight=w)
        nbest = bs(O.DecoderStepper(sd64, conf["decoder_conf"], memory), memory.shape[0], ctc_logp, dtype=torch.float64)[: int(g["nbest"])]
        assert len(nbest) == int(g["nbest"])
        for r, h in enumerate(nbest):
            assert h.yseq == g[f"nbest_ids_w{w}_{r}"].tolist(), (w, r)
            d = abs(h.score - float(g[f"nbest_score_w{w}_{r}"]))
            print(f"w={w} rank {r}: score {h.score:.6f} |d| {d:.2e} (bar {8 * float(g['gap_nbest_score']):.2e})")
            assert d <= 8 * float(g["gap_nbest_score"]), (w, r, d)
