"""E-Paraformer, CPU side: registry, the reference's state-dict names, shapes and ORDER at the recipe's and the tiny size, the recipe's
sections through a written config.yaml, refused options, and the float64 / float32 oracle of the predictor and the decoder against the
reference's recorded outputs (tests/golden/eparaformer.npz, written by tools/make_golden_eparaformer.py)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import synth
from funasr_amd.register import tables

from . import _eparaformer_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = ("s0", "s1", "b", "z")
_golden = {}


def load_golden(run=None):
    """the arrays of one run (its `<run>/` keys without the prefix) plus the shared ones"""
    if not _golden:
        _golden.update(np.load(os.path.join(GOLDEN, "eparaformer.npz"), allow_pickle=False))
    g = {k: v for k, v in _golden.items() if "/" not in k}
    if run is not None:
        g.update({k.split("/", 1)[1]: v for k, v in _golden.items() if k.startswith(run + "/")})
    return g


def golden_model():
    """the mirror with the recording's weights: synthetic from the recorded seed, the calibrated output layer from the file"""
    from funasr_amd.e_paraformer import EParaformer

    g = load_golden()
    conf = synth.eparaformer_conf(vocab=len(g["tokens"]))
    model = EParaformer(**conf)
    sd = synth.eparaformer_state_dict(int(g["seed"]), model)
    sd["decoder.output_layer.weight"] = torch.from_numpy(g["output_layer_weight"])
    sd["decoder.output_layer.bias"] = torch.from_numpy(g["output_layer_bias"])
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def pin_positional_rows(model, g):
    """the recording host's float32 positional table is part of the recording (its last bits depend on the host's exp()); where this
    host builds other bits, the recorded rows replace the model's own. Returns True when it had to."""
    rows = torch.from_numpy(g["pos_rows"])
    own = model.encoder.pos_rows(rows.shape[0])
    assert own.shape == rows.shape and float((own - rows).abs().max()) <= 1e-3
    if torch.equal(own, rows):
        return False
    own.copy_(rows)
    model.encoder.mark_dirty()
    return True


def _maxd(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _rel(a, b):
    return _maxd(a, b) / max(float(np.abs(np.asarray(b)).max()), 1e-30)


def test_registry_names_and_hip_classes():
    from funasr_amd.conformer import ConformerEncoder
    from funasr_amd.e_paraformer import EParaformer, ParaformerSANDecoder, PifPredictor
    from funasr_amd.install import hip_classes
    import funasr_amd.auto_model  # noqa: F401  (imports the module as AutoModel does)

    assert tables.model_classes["EParaformer"] is EParaformer
    assert tables.predictor_classes["PifPredictor"] is PifPredictor
    assert tables.decoder_classes["ParaformerSANDecoder"] is ParaformerSANDecoder
    assert tables.encoder_classes["ConformerEncoder"] is ConformerEncoder
    hc = hip_classes()
    for triple in (("model_classes", "EParaformer", EParaformer), ("predictor_classes", "PifPredictor", PifPredictor),
                   ("decoder_classes", "ParaformerSANDecoder", ParaformerSANDecoder)):
        assert triple in hc


def test_state_dict_names_shapes_and_order_are_the_references():
    from funasr_amd.e_paraformer import EParaformer

    ref = json.load(open(os.path.join(GOLDEN, "eparaformer_state_dict.json")))
    assert (ref["model"], ref["encoder"], ref["decoder"], ref["predictor"]) == ("EParaformer", "ConformerEncoder", "ParaformerSANDecoder", "PifPredictor")
    m = tables.model_classes[ref["model"]](encoder=ref["encoder"], encoder_conf=ref["encoder_conf"], decoder=ref["decoder"],
                                           decoder_conf=ref["decoder_conf"], predictor=ref["predictor"], predictor_conf=ref["predictor_conf"],
                                           vocab_size=ref["vocab_size"], input_size=80, specaug="SpecAug", specaug_conf={"apply_time_warp": True},
                                           **ref["model_conf"])
    assert isinstance(m, EParaformer) and m.ctc is None
    own = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert own == ref["shapes"] and list(own) == list(ref["shapes"])              # the order too: synth draws in it
    for k in ("predictor.cif_conv1d.weight", "predictor.cif_output.bias", "predictor.sigma", "predictor.bias", "decoder.embed.0.weight",
              "decoder.decoders.5.src_attn.linear_k.weight", "decoder.output_layer.bias"):
        assert k in own, k
    assert own["predictor.cif_conv1d.weight"] == [256, 1, 3] and own["predictor.sigma"] == [4] and own["decoder.embed.0.weight"] == [4234, 256]
    m.load_state_dict({k: torch.randn(shp) for k, shp in ref["shapes"].items()}, strict=True)
    big = synth.eparaformer_conf(**synth.EPARAFORMER_TEMPLATE)
    assert big["encoder_conf"] == ref["encoder_conf"] and big["decoder_conf"] == ref["decoder_conf"]
    assert big["predictor_conf"] == ref["predictor_conf"] and big["vocab_size"] == ref["vocab_size"]
    t = EParaformer(**synth.eparaformer_conf(vocab=40))
    shapes = {k: list(v.shape) for k, v in t.state_dict().items()}
    assert shapes == ref["tiny_shapes"] and list(shapes) == list(ref["tiny_shapes"])
    sd = synth.eparaformer_state_dict(3, t)
    t.load_state_dict(sd, strict=True)
    assert len(set(sd["predictor.sigma"].tolist())) == 4 and float(sd["predictor.cif_output.bias"]) < 0
    # ctc_weight > 0 builds and loads the CTC head's parameters
    c = EParaformer(**synth.eparaformer_conf(vocab=40, ctc_weight=0.3))
    assert "ctc.ctc_lo.weight" in c.state_dict() and list(c.state_dict())[-8:-6] == ["ctc.ctc_lo.weight", "ctc.ctc_lo.bias"]
    assert list(c.state_dict())[-6:] == ["predictor." + k for k in ("sigma", "bias", "cif_conv1d.weight", "cif_conv1d.bias", "cif_output.weight",
                                                                    "cif_output.bias")]


def test_the_recipes_sections_build_through_a_written_config_yaml(tmp_path):
    ref = json.load(open(os.path.join(GOLDEN, "eparaformer_state_dict.json")))
    path = tmp_path / "config.yaml"
    keys = ("model", "model_conf", "encoder", "encoder_conf", "decoder", "decoder_conf", "predictor", "predictor_conf")
    with open(path, "w", encoding="utf-8") as f:
        yaml.safe_dump({k: ref[k] for k in keys}, f)
    conf = yaml.safe_load(open(path, encoding="utf-8"))
    import funasr_amd.e_paraformer  # noqa: F401
    m = tables.model_classes[conf["model"]](vocab_size=4234, input_size=80, **{k: conf[k] for k in keys if k not in ("model", "model_conf")},
                                            **conf["model_conf"])
    e, d, p = m.encoder, m.decoder, m.predictor
    assert (e.output_size(), e.attention_heads, e.num_blocks, e.kernel, e.linear_units, e.macaron) == (256, 4, 12, 15, 2048, True)
    assert (d.d_model, d.attention_heads, d.num_blocks, d.linear_units, d.vocab_size, d.precision) == (256, 4, 6, 2048, 4234, "f16x2")
    assert (p.idim, p.l_order, p.r_order, p.sigma_heads) == (256, 1, 1, 4) and p.sigma.tolist() == [0.5] * 4 and p.bias.tolist() == [0.0] * 4
    c = d._make_config()
    assert (c.d_model, c.n_heads, c.ffn_dim, c.n_blocks, c.vocab_size, c.precision) == (256, 4, 2048, 6, 4234, 3)
    c = p._make_config()
    assert (c.d_model, c.l_order, c.r_order, c.sigma_heads, c.smooth_factor, c.noise_threshold) == (256, 1, 1, 4, 1.0, 0.0)
    m.set_precision("fp32")
    assert e.precision == "fp32" and d.precision == "fp32" and d._make_config().precision == 0


@pytest.mark.parametrize("where,conf,word", [
    ("model", {"encoder": "SANMEncoder"}, "SANMEncoder belongs to model: Paraformer"), ("model", {"encoder": "TransformerEncoder"}, "encoder"),
    ("model", {"decoder": "ParaformerSANMDecoder"}, "ParaformerSANMDecoder"), ("model", {"decoder": "TransformerDecoder"}, "decoder"),
    ("model", {"ctc_weight": 1.0}, "decoder"), ("model", {"predictor": "CifPredictorV2"}, "predictor"),
    ("model", {"share_embedding": True}, "share_embedding"), ("model", {"precision": "bf16"}, "bf16"), ("model", {"bf16": True}, "bf16"),
    ("decoder", {"input_layer": "linear"}, "input_layer"), ("decoder", {"normalize_before": False}, "normalize_before"),
    ("decoder", {"concat_after": True}, "concat_after"), ("decoder", {"use_output_layer": False}, "use_output_layer"),
    ("decoder", {"embeds_id": 2}, "embeds_id"), ("decoder", {"attention_heads": 4}, "attention_heads"),
    ("decoder", {"linear_units": 250}, "linear_units"), ("decoder", {"precision": "bf16x3"}, "precision"),
    ("predictor", {"sigma_heads": 9}, "sigma_heads"), ("predictor", {"sigma_heads": 3}, "sigma_heads"), ("predictor", {"sigma_heads": 8}, "sigma_heads"),
    ("predictor", {"l_order": 16}, "l_order"), ("predictor", {"r_order": 16}, "r_order"), ("predictor", {"idim": 64}, "idim"),
    ("encoder", {"input_layer": "linear"}, "input_layer")])
def test_unsupported_options_raise_and_name_the_option(where, conf, word):
    import funasr_amd.e_paraformer  # noqa: F401

    c = synth.eparaformer_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        tables.model_classes["EParaformer"](**c)


@pytest.mark.parametrize("kw,word", [({"decoding_ctc_weight": 0.3}, "decoding_ctc_weight"), ({"lm_weight": 0.2}, "lm_weight"),
                                     ({"pred_timestamp": True}, "pred_timestamp"), ({"bf16": True}, "bf16")])
def test_inference_options_of_the_beam_search_and_timestamps_are_refused_by_name(kw, word):
    from funasr_amd.e_paraformer import EParaformer

    m = EParaformer(**synth.eparaformer_conf())
    with pytest.raises(NotImplementedError, match=word):
        m.inference(torch.zeros(1, 50, 80), data_lengths=[50], key=["a"], data_type="fbank", **kw)
    with pytest.raises(NotImplementedError, match="bf16"):
        m.set_precision("bf16")


def test_cpu_parameters_raise_the_no_cpu_fallback_error():
    from funasr_amd.e_paraformer import EParaformer

    m = EParaformer(**synth.eparaformer_conf())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 50, 80), [50])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predictor(torch.zeros(1, 11, 128), lengths=[11])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.decoder(torch.zeros(1, 11, 128), [11], torch.zeros(1, 3, 128), [3])


@pytest.mark.parametrize("run", RUNS)
def test_oracle_reproduces_the_references_float64_run_and_stays_within_its_float32_gaps(run):
    """The predictor and the decoder restated from the formulas, on the RECORDED encoder rows of the padded batch. float64: 1e-9 relative
    on every recorded array, counts and ids equal. float32: another valid float32 evaluation of the same formulas stays within 4 x the
    recorded |fp32 - fp64| gap of the reference (the bar the GPU's fp32 mode is held to)."""
    g = load_golden(run)
    _, sd, conf = golden_model()
    enc, olens = torch.from_numpy(g["enc"]), g["olens"].tolist()
    for dt, check in ((torch.float64, lambda k, a: _rel(a, g[k]) <= 1e-9), (torch.float32, lambda k, a: _maxd(a, g[k]) <= 4 * float(g["gap_" + k]))):
        s = O.cast(sd, dt)
        p = O.predictor(s, conf["predictor_conf"], enc.to(dt), olens)
        assert p["counts"] == g["counts"].tolist()
        for k in ("token_num", "alphas", "align", "embeds"):
            print(f"{run} {dt} {k}: {_maxd(p[k], g[k]):.3e} (gap {float(g['gap_' + k]):.3e})")
            assert check(k, p[k]), (run, dt, k)
        # the decoder on the RECORDED embeddings (so that its check does not inherit the predictor's rounding)
        logp = O.decoder(s, conf["decoder_conf"], enc.to(dt), olens, torch.from_numpy(g["embeds"]).to(dt), p["counts"])
        valid = np.concatenate([np.asarray(logp[b, :n]) for b, n in enumerate(p["counts"])])
        want = np.concatenate([g["logp"][b, :n] for b, n in enumerate(p["counts"])])
        print(f"{run} {dt} logp: {_maxd(valid, want):.3e} (gap {float(g['gap_logp']):.3e})")
        assert (_rel(valid, want) <= 1e-9) if dt == torch.float64 else (_maxd(valid, want) <= 4 * float(g["gap_logp"]))
        for b, n in enumerate(p["counts"]):
            assert logp[b, :n].argmax(-1).tolist() == g[f"ids_{b}"].tolist()
            assert O.greedy(logp, p["counts"])[b] == g[f"token_int_{b}"].tolist()


def test_the_fixture_shows_what_it_must():
    """the conditions the generator asserts, seen from the file: token sums off the half-integers, at least 5 distinct ids per normal clip,
    the ragged batch is not a set of independent clips, the short clip of `z` has no token and an empty record"""
    s0, b, z = load_golden("s0"), load_golden("b"), load_golden("z")
    for run in RUNS:
        g = load_golden(run)
        tn = g["token_num"]
        assert float(np.abs(tn - np.floor(tn) - 0.5).min()) >= 0.05 and g["counts"].tolist() == np.rint(tn).astype(int).tolist()
        assert g["embeds"].shape[1] == int(g["counts"].max())
    assert s0["olens"].tolist() == [40] and b["olens"].tolist() == [41, 61] and z["olens"].tolist() == [61, 1]
    n0 = int(s0["counts"][0])
    assert np.abs(b["embeds"][0, :n0] - s0["embeds"][0, :n0]).max() > 100 * float(b["gap_embeds"])
    assert z["counts"].tolist()[1] == 0 and z["texts"].tolist()[1] == "" and z["token_int_1"].size == 0 and float(z["alphas"][1].max()) == 0.0
    for g, clips in ((s0, [0]), (b, [0, 1]), (z, [0])):
        for c in clips:
            assert len(set(g[f"token_int_{c}"].tolist())) >= 5


def test_kernel_oracles_are_the_torch_ops():
    """the restated predictor pieces against torch's own modules in float64"""
    g = torch.Generator().manual_seed(0)
    torch.set_grad_enabled(False)
    h = torch.randn(2, 9, 64, generator=g, dtype=torch.float64)
    for lo, ro in ((0, 0), (1, 1), (3, 0), (0, 15)):
        w = torch.randn(64, 1, lo + ro + 1, generator=g, dtype=torch.float64)
        cb, ow, ob = (torch.randn(n, generator=g, dtype=torch.float64) for n in (64, 64, 1))
        conv = torch.nn.Conv1d(64, 64, lo + ro + 1, groups=64).double()
        conv.weight.data, conv.bias.data = w, cb
        y = conv(torch.nn.ConstantPad1d((lo, ro), 0)(h.transpose(1, 2))) + h.transpose(1, 2)
        want = torch.sigmoid(torch.relu(y.transpose(1, 2)) @ ow + ob)
        want[1, 5:] = 0
        a, tn = O.pif_alphas(h, [9, 5], w, cb, ow, ob, lo, ro)
        assert float((a - want).abs().max()) <= 1e-14 and float((tn - want.sum(-1)).abs().max()) <= 1e-13
    a = torch.rand(3, 7, generator=g, dtype=torch.float64)
    a[2] = 0
    an, al = O.pif_align(a, a.sum(-1), [4, 0, 3])
    assert bool(torch.isfinite(an).all()) and float(an[1].abs().max()) == 0 and float(an[2].abs().max()) == 0
    assert abs(float(al[0, -1]) - 4.0) < 1e-12
    torch.set_grad_enabled(True)
