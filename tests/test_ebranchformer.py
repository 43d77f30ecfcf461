"""E-Branchformer, CPU side: registry (both model names), the reference's state-dict names, shapes and ORDER at the template's and
the tiny size, refused options, a config.yaml with the reference template's encoder section, and the float64 / float32 oracle
against the reference's recorded outputs (tests/golden/ebranchformer.npz, written by tools/make_golden_ebranchformer.py)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import synth
from funasr_amd.conformer import Conformer, TransformerDecoder
from funasr_amd.register import tables
from funasr_amd.transformer_search import BeamSearchTransformer

from . import _ebranchformer_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = {"latest_macaron": dict(rel_pos_type="latest", use_ffn=True, macaron=True, cgmlp_kernel=31, merge_kernel=31),
            "legacy_noffn": dict(rel_pos_type="legacy", use_ffn=False, macaron=False, cgmlp_kernel=15, merge_kernel=3)}
_golden = {}


def load_golden(variant):
    """the arrays of one variant (its `<variant>/` keys without the prefix) plus the shared ones"""
    if not _golden:
        _golden.update(np.load(os.path.join(GOLDEN, "ebranchformer.npz"), allow_pickle=False))
    g = {k: v for k, v in _golden.items() if "/" not in k}
    g.update({k.split("/", 1)[1]: v for k, v in _golden.items() if k.startswith(variant + "/")})
    return g


def golden_model(g, variant):
    from funasr_amd.ebranchformer import EBranchformer

    conf = synth.ebranchformer_conf(vocab=len(g["tokens"]), **VARIANTS[variant])
    model = EBranchformer(**conf)
    sd = synth.ebranchformer_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def pin_positional_rows(model, g):
    """as tests/test_conformer.py pin_positional_rows: the recording host's float32 table is part of the recording; where this host
    builds other bits, the recorded rows replace the model's own. Returns True when it had to."""
    rows = torch.from_numpy(g["pos_rows"])
    own = model.encoder.pos_rows((rows.shape[0] + 1) // 2 if not model.encoder.legacy else rows.shape[0])
    assert own.shape == rows.shape and float((own - rows).abs().max()) <= 1e-3
    if torch.equal(own, rows):
        return False
    own.copy_(rows)
    model.encoder.mark_dirty()
    return True


def test_both_registry_names_resolve_to_the_class():
    from funasr_amd.ebranchformer import EBranchformer, EBranchformerEncoder
    from funasr_amd.install import hip_classes

    assert tables.model_classes["EBranchformer"] is EBranchformer and tables.model_classes["Branchformer"] is EBranchformer
    assert tables.encoder_classes["EBranchformerEncoder"] is EBranchformerEncoder
    assert tables.decoder_classes["TransformerDecoder"] is TransformerDecoder
    assert not issubclass(EBranchformer, Conformer) and not issubclass(Conformer, EBranchformer)
    hc = hip_classes()
    for triple in (("model_classes", "EBranchformer", EBranchformer), ("model_classes", "Branchformer", EBranchformer),
                   ("encoder_classes", "EBranchformerEncoder", EBranchformerEncoder)):
        assert triple in hc


def test_state_dict_names_shapes_and_order_are_the_references():
    from funasr_amd.ebranchformer import EBranchformer

    ref = json.load(open(os.path.join(GOLDEN, "ebranchformer_state_dict.json")))
    assert ref["model"] == "Branchformer" and ref["encoder"] == "EBranchformerEncoder"
    m = tables.model_classes[ref["model"]](encoder=ref["encoder"], encoder_conf=ref["encoder_conf"], decoder=ref["decoder"],
                                           decoder_conf=ref["decoder_conf"], vocab_size=ref["vocab_size"], input_size=80, specaug="SpecAug",
                                           specaug_conf={"apply_time_warp": True}, **ref["model_conf"])
    assert isinstance(m, EBranchformer)
    own = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert own == ref["shapes"] and list(own) == list(ref["shapes"])              # the order too: synth draws in it
    assert not any("pe" == k.split(".")[-1] or "pos_table" in k for k in ref["shapes"])
    assert "encoder.encoders.0.attn.linear_pos.weight" in own and not any(".self_attn." in k for k in own if k.startswith("encoder."))
    sd = {k: torch.randn(shp) for k, shp in ref["shapes"].items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.encoder.encoders[11].cgmlp.csgu.conv.weight, sd["encoder.encoders.11.cgmlp.csgu.conv.weight"])
    big = synth.ebranchformer_conf(**synth.EBRANCHFORMER_TEMPLATE)
    assert big["encoder_conf"] == ref["encoder_conf"] and big["decoder_conf"] == ref["decoder_conf"] and big["vocab_size"] == ref["vocab_size"]
    for variant, kw in VARIANTS.items():
        t = EBranchformer(**synth.ebranchformer_conf(vocab=40, **kw))
        shapes = {k: list(v.shape) for k, v in t.state_dict().items()}
        assert shapes == ref["tiny_shapes"][variant] and list(shapes) == list(ref["tiny_shapes"][variant]), variant
        t.load_state_dict({k: torch.randn(shp) for k, shp in shapes.items()}, strict=True)
    assert not any("feed_forward" in k or "norm_ff" in k for k in ref["tiny_shapes"]["legacy_noffn"] if k.startswith("encoder."))


@pytest.mark.parametrize("where,conf,word", [
    ("model", {"encoder": "BranchformerEncoder"}, "BranchformerEncoder"), ("model", {"encoder": "ConformerEncoder"}, "ConformerEncoder"),
    ("encoder", {"attention_layer_type": "selfattn", "pos_enc_layer_type": "abs_pos"}, "pos_enc_layer_type"),
    ("encoder", {"attention_layer_type": "selfattn"}, "attention_layer_type"),
    ("encoder", {"attention_layer_type": "fast_selfattn"}, "attention_layer_type"),
    ("encoder", {"pos_enc_layer_type": "abs_pos"}, "pos_enc_layer_type"), ("encoder", {"pos_enc_layer_type": "scaled_abs_pos"}, "pos_enc_layer_type"),
    ("encoder", {"input_layer": "conv2d6"}, "input_layer"), ("encoder", {"input_layer": "linear"}, "input_layer"),
    ("encoder", {"input_layer": None}, "input_layer"), ("encoder", {"use_linear_after_conv": True}, "use_linear_after_conv"),
    ("encoder", {"gate_activation": "swish"}, "gate_activation"), ("encoder", {"zero_triu": True}, "zero_triu"),
    ("encoder", {"interctc_layer_idx": [1]}, "interctc_layer_idx"), ("encoder", {"interctc_use_conditioning": True}, "interctc_use_conditioning"),
    ("model", {"interctc_weight": 0.3}, "interctc_weight"), ("encoder", {"attention_heads": 4}, "attention_heads"),
    ("encoder", {"output_size": 192, "attention_heads": 2}, "output_size"), ("encoder", {"cgmlp_conv_kernel": 30}, "cgmlp_conv_kernel"),
    ("encoder", {"cgmlp_conv_kernel": 33}, "cgmlp_conv_kernel"), ("encoder", {"merge_conv_kernel": 4}, "merge_conv_kernel"),
    ("encoder", {"merge_conv_kernel": 33}, "merge_conv_kernel"), ("encoder", {"linear_units": 288}, "linear_units"),
    ("encoder", {"cgmlp_linear_units": 288}, "cgmlp_linear_units"), ("encoder", {"cgmlp_linear_units": 250}, "cgmlp_linear_units"),
    ("encoder", {"ffn_activation_type": "relu"}, "ffn_activation_type"), ("encoder", {"positionwise_layer_type": "conv1d"}, "positionwise_layer_type"),
    ("encoder", {"precision": "bf16"}, "precision"), ("encoder", {"precision": "bf16x3"}, "precision"),
    ("model", {"input_size": 6}, "input_size"), ("model", {"input_size": 257}, "input_size"),
    ("decoder", {"input_layer": "linear"}, "input_layer"), ("decoder", {"normalize_before": False}, "normalize_before"),
    ("decoder", {"concat_after": True}, "concat_after"), ("model", {"decoder": None}, "decoder"), ("model", {"ctc_weight": 1.0}, "decoder"),
    ("model", {"decoder": "ParaformerSANMDecoder"}, "decoder"), ("model", {"share_embedding": True}, "share_embedding")])
@pytest.mark.parametrize("name", ["EBranchformer", "Branchformer"])
def test_unsupported_options_raise_and_name_the_option(name, where, conf, word):
    import funasr_amd.ebranchformer  # noqa: F401

    c = synth.ebranchformer_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        tables.model_classes[name](**c)


def test_layer_drop_rate_is_accepted_and_ignored():
    from funasr_amd.ebranchformer import EBranchformer

    c = synth.ebranchformer_conf()
    c["encoder_conf"]["layer_drop_rate"] = 0.1
    a, b = EBranchformer(**c), EBranchformer(**synth.ebranchformer_conf())
    assert list(a.state_dict()) == list(b.state_dict())


def test_the_other_models_keep_refusing_the_branchformer_encoders_with_their_words():
    from funasr_amd.transformer import Transformer

    for cls, conf in ((Conformer, synth.conformer_conf()), (Transformer, synth.transformer_conf())):
        for enc in ("BranchformerEncoder", "EBranchformerEncoder"):
            conf["encoder"] = enc
            with pytest.raises(NotImplementedError, match="Branchformer famil"):
                cls(**conf)


def test_a_config_yaml_with_the_reference_templates_encoder_section_constructs(tmp_path):
    """the model / encoder / decoder sections of funasr/models/e_branchformer/template.yaml as recorded beside the shapes, through a
    written config.yaml and the registry, as AutoModel builds a model directory's class"""
    ref = json.load(open(os.path.join(GOLDEN, "ebranchformer_state_dict.json")))
    path = tmp_path / "config.yaml"
    with open(path, "w", encoding="utf-8") as f:
        yaml.safe_dump({k: ref[k] for k in ("model", "model_conf", "encoder", "encoder_conf", "decoder", "decoder_conf")}, f)
    conf = yaml.safe_load(open(path, encoding="utf-8"))
    import funasr_amd.ebranchformer  # noqa: F401
    m = tables.model_classes[conf["model"]](encoder=conf["encoder"], encoder_conf=conf["encoder_conf"], decoder=conf["decoder"],
                                            decoder_conf=conf["decoder_conf"], vocab_size=4234, input_size=80, **conf["model_conf"])
    e = m.encoder
    assert (e.output_size(), e.attention_heads, e.num_blocks, e.cgmlp_units, e.cgmlp_kernel, e.merge_kernel, e.linear_units) == \
        (256, 4, 12, 1024, 31, 31, 1024)
    assert e.use_ffn and e.macaron and not e.legacy and e.precision == "f16x2" and e.pos_table.shape == (9999, 256)
    c = e._make_config()
    assert (c.cgmlp_units, c.cgmlp_kernel, c.merge_kernel, c.use_ffn, c.macaron, c.legacy, c.precision) == (1024, 31, 31, 1, 1, 0, 3)


def test_cpu_parameters_raise_the_no_cpu_fallback_error():
    from funasr_amd.ebranchformer import EBranchformer

    m = EBranchformer(**synth.ebranchformer_conf())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 50, 80), [50])


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-30))


def _maxd(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_oracle_reproduces_the_references_float64_run_and_stays_within_its_float32_gaps(variant):
    """float64: 1e-9 relative on every recorded array. float32: the oracle is another valid float32 evaluation of the same formulas, so
    it stays within 4 x the recorded |fp32 - fp64| gap of the reference (the bar the GPU's fp32 mode is held to)."""
    g = load_golden(variant)
    _, sd, conf = golden_model(g, variant)
    sd64, sd32 = O.cast(sd), O.cast(sd, torch.float32)
    lens = [int(n) for n in g["lens"]]
    feats = [torch.from_numpy(g[f"feats_{i}"]) for i in range(len(lens))]
    assert [g[f"enc_{i}"].shape[0] for i in range(2)] == [40, 61] and g["batch_olens"].tolist() == [41, 61]
    for i, f in enumerate(feats):
        enc, olens = O.encoder(sd64, conf["encoder_conf"], f[None].double(), [lens[i]], pos_rows=g["pos_rows"])
        lp = O.ctc_log_softmax(sd64, enc)[0]
        assert olens == [g[f"enc_{i}"].shape[0]]
        assert _rel(enc[0], g[f"enc_{i}"]) <= 1e-9 and _rel(lp, g[f"ctc_{i}"]) <= 1e-9, i
        assert O.ctc_greedy(lp, olens[0]) == g[f"greedy_{i}"].tolist()
        e32, _ = O.encoder(sd32, conf["encoder_conf"], f[None], [lens[i]], pos_rows=g["pos_rows"])
        d = _maxd(e32[0], g[f"enc_{i}"])
        print(f"{variant} clip {i}: oracle fp32 vs recorded fp64 {d:.3e}, recorded gap {float(g[f'gap_enc_{i}']):.3e}")
        assert d <= 4 * float(g[f"gap_enc_{i}"])
    pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    enc, olens = O.encoder(sd64, conf["encoder_conf"], pad.double(), lens, pos_rows=g["pos_rows"])
    e32, _ = O.encoder(sd32, conf["encoder_conf"], pad, lens, pos_rows=g["pos_rows"])
    assert olens == g["batch_olens"].tolist()
    lp = O.ctc_log_softmax(sd64, enc)
    for i, n in enumerate(olens):
        assert _rel(enc[i, :n], g[f"batch_enc_{i}"]) <= 1e-9 and _rel(lp[i, :n], g[f"batch_ctc_{i}"]) <= 1e-9, i
        assert O.ctc_greedy(lp[i], n) == g[f"batch_greedy_{i}"].tolist()
        assert _maxd(e32[i, :n], g[f"batch_enc_{i}"]) <= 4 * float(g[f"gap_batch_enc_{i}"])
    # the ragged batch is NOT a set of independent clips: neither depthwise conv is masked, clip 0's frames differ from its solo run
    assert np.abs(g["batch_enc_0"][:40] - g["enc_0"]).max() > 100 * float(g["gap_batch_enc_0"])
    st = O.DecoderStepper(sd64, conf["decoder_conf"], torch.from_numpy(g["enc_0"]))
    for j, pre in enumerate(g["prefixes"]):
        got = O.score_prefix(st, [int(t) for t in str(pre).split(",")])
        assert _rel(got, g[f"step_{j}"]) <= 1e-9, j


def test_host_built_positional_rows_are_the_recorded_ones_up_to_the_hosts_exp():
    for variant in VARIANTS:
        g = load_golden(variant)
        model, _, _ = golden_model(g, variant)
        pin_positional_rows(model, g)
        assert g["pos_rows"].shape == ((61, 128) if variant.startswith("legacy") else (121, 128))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_host_beam_search_with_the_oracle_decoder_returns_the_references_nbest(variant):
    g = load_golden(variant)
    model, sd, conf = golden_model(g, variant)
    sd64 = O.cast(sd)
    memory = torch.from_numpy(g["enc_0"])
    ctc_logp = O.ctc_log_softmax(sd64, memory).numpy()
    for w in g["ctc_weights"].tolist():
        bs = BeamSearchTransformer(beam_size=int(g["beam"]), vocab_size=len(g["tokens"]), sos=model.sos, eos=model.eos, ctc_weight=w)
        nbest = bs(O.DecoderStepper(sd64, conf["decoder_conf"], memory), memory.shape[0], ctc_logp, dtype=torch.float64)[: int(g["nbest"])]
        assert len(nbest) == int(g["nbest"])
        for r, h in enumerate(nbest):
            assert h.yseq == g[f"nbest_ids_w{w}_{r}"].tolist(), (w, r)
            assert abs(h.score - float(g[f"nbest_score_w{w}_{r}"])) <= 8 * float(g["gap_nbest_score"]), (w, r)


def test_kernel_oracles_are_the_torch_modules():
    """the restated pieces against torch's own ops in float64: exact GELU, the depthwise convs (zero padding), the gating unit"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 9, 64, generator=g, dtype=torch.float64)
    assert float((O.gelu(x) - torch.nn.functional.gelu(x)).abs().max()) <= 1e-15
    for K in (1, 3, 15):
        w, b = torch.randn(64, 1, K, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
        want = torch.nn.functional.conv1d(x.transpose(1, 2), w, b, padding=(K - 1) // 2, groups=64).transpose(1, 2)
        assert float((O.dwconv(x, w, b) - want).abs().max()) <= 1e-13
        c = torch.cat([x[..., :32], x[..., 32:]], -1)
        assert float((O.merge(x[..., :32], x[..., 32:], w, b) - (c + want)).abs().max()) <= 1e-13
