"""SANM, CPU side: registry, the reference's state-dict names and shapes, refused options, the float64 restatement of the decoder step
against the reference's recorded float64 outputs (tests/golden/sanm.npz, written by tools/make_golden_sanm.py), the trap of the FSMN
cache rule (the step is NOT the teacher-forced forward when the right padding is not zero), the host beam search driven by the
oracle stepper against the reference's recorded n-best, and `AutoModel` on a `model: SANM` directory.

Bar of the float64 oracle against the recorded float64 run: 4 x the recorded fp32 - fp64 gap of the same quantity (the issue's bar;
the two float64 computations actually agree to ~1e-13, which is printed)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import synth
from funasr_amd.conformer import Conformer
from funasr_amd.register import tables
from funasr_amd.sanm import SANM, FsmnDecoder, fsmn_paddings
from funasr_amd.transformer_search import BeamSearchTransformer

from . import _sanm_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = {
    "A": dict(output_size=128, attention_heads=2, linear_units=64, enc_blocks=2, dec_blocks=3, att_layer_num=2, kernel=11, ctc_weight=0.3),
    "B": dict(output_size=256, attention_heads=2, linear_units=256, enc_blocks=2, dec_blocks=2, att_layer_num=2, kernel=4, sanm_shfit=0,
              ctc_weight=0.0),
}


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "sanm.npz"), allow_pickle=False))


def golden_model(g, name):
    conf = synth.sanm_conf(vocab=len(g["tokens"]), **CONFIGS[name])
    model = SANM(**conf)
    sd = synth.sanm_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def golden_prefix(g, n):
    return [1] + [3 + (5 + 11 * i) % (len(g["tokens"]) - 4) for i in range(n - 1)]


def test_registry_keys():
    from funasr_amd.install import hip_classes
    from funasr_amd.sanm_encoder import SANMEncoder
    from funasr_amd.transformer import Transformer

    assert tables.model_classes["SANM"] is SANM and tables.decoder_classes["FsmnDecoder"] is FsmnDecoder
    assert tables.encoder_classes["SANMEncoder"] is SANMEncoder
    assert not issubclass(SANM, Transformer) and not issubclass(SANM, Conformer)
    assert ("model_classes", "SANM", SANM) in hip_classes() and ("decoder_classes", "FsmnDecoder", FsmnDecoder) in hip_classes()


def test_state_dict_names_and_shapes_are_the_references_at_the_template():
    ref = json.load(open(os.path.join(GOLDEN, "sanm_state_dict.json")))
    m = SANM(encoder="SANMEncoder", encoder_conf=ref["encoder_conf"], decoder="FsmnDecoder", decoder_conf=ref["decoder_conf"],
             vocab_size=ref["vocab_size"], input_size=ref["input_size"], specaug="SpecAugLFR", specaug_conf={"lfr_rate": 6}, **ref["model_conf"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert m.ctc is None and not any(k.startswith("ctc.") for k in ref["shapes"])                 # the template's ctc_weight 0.0
    m.load_state_dict({k: torch.zeros(shp) for k, shp in ref["shapes"].items()}, strict=True)
    big = synth.sanm_conf(**synth.SANM_TEMPLATE)
    assert big["encoder_conf"] == ref["encoder_conf"] and big["decoder_conf"] == ref["decoder_conf"]
    assert big["vocab_size"] == ref["vocab_size"] and big["input_size"] == ref["input_size"] and big["ctc_weight"] == ref["model_conf"]["ctc_weight"]
    d = m.decoder
    assert (d.kernel_size, d.sanm_shfit, d.left_padding, d.right_padding, d.att_layer_num, d.num_blocks) == (11, 0, 5, 5, 16, 16)
    assert d.decoders2 is None and d.d_model // d.attention_heads == 128


def test_paddings_of_the_cache_rule():
    assert fsmn_paddings(11, None) == (10, 0) and fsmn_paddings(21, None) == (20, 0)      # the constructor's default: causal
    assert fsmn_paddings(11, 0) == (5, 5) and fsmn_paddings(4, 0) == (1, 2) and fsmn_paddings(4, None) == (2, 1)
    assert fsmn_paddings(11, 3) == (8, 2) and fsmn_paddings(1, None) == (0, 0) and fsmn_paddings(32, 0) == (15, 16)
    assert fsmn_paddings(11, 6)[1] < 0


@pytest.mark.parametrize("where,conf,word", [
    ("decoder", {"input_layer": "linear"}, "input_layer"), ("decoder", {"normalize_before": False}, "normalize_before"),
    ("decoder", {"use_output_layer": False}, "use_output_layer"), ("decoder", {"concat_after": True}, "concat_after"),
    ("decoder", {"concat_embeds": True}, "concat_embeds"), ("decoder", {"attention_dim": 64}, "attention_dim"),
    ("decoder", {"attention_heads": 4}, "attention_heads"), ("decoder", {"attention_heads": 0}, "attention_heads"),
    ("decoder", {"linear_units": 250}, "linear_units"), ("decoder", {"linear_units": 4096}, "linear_units"),
    ("decoder", {"kernel_size": 33}, "kernel_size"), ("decoder", {"kernel_size": 0}, "kernel_size"),
    ("decoder", {"sanm_shfit": 6}, "sanm_shfit"), ("decoder", {"sanm_shfit": -1}, "sanm_shfit"),
    ("decoder", {"att_layer_num": 4}, "att_layer_num"), ("decoder", {"att_layer_num": 0}, "att_layer_num"),
    ("model", {"decoder": None}, "decoder"), ("model", {"ctc_weight": 1.0}, "decoder"), ("model", {"decoder": "TransformerDecoder"}, "decoder"),
    ("model", {"decoder": "ParaformerSANMDecoder"}, "decoder"), ("model", {"encoder": "ConformerEncoder"}, "ConformerEncoder"),
    ("model", {"encoder": "TransformerEncoder"}, "encoder"), ("model", {"interctc_weight": 0.3}, "interctc_weight"),
    ("model", {"share_embedding": True}, "share_embedding"), ("model", {"precision": "bf16"}, "precision"),
    ("model", {"precision": "f16x2"}, "f16x2"), ("encoder", {"input_layer": "conv2d"}, "input_layer")])
def test_unsupported_options_raise_and_name_the_option(where, conf, word):
    c = synth.sanm_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        SANM(**c)


def test_accepted_options():
    assert SANM(**synth.sanm_conf(ctc_weight=0.0)).ctc is None
    m = SANM(**dict(synth.sanm_conf(), precision="fp32"))
    assert m.ctc is not None and m.encoder._mode() == "fp32"
    c = synth.sanm_conf()
    c["decoder_conf"]["attention_dim"] = 128                      # equal to the encoder's width
    SANM(**c)
    wide = SANM(**dict(synth.sanm_conf(output_size=256, linear_units=256), precision="f16x2"))
    assert wide.encoder._mode() == "f16x2" and wide.decoder.d_model // wide.decoder.attention_heads == 128


def test_conformer_and_transformer_refusals_are_unchanged():
    from funasr_amd.transformer import Transformer

    c = synth.conformer_conf()
    c["decoder"] = "FsmnDecoder"
    with pytest.raises(NotImplementedError) as e:
        Conformer(**c)
    assert str(e.value) == "Conformer(HIP): decoder: FsmnDecoder is not built (only TransformerDecoder)"
    c = synth.transformer_conf()
    c["decoder"] = "ParaformerSANMDecoder"
    with pytest.raises(NotImplementedError) as e:
        Transformer(**c)
    assert str(e.value) == "Transformer(HIP): decoder: ParaformerSANMDecoder is not built (only TransformerDecoder)"
    c = synth.transformer_conf()
    c["encoder"] = "SANMEncoder"
    with pytest.raises(NotImplementedError) as e:
        Transformer(**c)
    assert str(e.value) == ("Transformer(HIP): encoder: SANMEncoder is not built (only TransformerEncoder; ConformerEncoder belongs to model: "
                            "Conformer, the Branchformer family is another model)")
    c = synth.conformer_conf()
    c["encoder"] = "TransformerEncoder"
    with pytest.raises(NotImplementedError) as e:
        Conformer(**c)
    assert str(e.value) == ("Conformer(HIP): encoder: TransformerEncoder is not built (only ConformerEncoder; the Transformer / "
                            "Branchformer families are other models)")
    c = synth.sanm_conf()
    c["decoder"] = "TransformerDecoder"
    with pytest.raises(NotImplementedError) as e:
        SANM(**c)
    assert str(e.value) == "SANM(HIP): decoder: TransformerDecoder is not built (only FsmnDecoder)"


def test_cpu_parameters_raise_the_no_cpu_fallback_error():
    m = SANM(**synth.sanm_conf())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 50, 80), [50])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.decoder.set_memory(torch.zeros(5, 128))


def test_batch_decoding_without_a_ctc_head_raises_the_existing_error():
    m = SANM(**synth.sanm_conf(ctc_weight=0.0))
    with pytest.raises(RuntimeError, match="this model has none"):
        m.inference(torch.zeros(3, 50, 80), data_lengths=[50, 50, 50], batch_size=3)


@pytest.mark.parametrize("name", ["A", "B"])
def test_float64_oracle_step_equals_the_references_recorded_step(name):
    g = load_golden()
    _, sd, conf = golden_model(g, name)
    st = O.FsmnStepper(O.cast(sd), conf["decoder_conf"], torch.from_numpy(g[f"{name}_enc_1"]))
    K = conf["decoder_conf"]["kernel_size"]
    assert g[f"{name}_prefix_lengths"].tolist() == sorted({1, 2, K - 1, K, K + 1, K + 3})
    for n in g[f"{name}_prefix_lengths"].tolist():
        got = O.score_prefix(st, golden_prefix(g, n))
        d, gap = float(np.abs(O.to_np(got) - g[f"{name}_step_{n}"]).max()), float(g[f"{name}_gap_step_{n}"])
        print(f"{name} step after {n} tokens: max |d| {d:.3e}, recorded fp32 - fp64 gap {gap:.3e}")
        assert d <= 4 * gap, (name, n, d, gap)


def test_the_step_is_not_the_teacher_forced_forward_when_the_right_padding_is_not_zero():
    """the trap: configuration B (even kernel, sanm_shfit 0, R = 2) -- the cache rule puts R zeros between the first token and the
    second, the teacher-forced pass pads the END of the sequence. Configuration A (R = 0) is the causal memory: there they agree."""
    g = load_golden()
    for name, differs in (("A", False), ("B", True)):
        _, sd, conf = golden_model(g, name)
        sd64, dec = O.cast(sd), conf["decoder_conf"]
        memory = torch.from_numpy(g[f"{name}_enc_1"])
        K = dec["kernel_size"]
        pre = golden_prefix(g, K + 3)
        st = O.FsmnStepper(sd64, dec, memory)
        st.begin(len(pre), 1)
        steps = torch.cat([st.step([t], i) for i, t in enumerate(pre)])
        full = O.forward_teacher_forced(sd64, dec, memory, pre)
        d = float((steps - full).abs().max())
        print(f"{name}: L, R = {O.paddings(K, dec.get('sanm_shfit'))}, max |step - forward| over {len(pre)} positions {d:.3e}")
        assert (d > 1e-2) if differs else (d < 1e-9), (name, d)


def test_host_beam_search_with_the_oracle_stepper_returns_the_references_nbest():
    from ._conformer_oracle import ctc_log_softmax

    g = load_golden()
    for name in ("A", "B"):
        model, sd, conf = golden_model(g, name)
        sd64 = O.cast(sd)
        memory = torch.from_numpy(g[f"{name}_enc_0"])
        ctc_logp = ctc_log_softmax(sd64, memory).numpy() if model.ctc is not None else None
        for w in g[f"{name}_ctc_weights"].tolist():
            model.beam_search = None
            model.init_beam_search(token_list=g["tokens"].tolist(), decoding_ctc_weight=w, beam_size=int(g["beam"]))
            bs = model.beam_search
            assert isinstance(bs, BeamSearchTransformer) and (model.ctc is not None or bs.w_ctc == 0.0)
            nbest = bs(O.FsmnStepper(sd64, conf["decoder_conf"], memory), memory.shape[0], ctc_logp if bs.w_ctc != 0 else None,
                       dtype=torch.float64)[: int(g["nbest"])]
            assert len(nbest) == int(g["nbest"])
            for r, h in enumerate(nbest):
                assert h.yseq == g[f"{name}_nbest_ids_w{w}_{r}"].tolist(), (name, w, r)
                d = abs(h.score - float(g[f"{name}_nbest_score_w{w}_{r}"]))
                print(f"{name} w={w} rank {r}: score {h.score:.6f} |d| {d:.2e} (bar {8 * float(g[name + '_gap_nbest_score']):.2e})")
                assert d <= 8 * float(g[name + "_gap_nbest_score"]), (name, w, r, d)
        model.beam_search = None


def write_model_dir(path, name="A", seed=31):
    """a `model: SANM` directory of golden configuration `name` with synthetic weights -> (state dict, conf, tokens)"""
    os.makedirs(path, exist_ok=True)
    tokens = load_golden()["tokens"].tolist()
    c = synth.sanm_conf(vocab=len(tokens), **CONFIGS[name])
    conf = {"model": "SANM", "model_conf": {"ctc_weight": c["ctc_weight"], "lsm_weight": 0.1, "length_normalized_loss": True},
            "encoder": c["encoder"], "encoder_conf": c["encoder_conf"], "decoder": c["decoder"], "decoder_conf": c["decoder_conf"],
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "specaug": "SpecAugLFR", "specaug_conf": {"apply_time_warp": False, "lfr_rate": 6},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    sd = synth.sanm_state_dict(seed, SANM(**c))
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return sd, c, tokens


@pytest.mark.parametrize("name", ["A", "B"])
def test_automodel_resolves_a_sanm_directory(tmp_path, name):
    """construction only: no device"""
    from funasr_amd.auto_model import AutoModel

    sd, c, tokens = write_model_dir(str(tmp_path / "sanm"), name)
    am = AutoModel(model=str(tmp_path / "sanm"), device="cpu", disable_update=True)
    assert isinstance(am.model, SANM) and isinstance(am.model.decoder, FsmnDecoder)
    assert (am.model.ctc is None) == (name == "B")
    assert torch.equal(am.model.decoder.decoders[1].self_attn.fsmn_block.weight, sd["decoder.decoders.1.self_attn.fsmn_block.weight"])


from oracle import ref_import  # noqa: E402

REF_REGISTER = os.path.join(ref_import.REF_ROOT, "funasr", "register.py")


@pytest.mark.skipif(not os.path.exists(REF_REGISTER), reason="reference checkout not present")
def test_install_puts_sanm_into_the_references_registry_and_it_builds_by_name():
    """what funasr.AutoModel.build_model does after funasr_amd.install(): the class by its `model:` name, the config's sections as
    keywords (the reference's register.py loaded as a single file: importing the whole package takes a minute)"""
    import importlib.util

    from funasr_amd import install as inst

    spec = importlib.util.spec_from_file_location("_ref_register_sanm", REF_REGISTER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tables_ref = mod.tables

    @tables_ref.register("model_classes", "SANM")
    class Placeholder:                                                   # what the reference would have registered
        pass

    done = inst.install(tables_ref)
    assert ("model_classes", "SANM") in done and ("decoder_classes", "FsmnDecoder") in done
    assert tables_ref.model_classes.get("SANM") is SANM and tables_ref.decoder_classes.get("FsmnDecoder") is FsmnDecoder
    tmpl = yaml.safe_load(open(os.path.join(ref_import.REF_ROOT, "funasr", "models", "sanm", "template.yaml")))
    small = dict(tmpl["encoder_conf"], num_blocks=1), dict(tmpl["decoder_conf"], num_blocks=1, att_layer_num=1)
    m = tables_ref.model_classes.get(tmpl["model"])(encoder=tmpl["encoder"], encoder_conf=small[0], decoder=tmpl["decoder"], decoder_conf=small[1],
                                                    specaug=tmpl["specaug"], specaug_conf=tmpl["specaug_conf"], normalize=tmpl["normalize"],
                                                    ctc_conf=tmpl["ctc_conf"], vocab_size=30, input_size=560, **tmpl["model_conf"])
    assert isinstance(m, SANM) and m.ctc is None and m.decoder.right_padding == 5
