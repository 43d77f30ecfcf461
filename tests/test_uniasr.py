"""UniASR, CPU side: registry, the reference's state-dict names and shapes, refused options, the chunk geometry of the package
(index maps, the three masks, the key-visibility rule the kernel evaluates) and the float64 restatement (tests/_uniasr_oracle.py)
against the reference's recorded float64 outputs at every stage of the three decoding modes (tests/golden/uniasr.npz, written by
tools/make_golden_uniasr.py), the margins of the recorded search, and `AutoModel` on a `model: UniASR` directory.

Bars of the float64 oracle against the recorded float64 run: 4 x the recorded fp32 - fp64 gap of the same quantity, 8 x for n-best
scores (the bars of tests/test_sanm.py); masks, index maps, alignments and ids are equal outright."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import synth
from funasr_amd.register import tables
from funasr_amd.uniasr import ChunkLayout, FsmnDecoderSCAMAOpt, StrideConv, UniASR

from . import _uniasr_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ["fast", "normal", "offline"]
MARGIN = 1e-3


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "uniasr.npz"), allow_pickle=False))


def golden_model(g):
    conf = synth.uniasr_conf(vocab=len(g["tokens"]))
    model = UniASR(**conf)
    sd = synth.uniasr_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def runs(golden):
    """the float64 oracle over the recorded clip in the three modes, once"""
    model, sd, conf = golden_model(golden)
    sd64 = O.cast(sd, torch.float64)
    feats = torch.from_numpy(golden["feats"]).double()
    return {mode: O.recognize(sd64, conf, feats, mode, beam_size=int(golden["beam"]), token_num_relax=int(golden["relax"])) for mode in MODES}, \
        sd64, conf


def _close(tag, got, want, gap, factor=4.0):
    d = float(np.abs(np.asarray(O.to_np(got), np.float64) - np.asarray(want, np.float64)).max())
    print(f"{tag}: max |d| {d:.3e}, recorded fp32 gap {gap:.3e} (bar {factor:g} x)")
    assert d <= factor * gap, (tag, d, gap)


def test_registry_keys():
    from funasr_amd.install import hip_classes
    from funasr_amd.paraformer_streaming import SANMEncoderChunkOpt

    assert tables.model_classes["UniASR"] is UniASR and tables.decoder_classes["FsmnDecoderSCAMAOpt"] is FsmnDecoderSCAMAOpt
    assert tables.encoder_classes["SANMEncoderChunkOpt"] is SANMEncoderChunkOpt
    assert ("model_classes", "UniASR", UniASR) in hip_classes()
    assert ("decoder_classes", "FsmnDecoderSCAMAOpt", FsmnDecoderSCAMAOpt) in hip_classes()


def test_state_dict_names_and_shapes_are_the_references():
    ref = json.load(open(os.path.join(GOLDEN, "uniasr_state_dict.json")))
    m = UniASR(**ref["conf"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    m.load_state_dict({k: torch.zeros(shp) for k, shp in ref["shapes"].items()}, strict=True)
    assert m.ctc is None and m.ctc2 is None and not any(k.startswith("ctc") for k in ref["shapes"])
    assert m.decoder.right_padding == 5 and m.decoder2.right_padding == 0 and m.decoder.decoders2 is None and len(m.decoder2.decoders2) == 1
    assert m.encoder2._input_size == 80 + 128 and isinstance(m.stride_conv, StrideConv)


@pytest.mark.parametrize("where,conf,word", [
    ("decoder", {"concat_embeds": True}, "concat_embeds"), ("decoder2", {"concat_embeds": True}, "concat_embeds"),
    ("decoder", {"input_layer": "linear"}, "input_layer"), ("decoder", {"normalize_before": False}, "normalize_before"),
    ("decoder", {"use_output_layer": False}, "use_output_layer"), ("decoder2", {"concat_after": True}, "concat_after"),
    ("decoder", {"attention_dim": 64}, "attention_dim"), ("decoder", {"attention_heads": 4}, "attention_heads"),
    ("decoder", {"linear_units": 250}, "linear_units"), ("decoder2", {"kernel_size": 33}, "kernel_size"),
    ("decoder", {"sanm_shfit": 6}, "sanm_shfit"), ("decoder", {"att_layer_num": 4}, "att_layer_num"),
    ("model", {"encoder": "SANMEncoder"}, "encoder"), ("model", {"encoder2": "ConformerEncoder"}, "encoder2"),
    ("model", {"decoder": "FsmnDecoder"}, "decoder"), ("model", {"decoder2": "ParaformerSANMDecoder"}, "decoder2"),
    ("model", {"predictor": "CifPredictorV3"}, "predictor"), ("model", {"predictor2": "CifPredictor"}, "predictor2"),
    ("model", {"decoder_attention_chunk_type": "full"}, "decoder_attention_chunk_type"),
    ("model", {"decoder_attention_chunk_type2": "full"}, "decoder_attention_chunk_type2"),
    ("model", {"stride_conv_conf": None}, "stride_conv_conf"), ("model", {"share_embedding": True}, "share_embedding"),
    ("model", {"precision": "bf16"}, "precision"), ("model", {"precision": "f16x2"}, "f16x2"),
    ("predictor", {"tail_threshold": 0.45}, "tail_threshold"), ("predictor2", {"tail_threshold": 0.45}, "tail_threshold"),
    ("encoder", {"input_layer": "conv2d"}, "input_layer"), ("encoder2", {"input_layer": "linear"}, "input_layer"),
    ("stride_conv", {"pad": [0, 1, 2]}, "pad"), ("stride_conv", {"kernel_size": 9}, "kernel_size")])
def test_unsupported_options_raise_and_name_the_option(where, conf, word):
    c = synth.uniasr_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word) as e:
        UniASR(**c)
    if where.startswith("decoder"):
        assert str(e.value).startswith("FsmnDecoderSCAMAOpt(HIP): ")


def test_inference_refuses_a_batch_and_scorers_that_do_not_exist():
    m = UniASR(**synth.uniasr_conf())
    with pytest.raises(NotImplementedError, match="batch_size"):
        m.inference(torch.zeros(2, 10, 80), data_lengths=[10, 10], batch_size=2, data_type="fbank")
    with pytest.raises(NotImplementedError, match="lm_weight"):
        m.init_beam_search(lm_weight=0.3)
    assert UniASR.decoding("fast") == (0, 1) and UniASR.decoding("offline") == (1, 2) and UniASR.decoding("anything") == (0, 2)


# ------------------------------------------------------------------------------------------------ chunk geometry
def _layout(geo, dec_look_back=1):
    return ChunkLayout(geo["T"], geo["chunk"], geo["stride"], geo["pad_left"], geo["shift"], geo["look_back"], dec_look_back)


@pytest.mark.parametrize("mode", MODES)
def test_chunk_masks_equal_the_references(golden, runs, mode):
    """the oracle's dense masks and the package's index maps / periodic vectors / key rule against overlap_chunk's recorded masks"""
    conf = runs[2]
    ind = O.MODES[mode][0]
    passes = [("geo1", conf["encoder_conf"], golden["feats"].shape[0])]
    if O.MODES[mode][1] == 2:
        passes.append(("geo2", conf["encoder2_conf"], golden[f"{mode}_stride_conv"].shape[0]))
    for name, econf, T in passes:
        geo = O.geometry_of(econf, T, ind)
        ref = {k: golden[f"{mode}_{name}_{k}"] for k in ("add", "rm", "mask_shift", "mask_predictor", "mask_att", "mask_dec", "len_chunk")}
        assert int(ref["len_chunk"][0]) == geo["Tc"]
        for k in ("add", "rm", "mask_shift", "mask_predictor", "mask_att"):
            assert np.array_equal(geo[k], ref[k].astype(np.float32)), (mode, name, k)
        assert np.array_equal(ref["mask_dec"].astype(np.float32), geo["mask_shift"])
        lay = _layout(geo)
        add_index, rm_index = O.index_maps(geo)
        assert lay.Tc == geo["Tc"] and np.array_equal(lay.add_index, add_index) and np.array_equal(lay.rm_index, rm_index)
        assert np.array_equal(lay.mask_shift, ref["mask_shift"]) and np.array_equal(lay.mask_predictor, ref["mask_predictor"])
        assert np.array_equal(lay.att_mask(), ref["mask_att"].astype(np.float32))


@pytest.mark.parametrize("chunk,stride,pad_left,look_back", [(4, 2, 1, 0), (4, 2, 1, 1), (6, 4, 2, 1), (6, 4, 2, 50), (5, 5, 0, 2), (7, 3, 2, 3),
                                                             (3, 1, 1, 2)])
def test_key_rule_equals_the_dense_mask_at_every_length(chunk, stride, pad_left, look_back):
    """the rule of csrc/uniasr.hip (own chunk + the first `stride` frames of the look-back chunks for a chunk's first `stride` rows)
    is the dense mask for every length around the chunk boundaries -- the intervals are NOT contiguous when stride < chunk or shift > 0"""
    for shift in (0, 5):
        for T in list(range(1, 3 * stride + 3)) + [4 * stride, 4 * stride + 1, 37]:
            geo = O.geometry(T, chunk, stride, pad_left, shift, look_back)
            lay = _layout(geo)
            add_index, rm_index = O.index_maps(geo)
            assert lay.Tc == geo["Tc"], (T, shift)
            assert np.array_equal(lay.add_index, add_index) and np.array_equal(lay.rm_index, rm_index), (T, shift)
            assert np.array_equal(lay.mask_shift, geo["mask_shift"]) and np.array_equal(lay.mask_predictor, geo["mask_predictor"])
            assert np.array_equal(lay.att_mask(), geo["mask_att"]), (T, shift)


def test_bad_geometry_is_refused():
    with pytest.raises(ValueError, match="chunk geometry"):
        ChunkLayout(10, 4, 3, 2, 5, 0, 1)                          # stride + pad_left > chunk_size: a negative right context


# ------------------------------------------------------------------------------------------------ stages against the golden
@pytest.mark.parametrize("mode", MODES)
def test_oracle_equals_the_references_recorded_stages(golden, runs, mode):
    g, r = golden, runs[0][mode]
    gap = lambda k: float(g[f"{mode}_gap_{k}"])                      # noqa: E731
    _close(f"{mode} pass 1", r["enc1"], g[f"{mode}_enc1"], gap("enc1"))
    if O.MODES[mode][1] == 2:
        _close(f"{mode} stride_conv", r["stride_conv"], g[f"{mode}_stride_conv"], gap("stride_conv"))
        _close(f"{mode} pass 2", r["enc2"], g[f"{mode}_enc2"], gap("enc2"))
    _close(f"{mode} alphas", r["alphas"], g[f"{mode}_alphas"], gap("alphas"))
    _close(f"{mode} token count", r["token_num"], g[f"{mode}_token_num"], gap("token_num"))
    assert np.array_equal(r["alignments"], g[f"{mode}_alignments"])
    assert np.array_equal(r["scama_mask"], g[f"{mode}_scama_mask"])
    # the package's host ports of the same two
    lay = _layout(r["geo"], int(golden_dec_look_back(runs[2], mode)))
    align = lay.frame_alignments(torch.from_numpy(g[f"{mode}_alphas"]).float())
    assert np.array_equal(align, g[f"{mode}_alignments"])
    assert np.array_equal(lay.scama_mask(align), g[f"{mode}_scama_mask"])


def golden_dec_look_back(conf, mode):
    ind, which = O.MODES[mode]
    return conf["encoder_conf" if which == 1 else "encoder2_conf"]["decoder_att_look_back_factor"][ind]


@pytest.mark.parametrize("mode", MODES)
def test_oracle_steps_equal_the_references_recorded_log_probabilities(golden, runs, mode):
    g, (r, sd64, conf) = golden, (runs[0][mode], runs[1], runs[2])
    which = O.MODES[mode][1]
    memory = torch.from_numpy(g[f"{mode}_enc{which}"])
    dconf, dp = (conf["decoder_conf"], "decoder.") if which == 1 else (conf["decoder2_conf"], "decoder2.")
    st = O.ScamaStepper(sd64, dconf, memory, g[f"{mode}_scama_mask"], prefix=dp)
    prefix = g["prefix"].tolist()
    st.begin(len(prefix), 1)
    for j, tok in enumerate(prefix, 1):
        _close(f"{mode} step {j}", st.step([tok], j - 1)[0], g[f"{mode}_step_{j}"], float(g[f"{mode}_gap_step_{j}"]))
    empty = O.ScamaStepper(sd64, dconf, memory, np.zeros((1, memory.shape[0]), np.float32), prefix=dp)
    empty.begin(1, 1)
    _close(f"{mode} step under an all-zero mask row", empty.step([prefix[0]], 0)[0], g[f"{mode}_step_empty"], float(g[f"{mode}_gap_step_empty"]))


@pytest.mark.parametrize("mode", MODES)
def test_oracle_search_equals_the_references_nbest_with_a_margin(golden, runs, mode):
    g, r = golden, runs[0][mode]
    nbest = r["nbest"][: int(g["nbest"])]
    assert len(nbest) == int(g["nbest"])
    for k, h in enumerate(nbest):
        assert h.yseq == g[f"{mode}_nbest_ids_{k}"].tolist(), (mode, k)
        d = abs(h.score - float(g[f"{mode}_nbest_score_{k}"]))
        print(f"{mode} rank {k}: score {h.score:.6f} |d| {d:.2e} (bar {8 * float(g[mode + '_gap_nbest_score']):.2e})")
        assert d <= 8 * float(g[mode + "_gap_nbest_score"]), (mode, k, d)
    # no pruning decision of the recorded search, and no cumulative alpha sum, within 1e-3 of a tie: the GPU run may be asked for the
    # same ids and the same order outright
    print(f"{mode}: smallest gap at a pruning decision {r['margin']:.3e}, smallest |cumsum - integer| {r['cumsum_margin']:.3e}")
    assert r["margin"] >= MARGIN and r["cumsum_margin"] >= MARGIN


# ------------------------------------------------------------------------------------------------ AutoModel
def write_model_dir(path, seed=None):
    """a `model: UniASR` directory of the golden configuration with the golden's synthetic weights -> (state dict, conf, tokens)"""
    os.makedirs(path, exist_ok=True)
    g = load_golden()
    tokens = g["tokens"].tolist()
    c = synth.uniasr_conf(vocab=len(tokens))
    sections = {k: c[k] for k in c if k.endswith("_conf") or k in ("encoder", "encoder2", "decoder", "decoder2", "predictor", "predictor2",
                                                                   "stride_conv")}
    conf = dict(sections, model="UniASR", model_conf={"ctc_weight": 0.0, "lsm_weight": 0.1, "length_normalized_loss": True,
                                                      "decoder_attention_chunk_type": "chunk", "loss_weight_model1": 0.5},
                frontend="WavFrontend", frontend_conf={"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                       "lfr_m": 1, "lfr_n": 1},
                tokenizer="CharTokenizer", tokenizer_conf={"unk_symbol": "<unk>", "split_with_space": True})
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    sd = synth.uniasr_state_dict(int(g["seed"]) if seed is None else seed, UniASR(**c))
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return sd, c, tokens


def test_automodel_resolves_a_uniasr_directory(tmp_path):
    """construction only: no device"""
    from funasr_amd.auto_model import AutoModel

    sd, c, tokens = write_model_dir(str(tmp_path / "uniasr"))
    am = AutoModel(model=str(tmp_path / "uniasr"), device="cpu", disable_update=True)
    assert isinstance(am.model, UniASR) and isinstance(am.model.decoder2, FsmnDecoderSCAMAOpt)
    assert torch.equal(am.model.stride_conv.conv.weight, sd["stride_conv.conv.weight"])
    assert torch.equal(am.model.encoder2.encoders0[0].self_attn.linear_q_k_v.weight, sd["encoder2.encoders0.0.self_attn.linear_q_k_v.weight"])
    assert am.model.encoder._mode() == "fp32" and am.model.encoder.chunk_size == [4, 6]


from oracle import ref_import  # noqa: E402

REF_REGISTER = os.path.join(ref_import.REF_ROOT, "funasr", "register.py")


@pytest.mark.skipif(not os.path.exists(REF_REGISTER), reason="reference checkout not present")
def test_install_puts_uniasr_into_the_references_registry_and_it_builds_by_name():
    import importlib.util

    from funasr_amd import install as inst

    spec = importlib.util.spec_from_file_location("_ref_register_uniasr", REF_REGISTER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    done = inst.install(mod.tables)
    assert ("model_classes", "UniASR") in done and ("decoder_classes", "FsmnDecoderSCAMAOpt") in done
    m = mod.tables.model_classes.get("UniASR")(**synth.uniasr_conf())
    assert isinstance(m, UniASR) and mod.tables.decoder_classes.get("FsmnDecoderSCAMAOpt") is FsmnDecoderSCAMAOpt
