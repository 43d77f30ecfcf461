"""Paraformer-v2 without a GPU: registry, checkpoint format, and the CPU restatement of the posterior stage
(tests/_paraformer_v2_oracle.py) against what the reference recorded in tests/golden/paraformer_v2.npz
(tools/make_golden_paraformer_v2.py; where the reference tree is importable, against its live classes too)."""
import os
import sys

import numpy as np
import pytest
import torch

import funasr_amd.auto_model  # noqa: F401  (registers every class)
from funasr_amd import synth
from funasr_amd.register import tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _paraformer_v2_oracle as PO  # noqa: E402

GOLD = PO.load_golden()
CLIPS = [(s, T) for s in sorted(PO.SHAPES) for T in PO.CLIP_T]


def _state(shape):
    return PO.model_state(shape, int(GOLD[f"{shape}.seed"]), float(GOLD["ctc_gain"]), float(GOLD["blank_bias"]))


@pytest.fixture(scope="module")
def states():
    return {s: _state(s) for s in PO.SHAPES}


def test_registry_names_resolve():
    from funasr_amd.paraformer_v2 import Paraformer_v2_community, ParaformerSANMDecoder_v2_community
    assert tables.model_classes.get("Paraformer_v2_community") is Paraformer_v2_community
    assert tables.decoder_classes.get("ParaformerSANMDecoder_v2_community") is ParaformerSANMDecoder_v2_community
    from funasr_amd import install
    pairs = {(t, k) for t, k, _ in install.hip_classes()}
    assert ("model_classes", "Paraformer_v2_community") in pairs and ("decoder_classes", "ParaformerSANMDecoder_v2_community") in pairs


@pytest.mark.parametrize("shape", sorted(PO.SHAPES))
def test_strict_load_accepts_exactly_the_reference_keys(shape, states):
    conf, sd = states[shape]
    model = tables.model_classes.get("Paraformer_v2_community")(**conf)
    ref = dict(zip(GOLD[f"{shape}.keys"].tolist(), GOLD[f"{shape}.key_shapes"].tolist()))
    mine = {k: ",".join(str(d) for d in v.shape) for k, v in model.state_dict().items()}
    assert mine == ref
    assert set(sd) == set(ref)
    model.load_state_dict(sd, strict=True)
    for k in ("decoder.embed.0.weight", "decoder.embed.0.bias", "decoder.embed.1.weight", "decoder.embed.1.bias", "ctc.ctc_lo.weight"):
        assert k in ref


def test_constructor_refusals():
    cls = tables.model_classes.get("Paraformer_v2_community")
    conf = synth.paraformer_v2_conf(**PO.SHAPES["A"])
    for w in (0.0, 1.0):
        with pytest.raises(NotImplementedError, match="ctc_weight"):
            cls(**dict(conf, ctc_weight=w))
    with pytest.raises(NotImplementedError, match="input_layer"):
        cls(**dict(conf, decoder_conf=dict(conf["decoder_conf"], input_layer="embed")))
    m = cls(**dict(conf, specaug="SpecAugLFR", specaug_conf={"apply_time_warp": False}, report_cer=True))     # training-only: ignored
    for mode in ("bf16", "bf16x3"):
        with pytest.raises(ValueError, match="f16x2"):
            m.set_precision(mode)
    with pytest.raises(ValueError):
        cls(**dict(conf, precision="bf16"))
    assert cls(**dict(conf, precision="fp32")).decoder._mode() == "fp32"


def _weights(sd):
    return (sd["ctc.ctc_lo.weight"], sd["ctc.ctc_lo.bias"], sd["decoder.embed.0.weight"], sd["decoder.embed.0.bias"],
            sd["decoder.embed.1.weight"], sd["decoder.embed.1.bias"])


@pytest.mark.parametrize("shape,T", CLIPS)
def test_oracle_reproduces_the_reference_records(shape, T, states):
    conf, sd = states[shape]
    cw, cb, w0, b0, g, b = _weights(sd)
    p = f"{shape}.T{T}."
    enc = torch.from_numpy(GOLD[p + "enc"])
    probs, path = PO.greedy_path(enc, cw, cb)
    assert np.array_equal(path.numpy(), GOLD[p + "path"])
    runs = PO.runs_of(path, conf["blank_id"])
    merged = PO.merged_posteriors(probs, runs)
    assert merged.shape == GOLD[p + "merged"].shape and len(runs) > 0
    assert float((merged - torch.from_numpy(GOLD[p + "merged"])).abs().max()) <= 1e-6
    emb = PO.embed_merged(merged, w0, b0, g, b)
    ref_emb = torch.from_numpy(GOLD[p + "embed"])
    assert float((emb - ref_emb).abs().max()) <= 1e-6                      # torch fp32 against torch fp32: the same operations
    ids = GOLD[p + "raw_ids"]                                   # arg-max of the reference's decoder logits
    assert PO.filter_tokens(ids, conf["sos"], conf["eos"], conf["blank_id"]) == GOLD[p + "token_int"].tolist()
    assert GOLD[p + "gaps"].min() >= 0.02                       # the confidence condition the golden script asserts


@pytest.mark.parametrize("shape,T", CLIPS)
def test_frame_domain_identity(shape, T, states):
    """Linear(mean_t p_t) = mean_t(p_t W^T) + b: the frame-domain order the kernel uses against the reference's order, float64"""
    conf, sd = states[shape]
    cw, cb, w0, b0, g, b = _weights(sd)
    enc = torch.from_numpy(GOLD[f"{shape}.T{T}.enc"]).double()
    probs, path = PO.greedy_path(enc, cw.double(), cb.double())
    runs = PO.runs_of(path, conf["blank_id"])
    a = PO.embed_frame_domain(probs, runs, w0, b0, g, b)
    r = PO.embed_merged(PO.merged_posteriors(probs, runs), w0.double(), b0.double(), g, b)
    assert a.shape == r.shape and float((a - r).abs().max()) <= 1e-6


def test_all_blank_clip_has_no_runs():
    for shape in PO.SHAPES:
        path = GOLD[f"{shape}.blank.path"]
        assert path.shape == (PO.BLANK_T,) and PO.runs_of(path, 0) == []


def test_runs_of_edges():
    assert PO.runs_of([0, 0, 0], 0) == []
    assert PO.runs_of([5, 5, 0, 5], 0) == [(0, 2), (3, 4)]        # the same label on both sides of a blank: two runs
    assert PO.runs_of([1, 2, 2, 3], 0) == [(0, 1), (1, 3), (3, 4)]
    assert PO.runs_of([7], 0) == [(0, 1)]


def test_embedder_cases_are_confident_and_e_ref_is_recorded():
    for V in PO.EMBED_V:
        hid, lens, w = PO.embedder_case(V, int(GOLD[f"embed.V{V}.seed"]))
        ref64, gap = PO.embedder_reference(hid, lens, w, torch.float64)
        assert gap >= 0.02 and float(GOLD[f"embed.V{V}.e_ref"]) > 0
        assert sum(len(r[1]) for r in ref64) >= 8


def _reference_here():
    from oracle import ref_import
    return ref_import.available() and os.path.isdir(os.path.join(ref_import.REF_ROOT, "funasr", "models", "paraformer_v2_community"))


@pytest.mark.skipif(not _reference_here(), reason="reference tree not present")
def test_against_the_live_reference_classes():
    """The oracle and the committed golden against the reference's own classes. In a process of its own: importing the reference
    registers its classes, and other tests of the suite depend on which registration came last."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "make_golden_paraformer_v2.py"), "--check"], cwd=root,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "live reference ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def test_automodel_builds_the_class_from_a_model_dir(tmp_path):
    """config.yaml `model: Paraformer_v2_community` -> AutoModel builds the class; without a GPU it stops at construction"""
    import json
    import shutil
    import yaml
    from _model_dir import VOCAB
    from funasr_amd.auto_model import AutoModel

    conf = synth.paraformer_v2_conf(**dict(PO.SHAPES["A"], vocab=len(VOCAB)))
    sd = synth.paraformer_v2_state_dict(conf, seed=3)
    d = str(tmp_path / "v2")
    os.makedirs(d)
    cfg = {"model": "Paraformer_v2_community",
           "model_conf": {k: conf[k] for k in ("ctc_weight", "lsm_weight", "length_normalized_loss", "blank_id", "sos", "eos")},
           "encoder": conf["encoder"], "encoder_conf": conf["encoder_conf"], "decoder": conf["decoder"], "decoder_conf": conf["decoder_conf"],
           "ctc_conf": conf["ctc_conf"], "frontend": "WavFrontend",
           "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10, "lfr_m": 7, "lfr_n": 6},
           "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(d, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(cfg, f, allow_unicode=True)
    torch.save(sd, os.path.join(d, "model.pt"))
    with open(os.path.join(d, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(VOCAB, f, ensure_ascii=False)
    shutil.copy(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "am.mvn"), os.path.join(d, "am.mvn"))
    am = AutoModel(model=d, device="cpu", disable_update=True)
    assert type(am.model).__name__ == "Paraformer_v2_community"
    assert torch.equal(am.model.decoder.embed.state_dict()["0.weight"], sd["decoder.embed.0.weight"])
    with pytest.raises(RuntimeError, match="AMD GPU"):
        am.model.encoder(torch.zeros(1, 8, 560), [8])
