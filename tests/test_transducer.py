"""Transducer (RNN-T) without a GPU: the registry, the reference's state-dict names and shapes, strict loading with and without the
auxiliary heads, the refusals, and the float64 / float32 oracle restatement (tests/_transducer_oracle.py) against the reference's
recorded results (tests/golden/transducer.npz, written by tools/make_golden_transducer.py).

Bars: quantities within 4 x the reference's own fp32 - fp64 gap, search ids and evaluation counts exact, scores within
8 x gap_score -- the fp32 rules of tests/test_transformer_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import synth
from funasr_amd.register import tables

from . import _transducer_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "transducer.npz"), allow_pickle=False))


def golden_model(g):
    from funasr_amd.transducer import Transducer

    conf = synth.transducer_conf(vocab=len(g["tokens"]))
    model = Transducer(**conf)
    sd = synth.transducer_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def golden_searches():
    """(name, clip, frames or None for all, beam) of every recorded search"""
    return [("t1", 0, 1, 2)] + [(f"c{i}_b{b}", i, None, b) for i in range(3) for b in (1, 2, 5)]


def test_registry_keys():
    from funasr_amd.transducer import JointNetwork, RNNTDecoder, Transducer

    assert tables.model_classes["Transducer"] is Transducer
    assert tables.decoder_classes["rnnt_decoder"] is RNNTDecoder
    assert tables.joint_network_classes["joint_network"] is JointNetwork
    from funasr_amd.install import hip_classes
    got = hip_classes()
    assert ("model_classes", "Transducer", Transducer) in got and ("decoder_classes", "rnnt_decoder", RNNTDecoder) in got
    assert ("joint_network_classes", "joint_network", JointNetwork) in got


def _template_model(ref, **extra):
    from funasr_amd.transducer import Transducer

    return Transducer(encoder=ref["encoder"], encoder_conf=ref["encoder_conf"], decoder="rnnt_decoder", decoder_conf=ref["decoder_conf"],
                      joint_network="joint_network", joint_network_conf=ref["joint_network_conf"], vocab_size=ref["vocab_size"],
                      input_size=80, **dict(ref["model_conf"], **extra))


def test_state_dict_names_and_shapes_are_the_references():
    ref = json.load(open(os.path.join(GOLDEN, "transducer_state_dict.json")))
    m = _template_model(ref)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert [k for k in m.state_dict() if k.startswith(("decoder.", "joint_network."))] == \
        [k for k in ref["shapes"] if k.startswith(("decoder.", "joint_network."))]                      # and in the reference's order
    sd = {k: torch.randn(shp) for k, shp in ref["shapes"].items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.decoder.rnn[0].weight_hh_l0, sd["decoder.rnn.0.weight_hh_l0"])
    assert torch.equal(m.joint_network.lin_dec.weight, sd["joint_network.lin_dec.weight"]) and m.joint_network.lin_dec.bias is None
    t = synth.TRANSDUCER_TEMPLATE
    assert ref["decoder_conf"]["embed_size"] == t["embed_size"] and ref["decoder_conf"]["hidden_size"] == t["hidden_size"]
    assert ref["joint_network_conf"]["joint_space_size"] == t["joint_space_size"] and ref["vocab_size"] == t["vocab"]


def test_strict_load_with_the_auxiliary_heads():
    """ctc_lin.* / lm_lin.* exist exactly when their loss weights are positive, and are held unused"""
    ref = json.load(open(os.path.join(GOLDEN, "transducer_state_dict.json")))
    V, D, H = ref["vocab_size"], ref["encoder_conf"]["output_size"], ref["decoder_conf"]["hidden_size"]
    aux = {"ctc_lin.weight": [V, D], "ctc_lin.bias": [V], "lm_lin.weight": [V, H], "lm_lin.bias": [V]}
    m = _template_model(ref, auxiliary_ctc_weight=0.3, auxiliary_lm_loss_weight=0.2)
    shapes = dict(ref["shapes"], **aux)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == shapes
    m.load_state_dict({k: torch.randn(shp) for k, shp in shapes.items()}, strict=True)
    only_ctc = _template_model(ref, auxiliary_ctc_weight=0.3)
    assert set(only_ctc.state_dict()) == set(ref["shapes"]) | {"ctc_lin.weight", "ctc_lin.bias"}
    with pytest.raises(RuntimeError, match="ctc_lin"):
        _template_model(ref).load_state_dict({k: torch.randn(shp) for k, shp in shapes.items()}, strict=True)
    assert all(k.startswith(m._skip_keys) for k in aux)                                               # never sent to the handle


@pytest.mark.parametrize("where,conf,word", [
    ("decoder", {"rnn_type": "gru"}, "rnn_type: gru"),
    ("decoder", {"embed_size": 50}, "embed_size: 50"),
    ("decoder", {"hidden_size": 1028}, "hidden_size: 1028"),
    ("decoder", {"num_layers": 5}, "num_layers: 5"),
    ("joint_network", {"joint_activation_type": "relu"}, "joint_activation_type: relu"),
    ("joint_network", {"joint_space_size": 2048}, "joint_space_size: 2048"),
    ("model", {"encoder": "ChunkConformerEncoder"}, "encoder: ChunkConformerEncoder"),
    ("model", {"encoder": "RWKVEncoder"}, "encoder: RWKVEncoder"),
    ("model", {"encoder": "SANMEncoder"}, "encoder: SANMEncoder"),
    ("model", {"blank_id": 3}, "blank_id: 3"),
    ("model", {"decoder": "TransformerDecoder"}, "decoder: TransformerDecoder"),
])
def test_unsupported_options_raise_and_name_the_option(where, conf, word):
    from funasr_amd.transducer import Transducer

    c = synth.transducer_conf()
    if where == "model":
        c.update(conf)
    else:
        c[where + "_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        Transducer(**c)


def test_both_encoders_build_and_use_embed_mask_is_accepted_and_ignored():
    from funasr_amd.conformer import ConformerEncoder
    from funasr_amd.transducer import Transducer
    from funasr_amd.transformer import TransformerEncoder

    assert isinstance(Transducer(**synth.transducer_conf()).encoder, ConformerEncoder)
    assert isinstance(Transducer(**synth.transducer_conf(encoder="TransformerEncoder")).encoder, TransformerEncoder)
    c = synth.transducer_conf()
    c["decoder_conf"]["use_embed_mask"] = True                        # a training-time augmentation
    m = Transducer(**c)
    assert set(m.state_dict()) == set(Transducer(**synth.transducer_conf()).state_dict())
    with pytest.raises(ValueError, match="rnn_type=rnn"):             # the reference's own message for an unknown type
        c["decoder_conf"]["rnn_type"] = "rnn"
        Transducer(**c)


def test_inference_refusals_need_no_device(tmp_path):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.transducer import Transducer

    m = Transducer(**synth.transducer_conf())
    with pytest.raises(NotImplementedError) as e:
        m.inference(torch.zeros(2, 50, 80), batch_size=2)
    assert str(e.value) == "batch decoding is not implemented"        # the reference's message
    with pytest.raises(NotImplementedError, match="beam_size: 17"):
        m.inference(torch.zeros(1, 50, 80), beam_size=17)
    with pytest.raises(NotImplementedError, match="beam_size: 17"):
        m.search(torch.zeros(5, 128), beam_size=17)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.search(torch.zeros(5, 128), beam_size=2)
    with open(str(tmp_path / "config.yaml"), "w") as f:               # a model directory whose config names the sibling model
        f.write("model: BAT\nmodel_conf: {}\n")
    with pytest.raises(NotImplementedError, match="model: BAT"):
        AutoModel(model=str(tmp_path), device="cpu", disable_update=True)


# ------------------------------------------------------------------------------------------------ the oracle against the goldens
def _prefix_chain(sd, prefix):
    state = O.init_state(sd)
    for lab in prefix:
        d, state = O.pred_step(sd, lab, state)
    return d, state


@pytest.mark.parametrize("dt,factor", [(torch.float64, 1e-3), (torch.float32, 4.0)])
def test_oracle_reproduces_the_recorded_quantities(dt, factor):
    """the float64 restatement IS the reference's float64 run (1e-3 of a gap); the float32 one is within 4 x gap"""
    g = load_golden()
    _, sd, _ = golden_model(g)
    s = O.cast(sd, dt)
    prefixes = [[int(v) for v in p.split(",")] for p in g["prefixes"].tolist()]
    outs = []
    for j, pre in enumerate(prefixes):
        d, (h, c) = _prefix_chain(s, pre)
        outs.append(d)
        for name, got in (("dec_out", d), ("dec_h", h), ("dec_c", c)):
            err = float(np.abs(got.double().numpy() - g[f"{name}_{j}"]).max())
            assert err <= factor * max(float(g[f"gap_{name}_{j}"]), 1e-9), (name, j, err)
    enc = torch.from_numpy(g["enc_1"]).to(dt)
    ep = O.enc_proj(s, enc)
    for n, (t, j) in enumerate(g["pairs"].tolist()):
        lp = O.joint_logp(s, ep[t], O.dec_proj(s, outs[j]))
        err = float(np.abs(lp.double().numpy() - g[f"logp_{n}"]).max())
        print(f"logp {n} ({dt}): max |d| {err:.3e}, gap {float(g[f'gap_logp_{n}']):.3e}")
        assert err <= factor * float(g[f"gap_logp_{n}"]), (n, err)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("name,clip,frames,beam", golden_searches())
def test_oracle_search_reproduces_the_recorded_searches(dt, name, clip, frames, beam):
    g = load_golden()
    _, sd, _ = golden_model(g)
    enc = torch.from_numpy(g[f"enc_{clip}"]).to(dt)[:frames]
    res = O.search(O.cast(sd, dt), enc, beam, nbest=beam)
    n = int(g[f"search_{name}_n"])
    assert res["ids"] == [g[f"search_{name}_ids_{r}"].tolist() for r in range(n)]
    for c in ("joint_evals", "pred_steps", "max_frame_evals"):
        assert res[c] == int(g[f"search_{name}_{c}"]), c
    d = float(np.abs(np.asarray(res["scores"]) - g[f"search_{name}_scores"]).max())
    assert d <= 8 * float(g["gap_score"]), (name, d)


def test_the_goldens_meet_their_conditions():
    """what tools/make_golden_transducer.py enforces, read back from the file"""
    g = load_golden()
    assert float(g["min_margin"]) >= 1000 * float(g["gap_logp"]) > 0
    for name, clip, frames, beam in golden_searches():
        assert int(g[f"search_{name}_max_frame_evals"]) <= 64 * beam // 4
        if frames is None:
            n_tok = int((g[f"search_{name}_ids_0"] != 0).sum())
            assert 3 <= n_tok < g[f"enc_{clip}"].shape[0], (name, n_tok)
            assert int(g[f"search_{name}_n"]) == beam
