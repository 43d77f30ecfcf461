"""ERes2NetV2 speaker embedding, the CPU side: registry, the state-dict layout of the HIP module against the reference's recorded
one, both checkpoint layouts, the float64 oracle against the reference's recorded tensors, what the golden itself must satisfy,
the refusals, and AutoModel's resolution of a model directory. Nothing here needs a GPU."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import install, synth
from funasr_amd.auto_model import AutoModel
from funasr_amd.eres2net import ERes2NetV2SV
from funasr_amd.register import tables

from . import _eres2net_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = synth.eres2net_conf()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "eres2net.npz"))


def test_registered_under_both_names_and_installed():
    assert tables.model_classes["ERes2NetV2"] is ERes2NetV2SV
    assert tables.model_classes["iic/speech_eres2netv2_sv_zh-cn_16k-common"] is ERes2NetV2SV
    keys = {(t, k) for t, k, _ in install.hip_classes()}
    assert ("model_classes", "ERes2NetV2") in keys and ("model_classes", "iic/speech_eres2netv2_sv_zh-cn_16k-common") in keys


def test_state_dict_is_the_reference_layout():
    with open(os.path.join(GOLD, "eres2net_state_dict.json")) as f:
        ref = {k: tuple(v) for k, v in json.load(f).items()}
    assert len(ref) == 557
    m = ERes2NetV2SV()                                       # constructed without a GPU
    own = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert own == ref
    sd = synth.eres2net_state_dict(1, m)
    m.load_state_dict(sd, strict=True)
    for k in ("model.conv1.weight", "model.layer1.0.shortcut.0.weight", "model.layer3.0.fuse_models.0.local_att.0.weight",
              "model.layer4.2.bns.1.num_batches_tracked", "model.layer3_ds.weight", "model.fuse34.local_att.4.running_var",
              "model.seg_1.bias"):
        assert k in sd
    assert "model.layer1.1.shortcut.0.weight" not in sd      # identity shortcut
    assert "model.layer2.0.fuse_models.0.local_att.0.weight" not in sd     # layers 1, 2: the plain block
    assert tuple(sd["model.layer3.0.fuse_models.0.local_att.0.weight"].shape) == (26, 208, 1, 1)
    assert tuple(sd["model.seg_1.weight"].shape) == (192, 20480)
    assert sum(v.numel() for v in sd.values()) == 17896745


def test_both_checkpoint_layouts_load_the_same_tensors(tmp_path):
    sd = synth.eres2net_state_dict(2, ERes2NetV2SV(**TINY))
    bare = {k[len("model."):]: v for k, v in sd.items()}
    d1, d2, d3 = (str(tmp_path / n) for n in ("ckpt", "wrapped", "pt"))
    for d in (d1, d2, d3):
        os.makedirs(d)
    torch.save(bare, os.path.join(d1, "pretrained_eres2netv2.ckpt"))
    torch.save({"state_dict": bare}, os.path.join(d2, "pretrained_eres2netv2.ckpt"))
    torch.save(sd, os.path.join(d3, "model.pt"))
    models = [ERes2NetV2SV(model_path=d1, **TINY), ERes2NetV2SV(model_path=d2, **TINY),
              ERes2NetV2SV(init_param=os.path.join(d1, "pretrained_eres2netv2.ckpt"), **TINY),
              ERes2NetV2SV(init_param=os.path.join(d3, "model.pt"), **TINY)]
    for m in models:
        got = m.state_dict()
        assert set(got) == set(sd)
        for k, v in sd.items():
            assert torch.equal(got[k], v), k


def test_oracle_equals_reference_golden(golden):
    sd = synth.eres2net_state_dict(int(golden["seed"]), ERes2NetV2SV(**TINY))
    got = O.stages(torch.from_numpy(golden["x"]), sd)
    for name in O.STAGES:
        if name in ("stats", "emb"):
            out, ref = got[name].numpy(), golden[name]
        else:
            out, ref = got[name][1].numpy(), golden[f"{name}_c1"]
        assert out.shape == ref.shape, name
        assert np.abs(out - ref).max() <= 1e-9 * np.abs(ref).max(), name
    rsd = synth.eres2net_state_dict(int(golden["ragged_seed"]), ERes2NetV2SV(**dict(TINY, feat_dim=80)))
    out, ref = O.forward(torch.from_numpy(golden["ragged_x"]), rsd).numpy(), golden["ragged_emb"]
    assert np.abs(out - ref).max() <= 1e-9 * np.abs(ref).max()


def test_golden_exercises_the_clamp_and_has_embeddings_of_size(golden):
    """a network with a plain ReLU in place of clamp(0, 20) must not pass the parity tests, and the absolute bars must mean
    something: the counts the tool recorded, and the same counts from the oracle"""
    above, inside = golden["clamp_above"], golden["clamp_inside"]
    assert ((above >= 0.01) & (above <= 0.5)).any(), above
    assert (inside >= 0.10).all(), inside
    pre = []
    sd = synth.eres2net_state_dict(int(golden["seed"]), ERes2NetV2SV(**TINY))
    O.stages(torch.from_numpy(golden["x"]), sd, torch.float64, pre)
    assert len(pre) == sum(TINY["num_blocks"]) == len(above)
    assert np.allclose([(p > 20).double().mean().item() for p in pre], above, atol=1e-12)
    assert np.abs(golden["emb"]).max(axis=1).min() >= 0.05
    assert np.abs(golden["ragged_emb"]).max(axis=1).min() >= 0.05
    for name in O.STAGES:
        assert 0 < float(golden[f"gap_{name}"]) < 1e-2, name


@pytest.mark.parametrize("opt, val", [("baseWidth", 32), ("scale", 4), ("expansion", 4), ("pooling_func", "TAP"),
                                      ("pooling_func", "ASTP"), ("two_emb_layer", True), ("feat_dim", 20), ("feat_dim", 136),
                                      ("m_channels", 12), ("m_channels", 72), ("num_blocks", [3, 4, 6]), ("num_blocks", [1, 0, 1, 1]),
                                      ("embedding_size", 0), ("bf16", True), ("fp16", True), ("precision", "bf16")])
def test_unbuilt_options_are_refused_by_name(opt, val):
    with pytest.raises(NotImplementedError, match=opt):
        ERes2NetV2SV(**{opt: val})


def test_feat_dim_20_raises():
    with pytest.raises(NotImplementedError, match="feat_dim=20"):
        ERes2NetV2SV(**dict(TINY, feat_dim=20))


def test_eight_frames_are_refused():
    m = ERes2NetV2SV(**TINY)
    with pytest.raises(ValueError, match="standard deviation.*undefined.*reference returns NaN"):
        m(torch.zeros(1, 8, TINY["feat_dim"]))
    assert ERes2NetV2SV.frames_after_strides(9) == 2 and ERes2NetV2SV.frames_after_strides(8) == 1


def test_module_refuses_cpu_tensors():
    m = ERes2NetV2SV(**TINY)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        m(torch.zeros(1, 37, TINY["feat_dim"]))


def test_auto_model_resolves_a_model_directory(tmp_path):
    d = str(tmp_path / "eres2netv2")
    os.makedirs(d)
    with open(os.path.join(d, "config.yaml"), "w") as f:
        yaml.safe_dump({"model": "ERes2NetV2", "model_conf": dict(TINY)}, f)
    sd = synth.eres2net_state_dict(3, ERes2NetV2SV(**TINY))
    torch.save(sd, os.path.join(d, "model.pt"))
    m, kw = AutoModel.build_model(model=d, device="cuda:0" if torch.cuda.is_available() else "cpu")
    assert isinstance(m, ERes2NetV2SV) and m.m_channels == 16 and m.num_blocks == [1, 1, 2, 1]
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k].cpu(), v), k
    with pytest.raises(NotImplementedError, match="local CAM\\+\\+ model directory"):
        AutoModel(model=d, spk_model="iic/speech_eres2netv2_sv_zh-cn_16k-common", device="cpu")
