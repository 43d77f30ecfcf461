"""CAM++ speaker embedding, the CPU side: the float64 oracle against the reference's recorded outputs (and against the reference's
own module where the reference tree is present), the state-dict layout of the HIP module, its refusals, the C ABI without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from funasr_amd import _lib, synth
from funasr_amd.campplus import CAMPPlus
from funasr_amd.register import tables

from . import _campplus_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "campplus.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_state_dict_is_the_reference_layout():
    sd = synth.campplus_state_dict(1)
    assert len(sd) == 937
    m = CAMPPlus()
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd, strict=True)
    for k in ("head.layer1.0.shortcut.0.weight", "head.layer2.0.shortcut.1.running_var", "xvector.tdnn.linear.weight",
              "xvector.block3.tdnnd16.cam_layer.linear2.bias", "xvector.transit3.linear.weight",
              "xvector.dense.nonlinear.batchnorm.running_mean", "xvector.block1.tdnnd1.nonlinear1.batchnorm.num_batches_tracked"):
        assert k in sd
    assert "xvector.dense.nonlinear.batchnorm.weight" not in sd          # affine-free BatchNorm
    assert "head.layer1.1.shortcut.0.weight" not in sd                    # identity shortcut
    assert tuple(sd["xvector.block2.tdnnd24.linear1.weight"].shape) == (128, 256 + 23 * 32, 1)
    assert tables.model_classes["CAMPPlus"] is CAMPPlus


def test_unbuilt_options_are_refused():
    with pytest.raises(NotImplementedError, match="config_str"):
        CAMPPlus(config_str="batchnorm-prelu")
    with pytest.raises(NotImplementedError, match="frame"):
        CAMPPlus(output_level="frame")


def test_segment_mean_is_avg_pool_ceil_mode():
    h = torch.randn(2, 5, 250, dtype=torch.float64)
    seg = F.avg_pool1d(h, 100, 100, ceil_mode=True)
    ref = seg.unsqueeze(-1).expand(*seg.shape, 100).reshape(2, 5, -1)[..., :250]
    assert torch.allclose(O.seg_mean(h), ref, rtol=0, atol=1e-14)
    assert torch.allclose(O.seg_mean(h)[..., 249], h[..., 200:].mean(-1), rtol=0, atol=1e-14)    # true length of the last one


@pytest.mark.parametrize("case", ["a", "b"])
def test_oracle_equals_reference_golden(golden, case):
    sd = synth.campplus_state_dict(int(golden["seed"]))
    out = O.forward(torch.from_numpy(golden[f"x_{case}"]), sd).numpy()
    ref = golden[f"ref64_{case}"]
    assert np.abs(out - ref).max() <= 1e-9 * np.abs(ref).max()


def test_oracle_against_reference_module():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    ref_import.install()
    from funasr.models.campplus.model import CAMPPlus as Ref
    sd = synth.campplus_state_dict(9)
    m = Ref()
    m.load_state_dict(sd, strict=True)
    m.eval()
    g = torch.Generator().manual_seed(2)
    for T in (5, 148, 233):
        x = torch.randn(2, T, 80, generator=g, dtype=torch.float64)
        with torch.no_grad():
            r = m.double()(x)
        assert (r - O.forward(x, sd)).abs().max().item() <= 1e-9 * r.abs().max().item()


def test_create_without_gpu_fails_cleanly():
    lib = _lib.load()
    if lib.pf_device_count() != 0:
        pytest.skip("a GPU is visible")
    cfg = _lib.pf_campplus_config(80, 192, 32, 4, 128, 32, 1e-5)
    assert not lib.pf_campplus_create(ctypes.byref(cfg))
    assert "no HIP device" in _lib.last_error()


def test_module_refuses_cpu_tensors():
    m = CAMPPlus()
    with pytest.raises(RuntimeError, match="AMD GPU"):
        m(torch.zeros(1, 148, 80))
