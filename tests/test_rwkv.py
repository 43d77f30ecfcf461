"""RWKV encoder without a GPU: the registry, the reference's state-dict names and shapes, the length rule, the refusals, and the torch
restatement (tests/_rwkv_oracle.py) against the reference's recorded stages and searches (tests/golden/rwkv.npz, written by
tools/make_golden_rwkv.py).

Bars: the float64 restatement is the reference's float64 run to 1e-9; the float32 one within 4 x the reference's own fp32 - fp64 gap;
search ids exact, scores within 4 x gap_score."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from funasr_amd import synth
from funasr_amd.register import tables

from . import _rwkv_oracle as O
from . import _transducer_oracle as TO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = dict(encoder="RWKVEncoder", output_size=64, linear_units=160, enc_blocks=3)
P = "encoder."


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "rwkv.npz"), allow_pickle=False))


def golden_model(g):
    from funasr_amd.transducer import Transducer

    conf = synth.transducer_conf(vocab=len(g["tokens"]), **TINY)
    model = Transducer(**conf)
    sd = synth.transducer_state_dict(int(g["seed"]), model, n_planted=int(g["n_planted"]), threshold=float(g["threshold"]))
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def golden_searches():
    """(name, clip, beam) of every recorded search"""
    return [(f"c{i}_b{b}", i, b) for i in (2, 3, 4) for b in (1, 2, 5)]


@pytest.fixture(scope="module")
def golden():
    g = load_golden()
    model, sd, conf = golden_model(g)
    return g, model, sd, conf


@pytest.fixture(scope="module")
def oracle64(golden):
    """the float64 restatement of every golden clip, computed once"""
    g, _, sd, conf = golden
    s = O.cast(sd, torch.float64)
    r = conf["encoder_conf"]["time_reduction_factor"]
    return [O.encode(torch.from_numpy(g[f"feats_{i}"]).double(), s, r, P) for i in range(len(g["lens"]))]


def stages_of(res):
    out = {"front": res["front"], "embed_norm": res["embed_norm"], "enc": res["out"]}
    out.update({f"block_{j}": b for j, b in enumerate(res["blocks"])})
    return out


def recorded(g, i, name):
    return g[f"block_{i}_{name[6:]}"] if name.startswith("block_") else g[f"{name}_{i}"]


def recorded_gap(g, i, name):
    return float(g[f"gap_block_{i}_{name[6:]}"] if name.startswith("block_") else g[f"gap_{name}_{i}"])


# ------------------------------------------------------------------------------------------------ registry, state dict, lengths
def test_registry_keys():
    from funasr_amd.install import hip_classes
    from funasr_amd.rwkv_encoder import RWKVEncoder

    assert tables.encoder_classes["RWKVEncoder"] is RWKVEncoder
    assert ("encoder_classes", "RWKVEncoder", RWKVEncoder) in hip_classes()


def test_state_dict_names_and_shapes_are_the_references():
    from funasr_amd.transducer import Transducer

    ref = json.load(open(os.path.join(GOLDEN, "rwkv_state_dict.json")))
    assert ref["encoder"] == "RWKVEncoder" and ref["encoder_conf"]["output_size"] == 512 and ref["encoder_conf"]["num_blocks"] == 18
    m = Transducer(encoder=ref["encoder"], encoder_conf=ref["encoder_conf"], decoder="rnnt_decoder", decoder_conf=ref["decoder_conf"],
                   joint_network="joint_network", joint_network_conf=ref["joint_network_conf"], vocab_size=ref["vocab_size"], input_size=80,
                   **ref["model_conf"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert ref["shapes"]["encoder.rwkv_blocks.0.att.time_mix_key"] == [1, 1, 512] and ref["shapes"]["encoder.rwkv_blocks.17.att.time_decay"] == [512]
    assert ref["shapes"]["encoder.rwkv_blocks.0.ffn.proj_key.weight"] == [2048, 512]          # linear_size defaults to 4 D
    t = synth.RWKV_TEMPLATE
    assert all(ref["encoder_conf"][k] == v for k, v in t.items())
    m.load_state_dict({k: torch.zeros(shp) for k, shp in ref["shapes"].items()}, strict=True)
    assert m.encoder.precision == "fp32" and m.set_precision(None).encoder.precision == "fp32"


def test_length_rule_is_the_references():
    from funasr_amd.rwkv_encoder import subsampled_length

    g = load_golden()
    for r in (1, 2, 3):
        want = g[f"olens_r{r}"].tolist()
        assert [subsampled_length(T, r) for T in range(1, 41)] == want
        assert [O.olens(T, r) for T in range(1, 41)] == want
    for i, n in enumerate(g["lens"].tolist()):
        assert g[f"enc_{i}"].shape[0] == subsampled_length(n, 2)


def test_embed_output_permutation_against_conv2d_and_view():
    """the reference flattens the conv output [b, c, t, f] with transpose(1, 2).view(b, t, c f); the HIP convs are channels-last
    [t, f, c]: the permuted weight on the channels-last rows is the reference's linear"""
    from funasr_amd.rwkv_encoder import channels_last_output_weight

    g = torch.Generator().manual_seed(3)
    C, T, F2, D = 8, 5, 3, 8
    x = torch.relu(F.conv2d(torch.randn(1, 4, T, F2, generator=g, dtype=torch.float64), torch.randn(C, 4, 3, 3, generator=g, dtype=torch.float64),
                            padding=1))
    W, b = torch.randn(D, C * F2, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    want = F.linear(x.transpose(1, 2).contiguous().view(1, T, C * F2), W, b)[0]
    got = F.linear(x[0].permute(1, 2, 0).reshape(T, F2 * C), channels_last_output_weight(W, C), b)
    assert float((got - want).abs().max()) < 1e-12
    assert not torch.equal(channels_last_output_weight(W, C), W)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("conf,word", [
    ({"subsampling_factor": 6}, "subsampling_factor: 6"),
    ({"subsampling_factor": 1}, "subsampling_factor: 1"),
    ({"kernel": 5}, "kernel: 5"),
    ({"attention_size": 32}, "attention_size: 32"),
    ({"output_size": 48}, "output_size: 48"),
    ({"output_size": 1056}, "output_size: 1056"),
    ({"linear_size": 100}, "linear_size: 100"),
    ({"linear_size": 4128}, "linear_size: 4128"),
    ({"num_blocks": 0}, "num_blocks: 0"),
    ({"time_reduction_factor": 0}, "time_reduction_factor: 0"),
    ({"precision": "f16x2"}, "precision: f16x2"),
    ({"precision": "bf16"}, "precision: bf16"),
])
def test_unsupported_options_raise_and_name_the_option(conf, word):
    from funasr_amd.rwkv_encoder import RWKVEncoder
    from funasr_amd.transducer import Transducer

    with pytest.raises(NotImplementedError, match=word):
        RWKVEncoder(input_size=80, **dict(synth.rwkv_encoder_conf(), **conf))
    c = synth.transducer_conf(**TINY)
    c["encoder_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        Transducer(**c)


@pytest.mark.parametrize("input_size", [4, 6, 82, 260])
def test_input_size_off_the_range_is_refused(input_size):
    from funasr_amd.rwkv_encoder import RWKVEncoder

    with pytest.raises(NotImplementedError, match=f"input_size: {input_size}"):
        RWKVEncoder(input_size=input_size, **synth.rwkv_encoder_conf())


def test_foreign_encoder_conf_keys_are_refused_by_name():
    """the reference swallows them in **kwargs and builds the default geometry; here the model names them"""
    from funasr_amd.rwkv_encoder import RWKVEncoder
    from funasr_amd.transducer import Transducer

    c = synth.transducer_conf(**TINY)
    c["encoder_conf"].update({"attention_heads": 4, "input_layer": "conv2d"})
    with pytest.raises(NotImplementedError, match=r"encoder: RWKVEncoder does not take encoder_conf keys \['attention_heads', 'input_layer'\]"):
        Transducer(**c)
    with pytest.raises(NotImplementedError, match="attention_heads"):
        RWKVEncoder(input_size=80, attention_heads=4)
    m = Transducer(**synth.transducer_conf(**TINY))                              # every key of the reference constructor is taken
    assert m.encoder.output_size() == 64 and m.encoder.time_reduction_factor == 2
    with pytest.raises(NotImplementedError, match="precision: f16x2"):
        Transducer(precision="f16x2", **synth.transducer_conf(**TINY))
    assert Transducer(precision="fp32", **synth.transducer_conf(**TINY)).encoder.precision == "fp32"


def test_attention_size_equal_to_output_size_and_dropouts_are_accepted():
    from funasr_amd.rwkv_encoder import RWKVEncoder

    e = RWKVEncoder(input_size=80, output_size=64, attention_size=64, linear_size=None, att_dropout_rate=0.3, ffn_dropout_rate=0.2,
                    dropout_rate=0.1)
    assert e.linear_size == 256 and e.context_size == 1024


def test_context_size_is_honoured_as_the_reference_does():
    from funasr_amd.rwkv_encoder import RWKVEncoder

    e = RWKVEncoder(input_size=80, **synth.rwkv_encoder_conf(context_size=2))
    with pytest.raises(ValueError) as err:
        e(torch.zeros(1, 9, 80), [9])
    assert str(err.value) == "Context size is too short for current length: 9 versus 8"
    with pytest.raises(RuntimeError, match="AMD GPU"):                            # 8 frames pass the check and reach the handle
        e(torch.zeros(1, 8, 80), [8])


def test_transducer_conf_keeps_its_output_for_the_two_other_encoders():
    kw = dict(output_size=128, attention_heads=2, linear_units=256, enc_blocks=2)
    assert synth.transducer_conf()["encoder_conf"] == synth.conformer_conf(**kw)["encoder_conf"]
    assert synth.transducer_conf(encoder="TransformerEncoder")["encoder_conf"] == synth.transformer_conf(**kw)["encoder_conf"]
    c = synth.transducer_conf(**TINY)
    assert c["encoder"] == "RWKVEncoder" and set(c["encoder_conf"]) <= set(__import__("funasr_amd.rwkv_encoder", fromlist=["x"]).CONF_KEYS)


def test_synthetic_weights_cover_the_issue_ranges(golden):
    _, _, sd, _ = golden
    td = torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith("time_decay")])
    assert -5 <= float(td.min()) < -4 and 2 < float(td.max()) <= 3
    mixes = torch.cat([v.reshape(-1) for k, v in sd.items() if "time_mix_" in k])
    assert 0 <= float(mixes.min()) and float(mixes.max()) <= 1


# ------------------------------------------------------------------------------------------------ the oracle against the goldens
def test_oracle_float64_is_the_reference_at_every_recorded_stage(golden, oracle64):
    g = golden[0]
    worst = 0.0
    for i, res in enumerate(oracle64):
        for name, got in stages_of(res).items():
            want = recorded(g, i, name)
            assert tuple(got.shape) == want.shape, (i, name)
            worst = max(worst, float(np.abs(got.numpy() - want).max()))
    print(f"oracle float64 against the recorded stages: max |d| {worst:.3e}")
    assert worst <= 1e-9


def test_oracle_float32_is_within_the_reference_gap(golden):
    g, _, sd, conf = golden
    s = O.cast(sd, torch.float32)
    worst = 0.0
    for i in range(len(g["lens"])):
        res = O.encode(torch.from_numpy(g[f"feats_{i}"]), s, conf["encoder_conf"]["time_reduction_factor"], P)
        for name, got in stages_of(res).items():
            d, gap = float(np.abs(got.double().numpy() - recorded(g, i, name)).max()), recorded_gap(g, i, name)
            worst = max(worst, d / max(gap, 1e-30))
            assert d <= 4 * max(gap, 1e-9), (i, name, d, gap)
    print(f"oracle float32 against the recorded stages: largest ratio to the gap {worst:.2f}")


def test_oracle_ragged_batch_is_each_clip_alone(golden, oracle64):
    g, _, sd, conf = golden
    lens = g["lens"].tolist()
    xs = torch.zeros(len(lens), max(lens), 80, dtype=torch.float64)
    for i, n in enumerate(lens):
        xs[i, :n] = torch.from_numpy(g[f"feats_{i}"]).double()
    out, ol = O.encode_batch(xs, lens, O.cast(sd, torch.float64), 2, P)
    assert ol == [r["out"].shape[0] for r in oracle64] and out.shape[1] == O.olens(max(lens), 2)
    for i, r in enumerate(oracle64):
        assert torch.equal(out[i, : ol[i]], r["out"]) and not bool(out[i, ol[i]:].any())


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("name,clip,beam", golden_searches())
def test_oracle_search_reproduces_the_recorded_searches(golden, dt, name, clip, beam):
    """each precision from its OWN encoder output, as recorded"""
    g, _, sd, conf = golden
    s = O.cast(sd, dt)
    enc = O.encode(torch.from_numpy(g[f"feats_{clip}"]).to(dt), s, 2, P)["out"]
    res = TO.search(s, enc, beam, nbest=beam)
    n = int(g[f"search_{name}_n"])
    assert res["ids"] == [g[f"search_{name}_ids_{r}"].tolist() for r in range(n)]
    d = float(np.abs(np.asarray(res["scores"]) - g[f"search_{name}_scores"]).max())
    assert d <= 4 * float(g["gap_score"]), (name, d)
    if dt == torch.float64:
        for c in ("joint_evals", "pred_steps", "max_frame_evals"):
            assert res[c] == int(g[f"search_{name}_{c}"]), c


def test_the_goldens_meet_their_conditions():
    """what tools/make_golden_rwkv.py enforces, read back from the file; and the file stays below the smallest model golden"""
    g = load_golden()
    assert float(g["min_margin"]) >= 1000 * float(g["gap_logp"]) > 0
    for name, clip, beam in golden_searches():
        assert int(g[f"search_{name}_max_frame_evals"]) <= 64 * beam // 4
        n_tok = int((g[f"search_{name}_ids_0"] != 0).sum())
        assert 3 <= n_tok < g[f"enc_{clip}"].shape[0], (name, n_tok)
        assert int(g[f"search_{name}_n"]) == beam
    assert g["lens"].tolist() == [1, 5, 39, 55, 87]
    assert os.path.getsize(os.path.join(GOLDEN, "rwkv.npz")) < os.path.getsize(os.path.join(GOLDEN, "eres2net.npz"))
    assert not any("weight" in k for k in g)                                      # weights are never stored


# ------------------------------------------------------------------------------------------------ the WKV recurrence
def test_frame_zero_nan_is_the_oracles_too():
    """the reference's initial m is -1e-30, not -inf: with u + k0 below about -104 frame 0 is 0 / 0 in float32 and v0 in float64.
    The oracle's restatement reproduces it, it does not repair it (a check of the oracle alone; the kernel's frame 0 is
    tests/test_rwkv_gpu.py::test_wkv_frame_zero_is_the_references_zero_over_zero)"""
    D = 4
    k = torch.tensor([[-200.0] * D, [0.5] * D])
    v = torch.tensor([[1.0, 2.0, -3.0, 0.25]] * 2)
    w, u = -torch.exp(torch.zeros(D)), torch.zeros(D)
    o32 = O.wkv(k, v, w, u)
    assert bool(torch.isnan(o32[0]).all())
    o64 = O.wkv(k.double(), v.double(), w.double(), u.double())
    assert float((o64[0] - v[0].double()).abs().max()) < 1e-14 and bool(torch.isfinite(o64).all())
    assert bool(torch.isnan(O.wkv_chunked(k, v, w, u, 32)[0]).all())


@pytest.mark.parametrize("T,L", [(300, 32), (33, 32), (750, 64), (5, 32), (64, 32), (69, 32)])
def test_chunk_algebra_is_the_sequential_recurrence(T, L):
    """a check of the test-side restatements only (O.wkv against O.wkv_chunked; it runs no kernel and says nothing about
    csrc/rwkv.hip, which tests/test_rwkv_gpu.py holds to O.wkv): the chunk algebra in float64 is the recurrence to rounding; in
    float32 its distance to the float64 recurrence stays within 4 x the sequential float32 recurrence's own (floor: 8 roundings of
    the largest value), |k| up to 80"""
    g = torch.Generator().manual_seed(T + L)
    D = 16
    k = (30 * torch.randn(T, D, generator=g)).clamp(-80, 80)
    v = torch.randn(T, D, generator=g)
    w = -torch.exp(-5 + 8 * torch.rand(D, generator=g))
    u = 0.5 * torch.randn(D, generator=g)
    ref = O.wkv(k.double(), v.double(), w.double(), u.double())
    assert float((O.wkv_chunked(k.double(), v.double(), w.double(), u.double(), L) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    seq = float((O.wkv(k, v, w, u).double() - ref).abs().max())
    chk = float((O.wkv_chunked(k, v, w, u, L).double() - ref).abs().max())
    bar = max(4 * seq, 2.0 ** -21 * float(ref.abs().max()))
    print(f"T {T} L {L}: chunked fp32 {chk:.3e}, sequential fp32 {seq:.3e}, ratio {chk / bar:.2f} of the bar")
    assert chk <= bar
