"""ChunkConformerEncoder without a device: registry, the reference's state-dict names and shapes, refusals by name, the length rule and the chunk-window rule against what the reference itself gave (tests/golden/chunk_conformer.npz, written by
tools/make_golden_chunk_conformer.py), and the float64 oracle of tests/_chunk_conformer_oracle.py against every recorded stage.

The oracle's bar is the project's fp32 rule: 4 x the reference's own fp32 - fp64 gap of the quantity."""
import json
import math
import os

import numpy as np
import pytest
import torch

from funasr_amd import synth
from funasr_amd.register import tables

from . import _chunk_conformer_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZE_A = dict(output_size=64, attention_heads=1)
SIZE_B = dict(output_size=128, attention_heads=2)
MODES = ("full", "dynamic", "unified")
STAGES = ("front", "block_0", "block_1", "norm_blocks", "out")


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "chunk_conformer.npz"), allow_pickle=False))


def encoder_of(g, size, mode, **more):
    """(this package's encoder, its synthetic state dict, its conf) as tools/make_golden_chunk_conformer.py drew the reference's"""
    from funasr_amd.chunk_conformer import ChunkConformerEncoder

    conf = synth.chunk_conformer_conf(mode=mode, **size, **more)
    enc = ChunkConformerEncoder(input_size=80, **conf)
    sd = synth.conformer_state_dict(int(g["seed"]), enc)
    enc.load_state_dict(sd, strict=True)
    return enc, sd, conf


def dense_attention(qkv, P, u, v, vis, H):
    """the oracle's attention over all pairs at once, in the dtype and on the device of its inputs: qkv [B, T, 3 D], P [2 T - 1, D],
    vis [B, T, T] bool. Inputs must be finite everywhere (the caller hands the kernel a poisoned copy)."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    d = D // H
    q, k, val = (qkv[..., j * D:(j + 1) * D].reshape(B, T, H, d) for j in range(3))
    idx = (T - 1 - torch.arange(T, device=qkv.device)[:, None] + torch.arange(T, device=qkv.device)[None, :])
    ac = torch.einsum("bihd,bjhd->bhij", q + u, k)
    bd = torch.einsum("bihd,ijhd->bhij", q + v, P.reshape(-1, H, d)[idx])
    s = ((ac + bd) / math.sqrt(d)).masked_fill(~vis[:, None], float("-inf"))
    p = torch.softmax(s, dim=-1).masked_fill(~vis[:, None], 0.0)
    return torch.einsum("bhij,bjhd->bihd", p, val).reshape(B, T, D)


def golden_model(g, mode):
    """the Transducer over the tiny encoder in `mode`, with the weights tools/make_golden_chunk_conformer.py drew for the reference's"""
    from funasr_amd.transducer import Transducer

    conf = synth.transducer_conf(encoder="ChunkConformerEncoder", vocab=len(g["tokens"]), linear_units=128, **SIZE_A)
    conf["encoder_conf"] = synth.chunk_conformer_conf(mode=mode, **SIZE_A)
    model = Transducer(**conf)
    sd = synth.transducer_state_dict(int(g["seed"]), model, n_planted=int(g["n_planted"]), threshold=float(g["threshold"]))
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def golden_searches():
    """(name, mode, clip, beam) of every recorded search"""
    out = []
    for name in load_golden()["search_names"].tolist():
        mode, clip, beam = name.split("_")
        out.append((name, mode, int(clip[1:]), int(beam[1:])))
    return out


def stage_names(mode):
    return [s for s in STAGES if not (mode == "unified" and s == "front")]


def oracle_stages(res):
    out = {"front": res["front"], "norm_blocks": res["norm_blocks"], "out": res["out"]}
    out.update({f"block_{j}": b for j, b in enumerate(res["blocks"])})
    return out


def mode_chunk(conf):
    """(chunk size of the front, chunk mask on?) of `forward` in the conf's mode; unified: the utt branch"""
    if conf["unified_model_training"]:
        return conf["default_chunk_size"], False
    if conf["dynamic_chunk_training"]:
        return conf["default_chunk_size"], True
    return 0, False


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _report(tag, d, bar):
    print(f"{tag}: max |d| {d:.3e}, bar {bar:.3e}, ratio {d / max(bar, 1e-300):.3f}")
    assert d <= bar, (tag, d, bar)


# ------------------------------------------------------------------------------------------------ registry, state dict
def test_registry_keys():
    from funasr_amd.chunk_conformer import ChunkConformerEncoder
    from funasr_amd.install import hip_classes

    assert tables.encoder_classes["ChunkConformerEncoder"] is ChunkConformerEncoder
    assert ("encoder_classes", "ChunkConformerEncoder", ChunkConformerEncoder) in hip_classes()


def test_transducer_builds_with_the_references_state_dict_and_loads_strictly():
    from funasr_amd.chunk_conformer import ChunkConformerEncoder
    from funasr_amd.transducer import Transducer

    ref = json.load(open(os.path.join(GOLDEN, "chunk_conformer_state_dict.json")))
    conf = ref["conf"]
    assert conf["encoder"] == "ChunkConformerEncoder" and conf["encoder_conf"]["output_size"] == 512 and conf["encoder_conf"]["num_blocks"] == 12
    assert conf["encoder_conf"]["attention_heads"] == 8 and conf["encoder_conf"]["linear_units"] == 2048 and conf["vocab_size"] == 4234
    m = Transducer(**conf)
    assert isinstance(m.encoder, ChunkConformerEncoder) and m.encoder.precision == "fp32"
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref["shapes"]
    assert any(k.endswith("conv_mod.norm.running_var") for k in ref["shapes"])
    m.load_state_dict({k: torch.zeros(shp, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32)
                       for k, shp in ref["shapes"].items()}, strict=True)
    small = Transducer(**synth.transducer_conf(encoder="ChunkConformerEncoder"))
    assert small.set_precision(None).encoder.precision == "fp32"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        small.encoder(torch.zeros(1, 20, 80), [20])


@pytest.mark.parametrize("factor,k2", [(2, 3), (4, 3), (6, 5)])
def test_second_conv_and_output_linear_follow_the_subsampling_factor(factor, k2):
    from funasr_amd.chunk_conformer import ChunkConformerEncoder

    sd = ChunkConformerEncoder(input_size=80, **synth.chunk_conformer_conf(subsampling_factor=factor)).state_dict()
    f2 = {2: 37, 4: 19, 6: 12}[factor]                               # sub_factor_to_params at 80 features
    assert tuple(sd["embed.conv.2.weight"].shape) == (64, 64, k2, k2) and tuple(sd["embed.output.weight"].shape) == (64, 64 * f2)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("conf,word", [
    ({"embed_vgg_like": True}, "embed_vgg_like: true"),
    ({"simplified_att_score": True}, "simplified_att_score: true"),
    ({"subsampling_factor": 1}, "subsampling_factor: 1"),
    ({"subsampling_factor": 8}, "subsampling_factor: 8"),
    ({"attention_heads": 3}, "attention_heads: 3"),
    ({"cnn_module_kernel": 14}, "cnn_module_kernel: 14"),
    ({"cnn_module_kernel": 33}, "cnn_module_kernel: 33"),
    ({"linear_units": 100}, "linear_units: 100"),
    ({"activation_type": "relu"}, "activation_type: relu"),
    ({"positionwise_layer_type": "conv1d"}, "positionwise_layer_type: conv1d"),
    ({"normalize_before": False}, "normalize_before: false"),
    ({"concat_after": True}, "concat_after: true"),
    ({"zero_triu": True}, "zero_triu: true"),
    ({"use_cnn_module": False}, "use_cnn_module: false"),
    ({"pos_enc_layer_type": "abs_pos"}, "pos_enc_layer_type: abs_pos"),
    ({"selfattention_layer_type": "selfattn"}, "selfattention_layer_type: selfattn"),
    ({"time_reduction_factor": 0}, "time_reduction_factor: 0"),
    ({"default_chunk_size": 0}, "default_chunk_size: 0"),
    ({"precision": "f16x2"}, "precision: f16x2"),
])
def test_unsupported_options_raise_and_name_the_option(conf, word):
    from funasr_amd.chunk_conformer import ChunkConformerEncoder
    from funasr_amd.transducer import Transducer

    with pytest.raises(NotImplementedError, match=word):
        ChunkConformerEncoder(input_size=80, **dict(synth.chunk_conformer_conf(), **conf))
    c = synth.transducer_conf(encoder="ChunkConformerEncoder")
    c["encoder_conf"].update(conf)
    with pytest.raises(NotImplementedError, match=word):
        Transducer(**c)


def test_foreign_keys_are_refused_by_name():
    from funasr_amd.chunk_conformer import ChunkConformerEncoder, foreign_keys
    from funasr_amd.transducer import Transducer

    conf = dict(synth.chunk_conformer_conf(), input_layer="conv2d", padding_idx=-1)
    assert foreign_keys(conf) == ["input_layer", "padding_idx"] and foreign_keys(synth.chunk_conformer_conf()) == []
    with pytest.raises(NotImplementedError, match=r"encoder: ChunkConformerEncoder.*input_layer.*padding_idx"):
        ChunkConformerEncoder(input_size=80, **conf)
    c = synth.transducer_conf(encoder="ChunkConformerEncoder")
    c["encoder_conf"]["input_layer"] = "conv2d"
    with pytest.raises(NotImplementedError, match=r"encoder: ChunkConformerEncoder.*input_layer"):
        Transducer(**c)


# ------------------------------------------------------------------------------------------------ lengths, windows
def test_lengths_are_the_references_and_it_never_reports_a_too_short_clip(golden):
    """the reference hands its integer factor to subsampling.check_short_utt, an isinstance test of modules: nothing is ever too short,
    and the time-padded convs turn one frame into one frame. The recorded table says so, and so does the length rule here."""
    from funasr_amd.chunk_conformer import subsampled_length

    for factor in (2, 4, 6):
        assert not golden[f"short_f{factor}"].any()
        for r in (1, 2, 3):
            want = golden[f"olens_f{factor}_r{r}"].tolist()
            assert [subsampled_length(T, factor, r) for T in range(1, 49)] == want, (factor, r)
            assert [(O.front_length(T, factor) - 1) // r + 1 for T in range(1, 49)] == want


def test_window_rule_equals_the_recorded_chunk_masks(golden):
    from funasr_amd.chunk_conformer import chunk_window

    n_masks = 0
    for c in (1, 3, 4, 16):
        for left in (-1, 0, 1, 2):
            for n in (1, 5, 13, 20):
                want = golden[f"mask_c{c}_l{left}_n{n}"]
                for rule in (chunk_window, O.window):
                    got = np.zeros((n, n), bool)
                    for i in range(n):
                        s, e = rule(i, n, c, left)
                        got[i, s:e] = True
                    assert np.array_equal(got, want), (c, left, n)
                assert np.array_equal(O.visible(n, n, c, left).numpy(), want)
                n_masks += 1
    assert n_masks == 64
    assert chunk_window(7, 20, 0, 1) == (0, 20)                       # no chunk size: every key
    assert not golden["mask_c4_l0_n20"][4, 3] and golden["mask_c4_l0_n20"][4, 7]   # left 0: the own chunk only, whatever the docstring says


# ------------------------------------------------------------------------------------------------ the oracle against the goldens
@pytest.mark.parametrize("mode", MODES)
def test_oracle_reproduces_every_recorded_stage(golden, mode):
    g = golden
    _, sd, conf = encoder_of(g, SIZE_A, mode)
    s = O.cast(sd, torch.float64)
    chunk, masked = mode_chunk(conf)
    for i, n in enumerate(g["lens"].tolist()):
        res = oracle_stages(O.encoder(s, torch.from_numpy(g[f"feats_{i}"]).double()[None], [n], conf, chunk, masked))
        for name in stage_names(mode):
            want = g[f"{mode}_{i}_{name}"]
            assert tuple(res[name][0].shape) == want.shape, (mode, i, name)
            _report(f"oracle {mode} clip {i} {name}", float(np.abs(res[name][0].numpy() - want).max()), 4 * float(g[f"gap_{mode}_{i}_{name}"]))


def test_oracle_reproduces_the_fronts_simu_left_and_batch_records(golden):
    g = golden
    f3 = torch.from_numpy(g["feats_3"]).double()[None]
    for factor in (2, 6):
        _, sd, conf = encoder_of(g, SIZE_B, "dynamic", subsampling_factor=factor)
        s = O.cast(sd, torch.float64)
        for name, chunk in (("whole", 0), ("chunk", 4)):
            k = f"front_f{factor}_{name}"
            _report(f"oracle {k}", float(np.abs(O.front(s, f3, factor, chunk)[0].numpy() - g[k]).max()), 4 * float(g["gap_" + k]))
    _, sd, conf = encoder_of(g, SIZE_B, "dynamic")
    res = O.encoder(O.cast(sd, torch.float64), f3, [f3.shape[1]], conf, 3, True)
    _report("oracle simu_chunk_forward", float(np.abs(res["out"][0].numpy() - g["simu_out"]).max()), 4 * float(g["gap_simu_out"]))
    for name, left in (("left0", 0), ("leftall", -1)):
        _, sd, conf = encoder_of(g, SIZE_B, "dynamic", left_chunk_size=left)
        res = O.encoder(O.cast(sd, torch.float64), f3, [f3.shape[1]], conf, 4, True)
        _report(f"oracle {name}", float(np.abs(res["out"][0].numpy() - g[name + "_out"]).max()), 4 * float(g[f"gap_{name}_out"]))
    lens = [int(g["lens"][4]), int(g["lens"][2])]
    xb = torch.zeros(2, lens[0], 80, dtype=torch.float64)
    xb[0], xb[1, : lens[1]] = torch.from_numpy(g["feats_4"]).double(), torch.from_numpy(g["feats_2"]).double()
    for mode in MODES:
        _, sd, conf = encoder_of(g, SIZE_B, mode)
        chunk, masked = mode_chunk(conf)
        res = O.encoder(O.cast(sd, torch.float64), xb, lens, conf, chunk, masked)
        assert res["olens"] == g[f"batch_{mode}_olens"].tolist()
        _report(f"oracle batch {mode}", float(np.abs(res["out"].numpy() - g[f"batch_{mode}_x"]).max()), 4 * float(g[f"gap_batch_{mode}_x"]))


def test_dense_oracle_is_the_row_by_row_oracle():
    """the vectorised attention the GPU tests use as their oracle against tests/_chunk_conformer_oracle.window_attention, which touches
    visible pairs only"""
    g = torch.Generator().manual_seed(5)
    B, T, H = 2, 23, 2
    qkv, P = torch.randn(B, T, 384, generator=g, dtype=torch.float64), torch.randn(2 * T - 1, 128, generator=g, dtype=torch.float64)
    u, v = torch.randn(H, 64, generator=g, dtype=torch.float64), torch.randn(H, 64, generator=g, dtype=torch.float64)
    for c, left in ((0, 0), (4, 1), (5, 0), (3, -1)):
        lens = [T, 9]
        vis = torch.stack([O.visible(T, n, c, left) for n in lens])
        a, b = dense_attention(qkv, P, u, v, vis, H), O.window_attention(qkv, P, u, v, lens, c, left, H)
        assert float((a - b).abs().max()) < 1e-12


def test_recorded_searches_cover_both_modes_and_the_oracle_search_reproduces_them(golden):
    """the float64 search of tests/_transducer_oracle.py from the float64 oracle encoder gives the recorded ids and scores"""
    from . import _transducer_oracle as TO

    g = golden
    names = golden_searches()
    assert {m for _, m, _, _ in names} == {"dynamic", "unified"} and {b for _, _, _, b in names} == {1, 2, 5}
    assert {c for _, _, c, _ in names} >= {3, 4}
    for mode in ("dynamic", "unified"):
        _, sd, conf = golden_model(g, mode)
        sd64 = TO.cast(sd, torch.float64)
        chunk, masked = mode_chunk(conf["encoder_conf"])
        for clip in sorted({c for _, m, c, _ in names if m == mode}):
            x = torch.from_numpy(g[f"feats_{clip}"]).double()[None]
            enc = O.encoder(O.cast(sd, torch.float64), x, [x.shape[1]], conf["encoder_conf"], chunk, masked, prefix="encoder.")["out"][0]
            for name, m, c, beam in names:
                if (m, c) != (mode, clip):
                    continue
                res = TO.search(sd64, enc, beam, nbest=beam)
                n = int(g[f"search_{name}_n"])
                assert res["ids"] == [g[f"search_{name}_ids_{r}"].tolist() for r in range(n)], name
                _report(f"oracle search {name}", float(np.abs(np.asarray(res["scores"]) - g[f"search_{name}_scores"]).max()), 4 * float(g["gap_score"]))
