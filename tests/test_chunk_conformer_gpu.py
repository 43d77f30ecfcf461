"""ChunkConformerEncoder on the MI355X through the C ABI: the chunk-window attention, the causal convolution-module kernel and the
StreamingConvInput front against the float64 oracle (tests/_chunk_conformer_oracle.py) and the reference's records
(tests/golden/chunk_conformer.npz), the encoder against every recorded stage in its three modes, and the Transducer's encode over it.

Bars are the project's fp32 rules (tests/test_rwkv_gpu.py): 4 x the reference's own fp32 - fp64 gap where one is recorded; for the
random-input kernel tests 4 x max |oracle fp32 - oracle fp64| of the case, never below 2^-21 x the case's largest |oracle value|.
Every test prints its measured ratio."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import _lib, synth

from . import _chunk_conformer_oracle as O
from .test_chunk_conformer import (MODES, SIZE_A, SIZE_B, dense_attention, encoder_of, golden_model, golden_searches, load_golden, mode_chunk,
                                   stage_names)

pytestmark = pytest.mark.gpu
GUARD = 3                                      # NaN rows in front of and behind every buffer
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(tag, d, bar):
    print(f"{tag}: max |d| {d:.3e}, bar {bar:.3e}, ratio {d / max(bar, 1e-300):.3f}")
    assert d <= bar, (tag, d, bar)


def _guarded(rows, ld, cuda):
    buf = torch.full((rows + 2 * GUARD, ld), NAN, device=cuda)
    return buf, buf[GUARD: GUARD + rows]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


@pytest.fixture(scope="module")
def golden():
    return load_golden()


# ------------------------------------------------------------------------------------------------ window attention
def _window_lens(T, c):
    """the whole clip; a length inside a chunk; one that leaves whole windows empty; none"""
    inside = max(T - max(c, 2) // 2 - 1, 0)
    return [T, inside, T // 3, 0]


def _window_case(cuda, T, H, c, left, seed):
    D = 64 * H
    lens = _window_lens(T, c)
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * D, generator=g)
    P = torch.randn(2 * T - 1, D, generator=g)
    u, v = 0.3 * torch.randn(H, 64, generator=g), 0.3 * torch.randn(H, 64, generator=g)
    vis = torch.stack([O.visible(T, n, c, left) for n in lens])
    o64 = dense_attention(qkv.double().to(cuda), P.double().to(cuda), u.double().to(cuda), v.double().to(cuda), vis.to(cuda), H)
    o32 = dense_attention(qkv.to(cuda), P.to(cuda), u.to(cuda), v.to(cuda), vis.to(cuda), H)
    # the kernel's copy: NaN in K / V rows no query sees, in P rows outside the span of visible (query, key) offsets, and around every buffer
    qbuf, qv = _guarded(B * T, 3 * D, cuda)
    qv.copy_(qkv.reshape(B * T, 3 * D))
    seen = vis.any(dim=1)                                            # [B, T]: key j of clip b is in some window
    qv.view(B, T, 3 * D)[:, :, D:][~seen.to(cuda)] = NAN
    pbuf, pv = _guarded(2 * T - 1, D, cuda)
    pv.copy_(P)
    off = (torch.arange(T)[None, :] - torch.arange(T)[:, None])[None].expand(B, T, T)[vis]
    if off.numel():
        pv[: T - 1 + int(off.min())] = NAN
        pv[T + int(off.max()):] = NAN
    else:
        pv[:] = NAN
    obuf, ov = _guarded(B * T, D, cuda)
    kl = torch.tensor(lens, dtype=torch.int32, device=cuda)
    ud, vd = u.to(cuda).contiguous(), v.to(cuda).contiguous()
    lib = _lib.load()
    _lib.check(lib.pf_k_cc_window_attention(qv.data_ptr(), pv.data_ptr(), ud.data_ptr(), vd.data_ptr(), kl.data_ptr(), B, T, H, c, left,
                                            ov.data_ptr(), _stream()), "pf_k_cc_window_attention")
    torch.cuda.synchronize()
    assert _guards_intact(obuf)
    out = ov.view(B, T, D)
    empty = ~vis.any(dim=2).to(cuda)
    assert bool((out[empty] == 0).all()), "rows without a visible key are exactly zero"
    assert bool(torch.isfinite(out).all()), "a NaN row outside every window reached the result"
    gap = float((o32.double() - o64).abs().max())
    bar = max(4 * gap, 2.0 ** -21 * float(o64.abs().max()))
    d = float((out.double() - o64).abs().max())
    if c == 0:                                                       # no chunk mask: the existing "latest" kernel, within the same bar
        ref = torch.empty(B * T, D, device=cuda)
        qd, pd = qkv.to(cuda).reshape(B * T, 3 * D).contiguous(), P.to(cuda).contiguous()      # (kept alive across the launch)
        _lib.check(lib.pf_k_relpos_attention(qd.data_ptr(), pd.data_ptr(), ud.data_ptr(), vd.data_ptr(), kl.data_ptr(), B, T, H, 0,
                                             ref.data_ptr(), _stream()), "pf_k_relpos_attention")
        torch.cuda.synchronize()
        d_ref = float((ref.view(B, T, D).double() - o64).abs().max())
        assert d_ref <= bar, ("the existing latest kernel", T, H, d_ref, bar)
        d = max(d, float((out - ref.view(B, T, D)).abs().max()))
    return d, bar


def _window_lengths(c):
    base = [1, 2, 63, 64, 65, 127, 128, 129, 257]
    return sorted(set(base + [t for t in (c - 1, c, c + 1) if t >= 1]))


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("c", [0, 1, 3, 16, 25])
def test_window_attention_against_the_float64_oracle(cuda, c, H):
    """every tile and window edge: T around 1, the chunk size, 64, 128 and 257 (three workgroups); left -1 / 0 / 1 / 2; ragged key
    lengths including 0, one inside a chunk and one that leaves whole windows empty"""
    worst = (0.0, "")
    for T in _window_lengths(c):
        for left in ((0,) if c == 0 else (-1, 0, 1, 2)):
            d, bar = _window_case(cuda, T, H, c, left, seed=1000 * T + 10 * c + left + 5)
            assert d <= bar, (T, c, left, H, d, bar)
            worst = max(worst, (d / bar, f"T={T} left={left}"))
    print(f"window attention c={c} H={H}: worst ratio {worst[0]:.3f} at {worst[1]}")


# ------------------------------------------------------------------------------------------------ causal convolution module
def _glu_dw(cuda, g, dw, bias, sc, sh, causal, hook="pf_k_cc_glu_dw"):
    B, T, D2 = g.shape
    D = D2 // 2
    gbuf, gv = _guarded(B * T, D2, cuda)
    gv.copy_(g.reshape(B * T, D2))
    obuf, ov = _guarded(B * T, D, cuda)
    t = [x.to(cuda).contiguous() for x in (dw, bias, sc, sh)]
    lib = _lib.load()
    args = [gv.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), B, T, D, dw.shape[1]]
    if hook == "pf_k_cc_glu_dw":
        args.append(int(causal))
    _lib.check(getattr(lib, hook)(*args, ov.data_ptr(), _stream()), hook)
    torch.cuda.synchronize()
    assert _guards_intact(obuf)
    return ov.view(B, T, D).clone()


@pytest.mark.parametrize("taps", [3, 15, 31])
def test_causal_conv_kernel_against_the_float64_oracle(cuda, taps):
    D, B = 128, 2
    for T in (1, taps - 1, taps, taps + 1, 65):
        g = torch.Generator().manual_seed(100 * taps + T)
        x = torch.randn(B, T, 2 * D, generator=g)
        dw, bias = torch.randn(D, taps, generator=g) / taps ** 0.5, 0.1 * torch.randn(D, generator=g)
        sc, sh = 0.5 + torch.rand(D, generator=g), 0.2 * torch.randn(D, generator=g)
        o64 = O.glu_dw(x.double(), dw.double(), bias.double(), sc.double(), sh.double(), True)
        o32 = O.glu_dw(x, dw, bias, sc, sh, True)
        out = _glu_dw(cuda, x, dw, bias, sc, sh, True)
        bar = max(4 * float((o32.double() - o64).abs().max()), 2.0 ** -21 * float(o64.abs().max()))
        _report(f"causal conv taps={taps} T={T}", float((out.double().cpu() - o64).abs().max()), bar)
        # row t must not change when the rows after it do
        t0 = T // 2
        x2 = x.clone()
        x2[:, t0 + 1:] = 7.0 * torch.randn(B, T - t0 - 1, 2 * D, generator=g)
        assert torch.equal(_glu_dw(cuda, x2, dw, bias, sc, sh, True)[:, : t0 + 1], out[:, : t0 + 1]), (taps, T)
        # the symmetric form is the Conformer's kernel, bit for bit
        assert torch.equal(_glu_dw(cuda, x, dw, bias, sc, sh, False), _glu_dw(cuda, x, dw, bias, sc, sh, False, hook="pf_k_conformer_glu_dw"))


def test_strided_row_copy(cuda):
    lib = _lib.load()
    B, Ti, D = 3, 11, 64
    x = torch.randn(B, Ti, D, device=cuda)
    for step in (1, 2, 3, 11):
        To = (Ti - 1) // step + 1
        ybuf, yv = _guarded(B * To, D, cuda)
        _lib.check(lib.pf_k_cc_copy_rows(x.data_ptr(), Ti, step, yv.data_ptr(), B, To, D, _stream()), "pf_k_cc_copy_rows")
        torch.cuda.synchronize()
        assert _guards_intact(ybuf) and torch.equal(yv.view(B, To, D), x[:, ::step])


# ------------------------------------------------------------------------------------------------ front
@pytest.mark.parametrize("factor", [2, 4, 6])
def test_front_against_the_recorded_fronts(golden, cuda, factor):
    """clip 3 has 67 frames: no multiple of chunk x factor at any factor, so the last piece is zero-filled and its rows cut"""
    g = golden
    f3 = torch.from_numpy(g["feats_3"])[None]
    if factor == 4:
        cases = [("full_3_front", SIZE_A, 0), ("dynamic_3_front", SIZE_A, 4)]
    else:
        cases = [(f"front_f{factor}_whole", SIZE_B, 0), (f"front_f{factor}_chunk", SIZE_B, 4)]
    for key, size, chunk in cases:
        enc, _, _ = encoder_of(g, size, "dynamic", subsampling_factor=factor)
        out = enc.to(cuda).front(f3, chunk)
        torch.cuda.synchronize()
        assert tuple(out[0].shape) == g[key].shape
        _report(f"front factor {factor} {key}", float(np.abs(out[0].double().cpu().numpy() - g[key]).max()), 4 * float(g["gap_" + key]))
    # a batch of two clips, chunked, against the float64 oracle: every piece of every clip in one launch
    enc, sd, _ = encoder_of(g, SIZE_B, "dynamic", subsampling_factor=factor)
    x = torch.randn(2, 53, 80, generator=torch.Generator().manual_seed(factor))
    o64, o32 = O.front(O.cast(sd, torch.float64), x.double(), factor, 3), O.front(sd, x, factor, 3)
    out = enc.to(cuda).front(x, 3)
    _report(f"front factor {factor} batch of 2, chunk 3", float((out.double().cpu() - o64).abs().max()), 4 * float((o32.double() - o64).abs().max()))


# ------------------------------------------------------------------------------------------------ encoder
@pytest.fixture(scope="module")
def encoders(golden, cuda):
    return {mode: encoder_of(golden, SIZE_A, mode)[0].to(cuda) for mode in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_encoder_against_every_recorded_stage(golden, encoders, cuda, mode):
    g, enc = golden, encoders[mode]
    chunk, masked = mode_chunk(synth.chunk_conformer_conf(mode=mode, **SIZE_A))
    worst = 0.0
    for i, n in enumerate(g["lens"].tolist()):
        x = torch.from_numpy(g[f"feats_{i}"])[None]
        out, olens, taps = enc.forward_stages(x, [n], chunk, "chunk" if masked else "utt")
        got = {"front": taps[0], "norm_blocks": taps[-1], "out": out}
        got.update({f"block_{j}": taps[1 + j] for j in range(enc.num_blocks)})
        assert olens.tolist() == [g[f"{mode}_{i}_out"].shape[0]]
        for name in stage_names(mode):
            want = g[f"{mode}_{i}_{name}"]
            assert tuple(got[name][0].shape) == want.shape, (mode, i, name)
            d, gap = float(np.abs(got[name][0].double().cpu().numpy() - want).max()), float(g[f"gap_{mode}_{i}_{name}"])
            _report(f"encoder {mode} clip {i} {name}", d, 4 * gap)
            worst = max(worst, d / (4 * gap))
        res = enc(x, [n])                                            # forward returns what the reference returns in the mode
        if mode == "unified":
            assert len(res) == 3 and torch.equal(res[0], out) and res[2].tolist() == olens.tolist()
            assert torch.equal(res[1], encoders["dynamic"](x, [n])[0])           # same weights: the chunk branch is dynamic's x
            assert torch.equal(enc.forward_utt(x, [n])[0], out)
        else:
            assert res[2] is None and torch.equal(res[0], out) and res[1].tolist() == olens.tolist()
    print(f"encoder {mode}: worst ratio {worst:.3f}")


def test_simu_chunk_forward_left_chunk_sizes_and_ragged_batches(golden, cuda):
    g = golden
    f3 = torch.from_numpy(g["feats_3"])[None]
    enc = encoder_of(g, SIZE_B, "dynamic")[0].to(cuda)
    out = enc.simu_chunk_forward(f3, [f3.shape[1]], chunk_size=3)
    _report("simu_chunk_forward chunk 3", float(np.abs(out[0].double().cpu().numpy() - g["simu_out"]).max()), 4 * float(g["gap_simu_out"]))
    for name, left in (("left0", 0), ("leftall", -1)):
        e = encoder_of(g, SIZE_B, "dynamic", left_chunk_size=left)[0].to(cuda)
        out = e(f3, [f3.shape[1]])[0]
        _report(f"left_chunk_size {left}", float(np.abs(out[0].double().cpu().numpy() - g[name + "_out"]).max()), 4 * float(g[f"gap_{name}_out"]))
    lens = [int(g["lens"][4]), int(g["lens"][2])]
    xb = torch.zeros(2, lens[0], 80)
    xb[0], xb[1, : lens[1]] = torch.from_numpy(g["feats_4"]), torch.from_numpy(g["feats_2"])
    for mode in MODES:
        e = encoder_of(g, SIZE_B, mode)[0].to(cuda)
        res = e(xb, lens)
        olens = res[2] if mode == "unified" else res[1]
        assert olens.tolist() == g[f"batch_{mode}_olens"].tolist()
        bar = 4 * float(g[f"gap_batch_{mode}_x"])
        _report(f"ragged batch {mode}", float(np.abs(res[0].double().cpu().numpy() - g[f"batch_{mode}_x"]).max()), bar)
        if mode != "full":                                           # causal modes: a clip's valid rows do not depend on the padding
            alone = e(xb[1:, : lens[1]], [lens[1]])[0]
            n = int(olens[1])
            _report(f"ragged batch {mode}: clip 1 against its own run", float((res[0][1, :n] - alone[0, :n]).abs().max()), bar)
    with pytest.raises(NotImplementedError, match="pad to the longest clip"):
        enc(xb, [lens[1], lens[1]])


def test_two_runs_are_bitwise_equal_and_read_nothing_stale(golden, encoders, cuda):
    x = torch.from_numpy(golden["feats_4"])[None]
    for mode in MODES:
        enc = encoders[mode]
        a = [t.clone() for t in enc(x, [x.shape[1]])[:2] if t is not None]
        enc.debug_poison()
        b = [t for t in enc(x, [x.shape[1]])[:2] if t is not None]
        assert all(torch.equal(p, q) for p, q in zip(a, b)) and all(bool(torch.isfinite(p).all()) for p in a), mode


# ------------------------------------------------------------------------------------------------ Transducer
@pytest.fixture(scope="module")
def models(golden, cuda):
    out = {}
    for mode in ("dynamic", "unified"):
        model, sd, conf = golden_model(golden, mode)
        out[mode] = (model.to(cuda), sd, conf)
    return out


@pytest.mark.parametrize("name,mode,clip,beam", golden_searches())
def test_searches_from_the_handles_own_encoder_output(golden, models, cuda, name, mode, clip, beam):
    """encode (in unified mode the utt branch alone, with the true lengths) -> search: the recorded ids and scores"""
    g, model = golden, models[mode][0]
    feats = torch.from_numpy(g[f"feats_{clip}"])
    enc, olens = model.encode(feats[None].to(cuda), [feats.shape[0]])
    assert olens.tolist() == [enc.shape[1]]
    res = model.encoder(feats[None], [feats.shape[0]])
    assert torch.equal(enc, res[0]) and len(res) == 3 and (res[2] is None) == (mode == "dynamic")
    hyps, info = model.search(enc[0], beam_size=beam, nbest=beam)
    n = int(g[f"search_{name}_n"])
    assert [h[0] for h in hyps] == [g[f"search_{name}_ids_{r}"].tolist() for r in range(n)]
    d = float(np.abs(np.asarray([h[1] for h in hyps]) - g[f"search_{name}_scores"]).max())
    _report(f"search {name} scores ({info})", d, 4 * float(g["gap_score"]))


@pytest.mark.parametrize("mode", ["dynamic", "unified"])
def test_automodel_on_a_directory_written_from_the_tiny_config(golden, models, cuda, tmp_path, mode):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.chunk_conformer import ChunkConformerEncoder
    from funasr_amd.transducer import Transducer

    g, (_, sd, c) = golden, models[mode]
    conf = {"model": "Transducer", "model_conf": {"auxiliary_ctc_weight": 0.0},
            "encoder": c["encoder"], "encoder_conf": c["encoder_conf"], "decoder": c["decoder"], "decoder_conf": c["decoder_conf"],
            "joint_network": c["joint_network"], "joint_network_conf": c["joint_network_conf"],
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    assert conf["encoder"] == "ChunkConformerEncoder"
    path = str(tmp_path / "chunk_rnnt")
    os.makedirs(path)
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    tokens = g["tokens"].tolist()
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    am = AutoModel(model=path, device="cuda", disable_update=True)
    assert isinstance(am.model, Transducer) and isinstance(am.model.encoder, ChunkConformerEncoder) and am.model.encoder.precision == "fp32"
    clips = sorted({cl for _, m, cl, b in golden_searches() if m == mode and b == 2})
    assert set(clips) >= {3, 4}
    for clip in clips:
        feats = torch.from_numpy(g[f"feats_{clip}"])
        res = am.generate(input=feats, data_type="fbank", key=f"clip{clip}")
        want = [tokens[t] for t in g[f"search_{mode}_c{clip}_b2_ids_0"].tolist() if t not in (0, 1, 2)]
        assert len(res) == 1 and res[0]["token"] == want, (clip, res[0]["token"], want)


@pytest.mark.parametrize("factor", [2, 4, 6])
def test_clips_of_one_to_six_frames_run_as_in_the_reference(golden, cuda, factor):
    """nothing is too short for the reference's time-padded front; against the float64 oracle"""
    enc, sd, conf = encoder_of(golden, SIZE_A, "dynamic", subsampling_factor=factor)
    enc = enc.to(cuda)
    for L in (1, 2, 6):
        x = torch.randn(1, L, 80, generator=torch.Generator().manual_seed(L))
        out, olens, _ = enc(x, [L])
        o64 = O.encoder(O.cast(sd, torch.float64), x.double(), [L], conf, 4, True)
        o32 = O.encoder(sd, x, [L], conf, 4, True)
        assert olens.tolist() == o64["olens"] == [out.shape[1]]
        bar = max(4 * float((o32["out"].double() - o64["out"]).abs().max()), 2.0 ** -21 * float(o64["out"].abs().max()))
        _report(f"factor {factor}, {L} frames", float((out.double().cpu() - o64["out"]).abs().max()), bar)
