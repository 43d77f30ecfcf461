"""RWKV encoder on the MI355X through the C ABI: the chunked WKV scan and the token-shift mix against the float64 oracle on random
inputs (NaN guard rows around every buffer, rows past a length exactly zero), their bitwise independence properties, the encoder
against every recorded stage of the reference (tests/golden/rwkv.npz), ragged batches bitwise equal to single clips, and the
Transducer over it: recorded searches and AutoModel on a model directory written from the reference template's yaml at tiny size.

Bars are the project's fp32 rules (tests/test_conformer_gpu.py): 4 x the reference's own fp32 - fp64 gap where one is recorded;
elsewhere 4 x max |oracle fp32 - oracle fp64| of the case. For the random-input kernel tests only, the bar is never below 2^-21 x the
case's largest |oracle value| (8 fp32 roundings, about the count in one quotient of two two-term sums): the oracle's own fp32 run can
land within an ulp at T <= 2, and 4 x gap would then test the host's exp, not the kernel. Searches: ids equal, scores within
4 x gap_score. Every test prints its measured ratio."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from funasr_amd import _lib, synth
from funasr_amd.transducer import Transducer

from . import _rwkv_oracle as O
from .test_rwkv import GOLDEN, P, golden_model, golden_searches, load_golden, recorded, recorded_gap

pytestmark = pytest.mark.gpu
GUARD = 3                                      # NaN rows in front of and behind every buffer


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chunk():
    return int(_lib.load().pf_k_rwkv_chunk())


def _report(tag, d, bar):
    print(f"{tag}: max |d| {d:.3e}, bar {bar:.3e}, ratio {d / max(bar, 1e-300):.3f}")
    assert d <= bar, (tag, d, bar)


def _guarded(rows, ld, cuda):
    """a [GUARD + rows + GUARD, ld] buffer of NaN and the view of its middle rows"""
    buf = torch.full((rows + 2 * GUARD, ld), float("nan"), device=cuda)
    return buf, buf[GUARD: GUARD + rows]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


# ------------------------------------------------------------------------------------------------ WKV
def _wkv_lens(T):
    return [T, max(1, T - 3), 1]


def _wkv_inputs(T, D, seed, k_scale=4.0, time_decay=None, clamp=None, v_boost=False):
    g = torch.Generator().manual_seed(seed)
    B = 3
    k = k_scale * torch.randn(B, T, D, generator=g)
    if clamp is not None:
        k = k.clamp(-clamp, clamp)
    v = torch.randn(B, T, D, generator=g)
    if v_boost:
        v[1] = 1000.0 * v[0]
    r = 2.0 * torch.randn(B, T, D, generator=g)
    td = (-5 + 8 * torch.rand(D, generator=g)) if time_decay is None else torch.full((D,), float(time_decay))
    return k, v, r, -torch.exp(td), 0.5 * torch.randn(D, generator=g)


def _wkv_oracle(k, v, r, w, u, lens, dt):
    return [torch.sigmoid(r[b, :n].to(dt)) * O.wkv(k[b, :n].to(dt), v[b, :n].to(dt), w.to(dt), u.to(dt)) for b, n in enumerate(lens)]


def _wkv_gpu(cuda, k, v, r, w, u, lens):
    """k, v, r [B, T, D] -> (out [B, T, D], the guarded output buffer): the three operands as column slices of one guarded buffer of
    row stride 3 D + 4 whose rows past a length (and pad columns) hold NaN"""
    B, T, D = k.shape
    ld, ldo = 3 * D + 4, D + 4
    ibuf, iv = _guarded(B * T, ld, cuda)
    for b, n in enumerate(lens):
        rows = iv[b * T: b * T + n]
        rows[:, :D], rows[:, D: 2 * D], rows[:, 2 * D: 3 * D] = k[b, :n].to(cuda), v[b, :n].to(cuda), r[b, :n].to(cuda)
    obuf, ov = _guarded(B * T, ldo, cuda)
    lib = _lib.load()
    n_scr = B * ((T + _chunk() - 1) // _chunk()) * 3 * D
    scr = torch.full((n_scr + 8,), float("nan"), device=cuda)
    wd, ud = w.contiguous().to(cuda), u.contiguous().to(cuda)
    ld_t = torch.tensor(lens, dtype=torch.int32, device=cuda)
    base = iv.data_ptr()
    _lib.check(lib.pf_k_rwkv_wkv(base, base + 4 * D, base + 8 * D, ld, wd.data_ptr(), ud.data_ptr(), ld_t.data_ptr(), B, T, D, ov.data_ptr(), ldo,
                                 scr.data_ptr(), n_scr, _stream()), "pf_k_rwkv_wkv")
    torch.cuda.synchronize()
    assert _guards_intact(obuf) and bool(torch.isnan(ov[:, D:]).all()) and bool(torch.isnan(scr[n_scr:]).all())
    return ov[:, :D].reshape(B, T, D).clone(), obuf


def _wkv_case(cuda, tag, T, D, **kw):
    k, v, r, w, u = _wkv_inputs(T, D, seed=7 * T + D, **kw)
    lens = _wkv_lens(T)
    out, _ = _wkv_gpu(cuda, k, v, r, w, u, lens)
    o64, o32 = _wkv_oracle(k, v, r, w, u, lens, torch.float64), _wkv_oracle(k, v, r, w, u, lens, torch.float32)
    for b, n in enumerate(lens):
        assert bool((out[b, n:] == 0).all()), (tag, b)                # rows past a length: exactly zero
        gap = float((o32[b].double() - o64[b]).abs().max())
        bar = max(4 * gap, 2.0 ** -21 * float(o64[b].abs().max()))
        _report(f"wkv {tag} T={T} D={D} clip {b}", float((out[b, :n].double().cpu() - o64[b]).abs().max()), bar)
    return out


# the lengths follow the library's chunk length L = pf_k_rwkv_chunk(), read when the test runs
CHUNK_LENGTHS = {"1": lambda L: 1, "2": lambda L: 2, "L-1": lambda L: L - 1, "L": lambda L: L, "L+1": lambda L: L + 1,
                 "2L+5": lambda L: 2 * L + 5}


@pytest.mark.parametrize("D", [32, 96, 512])
@pytest.mark.parametrize("T", list(CHUNK_LENGTHS))
def test_wkv_against_the_float64_oracle(cuda, T, D):
    assert _chunk() >= 2
    _wkv_case(cuda, "random", CHUNK_LENGTHS[T](_chunk()), D)


def test_wkv_frame_zero_is_the_references_zero_over_zero(cuda):
    """the reference's initial running maximum is -1e-30, not -inf: with u + k0 far below -104 both exponentials of frame 0 are 0 in
    fp32 and its output is 0 / 0. The kernel reproduces that (NaN exactly where the fp32 oracle has it) and nothing else suffers: the
    state restarts from the next frame's key, and every later frame, in this chunk and the next, meets the float64 oracle"""
    T, D = _chunk() + 3, 96
    k, v, r, w, u = _wkv_inputs(T, D, seed=13)
    k[0, 0, ::2] = -200.0                                            # every second channel of clip 0
    lens = _wkv_lens(T)
    out, _ = _wkv_gpu(cuda, k, v, r, w, u, lens)
    o64, o32 = _wkv_oracle(k, v, r, w, u, lens, torch.float64), _wkv_oracle(k, v, r, w, u, lens, torch.float32)
    assert bool(torch.isnan(o32[0][0, ::2]).all()) and bool(torch.isfinite(o64[0]).all())
    got = out[0].cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(o32[0])) and int(torch.isnan(got).sum()) == D // 2
    for b in range(3):
        keep = ~torch.isnan(o32[b])
        gap = float((o32[b].double() - o64[b])[keep].abs().max())
        bar = max(4 * gap, 2.0 ** -21 * float(o64[b].abs().max()))
        _report(f"wkv frame-0 NaN clip {b}", float((out[b, : lens[b]].double().cpu() - o64[b])[keep].abs().max()), bar)


def test_wkv_overflow_range_and_the_two_ends_of_time_decay(cuda):
    """|k| up to 80 (e^80 overflows nothing only through the max trick); time_decay -8 everywhere (w = -3e-4: nothing is forgotten
    across chunks, the carries matter in full) and +4 (w = -55: the carry is gone within a frame)"""
    T = 2 * _chunk() + 5
    _wkv_case(cuda, "|k| <= 80", T, 96, k_scale=60.0, clamp=80.0)
    _wkv_case(cuda, "time_decay -8", T, 96, time_decay=-8.0)
    _wkv_case(cuda, "time_decay +4", T, 96, time_decay=4.0)


def test_wkv_carries_nothing_across_clips(cuda):
    """clip 1's v is 1000 x clip 0's: a carry (or a token shift) leaking from one clip into the next would show at once; and a clip in
    the batch has the bits it has alone"""
    T, D = 2 * _chunk() + 5, 96
    lens = _wkv_lens(T)
    out = _wkv_case(cuda, "v x 1000", T, D, v_boost=True)
    k, v, r, w, u = _wkv_inputs(T, D, seed=7 * T + D, v_boost=True)                # the inputs of that case again
    for b, n in enumerate(lens):
        alone, _ = _wkv_gpu(cuda, k[b: b + 1, :n].repeat(3, 1, 1), v[b: b + 1, :n].repeat(3, 1, 1), r[b: b + 1, :n].repeat(3, 1, 1), w, u,
                            [n, 1, 1])
        assert torch.equal(alone[0, :n], out[b, :n]), b


def test_wkv_prefix_is_bitwise_independent_of_what_follows(cuda):
    """T = 2 L + 5 against its first L + 1 frames computed with T = L + 1: chunk boundaries are fixed, so the bits agree"""
    L, D = _chunk(), 96
    k, v, r, w, u = _wkv_inputs(2 * L + 5, D, seed=11)
    full, _ = _wkv_gpu(cuda, k, v, r, w, u, [2 * L + 5] * 3)
    head, _ = _wkv_gpu(cuda, k[:, : L + 1].contiguous(), v[:, : L + 1].contiguous(), r[:, : L + 1].contiguous(), w, u, [L + 1] * 3)
    assert torch.equal(full[:, : L + 1], head)
    again, _ = _wkv_gpu(cuda, k, v, r, w, u, [2 * L + 5] * 3)
    assert torch.equal(full, again)


# ------------------------------------------------------------------------------------------------ mix
def _mix_oracle(x, gamma, beta, mus, lens, dt):
    out = []
    for b, n in enumerate(lens):
        y = F.layer_norm(x[b, :n].to(dt), (x.shape[-1],), gamma.to(dt), beta.to(dt), O.EPS)
        out.append(torch.cat([O.mix(y, mu.to(dt)) for mu in mus], dim=-1))
    return out


@pytest.mark.parametrize("n_out", [2, 3])
@pytest.mark.parametrize("D", [32, 96, 512, 1024])
@pytest.mark.parametrize("T", [1, 2, 33])
def test_mix_against_the_float64_oracle(cuda, T, D, n_out):
    """clip 1's rows are 1000 x clip 0's: the row before a clip's first row is zero, not the previous clip's last row"""
    g = torch.Generator().manual_seed(3 * T + D + n_out)
    B, lens = 3, [T, max(1, T - 3), 1]
    x = torch.randn(B, T, D, generator=g)
    x[1] = 1000.0 * x[0]
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    mus = [torch.rand(D, generator=g) for _ in range(n_out)]
    ldx, ldy = D + 8, 3 * D + 4
    xbuf, xv = _guarded(B * T, ldx, cuda)
    for b, n in enumerate(lens):
        xv[b * T: b * T + n, :D] = x[b, :n].to(cuda)
    ybuf, yv = _guarded(B * T, ldy, cuda)
    dev = [t.contiguous().to(cuda) for t in [gamma, beta] + mus]
    ld_t = torch.tensor(lens, dtype=torch.int32, device=cuda)
    _lib.check(_lib.load().pf_k_rwkv_mix(xv.data_ptr(), ldx, dev[0].data_ptr(), dev[1].data_ptr(), O.EPS, dev[2].data_ptr(), dev[3].data_ptr(),
                                        dev[4].data_ptr() if n_out == 3 else None, yv.data_ptr(), ldy, ld_t.data_ptr(), B, T, D, _stream()),
               "pf_k_rwkv_mix")
    torch.cuda.synchronize()
    assert _guards_intact(ybuf) and bool(torch.isnan(yv[:, n_out * D:]).all())
    got = yv[:, : n_out * D].reshape(B, T, n_out * D)
    o64, o32 = _mix_oracle(x, gamma, beta, mus, lens, torch.float64), _mix_oracle(x, gamma, beta, mus, lens, torch.float32)
    for b, n in enumerate(lens):
        assert bool((got[b, n:] == 0).all()), b
        gap = float((o32[b].double() - o64[b]).abs().max())
        bar = max(4 * gap, 2.0 ** -21 * float(o64[b].abs().max()))
        _report(f"mix T={T} D={D} n_out={n_out} clip {b}", float((got[b, :n].double().cpu() - o64[b]).abs().max()), bar)


# ------------------------------------------------------------------------------------------------ encoder
@pytest.fixture(scope="module")
def golden(cuda):
    g = load_golden()
    model, sd, conf = golden_model(g)
    return g, model.to(cuda), sd, conf


@pytest.fixture(scope="module")
def singles(golden, cuda):
    """every golden clip through the handle alone, with its stages: computed once, shared, never modified"""
    g, model, _, _ = golden
    out = []
    for i in range(len(g["lens"])):
        f = torch.from_numpy(g[f"feats_{i}"])
        enc, olens, taps = model.encoder.forward_stages(f[None].to(cuda), [f.shape[0]])
        out.append((enc[0].clone(), int(olens[0]), [t[0].clone() for t in taps]))
    return out


def test_encoder_meets_every_recorded_stage(golden, singles):
    g = golden[0]
    worst = 0.0
    for i, (enc, olen, taps) in enumerate(singles):
        assert olen == g[f"enc_{i}"].shape[0] == enc.shape[0]
        got = {"front": taps[0], "embed_norm": taps[1], "enc": enc}
        got.update({f"block_{j}": t for j, t in enumerate(taps[2:])})
        for name, t in got.items():
            d = float(np.abs(t.double().cpu().numpy() - recorded(g, i, name)).max())
            gap = recorded_gap(g, i, name)
            worst = max(worst, d / gap)
            print(f"clip {i} {name}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / gap:.2f} (bar 4)")
            assert d <= 4 * gap, (i, name, d, gap)
    print(f"encoder against the recorded stages: largest ratio {worst:.2f}")


def _ragged(g, cuda):
    lens = g["lens"].tolist()
    xs = torch.zeros(len(lens), max(lens), 80)
    for i, n in enumerate(lens):
        xs[i, :n] = torch.from_numpy(g[f"feats_{i}"])
    return xs.to(cuda), lens


def test_ragged_batch_is_bitwise_the_single_clips(golden, singles, cuda):
    """the five clips as one batch, twice, and once more over a poisoned workspace: bit for bit the singles, zeros behind"""
    g, model, _, _ = golden
    xs, lens = _ragged(g, cuda)
    out, olens, _ = model.encoder(xs, lens)
    assert olens.tolist() == [s[1] for s in singles]
    for i, (enc, olen, _) in enumerate(singles):
        assert torch.equal(out[i, :olen], enc), i
        assert bool((out[i, olen:] == 0).all()), i
    again, _, _ = model.encoder(xs, lens)
    assert torch.equal(again, out)
    model.encoder.debug_poison()
    poisoned, _, _ = model.encoder(xs, lens)
    assert torch.equal(poisoned, out)
    order = [4, 0, 3, 1, 2]                                           # another order, another padded length for most clips
    out2, _, _ = model.encoder(xs[order], [lens[i] for i in order])
    for j, i in enumerate(order):
        assert torch.equal(out2[j, : singles[i][1]], singles[i][0]), i


def test_batch_rows_are_bitwise_the_single_clips_across_the_gemm_tile_switch(cuda):
    """the fp32 GEMM takes 64-row block tiles while its grid is small and 128-row ones beyond (gemm_f32.hip): at D 512 / linear_size
    2048 one clip of 1024 frames (256 rows) is on the small side for every linear, sixteen (4096 rows) are on the large side for
    proj_key and on the small side for the D-wide ones. A clip's rows have the same bits either way."""
    from funasr_amd.rwkv_encoder import RWKVEncoder

    enc = RWKVEncoder(input_size=80, **synth.rwkv_encoder_conf(output_size=512, linear_size=2048, num_blocks=1, time_reduction_factor=1))
    enc.load_state_dict(synth.rwkv_encoder_state_dict(41, enc), strict=True)
    enc = enc.to(cuda)
    B, L = 16, 1024
    lens = [L - 37 * b for b in range(B)]
    xs = torch.randn(B, L, 80, generator=torch.Generator().manual_seed(42)).to(cuda)
    out, olens, _ = enc(xs, lens)
    for b in (0, 7, 15):
        alone, ol, _ = enc(xs[b: b + 1, : lens[b]], [lens[b]])
        assert int(ol[0]) == int(olens[b])
        assert torch.equal(alone[0], out[b, : int(ol[0])]), b
        assert bool((out[b, int(ol[0]):] == 0).all()), b


def test_first_frames_do_not_depend_on_what_follows(golden, singles, cuda):
    """behind the front every block looks back only (the front's 3x3 convs do look one frame ahead each, so the property starts at
    embed_norm): the blocks over the first n embed_norm rows alone give the first n rows of the blocks over the whole clip -- exactly
    so in the float64 oracle, and the handle's rows of the whole clip meet that shorter run within the recorded gap"""
    g, model, sd, conf = golden
    s = O.cast(sd, torch.float64, cuda)
    feats = torch.from_numpy(g["feats_4"]).double().to(cuda)
    full = O.encode(feats, s, 2, P)
    enc, olen, taps = singles[4]
    n = 9                                                            # the first n frames behind the front
    x = full["embed_norm"][:n]
    for i in range(O.num_blocks(s, P)):
        b = f"{P}rwkv_blocks.{i}."
        x = x + O.time_mix(O.layer_norm(x, s, b + "layer_norm_att."), s, b + "att.")
        x = x + O.channel_mix(O.layer_norm(x, s, b + "layer_norm_ffn."), s, b + "ffn.")
        assert float((x - full["blocks"][i][:n]).abs().max()) == 0.0
    gap = recorded_gap(g, 4, "block_2")
    _report("block 2 prefix of clip 4", float((taps[-1][:n].double() - x).abs().max()), 4 * gap)


def test_template_geometry_against_the_float64_oracle(cuda):
    """one 300-frame clip at the reference template's geometry (D 512, 18 blocks, linear_size 2048, every second frame): the oracle in
    float64 and float32 runs on the same GPU through torch"""
    from funasr_amd.rwkv_encoder import RWKVEncoder

    conf = synth.rwkv_encoder_conf(linear_size=None, **synth.RWKV_TEMPLATE)
    enc = RWKVEncoder(input_size=80, **conf)
    sd = synth.rwkv_encoder_state_dict(31, enc)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(cuda)
    feats = torch.randn(300, 80, generator=torch.Generator().manual_seed(32))
    out, olens, _ = enc(feats[None].to(cuda), [300])
    assert olens.tolist() == [38] and out.shape == (1, 38, 512)
    o64 = O.encode(feats.double().to(cuda), O.cast(sd, torch.float64, cuda), 2)["out"]
    o32 = O.encode(feats.to(cuda), O.cast(sd, torch.float32, cuda), 2)["out"]
    assert bool(torch.isfinite(o64).all())
    gap = float((o32.double() - o64).abs().max())
    _report("template geometry, 300 frames", float((out[0].double() - o64).abs().max()), 4 * gap)


# ------------------------------------------------------------------------------------------------ Transducer
@pytest.mark.parametrize("name,clip,beam", golden_searches())
def test_searches_from_the_handles_own_encoder_output(golden, singles, cuda, name, clip, beam):
    g, model, _, _ = golden
    hyps, info = model.search(singles[clip][0], beam_size=beam, nbest=beam)
    n = int(g[f"search_{name}_n"])
    assert [h[0] for h in hyps] == [g[f"search_{name}_ids_{r}"].tolist() for r in range(n)]
    d = float(np.abs(np.asarray([h[1] for h in hyps]) - g[f"search_{name}_scores"]).max())
    _report(f"search {name} scores ({info})", d, 4 * float(g["gap_score"]))


class _Tok:
    def __init__(self, tokens):
        self.tokens = tokens

    def ids2tokens(self, ids):
        return [self.tokens[i] for i in ids]

    def tokens2text(self, tokens):
        return "".join(tokens)


def test_inference_returns_the_recorded_tokens(golden, cuda):
    g, model, _, _ = golden
    tokens = g["tokens"].tolist()
    for clip in (2, 3, 4):
        feats = torch.from_numpy(g[f"feats_{clip}"])
        res, _ = model.inference(feats[None], data_lengths=[feats.shape[0]], key=[f"clip{clip}"], tokenizer=_Tok(tokens), data_type="fbank",
                                 beam_size=2)
        want = [tokens[t] for t in g[f"search_c{clip}_b2_ids_0"].tolist() if t not in (0, 1, 2)]
        assert len(res) == 1 and res[0]["token"] == want, (clip, res, want)
    with pytest.raises(NotImplementedError) as e:
        model.inference(torch.zeros(2, 50, 80), batch_size=2)
    assert str(e.value) == "batch decoding is not implemented"


def test_automodel_on_a_directory_written_from_the_template(golden, singles, cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.rwkv_encoder import RWKVEncoder

    g, _, sd, c = golden
    # every setting of the reference's funasr/models/rwkv_bat/template.yaml as tools/make_golden_rwkv.py recorded it; the sizes shrink
    with open(os.path.join(GOLDEN, "rwkv_state_dict.json"), encoding="utf-8") as f:
        conf = json.load(f)["template"]
    assert conf["model"] == "Transducer" and conf["encoder"] == "RWKVEncoder" and conf["frontend"] == "WavFrontend"
    assert conf["specaug"] == "SpecAugLFR" and conf["tokenizer"] == "CharTokenizer"
    conf["encoder_conf"].update({k: c["encoder_conf"][k] for k in ("output_size", "num_blocks", "linear_size")})
    conf["decoder_conf"].update(c["decoder_conf"])
    conf["joint_network_conf"].update(c["joint_network_conf"])
    path = str(tmp_path / "rwkv_bat")
    os.makedirs(path)
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    torch.save({"state_dict": sd}, os.path.join(path, "model.pt"))
    tokens = g["tokens"].tolist()
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    am = AutoModel(model=path, device="cuda", disable_update=True)
    assert isinstance(am.model, Transducer) and isinstance(am.model.encoder, RWKVEncoder) and am.model.encoder.precision == "fp32"
    for clip in (2, 3, 4):
        feats = torch.from_numpy(g[f"feats_{clip}"])
        enc, _ = am.model.encode(feats[None].to(cuda), [feats.shape[0]])
        assert torch.equal(enc[0], singles[clip][0])
        res = am.generate(input=feats, data_type="fbank", key=f"clip{clip}")
        want = [tokens[t] for t in g[f"search_c{clip}_b2_ids_0"].tolist() if t not in (0, 1, 2)]
        assert len(res) == 1 and res[0]["token"] == want, (clip, res[0]["token"], want)
    with pytest.raises(NotImplementedError, match="batch decoding is not implemented"):
        am.model.inference(torch.zeros(2, 50, 80), batch_size=2)
