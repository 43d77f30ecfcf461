"""UniASR on the MI355X through the C ABI: the chunk-masked encoder against the float64 oracle at the chunk boundaries, the kernels
with NaN in everything their masks exclude, the SCAMA decoder step under every window shape (beams of 1 and 5, a reorder between
steps, a `decoders2` layer), `stride_conv` with kernels and strides of 2 and 3, and the model against the reference's recorded float64
outputs in the three decoding modes (stages, n-best ids and scores), through AutoModel too.

Bars (those of tests/test_sanm_gpu.py; everything here is computed in exact fp32): 4 x the reference's recorded fp32 - fp64 gap, 8 x
for n-best scores; where no recorded gap exists (the runs at other shapes and on random inputs) 4 x max |oracle fp32 - oracle fp64|
-- another valid fp32 summation order may be that far off -- with a floor of 1e-7. Ids, alignments, masks and the order of the
hypotheses are equal outright (tests/test_uniasr.py asserts the margins of the recorded search)."""
import numpy as np
import pytest
import torch

from funasr_amd import _lib, synth
from funasr_amd.uniasr import ChunkLayout, FsmnDecoderSCAMAOpt, StrideConv, UniASR, chunk_layout

from . import _uniasr_oracle as O
from .test_uniasr import MODES, golden_model, load_golden, write_model_dir

pytestmark = pytest.mark.gpu
FLOOR = 1e-7


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _maxd(a, b):
    return float((torch.as_tensor(O.to_np(a)).double() - torch.as_tensor(O.to_np(b)).double()).abs().max())


def _check(tag, got, want64, gap, factor=4.0):
    d = _maxd(got, want64)
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / max(gap, 1e-30):.2f} (bar {factor:g})")
    assert bool(torch.isfinite(torch.as_tensor(O.to_np(got))).all()), tag
    assert d <= factor * gap, (tag, d, gap)


def _check_oracles(tag, got, want64, want32):
    _check(tag, got, want64, max(_maxd(want32, want64), FLOOR))


@pytest.fixture(scope="module")
def setup(cuda):
    """the golden model on the device and its weights in both oracle precisions, once"""
    g = load_golden()
    m, sd, conf = golden_model(g)
    m.to(cuda).eval()
    return g, m, O.cast(sd, torch.float64), O.cast(sd, torch.float32), conf


# ------------------------------------------------------------------------------------------------ chunked encoder
@pytest.mark.parametrize("ind,look_back", [(0, 0), (0, 50), (1, 1), (1, 50)])
def test_chunked_encoder_against_the_oracle_at_the_chunk_boundaries(cuda, setup, ind, look_back):
    """T: shorter than pad_left + 1, one partial chunk, exactly k strides, k strides + 1, several chunks with a partial last one"""
    g, m, sd64, sd32, conf = setup
    econf = dict(conf["encoder_conf"])
    lb = list(econf["encoder_att_look_back_factor"])
    lb[ind] = look_back
    econf["encoder_att_look_back_factor"] = lb
    saved = m.encoder.encoder_att_look_back_factor
    m.encoder.encoder_att_look_back_factor = lb
    stride, pad_left = econf["stride"][ind], econf["pad_left"][ind]
    try:
        for T in sorted({1, pad_left, stride - 1, stride + 1, 3 * stride, 3 * stride + 1, 61} - {0}):
            x = torch.randn(T, 80, generator=torch.Generator().manual_seed(100 * T + ind))
            geo = O.geometry_of(econf, T, ind)
            assert chunk_layout(m.encoder, T, ind).enc_look_back == look_back
            out, olens, _ = m.encoder(x[None].to(cuda), [T], ind=ind)
            assert olens.tolist() == [geo["Tc"]] and tuple(out.shape) == (1, geo["Tc"], 128)
            _check_oracles(f"ind {ind} look-back {look_back} T {T} (Tc {geo['Tc']})", out[0],
                           O.encoder_chunked(sd64, "encoder.", econf, x.double(), geo), O.encoder_chunked(sd32, "encoder.", econf, x, geo))
    finally:
        m.encoder.encoder_att_look_back_factor = saved
    # the whole-utterance forward of the class is what it was
    x = torch.randn(1, 9, 80, generator=torch.Generator().manual_seed(9))
    a, _, _ = m.encoder(x.to(cuda), [9])
    assert tuple(a.shape) == (1, 9, 128) and bool(torch.isfinite(a).all())


def _chunk_attention(cuda, qkv, T, H, dk, lay, klen=None):
    out = torch.full((T, H * dk), float("nan"), device=cuda)
    klens = torch.tensor([T if klen is None else klen], dtype=torch.int32, device=cuda)
    q = qkv.to(cuda).contiguous()
    _lib.check(_lib.load().pf_k_chunk_attention(q.data_ptr(), klens.data_ptr(), 1, T, H, dk, lay.chunk, lay.stride, lay.shift, lay.enc_look_back,
                                                out.data_ptr(), _stream()), "pf_k_chunk_attention")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("dk,H", [(64, 2), (80, 1), (128, 1), (32, 2)])
@pytest.mark.parametrize("chunk,stride,pad_left,shift,look_back", [(4, 2, 1, 5, 1), (6, 4, 2, 5, 2), (5, 5, 0, 0, 50), (70, 66, 2, 5, 1)])
def test_chunk_attention_reads_no_key_outside_the_mask(cuda, dk, H, chunk, stride, pad_left, shift, look_back):
    """per probed query row: NaN in the K and V of every row that row may not see; the row's output is the oracle's and finite. Rows:
    a shift row (zero), a chunk's first row (look-back), a row past the chunk's first `stride` (own chunk only), the last row of the
    partial last chunk. (70, 66): a row's keys span more than one 64-key tile."""
    T = 3 * stride + 1 if chunk < 70 else 2 * stride + 3
    lay = ChunkLayout(T, chunk, stride, pad_left, shift, look_back, 1)
    Tc, D = lay.Tc, H * dk
    qkv = torch.randn(Tc, 3 * D, generator=torch.Generator().manual_seed(Tc + dk))
    mask = torch.from_numpy(lay.att_mask())
    q, k, v = qkv.split(D, dim=-1)
    want64 = O.masked_attention(q.double(), k.double(), v.double(), H, mask)
    want32 = O.masked_attention(q, k, v, H, mask)
    _check_oracles(f"chunk attention d_k {dk} clean", _chunk_attention(cuda, qkv, Tc, H, dk, lay), want64, want32)
    P = lay.period
    last_chunk = (lay.n_chunks - 1) * P
    rows = sorted({min(r, Tc - 1) for r in (0 if shift else P - 1, last_chunk + shift, last_chunk + shift + stride, 2 * P + shift,
                                            2 * P + shift + chunk - 1, Tc - 1)})
    for r in rows:
        poisoned = qkv.clone()
        dead = mask[r] == 0
        poisoned[dead, D:] = float("nan")
        got = _chunk_attention(cuda, poisoned, Tc, H, dk, lay)[r]
        _check_oracles(f"chunk attention d_k {dk} row {r} ({int((~dead).sum())} visible keys) over poisoned keys", got, want64[r], want32[r])
    # keys at and past klens are padding even inside a row's chunk
    klen = Tc - 1
    short = mask.clone()
    short[:, klen:] = 0
    poisoned = qkv.clone()
    poisoned[klen:, D:] = float("nan")
    got = _chunk_attention(cuda, poisoned, Tc, H, dk, lay, klen)[:klen]
    _check_oracles(f"chunk attention d_k {dk} klens {klen}", got, O.masked_attention(q.double(), k.double(), v.double(), H, short)[:klen],
                   O.masked_attention(q, k, v, H, short)[:klen])


def test_chunk_fsmn_reads_no_masked_row(cuda):
    T, C, K, left = 41, 128, 11, 5
    lay = ChunkLayout(17, 4, 2, 1, 5, 0, 1)
    assert lay.Tc >= T
    gen = torch.Generator().manual_seed(5)
    x, w = torch.randn(T, 3 * C, generator=gen), torch.randn(C, 1, K, generator=gen) * K ** -0.5
    m = torch.from_numpy(lay.mask_shift[:T]).clone()
    m[T - 3:] = 0                                                    # lens = T - 3
    want64, want32 = O.fsmn_memory(x[:, 2 * C:].double(), w.double(), m.double(), left), O.fsmn_memory(x[:, 2 * C:], w, m, left)
    xp = x.clone()
    xp[m == 0] = float("nan")
    out = torch.full((T, C), float("nan"), device=cuda)
    xd, wd = xp.to(cuda), w.to(cuda).contiguous()
    lens = torch.tensor([T - 3], dtype=torch.int32, device=cuda)
    _lib.check(_lib.load().pf_k_chunk_fsmn(xd.data_ptr() + 4 * 2 * C, 3 * C, wd.data_ptr(), lens.data_ptr(), 1, T, C, K, left, lay.chunk, lay.stride,
                                           lay.shift, out.data_ptr(), _stream()), "pf_k_chunk_fsmn")
    torch.cuda.synchronize()
    _check_oracles("chunk FSMN over poisoned masked rows", out, want64, want32)
    assert bool((out.cpu()[m == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ decoder step
def _windows(T):
    """mask rows: the first frame, the last frame, one frame in the middle, the whole memory, nothing, a window with holes"""
    rows = np.zeros((6, T), np.float32)
    rows[0, 0] = rows[1, T - 1] = rows[2, T // 2] = 1
    rows[3] = 1
    rows[5, 3: T - 2: 3] = 1
    return rows


@pytest.mark.parametrize("which", ["decoder", "decoder2"])
@pytest.mark.parametrize("n", [1, 5])
def test_decoder_step_against_the_oracle_under_every_window(cuda, setup, which, n):
    """decoder: cross-attention in both layers, R = 5; decoder2: one `decoders2` layer (att_layer_num 1 of 2), R = 0. Eight positions (the
    last two reuse the last row), random parents from the second position on."""
    g, m, sd64, sd32, conf = setup
    dec, dconf = getattr(m, which), conf[which + "_conf"]
    assert isinstance(dec, FsmnDecoderSCAMAOpt) and (dec.decoders2 is not None) == (which == "decoder2")
    T = 37
    gen = torch.Generator().manual_seed(7 + n)
    memory = torch.randn(T, 128, generator=gen)
    rows = _windows(T)
    o64 = O.ScamaStepper(sd64, dconf, memory.double(), rows, prefix=which + ".")
    o32 = O.ScamaStepper(sd32, dconf, memory, rows, prefix=which + ".")
    dec.set_memory(memory.to(cuda), rows)
    for s in (o64, o32, dec):
        s.begin(8, n)
    for pos in range(8):
        tokens = [1] * n if pos == 0 else torch.randint(3, 29, (n,), generator=gen).tolist()
        if pos > 0 and n > 1:
            parents = torch.randint(0, n, (n,), generator=gen).tolist()
            for s in (o64, o32, dec):
                s.reorder(parents)
        _check_oracles(f"{which} beam {n} position {pos} ({int(rows[min(pos, 5)].sum())} visible keys)", dec.step(tokens, pos), o64.step(tokens, pos),
                       o32.step(tokens, pos))
    # no mask at all is the SAN-M step
    dec.set_memory(memory.to(cuda))
    plain64, plain32 = O.ScamaStepper(sd64, dconf, memory.double(), None, prefix=which + "."), O.ScamaStepper(sd32, dconf, memory, None, prefix=which + ".")
    for s in (plain64, plain32, dec):
        s.begin(1, 1)
    _check_oracles(f"{which} without a mask", dec.step([1], 0), plain64.step([1], 0), plain32.step([1], 0))


def test_empty_window_is_the_references_all_masked_row(cuda, setup):
    """the reference under an all-zero mask row (recorded): scores filled with the dtype's minimum, softmax, probabilities filled with 0"""
    g, m, sd64, sd32, conf = setup
    for mode in MODES:
        which = O.MODES[mode][1]
        dec = m.decoder if which == 1 else m.decoder2
        memory = torch.from_numpy(g[f"{mode}_enc{which}"]).float()
        dec.set_memory(memory.to(cuda), np.zeros((1, memory.shape[0]), np.float32))
        dec.begin(1, 1)
        _check(f"{mode} step under an all-zero row", dec.step([int(g["prefix"][0])], 0)[0], g[f"{mode}_step_empty"], float(g[f"{mode}_gap_step_empty"]))
        dec.set_memory(memory.to(cuda), np.zeros((0, memory.shape[0]), np.float32))      # no token fired: nothing is visible either
        dec.begin(1, 1)
        _check(f"{mode} step without any mask row", dec.step([int(g["prefix"][0])], 0)[0], g[f"{mode}_step_empty"], float(g[f"{mode}_gap_step_empty"]))


@pytest.mark.parametrize("dk,H", [(64, 2), (128, 1)])
def test_scama_attention_reads_no_key_outside_the_window(cuda, dk, H):
    T, n, D = 50, 3, H * dk
    gen = torch.Generator().manual_seed(dk)
    q, kv = torch.randn(n, D, generator=gen), torch.randn(T, 2 * D, generator=gen)
    for name, row in zip(("first", "last", "one", "whole", "empty", "holes"), _windows(T)):
        nz = np.flatnonzero(row)
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        poisoned = kv.clone()
        poisoned[torch.from_numpy(row) == 0] = float("nan")
        out = torch.full((n, D), float("nan"), device=cuda)
        qd, kd, md = q.to(cuda), poisoned.to(cuda), torch.from_numpy(row).to(cuda)
        _lib.check(_lib.load().pf_k_scama_attention(qd.data_ptr(), kd.data_ptr(), T, md.data_ptr(), lo, hi, n, H, dk, out.data_ptr(), _stream()),
                   "pf_k_scama_attention")
        torch.cuda.synchronize()
        _check_oracles(f"scama attention d_k {dk} window {name}", out, O.masked_cross_attention(q.double(), kv.double(), H, row),
                       O.masked_cross_attention(q, kv, H, row))
        if name == "empty":
            assert bool((out == 0).all())


# ------------------------------------------------------------------------------------------------ stride_conv
@pytest.mark.parametrize("kernel,stride,pad", [(2, 2, [0, 1]), (3, 3, 1), (3, 2, [1, 1]), (2, 3, (0, 1))])
def test_stride_conv_against_the_oracle(cuda, kernel, stride, pad):
    conv = StrideConv(idim=208, odim=208, kernel_size=kernel, stride=stride, pad=pad)
    gen = torch.Generator().manual_seed(10 * kernel + stride)
    w, b = torch.randn(208, 208, kernel, generator=gen) * (208 * kernel) ** -0.5, 0.1 * torch.randn(208, generator=gen)
    conv.load_state_dict({"conv.weight": w, "conv.bias": b}, strict=True)
    conv.to(cuda)
    for T in (1, 7, 8, 10, 23):
        x = torch.randn(T, 208, generator=gen)
        got = conv(x[:, :80].to(cuda), x[:, 80:].to(cuda))
        assert got.shape[0] == (T - 1) // stride + 1
        _check_oracles(f"stride_conv kernel {kernel} stride {stride} pad {pad} T {T}", got, O.stride_conv(w.double(), b.double(), x.double(), stride, pad),
                       O.stride_conv(w, b, x, stride, pad))


def test_stride_conv_refuses_a_geometry_that_yields_too_few_rows(cuda):
    conv = StrideConv(idim=208, odim=208, kernel_size=3, stride=2, pad=0).to(cuda)
    with pytest.raises(ValueError, match="stride_conv"):
        conv(torch.zeros(8, 80, device=cuda), torch.zeros(8, 128, device=cuda))


# ------------------------------------------------------------------------------------------------ the model against the golden
@pytest.mark.parametrize("mode", MODES)
def test_model_against_the_references_recorded_outputs(cuda, setup, mode):
    g, m, sd64, sd32, conf = setup
    gap = lambda k: float(g[f"{mode}_gap_{k}"])                      # noqa: E731
    feats = torch.from_numpy(g["feats"])
    m.beam_search = None
    m.init_beam_search(token_list=g["tokens"].tolist(), beam_size=int(g["beam"]))
    nbest = m.recognize(feats[None].to(cuda), [feats.shape[0]], mode, int(g["relax"]))[: int(g["nbest"])]
    st = m._stages
    which = O.MODES[mode][1]
    if which == 2:
        _check(f"{mode} stride_conv", m._stride_out, g[f"{mode}_stride_conv"], gap("stride_conv"))
    _check(f"{mode} pass {which}", st["encoder_out"][0], g[f"{mode}_enc{which}"], gap(f"enc{which}"))
    _check(f"{mode} alphas", st["alphas"], g[f"{mode}_alphas"], gap("alphas"))
    # the count is an fp32 sum of n non-zero alphas: each term within the alphas' bar, each of the n - 1 additions rounded to half an
    # ulp of a partial sum that is at most the total (the recorded fp32 - fp64 gap of this ONE number can fall below a single ulp of
    # the total and is no bar); tests/test_uniasr.py keeps every cumulative sum 1e-3 away from the integer that would change a count
    n_alpha, total = int((g[f"{mode}_alphas"] > 0).sum()), float(g[f"{mode}_token_num"])
    _check(f"{mode} token count", st["token_num"], g[f"{mode}_token_num"], n_alpha * 4 * gap("alphas") + (n_alpha - 1) * 2.0 ** -24 * total, 1.0)
    assert np.array_equal(st["alignments"], g[f"{mode}_alignments"]) and np.array_equal(st["scama_mask"], g[f"{mode}_scama_mask"])
    assert len(nbest) == int(g["nbest"])
    for r, h in enumerate(nbest):
        assert h.yseq == g[f"{mode}_nbest_ids_{r}"].tolist(), (mode, r)
        d = abs(h.score - float(g[f"{mode}_nbest_score_{r}"]))
        print(f"{mode} rank {r}: |d score| {d:.3e}, gap {float(g[mode + '_gap_nbest_score']):.3e}")
        assert d <= 8 * float(g[mode + "_gap_nbest_score"]), (mode, r, d)
    # the recorded steps over the recorded memory and mask
    dec = m.decoder if which == 1 else m.decoder2
    dec.set_memory(torch.from_numpy(g[f"{mode}_enc{which}"]).float().to(cuda), g[f"{mode}_scama_mask"])
    prefix = g["prefix"].tolist()
    dec.begin(len(prefix), 1)
    for j, tok in enumerate(prefix, 1):
        _check(f"{mode} step {j}", dec.step([tok], j - 1)[0], g[f"{mode}_step_{j}"], gap(f"step_{j}"))
    m.beam_search = None


def test_pass_one_output_is_the_recorded_one(cuda, setup):
    g, m, *_ = setup
    feats = torch.from_numpy(g["feats"])
    for mode, ind in (("fast", 0), ("offline", 1)):
        _, out, olens = m.encode(feats[None].to(cuda), [feats.shape[0]], ind=ind)
        _check(f"pass 1 ind {ind}", out[0], g[f"{mode}_enc1"], float(g[f"{mode}_gap_enc1"]))


def test_automodel_end_to_end(cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.tokenizer import sentence_postprocess

    from ._model_dir import write_wav

    g = load_golden()
    sd, c, tokens = write_model_dir(str(tmp_path / "uniasr"))
    am = AutoModel(model=str(tmp_path / "uniasr"), device="cuda", disable_update=True)
    assert isinstance(am.model, UniASR)
    feats = torch.from_numpy(g["feats"])
    for mode in MODES:
        am.model.beam_search = None
        res, _ = am.model.inference(feats, data_lengths=[feats.shape[0]], key=["clip"], tokenizer=am.kwargs["tokenizer"],
                                    frontend=am.kwargs["frontend"], data_type="fbank", device="cuda", decoding_model=mode, nbest=int(g["nbest"]),
                                    beam_size=int(g["beam"]), token_num_relax=int(g["relax"]))
        assert len(res) == int(g["nbest"])
        for r, rec in enumerate(res):
            ids = [t for t in g[f"{mode}_nbest_ids_{r}"].tolist()[1:-1] if t != 0]
            assert set(rec) == {"key", "text"} and rec["key"] == "clip"
            assert rec["text"] == sentence_postprocess([tokens[t] for t in ids])[0], (mode, r)
    am.model.beam_search = None
    p = str(tmp_path / "utt0.wav")
    write_wav(p, synth.speech_like(12000, seed=3))
    res = am.generate(input=p, batch_size=1, decoding_model="offline")
    assert len(res) == 1 and set(res[0]) >= {"key", "text"} and res[0]["key"] == "utt0"
    with pytest.raises(NotImplementedError, match="batch_size"):
        am.generate(input=[p, p], batch_size=2)
