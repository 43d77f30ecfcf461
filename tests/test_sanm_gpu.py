"""SANM on the MI355X through the C ABI: the fused FSMN step kernel and the cross-attention step kernel against the float64 oracle
on random inputs, the decoder's reorder through the handle, the model against the reference's recorded float64 outputs for both
golden configurations (encoder, every recorded step, n-best), AutoModel end to end, and one template-size run.

Bars (those of tests/test_transformer_gpu.py): 4 x the reference's recorded fp32 - fp64 gap for what is computed in fp32, 8 x for
what lies downstream of the f16x2 encoder (and for n-best scores); where no recorded gap exists (random-input kernel tests, the
reorder runs, the template-size run) 4 x max |oracle fp32 - oracle fp64| -- another valid fp32 summation order may be that far off
-- with a floor of 1e-7."""
import pytest
import torch

from funasr_amd import _lib, synth
from funasr_amd.sanm import SANM

from . import _sanm_oracle as O
from ._model_dir import write_wav
from .test_sanm import CONFIGS, golden_model, golden_prefix, load_golden, write_model_dir

pytestmark = pytest.mark.gpu
FACTOR = {"fp32": 4.0, "f16x2": 8.0}
EPS = 1e-12


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _maxd(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _check(tag, got, want64, gap, factor):
    d = _maxd(got, want64)
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / max(gap, 1e-30):.2f} (bar {factor:g})")
    assert d <= factor * gap, (tag, d, gap)


# ------------------------------------------------------------------------------------------------ the FSMN step kernel
def _fsmn_kernel(cuda, t, x, g2, b2, w, win_in, win_out, parents, pos, K, left, g3, b3):
    n, D = t.shape
    x_out = torch.empty(n, D, device=cuda)
    xn_out = torch.full((n, D), float("nan"), device=cuda)
    par = None if parents is None else torch.tensor(parents, dtype=torch.int32, device=cuda)
    _lib.check(_lib.load().pf_k_fsmn_step(t.data_ptr(), x.data_ptr(), g2.data_ptr(), b2.data_ptr(), w.data_ptr(), win_in.data_ptr(),
                                          win_out.data_ptr(), None if par is None else par.data_ptr(), pos, n, D, K, left,
                                          None if g3 is None else g3.data_ptr(), None if b3 is None else b3.data_ptr(), EPS,
                                          x_out.data_ptr(), xn_out.data_ptr(), _stream()), "pf_k_fsmn_step")
    torch.cuda.synchronize()
    return x_out, xn_out


def _fsmn_run(cuda, K, shift, D, n, norm3, slots):
    """steps 0 .. K + 1 of n slots over window buffers of `slots` slots, random parents (repeats included) from step 1 on; the
    oracle runs the same on its append-only histories in float64 and float32. Compared at positions 0, 1, K - 2, K - 1, K, K + 1."""
    left, right = O.paddings(K, shift)
    assert right >= 0
    g = torch.Generator().manual_seed(1000 * K + 10 * D + n)
    g2, b2 = 1.0 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    g3, b3 = 1.0 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    w = torch.randn(D, 1, K, generator=g) * (1.0 / K) ** 0.5
    dev = [v.to(cuda) for v in (g2, b2, w, g3, b3)]
    wins = [torch.full((slots, K, D), float("nan"), device=cuda), torch.full((slots, K, D), float("nan"), device=cuda)]
    h64 = h32 = None
    at = {0, 1, K - 2, K - 1, K, K + 1}
    for pos in range(K + 2):
        t, x = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
        parents = None if pos == 0 or n == 1 else torch.randint(0, n, (n,), generator=g).tolist()
        if parents is not None:
            h64, h32 = h64[parents], h32[parents]
        x_out, xn_out = _fsmn_kernel(cuda, t.to(cuda), x.to(cuda), dev[0], dev[1], dev[2], wins[pos % 2], wins[(pos + 1) % 2], parents, pos, K,
                                     left, dev[3] if norm3 else None, dev[4] if norm3 else None)
        y64, yn64, h64 = O.fsmn_step(t.double(), x.double(), h64, g2.double(), b2.double(), w.double(), K, left,
                                     g3.double() if norm3 else None, b3.double() if norm3 else None, EPS)
        y32, yn32, h32 = O.fsmn_step(t, x, h32, g2, b2, w, K, left, g3 if norm3 else None, b3 if norm3 else None, EPS)
        if pos not in at:
            continue
        tag = f"fsmn K={K} shift={shift} (L {left}, R {right}) D={D} n={n} norm3={norm3} pos={pos}"
        _check(tag + " x", x_out, y64, max(_maxd(y32, y64), 1e-7), 4.0)
        win64 = O.fsmn_window(h64, K)
        _check(tag + " window", wins[(pos + 1) % 2][:n], win64, max(_maxd(O.fsmn_window(h32, K), win64), 1e-7), 4.0)
        if norm3:
            _check(tag + " norm3", xn_out, yn64, max(_maxd(yn32, yn64), 1e-7), 4.0)
        else:
            assert bool(torch.isnan(xn_out).all())                   # untouched without norm3
        if n < slots:
            assert bool(torch.isnan(wins[(pos + 1) % 2][n:]).all())  # no slot past n written


@pytest.mark.parametrize("K,shift", [(1, None), (1, 0), (4, None), (4, 0), (11, None), (11, 0), (11, 3), (21, None), (21, 0), (21, 3),
                                     (32, None), (32, 0), (32, 3)])
def test_fsmn_step_kernel_against_the_oracle(cuda, K, shift):
    """kernels of 1 tap, an even one, the template's, the constructor's default and the largest; the constructor's default shift
    (R = 0 for odd K), the template's 0 and 3 wherever the right padding stays >= 0; widths of one partial wave, half a workgroup and
    two elements per thread; 1, 3 and 256 (the handle's limit) running slots; with and without the norm3 output"""
    for D, n, norm3 in [(64, 1, True), (64, 3, False), (64, 256, True), (128, 1, False), (128, 3, True), (128, 256, False),
                        (512, 1, True), (512, 3, True), (512, 3, False), (512, 256, True)]:
        _fsmn_run(cuda, K, shift, D, n, norm3, slots=256 if n == 256 else 5)


def test_fsmn_step_kernel_at_the_widest_row(cuda):
    """D = 2048: all eight elements per thread; D = 2044: the last thread rows partly past the end"""
    for D in (2048, 2044):
        _fsmn_run(cuda, 11, 0, D, 3, True, slots=4)


# ------------------------------------------------------------------------------------------------ the cross-attention step kernel
@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("H", [1, 4])
def test_cross_attention_step_kernel_against_the_oracle(cuda, dk, H):
    """one key, one below / on / above the 64 lanes of a wave, several rounds; 1 and 7 queries"""
    D = H * dk
    for T in (1, 63, 64, 65, 257):
        for n in (1, 7):
            g = torch.Generator().manual_seed(T * 10 + n)
            q, kv = torch.randn(n, D, generator=g), torch.randn(T, 2 * D, generator=g)
            out = torch.empty(n, D, device=cuda)
            qd, kvd = q.to(cuda), kv.to(cuda)
            _lib.check(_lib.load().pf_k_cross_attention_step(qd.data_ptr(), kvd.data_ptr(), T, n, H, dk, out.data_ptr(), _stream()),
                       "pf_k_cross_attention_step")
            torch.cuda.synchronize()
            r64 = O.cross_attention(q.double(), kv.double(), H)
            _check(f"cross attention dk={dk} H={H} T={T} n={n}", out, r64, max(_maxd(O.cross_attention(q, kv, H), r64), 1e-7), 4.0)


# ------------------------------------------------------------------------------------------------ the handle: reorder
@pytest.fixture(scope="module")
def models(cuda):
    g = load_golden()
    out = {}
    for name in CONFIGS:
        m, sd, conf = golden_model(g, name)
        out[name] = (m.to(cuda), sd, conf)
    return g, out


# (parents or None, tokens): identity, a permutation, repeated parents, shrinking 5 -> 2, growing 2 -> 5, no reorder at all, then on
# past the kernel of both configurations
_SCRIPT = [(None, 5), ([0, 1, 2, 3, 4], 5), ([3, 0, 4, 1, 2], 5), ([2, 2, 0], 3), ([0, 1, 2, 1, 0], 5), ([4, 1], 2), ([1, 0, 1, 0, 1], 5),
           (None, 5), ([4, 4, 4, 4, 4], 5), ([0, 2], 2), (None, 2), ([1, 1, 0, 0, 1], 5), ([2, 3, 4, 0, 1], 5), (None, 5)]


def _scripted_run(stepper, g, n_vocab):
    gen = torch.Generator().manual_seed(9)
    outs = []
    stepper.begin(len(_SCRIPT), 5)
    for pos, (parents, n) in enumerate(_SCRIPT):
        if parents is not None:
            stepper.reorder(parents)
        tokens = [1] * n if pos == 0 else torch.randint(3, n_vocab - 1, (n,), generator=gen).tolist()
        outs.append(torch.as_tensor(stepper.step(tokens, pos)).detach().cpu())
    return outs


@pytest.mark.parametrize("name", ["A", "B"])
def test_reorder_then_step_against_the_oracle_on_the_reordered_histories(cuda, models, name):
    g, ms = models
    m, sd, conf = ms[name]
    memory = torch.from_numpy(g[f"{name}_enc_1"]).float()
    V = len(g["tokens"])
    got = _scripted_run(m.decoder.set_memory(memory.to(cuda)), g, V)
    r64 = _scripted_run(O.FsmnStepper(O.cast(sd), conf["decoder_conf"], memory.double()), g, V)
    r32 = _scripted_run(O.FsmnStepper(O.cast(sd, torch.float32), conf["decoder_conf"], memory), g, V)
    for pos, (parents, n) in enumerate(_SCRIPT):
        assert got[pos].shape == (n, V)
        _check(f"{name} pos {pos} parents {parents}", got[pos], r64[pos], max(_maxd(r32[pos], r64[pos]), 1e-7), 4.0)
    again = _scripted_run(m.decoder.set_memory(memory.to(cuda)), g, V)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_the_handle_refuses_what_its_state_cannot_serve(cuda, models):
    g, ms = models
    dec = ms["B"][0].decoder.set_memory(torch.from_numpy(g["B_enc_1"]).float().to(cuda))
    dec.begin(4, 3)
    with pytest.raises(_lib.HipRuntimeError, match="in order"):
        dec.step([1], 1)                                             # position 0 first
    dec.step([1, 1], 0)
    with pytest.raises(_lib.HipRuntimeError, match="in order"):
        dec.step([1, 1], 0)                                          # every position once
    with pytest.raises(_lib.HipRuntimeError, match="did not run"):
        dec.reorder([0, 2])                                          # slot 2 held no hypothesis at position 0
    with pytest.raises(_lib.HipRuntimeError, match="without a parent"):
        dec.step([3, 4, 5], 1)                                       # three slots, two parents, no reorder
    dec.reorder([1, 1, 0])
    with pytest.raises(_lib.HipRuntimeError, match="last reorder"):
        dec.step([3, 4], 1)
    with pytest.raises(_lib.HipRuntimeError, match="max_hyp"):
        dec.step([3, 4, 5, 6], 1)
    with pytest.raises(_lib.HipRuntimeError, match="vocabulary"):
        dec.step([3, 4, len(g["tokens"])], 1)
    assert bool(torch.isfinite(dec.step([3, 4, 5], 1)).all())
    with pytest.raises(ValueError, match="257 hypotheses"):
        dec.begin(4, 257)
    with pytest.raises(ValueError, match="5001 output positions"):
        dec.begin(5001, 3)


# ------------------------------------------------------------------------------------------------ model against the golden
def _modes(m):
    if m.encoder._default_precision() == "f16x2":
        return ["fp32", "f16x2"]
    print("the encoder's f16x2 kernels do not cover this width (d_k 64): fp32 only")
    with pytest.raises(NotImplementedError, match="f16x2"):
        m.set_precision("f16x2")
    return ["fp32"]


@pytest.mark.parametrize("name", ["A", "B"])
def test_model_against_the_references_recorded_outputs(cuda, models, name):
    g, ms = models
    m, sd, conf = ms[name]
    lens = [int(n) for n in g["lens"]]
    feats = [torch.from_numpy(g[f"feats_{i}"]) for i in range(len(lens))]
    for mode in _modes(m):
        m.set_precision(mode)
        for i, f in enumerate(feats):
            enc, olens = m.encode(f[None].to(cuda), [lens[i]])
            assert olens.tolist() == [lens[i]] and enc.shape[1] == lens[i]
            _check(f"{name} {mode} enc {i}", enc[0], g[f"{name}_enc_{i}"], float(g[f"{name}_gap_enc_{i}"]), FACTOR[mode])
            if m.ctc is not None:
                _check(f"{name} {mode} ctc {i}", m.ctc.log_softmax(enc)[0], g[f"{name}_ctc_{i}"], float(g[f"{name}_gap_ctc_{i}"]), FACTOR[mode])
                assert m.ctc_greedy(enc, olens)[0] == g[f"{name}_greedy_{i}"].tolist()
        # the ragged batch of the two: a clip's frames are what they are alone (the encoder masks by length)
        pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
        enc, olens = m.encode(pad.to(cuda), lens)
        assert olens.tolist() == lens
        for i, n in enumerate(lens):
            _check(f"{name} {mode} batch enc {i}", enc[i, :n], g[f"{name}_enc_{i}"], float(g[f"{name}_gap_enc_{i}"]), FACTOR[mode])
    # the recorded steps over the recorded memory: exact fp32 in every mode
    dec = m.decoder.set_memory(torch.from_numpy(g[f"{name}_enc_1"]).float().to(cuda))
    for n in g[f"{name}_prefix_lengths"].tolist():
        got = O.score_prefix(dec, golden_prefix(g, n))
        _check(f"{name} step after {n} tokens", got, g[f"{name}_step_{n}"], float(g[f"{name}_gap_step_{n}"]), 4.0)


@pytest.mark.parametrize("name", ["A", "B"])
def test_beam_search_nbest_equals_the_references(cuda, models, name):
    g, ms = models
    m, sd, conf = ms[name]
    f = torch.from_numpy(g["feats_0"])
    for mode in _modes(m):
        m.set_precision(mode)
        enc, _ = m.encode(f[None].to(cuda), [f.shape[0]])
        for w in g[f"{name}_ctc_weights"].tolist():
            m.beam_search = None
            m.init_beam_search(token_list=g["tokens"].tolist(), decoding_ctc_weight=w, beam_size=int(g["beam"]))
            nbest = m.beam_search_features(enc[0])[: int(g["nbest"])]
            assert len(nbest) == int(g["nbest"])
            for r, h in enumerate(nbest):
                assert h.yseq == g[f"{name}_nbest_ids_w{w}_{r}"].tolist(), (name, mode, w, r)
                d = abs(h.score - float(g[f"{name}_nbest_score_w{w}_{r}"]))
                print(f"{name} {mode} w={w} rank {r}: |d score| {d:.3e}, gap {float(g[name + '_gap_nbest_score']):.3e}")
                assert d <= 8 * float(g[name + "_gap_nbest_score"]), (name, mode, w, r, d)
    m.beam_search = None
    m.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ AutoModel
def test_automodel_end_to_end(cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel
    from funasr_amd.tokenizer import sentence_postprocess
    from oracle import paraformer_oracle as PO

    from ._conformer_oracle import ctc_greedy, ctc_log_softmax

    sd, c, tokens = write_model_dir(str(tmp_path / "sanm_a"), "A")
    wavs = []
    for i, n in enumerate((16000, 27001, 21503)):
        p = str(tmp_path / f"utt{i}.wav")
        write_wav(p, synth.speech_like(n, seed=20 + i))
        wavs.append(p)
    am = AutoModel(model=str(tmp_path / "sanm_a"), device="cuda", disable_update=True)
    assert isinstance(am.model, SANM)
    res = am.generate(input=wavs[0], batch_size=1, beam_size=5, decoding_ctc_weight=0.3, nbest=2, maxlenratio=-12)
    assert len(res) == 2 and set(res[0]) >= {"key", "token", "text"} and res[0]["key"] == "utt0"
    res = am.generate(input=wavs, batch_size=3)
    assert [r["key"] for r in res] == ["utt0", "utt1", "utt2"] and all(set(r) >= {"key", "text"} and "token" not in r for r in res)
    # what the oracle decodes from the same feature batch with the true lengths
    from funasr_amd.audio import batch_to_features
    speech, lens, _ = batch_to_features(wavs, None, am.kwargs["frontend"], dict(am.kwargs, device="cuda"))
    lens = torch.as_tensor([int(v) for v in lens.tolist()])
    sd64 = O.cast(sd)
    enc_sd = {k[len("encoder."):]: v for k, v in sd64.items() if k.startswith("encoder.")}
    enc, olens = PO.sanm_encoder(speech.double().cpu(), lens, enc_sd, c["encoder_conf"])
    lp = ctc_log_softmax(sd64, enc)
    for b, r in enumerate(res):
        want, _ = sentence_postprocess([tokens[t] for t in ctc_greedy(lp[b], int(olens[b]))])
        assert r["text"] == want, b
    # without a CTC head: the beam search runs with the decoder alone, the batched route has nothing to decode
    write_model_dir(str(tmp_path / "sanm_b"), "B")
    bm = AutoModel(model=str(tmp_path / "sanm_b"), device="cuda", disable_update=True)
    res = bm.generate(input=wavs[0], batch_size=1, beam_size=5, nbest=1, maxlenratio=-12)
    assert len(res) == 1 and set(res[0]) >= {"key", "token", "text"}
    with pytest.raises(RuntimeError, match="this model has none"):
        bm.generate(input=wavs, batch_size=3)


# ------------------------------------------------------------------------------------------------ one template-size run
def test_template_size_10_seconds_beam_10(cuda):
    """SANM_TEMPLATE (D 512, d_k 128, FFN 2048, 50 + 16 blocks, kernel 11 with sanm_shfit 0, no CTC head, 8404 tokens): a 10 s clip
    (167 LFR frames), beam 10, 20 positions. Finite, the whole search bitwise repeatable, and the step after the best hypothesis'
    20 tokens within bar of the oracle's over the same memory."""
    conf = synth.sanm_conf(**synth.SANM_TEMPLATE)
    m = SANM(**conf)
    sd = synth.sanm_state_dict(13, m)
    m.load_state_dict(sd, strict=True)
    m = m.to(cuda)
    feats = torch.randn(1, 167, 560, generator=torch.Generator().manual_seed(2))
    enc, olens = m.encode(feats.to(cuda), [167])
    assert olens.tolist() == [167] and bool(torch.isfinite(enc).all())
    m.init_beam_search(decoding_ctc_weight=0.0, beam_size=10)
    a = m.beam_search_features(enc[0], maxlenratio=-20)
    b = m.beam_search_features(enc[0], maxlenratio=-20)
    assert len(a) >= 1 and [h.yseq for h in a] == [h.yseq for h in b] and [h.score for h in a] == [h.score for h in b]
    assert all(torch.isfinite(torch.tensor(h.score)) for h in a) and len(a[0].yseq) <= 22      # <sos>, at most 20 tokens, <eos>
    pre = a[0].yseq[:-1][:20]                                        # what the last position's step had behind it
    memory = enc[0].cpu()
    dsd = {k: v for k, v in sd.items() if k.startswith("decoder.")}
    got = O.score_prefix(m.decoder.set_memory(enc[0]), pre)
    r64 = O.score_prefix(O.FsmnStepper(O.cast(dsd), conf["decoder_conf"], memory.double()), pre)
    r32 = O.score_prefix(O.FsmnStepper(O.cast(dsd, torch.float32), conf["decoder_conf"], memory), pre)
    assert bool(torch.isfinite(got).all())
    _check(f"template step after {len(pre)} tokens", got, r64, max(_maxd(r32, r64), 1e-7), 4.0)
