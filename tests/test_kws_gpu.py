"""Keyword spotting on the GPU: the FSMN memory block with a right context and the candidate kernel at their edges against the
float64 restatement (tests/_kws_oracle.py), the two networks' logits, both models end to end on the golden batches of the
reference's own classes (tests/golden/kws.npz, tools/make_golden_kws.py), and AutoModel from a synthetic model directory.

Bars: a kernel is within 4 x the fp32 restatement's own distance from float64 (the project's kernel bar); ids and counts are exact
wherever the decision's margin exceeds that distance; end-to-end scores are within 8 x gap_score."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import _lib, synth
from tests import _kws_oracle as KO

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "kws.npz"), allow_pickle=False)


# ------------------------------------------------------------------------------------------------------ memory block
def _block(cuda, x, wl, wr, ls, rs):
    lib = _lib.load()
    B, T, Cc = x.shape
    xd, y = x.to(cuda).contiguous(), torch.full((B, T, Cc), float("nan"), device=cuda)
    wld = wl.to(cuda).contiguous()
    wrd = wr.to(cuda).contiguous() if wr is not None else None
    _lib.check(lib.pf_k_kws_fsmn(xd.data_ptr(), Cc, wld.data_ptr(), wrd.data_ptr() if wrd is not None else None, y.data_ptr(), Cc, B, T, Cc,
                                 wl.shape[1], ls, 0 if wr is None else wr.shape[1], rs, torch.cuda.current_stream().cuda_stream), "pf_k_kws_fsmn")
    return y.cpu()


BLOCK_CASES = [  # (B, T, C, lorder, lstride, rorder, rstride)
    (3, 1, 4, 4, 1, 2, 1),          # T = 1: only the centre taps
    (3, 2, 16, 4, 1, 2, 1),         # T <= rorder * rstride
    (2, 3, 16, 4, 2, 2, 2),         # T <= rorder * rstride at stride 2, and T = lorder - 1
    (3, 3, 128, 4, 1, 2, 1),        # T = lorder - 1
    (3, 19, 16, 4, 1, 2, 1),        # more than one block of 8 frames, not a multiple of it
    (3, 21, 128, 10, 1, 2, 1),      # the recipe's orders
    (2, 37, 16, 4, 2, 2, 2),        # strides 2
    (1, 9, 4, 3, 2, 3, 1),
]


@pytest.mark.parametrize("B,T,Cc,L,LS,R,RS", BLOCK_CASES)
def test_memory_block_against_float64(cuda, B, T, Cc, L, LS, R, RS):
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + Cc)
    x, wl, wr = torch.randn(B, T, Cc, generator=g), 0.5 * torch.randn(Cc, L, generator=g), 0.5 * torch.randn(Cc, R, generator=g)
    want = KO.memory_block(x.double(), wl.double(), wr.double(), LS, RS)
    gap = float((KO.memory_block(x, wl, wr, LS, RS).double() - want).abs().max())
    got = _block(cuda, x, wl, wr, LS, RS)
    err = float((got.double() - want).abs().max())
    print(f"memory block B{B} T{T} C{Cc} L{L}x{LS} R{R}x{RS}: err {err:.3e} gap {gap:.3e}")
    assert not torch.isnan(got).any() and err <= 4 * gap
    # the rows of different clips do not mix: every clip alone gives the same bits
    for b in range(B):
        assert torch.equal(_block(cuda, x[b: b + 1], wl, wr, LS, RS)[0], got[b])


@pytest.mark.parametrize("B,T,Cc,L,LS", [(3, 1, 4, 4, 1), (2, 19, 16, 4, 2), (3, 37, 128, 20, 1)])
def test_memory_block_without_right_context_is_the_left_only_block_bitwise(cuda, B, T, Cc, L, LS):
    lib = _lib.load()
    g = torch.Generator().manual_seed(T)
    x, wl = torch.randn(B, T, Cc, generator=g), 0.5 * torch.randn(Cc, L, generator=g)
    got = _block(cuda, x, wl, None, LS, 1)
    xd, wld, y = x.to(cuda), wl.to(cuda), torch.empty(B, T, Cc, device=cuda)
    _lib.check(lib.pf_k_vad_fsmn(xd.data_ptr(), Cc, wld.data_ptr(), y.data_ptr(), Cc, B, T, Cc, L, LS, torch.cuda.current_stream().cuda_stream),
               "pf_k_vad_fsmn")
    assert torch.equal(got, y.cpu())


# ------------------------------------------------------------------------------------------------------ candidate kernel
def _mask(V, token_set, cuda):
    m = np.zeros((V + 31) // 32, np.uint32)
    for i in token_set:
        m[i >> 5] |= np.uint32(1 << (i & 31))
    return torch.from_numpy(m.view(np.int32)).to(cuda)


def _cand(cuda, logits, token_set, out=None):
    lib = _lib.load()
    M, V = logits.shape
    x = logits.to(cuda).contiguous()
    out = torch.empty(M, 7, device=cuda, dtype=torch.int32) if out is None else out
    rc = lib.pf_kws_candidates(x.data_ptr(), V, M, V, _mask(V, token_set, cuda).data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "pf_kws_candidates")
    o = out.cpu().numpy()
    return o[:, 0], o[:, 1:4], np.ascontiguousarray(o[:, 4:7]).view(np.float32)


def _check_candidates(cuda, logits, token_set, what):
    n, ids, ps = _cand(cuda, logits, token_set)
    n64, i64, p64 = KO.candidates(logits.double(), token_set)
    full64, full32 = torch.softmax(logits.double(), -1), torch.softmax(logits, -1)
    gap = float((full64 - full32.double()).abs().max())                      # the fp32 softmax's own distance from float64
    order = torch.sort(logits, dim=-1, descending=True, stable=True)[1][:, :3]
    worst = 0.0
    for r in range(logits.shape[0]):
        top_p = [float(full64[r, int(i)]) for i in order[r]]
        clear = all(abs(p - 0.05) > 4 * gap or int(i) not in token_set or not np.isfinite(p) for p, i in zip(top_p, order[r]))
        if clear:                                                            # every p > 0.05 decision of this row has a margin
            assert int(n[r]) == int(n64[r]) and ids[r].tolist() == i64[r].tolist(), (what, r, n[r], ids[r], i64[r])
            worst = max(worst, float(np.abs(ps[r].astype(np.float64) - p64[r].numpy()).max()))
        assert (ids[r, int(n[r]):] == -1).all() and (ps[r, int(n[r]):] == 0).all()
    print(f"candidates {what}: M {logits.shape[0]} V {logits.shape[1]} kept {int(n.sum())} err {worst:.3e} gap {gap:.3e}")
    assert worst <= 4 * gap
    return n, ids, ps


@pytest.mark.parametrize("V", [3, 63, 64, 65, 2599, 65536])
@pytest.mark.parametrize("M", [1, 4, 5])
def test_candidates_against_float64(cuda, V, M):
    g = torch.Generator().manual_seed(V + M)
    logits = torch.randn(M, V, generator=g) * (3.0 if V > 100 else 1.5)
    token_set = {0} | set(torch.randperm(V, generator=g)[: max(1, V // 2)].tolist())
    _check_candidates(cuda, logits, token_set, "random")


def test_candidates_edges(cuda):
    V = 65
    every = set(range(V))
    x = torch.zeros(6, V)
    x[0, [7, 3, 64]] = 2.0                                                   # equal logits: the lower index first
    x[1, 10], x[1, 40], x[1, 41], x[1, 5] = 3.0, 2.5, 2.5, 2.5               # three equal behind the first: 5 and 40 make it, 41 does not
    x[2] = float("-inf")
    x[2, [64, 0, 33]] = torch.tensor([1.0, 0.5, 0.25])                       # -inf entries
    x[3] = 1e4 + torch.linspace(0, 3, V)                                     # logits around 1e4
    x[4, 20], x[4, 21] = 5.0, 4.0                                            # row 4 is read with an empty keyword set below
    x[5] = float("-inf")
    x[5, 9] = 0.0                                                            # one finite entry: p = 1, the -inf entries are never kept
    n, ids, ps = _check_candidates(cuda, x, every, "edges")
    assert ids[0].tolist() == [3, 7, 64] and ids[1].tolist() == [10, 5, 40]
    assert ids[2].tolist() == [64, 0, 33] and n[5] == 1 and ids[5, 0] == 9 and ps[5, 0] == 1.0
    n, ids, _ = _check_candidates(cuda, x, {0}, "blank only")               # an empty keyword set beyond blank
    assert n[4] == 0 and n[2] == 1 and ids[2, 0] == 0
    u = torch.full((5, 64), 0.7)                                             # uniform rows: p = 1 / 64 < 0.05 everywhere
    n, ids, ps = _check_candidates(cuda, u, set(range(64)), "uniform")
    assert (n == 0).all() and (ids == -1).all() and (ps == 0).all()
    n, ids, ps = _check_candidates(cuda, torch.full((1, 3), -2.0), {0, 1, 2}, "uniform V=3")
    assert n[0] == 3 and ids[0].tolist() == [0, 1, 2]


def test_candidates_write_every_slot(cuda):
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(5, 131, generator=g) * 3
    first = _cand(cuda, logits, {0, 5, 9, 77})
    poisoned = torch.full((5, 7), 0x7F7F7F7F, device=cuda, dtype=torch.int32)
    second = _cand(cuda, logits, {0, 5, 9, 77}, out=poisoned)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert not (poisoned.cpu().numpy() == 0x7F7F7F7F).any()


def test_candidates_refuse_fewer_than_three_columns(cuda):
    lib = _lib.load()
    x, out = torch.zeros(2, 2, device=cuda), torch.empty(2, 7, device=cuda, dtype=torch.int32)
    assert lib.pf_kws_candidates(x.data_ptr(), 2, 2, 2, _mask(2, {0}, cuda).data_ptr(), out.data_ptr(), None) != 0
    assert "V < 3" in _lib.last_error()


# ------------------------------------------------------------------------------------------------------ networks
def _tokens(gold):
    return [str(t) for t in gold["tokens"]]


class _Tok:
    seg_dict = None

    def __init__(self, token_list):
        self.token_list = token_list


META = json.load(open(os.path.join(GOLD, "kws.json"), encoding="utf-8"))     # the tiny models' settings, as the golden tool used them


def _model(gold, m, cuda):
    from funasr_amd.kws import FsmnKWS, SanmKWS
    spec = META["models"][m]
    conf = (synth.kws_fsmn_conf if spec["kind"] == "fsmn" else synth.kws_sanm_conf)(vocab=len(META["tokens"]), **spec["conf"])
    model = (FsmnKWS if spec["kind"] == "fsmn" else SanmKWS)(**conf)
    sd = synth.kws_state_dict(int(gold[f"{m}_seed"]), model, planted=META["planted"], **spec["plant"])
    model.load_state_dict(sd, strict=True)
    return model.to(cuda).eval(), conf, sd


def test_fsmn_logits_at_the_recipe_size_past_512_outputs(cuda):
    from funasr_amd.fsmn_vad import FSMN
    conf = synth.kws_fsmn_conf(**synth.KWS_FSMN_RECIPE)["encoder_conf"]
    assert conf["output_dim"] == 2599 and conf["rorder"] == 2
    enc = FSMN(**conf)
    sd = {k[len("encoder."):]: v for k, v in synth.kws_state_dict(4, torch.nn.ModuleDict({"encoder": enc}), planted=(5, 9)).items()}
    enc.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(2, 37, conf["input_dim"], generator=g)
    want = KO.fsmn_logits(KO.cast(sd, torch.float64), conf, feats.double())
    gap = float((KO.fsmn_logits(sd, conf, feats).double() - want).abs().max())
    got = enc.to(cuda)(feats.to(cuda)).cpu()
    assert got.shape == (2, 37, 2599)
    err = float((got.double() - want).abs().max())
    print(f"fsmn recipe logits: err {err:.3e} gap {gap:.3e}")
    assert err <= 4 * gap
    with pytest.raises(ValueError, match="cache"):
        enc.logits(feats[:1].to(cuda), cache={})


@pytest.mark.parametrize("m", ["fsmn", "fsmn2", "sanm"])
def test_models_on_the_golden_batches(cuda, gold, m):
    from funasr_amd.kws_utils import KwsCtcPrefixDecoder
    model, conf, _ = _model(gold, m, cuda)
    lens = [int(v) for v in gold["lens"]]
    feats = torch.from_numpy(gold[f"{m}_feats"]).to(cuda)
    dec = KwsCtcPrefixDecoder(model.ctc, str(gold["model_keywords"]), _tokens(gold), None)
    logits, olens = model._logits(feats, lens)
    want = torch.from_numpy(gold[f"{m}_logits"])
    gap = float(gold[f"gap_logits_{m}"])
    rows = torch.zeros(want.shape[:2], dtype=torch.bool)
    for b, n in enumerate(lens):
        rows[b, : (n if m == "sanm" else want.shape[1])] = True            # the FSMN computes every row of the padded batch
    err = float((logits.cpu().double() - want)[rows].abs().max())
    print(f"{m} logits: err {err:.3e} gap {gap:.3e}")
    assert olens == lens and err <= 4 * gap
    names = dec.keywords

    def check(results, nbest_of, tag_of):
        for i, (hit, kw, score) in enumerate(results):
            tag = tag_of(i)
            w = int(gold[f"{tag}_hit"])
            assert hit == (w >= 0) and kw == (names[w] if w >= 0 else None), (tag, hit, kw, w)
            if hit:
                assert abs(score - float(gold[f"{tag}_score"])) <= 8 * float(gold["gap_score"]), (tag, score, float(gold[f"{tag}_score"]))
            nb = nbest_of(i)
            ln = gold[f"{tag}_nbest_len"]
            assert [list(h["prefix"]) for h in nb] == [gold[f"{tag}_nbest_prefix"][j, : ln[j]].tolist() for j in range(len(ln))], tag
            assert [[nd["frame"] for nd in h["nodes"]] for h in nb] == [gold[f"{tag}_node_frame"][j, : ln[j]].tolist() for j in range(len(ln))], tag
            assert [[nd["token"] for nd in h["nodes"]] for h in nb] == [gold[f"{tag}_node_token"][j, : ln[j]].tolist() for j in range(len(ln))], tag

    check(model.detect(feats, lens, dec), lambda i: dec.search.nbest(i), lambda i: f"{m}_c{i}")
    # every clip alone: for the FSMN the last frames of a shorter clip no longer see the padding behind it, in the reference too
    for i, n in enumerate(lens):
        check(model.detect(feats[i: i + 1, :n], [n], dec), lambda _: dec.search.nbest(0),
              lambda _: f"{m}_alone{i}" if m != "sanm" else f"{m}_c{i}")      # (the SAN-M encoder masks by length: alone is the batch)
    if m != "sanm":
        i = int(np.argmin(lens))
        assert np.abs(gold[f"{m}_logits"][i, : lens[i]] - gold[f"{m}_alone{i}_logits"]).max() > 1e-3


def test_inference_records_fbank_input_and_refusals(cuda, gold, tmp_path):
    model, conf, _ = _model(gold, "fsmn", cuda)
    lens = [int(v) for v in gold["lens"]]
    feats = torch.from_numpy(gold["fsmn_feats"])
    tok = _Tok(_tokens(gold))
    keys = [f"clip{i}" for i in range(len(lens))]
    res, _ = model.inference(feats, data_lengths=torch.tensor(lens), key=keys, tokenizer=tok, data_type="fbank", device=str(cuda),
                             keywords=str(gold["model_keywords"]), output_dir=str(tmp_path))
    names = str(gold["model_keywords"]).split(",")
    for i, r in enumerate(res):
        assert set(r) == {"key", "text"} and r["key"] == keys[i]
        w = int(gold[f"fsmn_c{i}_hit"])
        if w < 0:
            assert r["text"] == "rejected"
        else:
            head, kw, score = r["text"].split(" ")
            assert head == "detected" and kw == names[w] and score == str(float(score))
            assert abs(float(score) - float(gold[f"fsmn_c{i}_score"])) <= 8 * float(gold["gap_score"])
    written = dict(ln.rstrip("\n").split(" ", 1) for ln in open(os.path.join(str(tmp_path), "detect"), encoding="utf-8"))
    assert written == {r["key"]: r["text"] for r in res}
    with pytest.raises(ValueError, match="keywords"):
        model.inference(feats, data_lengths=torch.tensor(lens), key=keys, tokenizer=tok, data_type="fbank", device=str(cuda))
    with pytest.raises(NotImplementedError, match="bf16"):
        model.inference(feats, data_lengths=torch.tensor(lens), key=keys, tokenizer=tok, data_type="fbank", device=str(cuda),
                        keywords="a", bf16=True)


def test_auto_model_from_a_model_directory(cuda, gold, tmp_path):
    import yaml
    from funasr_amd.auto_model import AutoModel
    from tests._model_dir import write_wav
    class MG:
        TOKENS, PLANTED, MODELS = META["tokens"], META["planted"], META["models"]

    d = str(tmp_path / "kws")
    os.makedirs(d)
    conf = synth.kws_fsmn_conf(vocab=len(MG.TOKENS))
    from funasr_amd.kws import FsmnKWS
    sd = synth.kws_state_dict(int(gold["fsmn_seed"]), FsmnKWS(**conf), planted=MG.PLANTED, **MG.MODELS["fsmn"]["plant"])
    yaml.safe_dump({"model": "FsmnKWS", "model_conf": {"ctc_weight": 1.0}, "encoder": "FSMN", "encoder_conf": conf["encoder_conf"],
                    "ctc_conf": conf["ctc_conf"], "frontend": "WavFrontend",
                    "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 40, "frame_length": 25, "frame_shift": 10, "lfr_m": 1, "lfr_n": 1},
                    "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}},
                   open(os.path.join(d, "config.yaml"), "w", encoding="utf-8"), allow_unicode=True)
    torch.save(sd, os.path.join(d, "model.pt"))
    json.dump(MG.TOKENS, open(os.path.join(d, "tokens.json"), "w", encoding="utf-8"), ensure_ascii=False)
    g = torch.Generator().manual_seed(11)
    wavs = []
    for i, n in enumerate((9000, 14500, 4000)):
        p = os.path.join(str(tmp_path), f"w{i}.wav")
        write_wav(p, 0.3 * torch.randn(n, generator=g))
        wavs.append(p)
    am = AutoModel(model=d, device=str(cuda), keywords=str(gold["model_keywords"]), disable_update=True)
    out_dir = str(tmp_path / "out")
    res = am.generate(input=wavs, batch_size=3, output_dir=out_dir)
    assert [r["key"] for r in res] == ["w0", "w1", "w2"]
    # the same through the parts: frontend features of the padded batch, the float64 restatement, the oracle search
    fe, tok = am.kwargs["frontend"], am.kwargs["tokenizer"]
    assert tok.seg_dict is None
    from funasr_amd.audio import batch_to_features
    speech, slens, _ = batch_to_features(wavs, None, fe, {"device": str(cuda)})
    speech = speech.clone()
    for b, n in enumerate(slens.tolist()):
        speech[b, n:] = 0
    logits = KO.fsmn_logits(KO.cast(sd, torch.float64), conf["encoder_conf"], speech.cpu().double(), prefix="encoder.")
    from funasr_amd.kws_utils import parse_keywords
    table, idxset = parse_keywords(str(gold["model_keywords"]), MG.TOKENS, None)
    for b, n in enumerate(slens.tolist()):
        nn, ids, ps = KO.candidates(logits[b, :n], idxset)
        w, _, score = KO.decide(KO.beam_search(nn, ids, ps.float().double()), list(table.values()))
        if w < 0:
            assert res[b]["text"] == "rejected"
        else:
            head, kw, sc = res[b]["text"].split(" ")
            # a hit score is the root of a product of one or two posteriors of order 1; the fp32 network's logits are within 1e-5 of
            # float64 at this size (gap_logits_fsmn of the goldens), so the score moves by a few 1e-6: 1e-4 is two decades of room
            assert (head, kw) == ("detected", list(table)[w]) and abs(float(sc) - score) < 1e-4
    assert len(open(os.path.join(out_dir, "detect"), encoding="utf-8").read().splitlines()) == 3
    # keywords at call time override the constructor's; none at all is an error that names them
    res2 = am.generate(input=wavs[:1], keywords=MG.TOKENS[40])
    assert res2[0]["text"] == "rejected" or res2[0]["text"].startswith("detected " + MG.TOKENS[40])
    am2 = AutoModel(model=d, device=str(cuda), disable_update=True)
    with pytest.raises(ValueError, match="keywords"):
        am2.generate(input=wavs[:1])
