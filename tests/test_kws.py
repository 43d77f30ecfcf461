"""Keyword spotting without a GPU: registry and state-dict keys against the reference's recipes, keyword parsing against outputs
recorded from the reference's functions, the float64 restatement (tests/_kws_oracle.py) and the library's host search
(`pf_kws_search`) against the goldens of the reference's own KwsCtcPrefixDecoder (tests/golden/kws.npz / kws.json,
tools/make_golden_kws.py), and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import _lib, synth
from funasr_amd.kws_utils import KwsCtcPrefixDecoder, KwsSearch, pack_candidates, parse_keywords, query_token_set, split_mixed_label
from tests import _kws_oracle as KO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "kws.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def meta():
    return json.load(open(os.path.join(GOLD, "kws.json"), encoding="utf-8"))


def _clips(gold):
    """(name, keyword string) of every recorded clip"""
    names = []
    for m in [str(v) for v in gold["models"]]:
        for i in range(len(gold["lens"])):
            names += [(f"{m}_c{i}", str(gold["model_keywords"]))]
            if f"{m}_alone{i}_hit" in gold.files:                     # the FSMN models: every clip alone too
                names += [(f"{m}_alone{i}", str(gold["model_keywords"]))]
    return names + [(f"search{j}", str(gold["keywords"])) for j in range(int(gold["n_search"]))]


def _keyword_ids(gold, keywords):
    table, idxset = parse_keywords(keywords, [str(t) for t in gold["tokens"]], None)
    return table, idxset


# ------------------------------------------------------------------------------------------------------ registry, keys
def test_registered_and_state_dict_keys_match_the_recipes(meta):
    from funasr_amd import auto_model  # noqa: F401  (imports register everything AutoModel knows)
    from funasr_amd.register import tables
    assert "FsmnKWS" in tables.model_classes and "SanmKWS" in tables.model_classes
    for name, rec in meta["recipes"].items():
        extra = {"input_size": rec["input_size"]} if "input_size" in rec else {}
        model = tables.model_classes[rec["model"]](encoder=rec["encoder"], encoder_conf=rec["encoder_conf"], ctc_conf=rec["ctc_conf"],
                                                   vocab_size=rec["vocab_size"], **rec["model_conf"], **extra)
        mine = {k: list(v.shape) for k, v in model.state_dict().items()}
        assert mine == rec["shapes"], (name, sorted(set(mine) ^ set(rec["shapes"])))
        model.load_state_dict({k: torch.zeros(s) for k, s in rec["shapes"].items()}, strict=True)
    assert any(k.endswith("fsmn_block.conv_right.weight") for k in meta["recipes"]["fsmn_4e_l10r2_250_128_fdim80_t2599"]["shapes"])


def test_fsmn_encoder_accepts_the_kws_configuration():
    from funasr_amd.fsmn_vad import FSMN
    conf = synth.kws_fsmn_conf()["encoder_conf"]
    enc = FSMN(**conf)
    assert not enc.use_softmax and enc.fsmn[0].fsmn_block.conv_right.weight.shape == (16, 1, 2, 1)
    assert not hasattr(FSMN(**dict(conf, rorder=0, use_softmax=True)).fsmn[0].fsmn_block, "conv_right")
    with pytest.raises(NotImplementedError, match="use_softmax"):
        FSMN(**dict(conf, output_dim=2599, use_softmax=True))
    with pytest.raises(ValueError, match="cache"):                    # refused before any device work
        enc.logits(torch.zeros(1, 4, 40), cache={})


# ------------------------------------------------------------------------------------------------------ keyword parsing
def test_keyword_parsing_against_the_recorded_outputs(meta):
    table = {t: i for i, t in enumerate(meta["tokens"])}
    assert len(meta["parse"]) >= 12
    for rec in meta["parse"]:
        assert split_mixed_label(rec["txt"]) == rec["split"], rec["txt"]
        strs, idx = query_token_set(rec["txt"], table, meta["seg_dict"])
        assert list(strs) == rec["tokens_str"] and list(idx) == rec["tokens_idx"], rec["txt"]
    d = meta["decoder"]
    got, idxset = parse_keywords(d["keywords"], meta["tokens"], meta["seg_dict"])
    assert {k: list(v) for k, v in got.items()} == d["table"] and list(got) == list(d["table"])    # repeated keywords collapse, order kept
    assert sorted(idxset) == d["idxset"] and 0 in idxset
    # a missing lexicon is an empty one
    assert query_token_set("world", table, None) == query_token_set("world", table, {})


def test_char_tokenizer_seg_dict(tmp_path):
    from funasr_amd.tokenizer import CharTokenizer
    assert CharTokenizer(token_list=["a", "b"]).seg_dict is None
    p = tmp_path / "seg_dict"
    p.write_text("world wor@@ ld\nhello hello\n", encoding="utf-8")
    assert CharTokenizer(token_list=["a"], seg_dict=str(p)).seg_dict == {"world": "wor@@ ld", "hello": "hello"}
    assert CharTokenizer(token_list=["a"], seg_dict_file=str(p)).seg_dict["hello"] == "hello"


# ------------------------------------------------------------------------------------------------------ oracle and library search
def test_goldens_cover_what_they_must(gold):
    names = [n for n, _ in _clips(gold)]
    hit = {n: (int(gold[f"{n}_hit"]), int(gold[f"{n}_offset"])) for n in names}
    assert any(h == (0, 0) for h in hit.values())
    assert any(w == 1 and off > 0 for w, off in hit.values())
    assert any(hit[n][0] < 0 and gold[f"{n}_nbest_len"][0] > 0 for n in names)
    assert any(gold[f"{n}_cand"][:, 0].sum() == 0 for n in names)
    assert any(int(gold[f"{n}_max_hyps"]) > 20 for n in names)
    assert any(int(gold[f"{n}_both_branches"]) for n in names)
    assert any(int(gold[f"{n}_deep_differs"]) for n in names)
    for k, g in (("margin_p", "gap_prob"), ("margin_s", "gap_prob"), ("margin_r", "gap_path_rel"), ("margin_x", "gap_logits")):
        assert (gold["part_" + k] >= 1000 * gold["part_" + g]).all(), k      # per part, each against its own gaps


def _gold_nbest(gold, n):
    ln = gold[f"{n}_nbest_len"]
    return [(tuple(gold[f"{n}_nbest_prefix"][j, : ln[j]].tolist()), float(gold[f"{n}_nbest_score"][j]),
             [dict(token=int(gold[f"{n}_node_token"][j, k]), frame=int(gold[f"{n}_node_frame"][j, k]), prob=float(gold[f"{n}_node_prob"][j, k]))
              for k in range(ln[j])]) for j in range(len(ln))]


def test_oracle_against_the_goldens(gold):
    for n, keywords in _clips(gold):
        table, idxset = _keyword_ids(gold, keywords)
        logits = torch.from_numpy(gold[f"{n}_logits"]) if f"{n}_logits" in gold.files else None
        if logits is None:                                            # a clip of a batch
            m, i = n.rsplit("_c", 1)
            logits = torch.from_numpy(gold[f"{m}_logits"][int(i), : int(gold["lens"][int(i)])])
        nn, ids, ps = KO.candidates(logits, idxset)
        cand = gold[f"{n}_cand"]
        assert np.array_equal(cand[:, 0], nn.numpy()) and np.array_equal(cand[:, 1:4], ids.numpy())
        assert np.abs(cand[:, 4:7] - ps.numpy()).max() <= 1e-15
        hyps = KO.beam_search(cand[:, 0].astype(int), cand[:, 1:4].astype(int), cand[:, 4:7])
        assert hyps == _gold_nbest(gold, n), n
        w, off, score = KO.decide(hyps, list(table.values()))
        assert (w, off) == (int(gold[f"{n}_hit"]), int(gold[f"{n}_offset"])) and (w < 0 or score == float(gold[f"{n}_score"])), n
        deep = KO.beam_search(cand[:, 0].astype(int), cand[:, 1:4].astype(int), cand[:, 4:7], deep_copy=True)
        wd, offd, scored = KO.decide(deep, list(table.values()))
        differs = (wd, offd) != (w, off) or scored != score or [[nd["frame"] for nd in h[2]] for h in deep] != [[nd["frame"] for nd in h[2]] for h in hyps]
        assert differs == bool(gold[f"{n}_deep_differs"]), n


def test_fsmn_restatement_against_the_reference_logits(gold, meta):
    from funasr_amd.kws import FsmnKWS
    for m, spec in meta["models"].items():
        if spec["kind"] != "fsmn":
            continue
        conf = synth.kws_fsmn_conf(vocab=len(meta["tokens"]), **spec["conf"])
        sd = synth.kws_state_dict(int(gold[f"{m}_seed"]), FsmnKWS(**conf), planted=meta["planted"], **spec["plant"])
        got = KO.fsmn_logits(KO.cast(sd, torch.float64), conf["encoder_conf"], torch.from_numpy(gold[f"{m}_feats"]).double(), prefix="encoder.")
        assert float((got - torch.from_numpy(gold[f"{m}_logits"])).abs().max()) < 1e-12
        lens = [int(v) for v in gold["lens"]]
        i = int(np.argmin(lens))                                       # a shorter clip alone: its last frames lose the padding behind them
        alone = KO.fsmn_logits(KO.cast(sd, torch.float64), conf["encoder_conf"], torch.from_numpy(gold[f"{m}_feats"][i: i + 1, : lens[i]]).double(),
                               prefix="encoder.")[0]
        assert float((alone - torch.from_numpy(gold[f"{m}_alone{i}_logits"])).abs().max()) < 1e-12
        assert float((alone - got[i, : lens[i]]).abs().max()) > 1e-3


def test_library_search_against_the_goldens(gold):
    tokens = [str(t) for t in gold["tokens"]]
    by_kw = {}
    for n, keywords in _clips(gold):
        by_kw.setdefault(keywords, []).append(n)
    for keywords, names in by_kw.items():
        dec = KwsCtcPrefixDecoder(None, keywords, tokens, None)
        T = max(gold[f"{n}_cand"].shape[0] for n in names)
        cand = np.zeros((len(names), T, 7), np.int32)
        cand[:, :, 1:4] = -1
        lens = []
        for b, n in enumerate(names):                                  # one batched call over clips of different lengths
            c = gold[f"{n}_cand"]
            cand[b, : c.shape[0]] = pack_candidates(c[:, 0], c[:, 1:4], c[:, 4:7].astype(np.float32))
            cand[b, c.shape[0]:, 0] = 3                                # frames past the length are never read
            cand[b, c.shape[0]:, 1:4] = 5
            lens.append(c.shape[0])
        results = dec.decode_candidates(cand, lens)
        for b, n in enumerate(names):
            want = _gold_nbest(gold, n)
            got = dec.search.nbest(b)
            assert [h["prefix"] for h in got] == [h[0] for h in want], n
            assert [[(nd["token"], nd["frame"]) for nd in h["nodes"]] for h in got] == [[(nd["token"], nd["frame"]) for nd in h[2]] for h in want], n
            for h, w in zip(got, want):                                # path scores span decades: the relative fp32 gap of the reference
                assert abs(h["score"] - w[1]) <= 8 * float(gold["gap_path_rel"]) * abs(w[1]), n
                assert all(abs(a["prob"] - b_["prob"]) <= 8 * float(gold["gap_prob"]) for a, b_ in zip(h["nodes"], w[2])), n
            hit, kw, score = results[b]
            w = int(gold[f"{n}_hit"])
            assert hit == (w >= 0) and kw == (dec.keywords[w] if w >= 0 else None), n
            if hit:
                assert abs(score - float(gold[f"{n}_score"])) <= 8 * float(gold["gap_score"]), (n, score, float(gold[f"{n}_score"]))
            else:
                assert score is None


def test_deep_copy_variant_differs_where_the_goldens_say(gold):
    n = next(n for n, _ in _clips(gold) if n.startswith("search") and int(gold[f"{n}_deep_differs"]))
    table, _ = _keyword_ids(gold, str(gold["keywords"]))
    cand = gold[f"{n}_cand"]
    args = (cand[:, 0].astype(int), cand[:, 1:4].astype(int), cand[:, 4:7])
    right, wrong = KO.decide(KO.beam_search(*args), list(table.values())), KO.decide(KO.beam_search(*args, deep_copy=True), list(table.values()))
    assert right[0] >= 0 and right[:2] == (int(gold[f"{n}_hit"]), int(gold[f"{n}_offset"])) and right[2] == float(gold[f"{n}_score"])
    assert wrong != right
    # the library sides with the reference
    dec = KwsCtcPrefixDecoder(None, str(gold["keywords"]), [str(t) for t in gold["tokens"]], None)
    hit, kw, score = dec.decode_candidates(pack_candidates(cand[:, 0], cand[:, 1:4], cand[:, 4:7].astype(np.float32))[None], [len(cand)])[0]
    assert hit and abs(score - right[2]) <= 8 * float(gold["gap_score"]) and abs(score - wrong[2]) > 1000 * float(gold["gap_score"])


def test_search_details():
    s = KwsSearch(10, [(3, 4), (4,)])
    assert s.token_mask().tolist() == [1 | 1 << 3 | 1 << 4]
    # no frames, and frames without candidates: the empty prefix, rejected
    hit, off, score = s.decode(np.zeros((2, 3, 7), np.int32), [0, 3])
    assert hit == [-1, -1] and [h["prefix"] for h in s.nbest(1)] == [()] and s.nbest(0)[0]["score"] == 1.0
    # is_sublist: equal lengths compare whole lists; keywords in the order given, the first hit wins
    c = pack_candidates([1, 1], [[4, -1, -1], [3, -1, -1]], [[0.5, 0, 0], [0.25, 0, 0]])
    hit, off, score = s.decode(c[None], [2])
    assert (hit, off) == ([1], [0]) and score[0] == pytest.approx(0.5 ** 0.5, abs=1e-12)      # (4, 3): keyword (4,) at offset 0
    assert KO.is_sublist((4, 3), (3, 4)) == -1 and KO.is_sublist((1, 3, 4), (3, 4)) == 1
    with pytest.raises(IndexError):
        s.nbest(5)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals(meta):
    lib = _lib.load()
    assert not lib.pf_kws_search_create(2) and "V < 3" in _lib.last_error()
    with pytest.raises(_lib.HipRuntimeError, match="V < 3"):
        KwsCtcPrefixDecoder(None, "a", ["<blank>", "a"], None)
    with pytest.raises(ValueError, match="keywords"):
        KwsCtcPrefixDecoder(None, None, ["<blank>", "a", "b"], None)
    with pytest.raises(ValueError, match="no tokens"):
        KwsCtcPrefixDecoder(None, "a,,b", ["<blank>", "a", "b"], None)
    s = KwsSearch(5, [(1, 2)])
    with pytest.raises(_lib.HipRuntimeError, match="outside the vocabulary"):
        s.decode(pack_candidates([[1]], [[[7, -1, -1]]], [[[0.5, 0, 0]]]), [1])
    from funasr_amd.kws import FsmnKWS, SanmKWS, refuse_not_built
    for name in ("FsmnKWSMT", "SanmKWSStreaming", "FsmnKWSConvert", "FsmnKWSMTConvert"):
        with pytest.raises(NotImplementedError, match=name):
            refuse_not_built(name)
    conf = synth.kws_fsmn_conf()
    model = FsmnKWS(**conf)
    tok = type("Tok", (), {"token_list": ["<blank>"] + [f"t{i}" for i in range(66)], "seg_dict": None})()
    with pytest.raises(ValueError, match="keywords"):                    # before any device work
        model.inference(torch.zeros(1, 8, 40), tokenizer=tok, data_type="fbank")
    with pytest.raises(NotImplementedError, match="bf16"):
        FsmnKWS(**conf, bf16=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        SanmKWS(**synth.kws_sanm_conf()).set_precision("bf16")
    with pytest.raises(NotImplementedError, match="export"):
        model.export()
    with pytest.raises(NotImplementedError, match="SANMEncoderChunkOpt"):
        SanmKWS(**dict(synth.kws_sanm_conf(), encoder="SANMEncoderChunkOpt"))


def test_auto_model_refuses_the_classes_that_are_not_built(tmp_path):
    import yaml
    from funasr_amd.auto_model import AutoModel
    d = str(tmp_path / "mt")
    os.makedirs(d)
    yaml.safe_dump({"model": "FsmnKWSMT", "encoder": "FSMN", "encoder_conf": synth.kws_fsmn_conf()["encoder_conf"]},
                   open(os.path.join(d, "config.yaml"), "w"))
    with pytest.raises(NotImplementedError, match="FsmnKWSMT"):
        AutoModel(model=d, device="cpu", disable_update=True)
