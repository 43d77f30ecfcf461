"""SenseVoiceSmall `output_timestamp` through the batched device alignment, on the weights and features of
tests/golden/sensevoice_ts.npz: the records of the REFERENCE class, the records of the per-clip host path on the same encoder
output, and the three-part form of `inference`."""
import json
import os

import pytest
import torch

from funasr_amd.tokenizer import SentencepiecesTokenizer

from .test_sensevoice_timestamps import GOLD, _gold, _model

MODES = ("fp32", "f16x2")


@pytest.fixture(scope="module")
def setup(cuda):
    g = _gold()
    tok = SentencepiecesTokenizer(os.path.join(GOLD, "sv_bpe.model"))
    model = _model(g).to(cuda)
    kw = dict(key=[f"u{i}" for i in range(3)], tokenizer=tok, frontend=None, device=cuda, data_type="fbank", language="auto",
              output_timestamp=True)
    return g, tok, model, torch.from_numpy(g["feats"]).to(cuda), torch.from_numpy(g["lens"]), kw


def _check_golden(res, g, what):
    e2e = json.loads(str(g["e2e"]))
    assert len(res) == len(e2e)
    for r, e in zip(res, e2e):
        assert r["text"] == e["text"], what
        assert ("timestamp" in r) == e["has_ts"], what
        if e["has_ts"]:
            assert r["words"] == e["words"] and [[float(a), float(b)] for a, b in r["timestamp"]] == e["timestamp"], what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_batched_records_equal_the_reference_and_the_host_path(setup, mode):
    g, tok, model, feats, lens, kw = setup
    model.set_precision(mode)
    res, _ = model.inference(feats, data_lengths=lens, **kw)
    _check_golden(res, g, mode)
    assert any(e["has_ts"] for e in json.loads(str(g["e2e"])))
    # the per-clip host path from the same encoder output: whole log-probabilities to the host, `ctc_timestamps` clip by clip
    out = model.recognize_features(feats, lens, "auto", "woitn", return_intermediate=True)
    logp = model.ctc.log_softmax(out["enc"]).cpu()
    for i, r in enumerate(res):
        text = tok.decode(out["ids"][i])
        assert text == r["text"]
        ts = model.ctc_timestamps(text, logp[i, 4:int(out["olens"][i])].numpy(), tok)
        assert (ts is not None) == ("timestamp" in r)
        if ts is not None:
            assert (r["timestamp"], r["words"]) == ts
            assert all(isinstance(v, int) for span in r["timestamp"] for v in span)       # same keys, same number types
        assert sorted(r) == (["key", "text", "timestamp", "words"] if ts is not None else ["key", "text"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_three_part_inference_with_timestamps(setup, mode):
    g, tok, model, feats, lens, kw = setup
    model.set_precision(mode)
    whole, _ = model.inference(feats, data_lengths=lens, **kw)
    first = model.inference_begin(feats, data_lengths=lens, **kw)
    assert first is not None, "output_timestamp must not turn the split form off"
    second = model.inference_begin(feats[:2], data_lengths=lens[:2], **dict(kw, key=["v0", "v1"]))   # batch i + 1 before batch i's alignment
    assert model.inference_launch(first) is None
    res, _ = model.inference_end(first)
    assert res == whole
    _check_golden(res, g, mode)
    res2, _ = model.inference_end(second)                        # never launched: inference_end does both
    assert [dict(r, key=None) for r in res2] == [dict(r, key=None) for r in whole[:2]]
    # without timestamps the split form gives the plain records, as before
    assert model.inference_begin(feats, data_lengths=lens, **dict(kw, output_timestamp=False)) is None


@pytest.mark.gpu
def test_a_clip_without_pieces_gets_no_timestamp(setup):
    """an all-blank CTC path decodes to the empty text: no record keys beside key and text, beside clips that have stamps"""
    g, tok, model, feats, lens, kw = setup
    model.set_precision("fp32")
    out = model.recognize_features(feats, lens, "auto", "woitn", return_intermediate=True)
    out["ids"][1] = []                                           # clip 1 decoded nothing
    res, _ = model._records(out, kw["key"], tok, {}, True)
    assert res[1] == {"key": "u1", "text": ""}
    whole, _ = model.inference(feats, data_lengths=lens, **kw)
    assert res[0] == whole[0] and res[2] == whole[2]


@pytest.mark.gpu
def test_clips_above_the_kernel_limits_take_the_host_path(setup, monkeypatch):
    """the limits lowered for the test: some clips, then all, go through `ctc_timestamps` on the host -- the same records"""
    from funasr_amd import ops
    g, tok, model, feats, lens, kw = setup
    model.set_precision("fp32")
    whole, _ = model.inference(feats, data_lengths=lens, **kw)
    n_ids = sorted(len(model.timestamp_targets(r["text"], tok)[1]) for r in whole)
    assert n_ids[0] < n_ids[-1]
    monkeypatch.setattr(ops, "CTC_ALIGN_MAX_L", n_ids[0])        # only the clip with the fewest ids stays on the device
    some, _ = model.inference(feats, data_lengths=lens, **kw)
    monkeypatch.setattr(ops, "CTC_ALIGN_MAX_T", 1)               # none does
    none, _ = model.inference(feats, data_lengths=lens, **kw)
    assert some == whole and none == whole
