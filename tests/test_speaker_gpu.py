"""The speaker branch of AutoModel on the MI355X: a synthetic CAM++ model directory as spk_model over a multi-voice recording;
every sentence's `spk` equals what the float64 oracle pipeline gives (fp64 embeddings of the same chunks -> the same host
clustering -> postprocess -> distribute_spk)."""
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import speaker, synth
from funasr_amd.auto_model import AutoModel

from . import _campplus_oracle as O
from .test_vad_pipeline import _FakeASR, _FakePunc, _FakeVAD, _auto

pytestmark = pytest.mark.gpu

SEGS = [[500, 4200], [4600, 5300], [5800, 11500], [12100, 13000], [13500, 21000], [21300, 27900], [28500, 29200],
        [29800, 36000]]
VOICE = [0, 1, 1, 0, 1, 0, 1, 0]


def _recording():
    n = 37 * 16000
    wav = torch.zeros(n)
    for (b, e), v in zip(SEGS, VOICE):
        s0, s1 = b * 16, e * 16
        x = synth.speech_like(s1 - s0, seed=100 + v)
        wav[s0:s1] = x * (0.3 if v == 0 else 0.08) * (1 + v * torch.sin(torch.arange(s1 - s0) / 3.0))
    return wav


@pytest.fixture(scope="module")
def spk_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("campplus"))
    with open(os.path.join(d, "config.yaml"), "w") as f:
        yaml.safe_dump({"model": "CAMPPlus", "model_conf": {"feat_dim": 80, "embedding_size": 192},
                        "frontend": "WavFrontend", "frontend_conf": {"fs": 16000}}, f)
    torch.save(synth.campplus_state_dict(12), os.path.join(d, "model.pt"))
    return d


def _expected(spk_model, wav, sentences, preset):
    chunks = speaker.sv_chunk([[b / 1000, e / 1000, wav[b * 16: e * 16].numpy()] for b, e in SEGS])
    feats = torch.stack([spk_model.fbank(torch.from_numpy(c[2]).cuda()) for c in chunks]).cpu()
    emb = O.forward(feats, synth.campplus_state_dict(12)).numpy()
    labels = speaker.ClusterBackend()(emb, oracle_num=preset)
    turns = speaker.postprocess([c[:2] for c in chunks], None, labels, emb)
    sents = [{"start": s["start"], "end": s["end"]} for s in sentences]
    return [s["spk"] for s in speaker.distribute_spk(sents, turns)]


def _pipeline(cuda, spk_dir, punc=True, **kw):
    spk_model, spk_kwargs = AutoModel.build_model(model=spk_dir, device="cuda:0")
    am = _auto(_FakeVAD([SEGS]), _FakeASR(), batch_size_s=300)
    if punc:
        am.punc_model, am.punc_kwargs = _FakePunc(), {}
    am.spk_model, am.spk_kwargs, am.cb_kwargs, am.spk_mode = spk_model, spk_kwargs, {}, "punc_segment"
    return am, spk_model


@pytest.mark.parametrize("preset", [2, None])
def test_sentence_speakers_equal_oracle_pipeline(cuda, spk_dir, preset):
    am, spk_model = _pipeline(cuda, spk_dir)
    wav = _recording()
    kw = {"preset_spk_num": preset} if preset else {}
    out = am.generate(wav, **kw)[0]
    info = out["sentence_info"]
    assert info and all("spk" in s for s in info)
    assert "spk_embedding" not in out
    assert [s["spk"] for s in info] == _expected(spk_model, wav, info, preset)
    if preset == 2:
        assert len({s["spk"] for s in info}) == 2


def test_vad_segment_fallback_and_centers(cuda, spk_dir):
    am, spk_model = _pipeline(cuda, spk_dir, punc=False)
    wav = _recording()
    out = am.generate(wav, preset_spk_num=2, return_spk_center=True)[0]
    info = out["sentence_info"]
    assert [(s["start"], s["end"]) for s in info] == [tuple(s) for s in SEGS]          # one record per VAD segment
    assert [s["spk"] for s in info] == _expected(spk_model, wav, info, 2)
    assert out["spk_embedding_center"].shape == (2, 192)
    assert am.spk_mode == "punc_segment"                         # the fallback is per call, not stored on the object


def test_spk_model_directory_loads_the_weights(cuda, spk_dir):
    m, _ = AutoModel.build_model(model=spk_dir, device="cuda:0")
    sd = synth.campplus_state_dict(12)
    assert torch.equal(m.state_dict()["xvector.block2.tdnnd3.linear1.weight"].cpu(), sd["xvector.block2.tdnnd3.linear1.weight"])
    x = torch.randn(2, 148, 80)
    x = x - x.mean(1, keepdim=True)
    ref = O.forward(x, sd)
    assert torch.nn.functional.cosine_similarity(m(x.cuda()).cpu().double(), ref, dim=-1).min() >= 1 - 1e-6
