"""Host-side diarization (funasr_amd/speaker.py) against the reference's recorded outputs, a fuzz against the reference's own
functions where its tree is present, and the AutoModel surface of spk_model without a GPU."""
import copy
import json
import os

import numpy as np
import pytest

from funasr_amd import speaker

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "campplus_speaker.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same_partition(a, b):
    return list(speaker.relabel_by_first_appearance(a)) == list(speaker.relabel_by_first_appearance(b))


def test_sv_chunk_matches_golden(golden):
    segs = [[b, e, np.zeros(int(round((e - b) * 16000)), np.float32)] for b, e in golden["vad"]]
    got = speaker.sv_chunk(segs)
    assert len(got) == len(golden["chunks"])
    for (b, e, w), (rb, re_) in zip(got, golden["chunks"]):
        assert abs(b - rb) < 1e-9 and abs(e - re_) < 1e-9 and w.shape[0] == 24000


def test_sv_chunk_pads_short_segment():
    data = np.arange(1, 8001, dtype=np.float32)
    (b, e, w), = speaker.sv_chunk([[2.0, 2.5, data]])
    assert (b, e) == (2.0, 2.5) and w.shape[0] == 24000 and w[7999] == 8000 and not w[8000:].any()
    assert speaker.sv_chunk_bounds(40000) == [(0, 24000), (12000, 36000), (16000, 40000)]


def test_cluster_backend_matches_golden(golden):
    X = np.array(golden["embeddings"])
    cb = speaker.ClusterBackend()
    assert _same_partition(cb(X), golden["labels_eigengap"])
    assert _same_partition(cb(X, oracle_num=3), golden["labels_oracle3"])
    assert (cb(X[:19]) == 0).all()                          # fewer than 20 embeddings: one speaker


def test_postprocess_and_distribute_match_golden(golden):
    turns = speaker.postprocess([c[:] for c in golden["chunks"]], None, np.array(golden["labels_eigengap"]),
                                np.array(golden["embeddings"]))
    assert [[round(a, 6), round(b, 6), int(c)] for a, b, c in turns] == [[round(a, 6), round(b, 6), c] for a, b, c in golden["turns"]]
    sents = [{"start": s["start"], "end": s["end"]} for s in golden["sentences"]]
    speaker.distribute_spk(sents, turns)
    assert [s["spk"] for s in sents] == [s["spk"] for s in golden["sentences"]]


def test_kmeans_large_set_with_preset_and_centers():
    rng = np.random.default_rng(0)
    c = rng.standard_normal((4, 32))
    truth = rng.integers(0, 4, 2100)
    X = c[truth] + 0.05 * rng.standard_normal((2100, 32))
    lab = speaker.ClusterBackend()(X, oracle_num=4)
    assert _same_partition(lab, truth)
    segs = [[i * 0.75, i * 0.75 + 1.5] for i in range(len(lab))]
    _, centers = speaker.postprocess(segs, None, lab, X, return_spk_center=True)
    assert centers.shape == (4, 32)


def test_large_set_without_preset_needs_umap_or_says_so():
    try:
        import umap  # noqa: F401
        pytest.skip("umap is installed")
    except ImportError:
        pass
    with pytest.raises(NotImplementedError, match="preset_spk_num"):
        speaker.ClusterBackend()(np.random.default_rng(1).standard_normal((2048, 8)))


def test_fuzz_against_reference_functions():
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference tree not present")
    try:
        ref_import.install()
        from funasr.models.campplus.cluster_backend import ClusterBackend
        from funasr.models.campplus.utils import distribute_spk, postprocess, sv_chunk
    except ImportError as e:
        pytest.skip(f"reference clustering needs {e.name}")
    rng = np.random.default_rng(11)
    for case in range(40):
        # segments with gaps, some shorter than a chunk
        t, vad = 0.0, []
        for _ in range(int(rng.integers(1, 8))):
            t += float(rng.uniform(0.0, 1.0))
            d = float(rng.uniform(0.3, 6.0))
            vad.append([round(t, 3), round(t + d, 3)])
            t += d
        segs = [[b, e, rng.standard_normal(int((e - b) * 16000)).astype(np.float32)] for b, e in vad]
        ref_chunks, got_chunks = sv_chunk(copy.deepcopy(segs)), speaker.sv_chunk(segs)
        assert len(ref_chunks) == len(got_chunks)
        for r, g in zip(ref_chunks, got_chunks):
            assert abs(r[0] - g[0]) < 1e-12 and abs(r[1] - g[1]) < 1e-12 and np.array_equal(r[2], g[2])
        k = int(rng.integers(1, 5))
        centres = 3 * rng.standard_normal((k, 24))
        spk = rng.integers(0, k, len(got_chunks))
        X = centres[spk] + 0.1 * rng.standard_normal((len(spk), 24))
        ref_lab = ClusterBackend()(X.copy(), **({"oracle_num": k} if case % 2 else {}))
        got_lab = speaker.ClusterBackend()(X, oracle_num=k if case % 2 else None)
        assert _same_partition(ref_lab, got_lab), case
        bounds = [c[:2] for c in got_chunks]
        ref_turns = postprocess([list(b) for b in bounds], None, np.array(ref_lab), X)
        got_turns = speaker.postprocess([list(b) for b in bounds], None, np.array(got_lab), X)
        assert [list(map(float, r[:2])) + [int(r[2])] for r in ref_turns] == [list(map(float, g[:2])) + [int(g[2])] for g in got_turns]
        sents = [{"start": int(rng.uniform(0, t * 1000)), "end": 0} for _ in range(6)]
        for s in sents:
            s["end"] = s["start"] + int(rng.uniform(100, 4000))
        rs, gs = copy.deepcopy(sents), copy.deepcopy(sents)
        distribute_spk(rs, [list(x) for x in ref_turns])
        speaker.distribute_spk(gs, got_turns)
        assert [s["spk"] for s in rs] == [s["spk"] for s in gs], case


def test_automodel_spk_model_hub_name_still_refused():
    from funasr_amd.auto_model import AutoModel
    with pytest.raises(NotImplementedError, match="spk_model"):
        AutoModel(model="/nonexistent", spk_model="cam++")
