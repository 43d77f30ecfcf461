"""CAM++ speaker embedding on the MI355X: the HIP network against the reference's recorded outputs and the float64 oracle,
batch invariance and determinism (bitwise), and the waveform-chunk path against fbank -> forward."""
import os

import numpy as np
import pytest
import torch

from funasr_amd import synth
from funasr_amd.campplus import CAMPPlus

from . import _campplus_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "campplus.npz")


def _model(cuda, seed, max_batch=256):
    m = CAMPPlus(max_batch=max_batch)
    m.load_state_dict(synth.campplus_state_dict(seed), strict=True)
    return m.to(cuda)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.mark.parametrize("case", ["a", "b"])
def test_against_reference_golden(cuda, golden, case):
    m = _model(cuda, int(golden["seed"]))
    out = m(torch.from_numpy(golden[f"x_{case}"]).to(cuda)).cpu().double().numpy()
    r32, r64 = golden[f"ref32_{case}"], golden[f"ref64_{case}"]
    bar = 4 * np.abs(r32 - r64).max() + 1e-6
    err = np.abs(out - r64).max()
    assert err <= bar, (err, bar)
    assert _cos(out, r64).min() >= 1 - 1e-6


@pytest.mark.parametrize("T", [148, 131, 7, 421])
def test_against_float64_oracle(cuda, T):
    """T' = 74 (the diarization chunk), 66 (no tile multiple), 4 (shorter than one tile), 211 (three segments, partial last)"""
    sd = synth.campplus_state_dict(3)
    m = _model(cuda, 3)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(3, T, 80, generator=g)
    x = x - x.mean(1, keepdim=True)
    out = m(x.to(cuda)).cpu().double()
    ref = O.forward(x, sd)
    ref32 = O.forward(x, sd, torch.float32).double()
    bar = 4 * (ref32 - ref).abs().max().item() + 1e-6
    assert (out - ref).abs().max().item() <= bar
    assert torch.nn.functional.cosine_similarity(out, ref, dim=-1).min().item() >= 1 - 1e-6


def test_batch_invariance_and_determinism(cuda):
    m = _model(cuda, 4)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(300, 148, 80, generator=g).to(cuda)
    full = m(x)
    again = m(x)
    assert torch.equal(full, again)
    for i in (0, 1, 137, 299):
        assert torch.equal(m(x[i:i + 1].contiguous()), full[i:i + 1])
    m.set_max_batch(7)                       # sub-batched launches: the same bits
    assert torch.equal(m(x), full)


def test_weights_replaced_on_a_live_handle(cuda):
    """a second state dict loaded into a module that already ran: every folded / repacked weight is rebuilt from it"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 20, 80, generator=g).to(cuda)
    m = _model(cuda, 4)
    m(x)
    m.load_state_dict(synth.campplus_state_dict(1), strict=True)
    assert torch.equal(m(x), _model(cuda, 1)(x))


def test_embed_chunks_equals_fbank_then_forward(cuda):
    m = _model(cuda, 6)
    wav = synth.speech_like(16000 * 6, seed=3).to(cuda) * 0.3
    L = 24000
    starts = [0, 12000, 24000, 36000, 70000, 80000]
    valid = [L, L, L, L, 10000, 16000]                           # two short segments, zero-padded to 1.5 s (sv_chunk)
    emb = m.embed_chunks(wav, starts, L, valid)
    chunks = []
    for s, v in zip(starts, valid):
        c = torch.zeros(L, device=cuda)
        c[:v] = wav[s:s + v]
        chunks.append(c)
    feats = torch.stack([m.fbank(c) for c in chunks])
    ref = m(feats)
    assert (emb - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    # a chunk embeds to the same bits alone and inside the batch
    one = m.embed_chunks(wav, starts[4:5], L, valid[4:5])
    assert torch.equal(one, emb[4:5])
    # inference() on the list of numpy chunks AutoModel passes
    res, _ = m.inference([c.cpu().numpy() for c in chunks])
    assert (res[0]["spk_embedding"] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_too_short_input_is_refused(cuda):
    m = _model(cuda, 6)
    with pytest.raises(ValueError, match="fewer than 2"):
        m(torch.zeros(1, 2, 80, device=cuda))


def test_fbank_against_kaldi_native_fbank_golden(cuda):
    """the CAM++ feature path (80 bins, povey, no 2^15 scaling, dither 0, snip_edges) of both the module's fbank and the
    handle's own frontend inside embed_chunks, against kaldi-native-fbank on a chunk with a zero-padded tail (log floor)"""
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "campplus_fbank.npz"))
    wav, ref = torch.from_numpy(g["wav"]), torch.from_numpy(g["fbank"])
    ref_norm = ref - ref.mean(0, keepdim=True)
    m = _model(cuda, 8)
    got = m.fbank(wav.to(cuda)).cpu()
    assert got.shape == ref.shape
    assert (got - ref_norm).abs().max().item() < 2e-3
    emb = m.embed_chunks(wav.to(cuda), [0], 24000, [9600])
    ref_emb = m(ref_norm[None].to(cuda))
    assert (emb - ref_emb).abs().max().item() <= 1e-3 * ref_emb.abs().max().item()
