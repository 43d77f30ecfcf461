"""Writes tests/golden/campplus.npz: outputs of the reference's own CAMPPlus.forward (funasr/models/campplus/model.py), imported
read-only through oracle.ref_import, in float32 AND float64, on synthetic weights (funasr_amd.synth.campplus_state_dict(seed);
weights are never stored) and stored feature batches:
  (a) four 1.5-s chunks (148 frames), the last one a short segment zero-padded to 1.5 s: its padded frames sit at the fbank log
      floor (log of float epsilon in every bin) before the time mean is removed;
  (b) a zero-padded batch of two utterances (420 and 301 frames: 210 frames after the TDNN, i.e. three 100-frame segments with a
      partial last one).
And tests/golden/campplus_speaker.json: the reference's sv_chunk, ClusterBackend (eigengap and oracle_num), postprocess and
distribute_spk on stored inputs (embeddings with clear cluster margins, so k-means seeding cannot matter).
And tests/golden/campplus_fbank.npz: a 1.5-s chunk in [-1, 1] whose last 0.9 s are zero padding, and its kaldi fbank from the
kaldi-native-fbank oracle (oracle/_ref/libknf_ref.so, built by oracle/Makefile) with CAM++'s options: 80 bins, povey window,
no 2^15 scaling, dither 0, snip_edges, preemphasis 0.97 and DC removal (kaldi defaults) -- the padded frames hit the log floor.
Build container only (needs the reference tree)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 5
LOG_FLOOR = float(np.log(np.finfo(np.float32).eps))


def _utterance(g: torch.Generator, T: int, speech: int) -> torch.Tensor:
    """log-mel-like frames: a smooth spectral envelope + noise for `speech` frames, the log floor after; minus the time mean"""
    env = torch.linspace(2.0, -3.0, 80)[None] + 0.8 * torch.sin(torch.arange(80)[None] / 7.0 + torch.rand(1, generator=g) * 6)
    f = env + 1.5 * torch.randn(T, 80, generator=g) + 0.5 * torch.sin(torch.arange(T)[:, None] / 9.0)
    f[speech:] = LOG_FLOOR
    return f - f.mean(0, keepdim=True)


def main():
    from oracle import ref_import
    from funasr_amd import synth

    ref_import.install()
    from funasr.models.campplus.model import CAMPPlus

    sd = synth.campplus_state_dict(SEED)
    model = CAMPPlus()
    model.load_state_dict(sd, strict=True)
    model.eval()
    g = torch.Generator().manual_seed(SEED)
    xa = torch.stack([_utterance(g, 148, 148) for _ in range(3)] + [_utterance(g, 148, 61)]).float()
    ub = [_utterance(g, 420, 420), _utterance(g, 301, 301)]
    xb = torch.zeros(2, 420, 80)
    for i, u in enumerate(ub):
        xb[i, : u.shape[0]] = u
    out = dict(seed=np.int64(SEED), x_a=xa.numpy(), x_b=xb.numpy())
    with torch.no_grad():
        for name, x in (("a", xa), ("b", xb)):
            out[f"ref32_{name}"] = model.float()(x).numpy()
            out[f"ref64_{name}"] = model.double()(x.double()).numpy()
    path = os.path.join(ROOT, "tests", "golden", "campplus.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for name in ("a", "b"):
        print(name, "fp32 vs fp64 max |d|", np.abs(out[f"ref32_{name}"] - out[f"ref64_{name}"]).max())


def speaker_case(seed: int = 7):
    """inputs + the reference's outputs of the host-side diarization functions"""
    from funasr.models.campplus.cluster_backend import ClusterBackend
    from funasr.models.campplus.utils import distribute_spk, postprocess, sv_chunk

    rng = np.random.default_rng(seed)
    # VAD segments of a recording (seconds) with speaker turns; embeddings = speaker centre + small noise
    vad = [[0.0, 4.1], [4.5, 5.2], [5.6, 11.3], [12.0, 12.9], [13.4, 21.0], [21.2, 27.5]]
    spk_of_seg = [0, 1, 1, 2, 0, 2]
    segs = [[b, e, np.zeros(int(round((e - b) * 16000)), np.float32)] for b, e in vad]
    chunks = sv_chunk(segs)
    seg_idx = []
    for i, (b, e, d) in enumerate(segs):
        seg_idx += [i] * len(sv_chunk([[b, e, d]]))
    centres = rng.standard_normal((3, 192))
    emb = np.stack([centres[spk_of_seg[i]] + 0.15 * rng.standard_normal(192) for i in seg_idx])
    cb = ClusterBackend()
    lab_gap = cb(emb.copy())
    lab_k = cb(emb.copy(), oracle_num=3)
    turns = postprocess([c[:2] for c in chunks], None, lab_gap, emb)
    sentences = [{"start": int(b * 1000) + 50, "end": int(e * 1000) - 50} for b, e in vad] + [{"start": 3000, "end": 6000}]
    distribute_spk(sentences, [list(t) for t in turns])
    return dict(vad=vad, chunks=[[float(c[0]), float(c[1])] for c in chunks], embeddings=emb.round(6).tolist(),
                labels_eigengap=[int(x) for x in lab_gap], labels_oracle3=[int(x) for x in lab_k],
                turns=[[float(a), float(b), int(c)] for a, b, c in turns], sentences=sentences)


if __name__ == "__main__":
    main()
    import json
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from make_golden_fbank_options import knf_fbank_opts
    from funasr_amd import synth as _synth
    wav = np.zeros(24000, np.float32)
    wav[:9600] = (_synth.speech_like(9600, seed=41) * 0.4).numpy()
    fb = knf_fbank_opts(wav, "povey", True)
    path = os.path.join(ROOT, "tests", "golden", "campplus_fbank.npz")
    np.savez_compressed(path, wav=wav, fbank=fb)
    print(path, os.path.getsize(path), "bytes", fb.shape, fb[-1, :3])
    from oracle import ref_import
    ref_import.install()
    path = os.path.join(ROOT, "tests", "golden", "campplus_speaker.json")
    with open(path, "w") as f:
        json.dump(speaker_case(), f)
    print(path, os.path.getsize(path), "bytes")
