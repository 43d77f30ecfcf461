"""CPU restatement of the Paraformer-v2 posterior stage (funasr/models/paraformer_v2_community/model.py:451-482,545-585 and
decoder.py:318-325) in plain torch, and the seeded inputs the tests and tools/make_golden_paraformer_v2.py share. No reference code.

Two orders of the same computation:
  * the reference's: softmax -> mean of the posteriors of each run -> Linear -> LayerNorm -> ReLU -> x sqrt(D) + pe   (`embed_merged`)
  * the frame domain (what the device stage computes): Linear per frame, then the mean over the run + bias             (`embed_frame_domain`)
They agree because the first layer is linear and a run's weights sum to one; tests/test_paraformer_v2.py pins that to 1e-6.
"""
from __future__ import annotations

import math
import os
from typing import List, Tuple

import numpy as np
import torch

from funasr_amd import synth
from funasr_amd.conformer import abs_pos_table

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paraformer_v2.npz")
CLIP_T = (1, 7, 31, 65, 130)
SHORT_BLANK_T = 4                               # a short clip the main state dict itself decodes as all blank (seed in the golden)
BLANK_T = 31                                    # the clip that the second state dict (large blank bias) turns all blank
# shape A: the fp32 route (V above 256 and no multiple of 4); shape B: the f16x2 route (head dim 128, d_model % 256 == 0)
SHAPES = {"A": dict(d_model=64, heads=4, ffn=128, enc_blocks=2, dec_blocks=2, vocab=261),
          "B": dict(d_model=256, heads=2, ffn=512, enc_blocks=2, dec_blocks=2, vocab=261)}
EMBED_D, EMBED_B, EMBED_T, EMBED_V = 320, 3, 65, (5, 261, 8404)      # the kernel-level embedder cases (B * T = 195 rows)
EMBED_LENS = (65, 64, 1)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def clip_features(T: int, seed: int, dim: int = 560) -> torch.Tensor:
    """fbank-like features [T, dim], piecewise constant over 3 to 5 frames (multi-frame CTC runs), seeded"""
    g = torch.Generator().manual_seed(9000 + seed)
    rows, t = [], 0
    while t < T:
        n = int(torch.randint(3, 6, (1,), generator=g))
        rows.append(torch.randn(1, dim, generator=g).expand(min(n, T - t), dim))
        t += n
    return torch.cat(rows)[:T].contiguous()


def model_state(shape: str, seed: int, ctc_gain: float, blank_bias: float):
    conf = synth.paraformer_v2_conf(**SHAPES[shape])
    return conf, synth.paraformer_v2_state_dict(conf, seed=seed, ctc_gain=ctc_gain, blank_bias=blank_bias)


# ------------------------------------------------------------------------------------------------ the stage, in torch
def greedy_path(hidden: torch.Tensor, ctc_w: torch.Tensor, ctc_b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """hidden [T, D] -> (posteriors [T, V], greedy path [T]) as CTC.softmax / argmax do (ctc.py:192-216)"""
    probs = torch.softmax(torch.nn.functional.linear(hidden, ctc_w, ctc_b), dim=-1)
    return probs, probs.argmax(dim=-1)


def runs_of(path, blank: int) -> List[Tuple[int, int]]:
    """maximal stretches of one non-blank label as (start, end) frame ranges: a plain Python loop"""
    path = [int(v) for v in path]
    out, t = [], 0
    while t < len(path):
        e = t
        while e < len(path) and path[e] == path[t]:
            e += 1
        if path[t] != blank:
            out.append((t, e))
        t = e
    return out


def merged_posteriors(probs: torch.Tensor, runs) -> torch.Tensor:
    """average_repeats_inference (model.py:451-482): the mean posterior of each run, [N, V]"""
    if not runs:
        return torch.zeros(0, probs.shape[1], dtype=probs.dtype)
    return torch.stack([probs[s:e].mean(dim=0) for s, e in runs])


def _ln_relu_pe(x: torch.Tensor, g, b) -> torch.Tensor:
    D = x.shape[-1]
    y = torch.relu(torch.nn.functional.layer_norm(x, (D,), g.to(x.dtype), b.to(x.dtype), 1e-5))
    return y * math.sqrt(D) + abs_pos_table(D)[: x.shape[0]].to(x.dtype)


def embed_merged(merged: torch.Tensor, w0, b0, g, b) -> torch.Tensor:
    """decoder.embed on merged posteriors [N, V] -> [N, D] (the reference's order), in the dtype of `merged`"""
    dt = merged.dtype
    return _ln_relu_pe(torch.nn.functional.linear(merged, w0.to(dt), b0.to(dt)), g, b)


def embed_frame_domain(probs: torch.Tensor, runs, w0, b0, g, b) -> torch.Tensor:
    """the same in the frame domain and float64: E = probs W^T per frame, mean over the run, + bias, LayerNorm, ReLU, PE"""
    E = probs.double() @ w0.double().T
    if not runs:
        return torch.zeros(0, w0.shape[0], dtype=torch.float64)
    x = torch.stack([E[s:e].mean(dim=0) for s, e in runs]) + b0.double()
    return _ln_relu_pe(x, g, b)


def filter_tokens(ids, sos: int, eos: int, blank: int) -> List[int]:
    """model.py:581-585"""
    return [int(t) for t in ids if int(t) not in (eos, sos, blank)]


# ------------------------------------------------------------------------------------------------ kernel-level embedder cases
def embedder_case(V: int, seed: int, D: int = EMBED_D, B: int = EMBED_B, T: int = EMBED_T, ctc_gain: float = 8.0, blank_bias: float = 6.0):
    """a fixed `hidden` [B, T, D] (piecewise constant over 3 to 5 frames plus a little per-frame noise, so that runs have several
    DIFFERENT frames), a confident CTC head and an input layer, all seeded"""
    g = torch.Generator().manual_seed(7000 + 13 * seed + V)
    hid = torch.stack([clip_features(T, 100 * seed + b, D) for b in range(B)]) + 0.02 * torch.randn(B, T, D, generator=g)
    rnd = lambda *s, std=1.0: torch.randn(*s, generator=g) * std                      # noqa: E731
    w = dict(ctc_w=rnd(V, D, std=ctc_gain / math.sqrt(D)), ctc_b=rnd(V, std=0.02), w0=rnd(D, V), b0=rnd(D, std=0.02),
             g=1.0 + rnd(D, std=0.1), b=rnd(D, std=0.05))
    w["ctc_b"][0] += blank_bias
    return hid.contiguous(), list(EMBED_LENS[:B]), w


def embedder_reference(hid: torch.Tensor, lens, w, dtype=torch.float64, blank: int = 0):
    """per clip: (path over the valid frames, runs, embeds [n_b, D]) in `dtype`, the reference's order; also the smallest top-2 gap
    of the CTC logits over the valid frames"""
    out, gap = [], float("inf")
    for bidx, n in enumerate(lens):
        h = hid[bidx, :n].to(dtype)
        logits = torch.nn.functional.linear(h, w["ctc_w"].to(dtype), w["ctc_b"].to(dtype))
        top = logits.topk(min(2, logits.shape[1]), dim=-1).values
        gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
        probs = torch.softmax(logits, dim=-1)
        path = probs.argmax(dim=-1)
        runs = runs_of(path, blank)
        emb = embed_merged(merged_posteriors(probs, runs), w["w0"], w["b0"], w["g"], w["b"]) if runs else torch.zeros(0, hid.shape[-1], dtype=dtype)
        out.append((path, runs, emb))
    return out, gap
