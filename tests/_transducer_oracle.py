"""Restatement of the reference's transducer search pieces (funasr/models/transducer/{rnnt_decoder,joint_network,
beam_search_transducer}.py) in plain torch, dtype- and device-generic (the bench runs it in float32 on the GPU). Written from the
formulas:
    prediction step   x = embed[label]; per layer gates = W_ih x + b_ih + W_hh h + b_hh (i, f, g, o),
                      c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c'), x = h';   dec_out = h' of the last layer
    joint             log_softmax(lin_out(tanh(lin_enc(enc_t) + lin_dec(dec_out))))
    search            default_beam_search as the reference's Transducer drives it (is_final, no LM, nbest by score): Python floats
                      for the scores, `max` = the first of the largest, the prediction step cached by label prefix
The weights are a state dict under the model's keys ("decoder.embed.weight", "joint_network.lin_out.bias", ...); the dtype and
device of the arithmetic are the tensors'. `search(..., margins=True)` also measures the smallest decision margin: the picked
hypothesis against the runner-up, rank k against rank k + 1 of the label scores, every kept score against the termination bound,
and neighbours of the final order."""
from __future__ import annotations

from typing import Dict, List

import torch


def cast(sd: Dict[str, torch.Tensor], dtype, device=None) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype=dtype, device=device) for k, v in sd.items() if k.startswith(("decoder.", "joint_network."))}


def num_layers(sd) -> int:
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("decoder.rnn."))


def init_state(sd):
    w = sd["decoder.rnn.0.weight_hh_l0"]
    L, H = num_layers(sd), w.shape[1]
    return torch.zeros(L, H, dtype=w.dtype, device=w.device), torch.zeros(L, H, dtype=w.dtype, device=w.device)


def pred_step(sd, label: int, state):
    """(h [L, H], c [L, H]) + label -> dec_out [H], (h', c')"""
    h, c = state
    x = sd["decoder.embed.weight"][label]
    hs, cs = [], []
    for l in range(h.shape[0]):
        p = f"decoder.rnn.{l}."
        gates = (sd[p + "weight_ih_l0"] @ x + sd[p + "bias_ih_l0"]) + (sd[p + "weight_hh_l0"] @ h[l] + sd[p + "bias_hh_l0"])
        i, f, g, o = gates.chunk(4)
        cn = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
        x = torch.sigmoid(o) * torch.tanh(cn)
        hs.append(x)
        cs.append(cn)
    return x, (torch.stack(hs), torch.stack(cs))


def dec_proj(sd, dec_out):
    return sd["joint_network.lin_dec.weight"] @ dec_out


def enc_proj(sd, enc_out):
    """[T, D] -> [T, J]"""
    return enc_out @ sd["joint_network.lin_enc.weight"].T + sd["joint_network.lin_enc.bias"]


def joint_logits(sd, enc_p, dec_p):
    return sd["joint_network.lin_out.weight"] @ torch.tanh(enc_p + dec_p) + sd["joint_network.lin_out.bias"]


def joint_logp(sd, enc_p, dec_p):
    return torch.log_softmax(joint_logits(sd, enc_p, dec_p), dim=-1)


def topk_lower_index_first(logp, k: int):
    """the k best of logp[1:], larger first, equal values by lower index -> (values, ids in the full vocabulary)"""
    v, i = torch.sort(logp[1:], descending=True, stable=True)
    return v[:k], i[:k] + 1


def search(sd, enc_out, beam_size: int, nbest: int = 1, margins: bool = False, max_expansions_per_frame: int = None):
    """-> {"ids": [yseq ...], "scores": [...], "joint_evals", "pred_steps", "max_frame_evals" (, "min_margin")}"""
    V = sd["joint_network.lin_out.bias"].shape[0]
    beam_k = min(beam_size, V - 1)
    ep = enc_proj(sd, enc_out)
    cache = {}
    stats = {"joint_evals": 0, "pred_steps": 0, "max_frame_evals": 0}
    margin = [float("inf")]

    def note(d):
        margin[0] = min(margin[0], abs(float(d)))

    kept = [(0.0, [0], init_state(sd))]
    for t in range(enc_out.shape[0]):
        hyps, kept, frame = kept, [], 0
        while True:
            at = max(range(len(hyps)), key=lambda j: hyps[j][0])
            if margins and len(hyps) > 1:
                note(hyps[at][0] - max(h[0] for j, h in enumerate(hyps) if j != at))
            score, yseq, state = hyps.pop(at)
            if max_expansions_per_frame is not None and frame >= max_expansions_per_frame:
                raise RuntimeError(f"frame {t} needs more than {max_expansions_per_frame} joint evaluations")
            key = tuple(yseq)
            if key not in cache:
                dec_out, new_state = pred_step(sd, yseq[-1], state)
                cache[key] = (dec_proj(sd, dec_out), new_state)
                stats["pred_steps"] += 1
            dp, new_state = cache[key]
            logp = joint_logp(sd, ep[t], dp)
            stats["joint_evals"] += 1
            frame += 1
            stats["max_frame_evals"] = max(stats["max_frame_evals"], frame)
            vals, ids = topk_lower_index_first(logp, min(beam_k + 1, V - 1))
            if margins and vals.shape[0] > beam_k:
                note(vals[beam_k - 1] - vals[beam_k])
            kept.append((score + float(logp[0]), yseq, state))
            for v, i in zip(vals[:beam_k].tolist(), ids[:beam_k].tolist()):
                hyps.append((score + v, yseq + [i], new_state))
            hyps_max = max(h[0] for h in hyps)
            if margins:
                for h in kept:
                    note(h[0] - hyps_max)
            most = sorted([h for h in kept if h[0] > hyps_max], key=lambda h: h[0])
            if len(most) >= beam_size:
                kept = most
                break
    kept.sort(key=lambda h: h[0], reverse=True)
    if margins:
        for a, b in zip(kept, kept[1:]):
            note(a[0] - b[0])
    out = dict(stats, ids=[h[1] for h in kept[:nbest]], scores=[h[0] for h in kept[:nbest]])
    if margins:
        out["min_margin"] = margin[0]
    return out
