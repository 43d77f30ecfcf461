"""Float64 / float32 torch restatement of the keyword spotters' own arithmetic, for the tests and for tools/make_golden_kws.py:
the FSMN with a right context (fsmn_vad_streaming/encoder.py), the candidate rule and the CTC prefix search with its hit test
(utils/kws_utils.py:125-292). The search keeps the reference's object semantics -- nodes are dicts shared between hypotheses,
`copy()` is shallow -- and records what the golden conditions need (decision margins, the largest hypothesis count before a
prune, whether a hypothesis took both `s == last` sub-branches). `deep_copy=True` is a deliberately WRONG variant in which every
hypothesis owns its nodes: the goldens hold a clip on which it gives another answer."""
from __future__ import annotations

import copy
import math
from collections import defaultdict
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F


def cast(sd: Dict[str, torch.Tensor], dt) -> Dict[str, torch.Tensor]:
    return {k: v.to(dt) if v.is_floating_point() else v for k, v in sd.items()}


def memory_block(x: torch.Tensor, w_left: torch.Tensor, w_right: Optional[torch.Tensor], lstride: int, rstride: int) -> torch.Tensor:
    """x [B, T, C], w_left [C, lorder], w_right [C, rorder] or None:
    out[t] = x[t] + sum_j wl[c, j] x[t - (L-1-j) ls] + sum_j wr[c, j] x[t + (j+1) rs], rows outside 0 .. T-1 zero"""
    B, T, C = x.shape
    out = x.clone()
    L = w_left.shape[1]
    for j in range(L):
        d = (L - 1 - j) * lstride
        if d < T:
            out[:, d:] += w_left[:, j] * x[:, : T - d]
    if w_right is not None:
        for j in range(w_right.shape[1]):
            d = (j + 1) * rstride
            if d < T:
                out[:, : T - d] += w_right[:, j] * x[:, d:]
    return out


def fsmn_logits(sd: Dict[str, torch.Tensor], conf: dict, feats: torch.Tensor, prefix: str = "") -> torch.Tensor:
    """the FSMN of `conf` (encoder_conf) without its softmax over feats [B, T, input_dim], in the dtype of `sd`; every row of the
    padded batch is computed, as the reference's `encoder(speech)` does"""
    g = lambda k: sd[prefix + k]                                                                     # noqa: E731
    x = F.linear(feats, g("in_linear1.linear.weight"), g("in_linear1.linear.bias"))
    x = torch.relu(F.linear(x, g("in_linear2.linear.weight"), g("in_linear2.linear.bias")))
    for i in range(conf["fsmn_layers"]):
        p = f"fsmn.{i}."
        h = F.linear(x, g(p + "linear.linear.weight"))
        wr = g(p + "fsmn_block.conv_right.weight")[:, 0, :, 0] if conf["rorder"] > 0 else None
        h = memory_block(h, g(p + "fsmn_block.conv_left.weight")[:, 0, :, 0], wr, conf["lstride"], conf["rstride"])
        x = torch.relu(F.linear(h, g(p + "affine.linear.weight"), g(p + "affine.linear.bias")))
    x = F.linear(x, g("out_linear1.linear.weight"), g("out_linear1.linear.bias"))
    return F.linear(x, g("out_linear2.linear.weight"), g("out_linear2.linear.bias"))


def candidates(logits: torch.Tensor, token_set, margins: bool = False):
    """logits [M, V] -> n [M], ids [M, 3] (-1 from n on), probs [M, 3] (0 from n on) in the dtype of the logits; with `margins`
    also (margin_p, margin_x): the smallest |p - 0.05| over the top-3 ids of the set, and the smallest gap between the third and
    the fourth logit over the rows where either could be kept (p of the third above 0.05)"""
    M, V = logits.shape
    if V < 3:
        raise RuntimeError("selected index k out of range")
    probs = torch.softmax(logits, dim=-1)
    order = torch.sort(logits, dim=-1, descending=True, stable=True)[1]            # equal values: the lower index first
    n = torch.zeros(M, dtype=torch.int64)
    ids = torch.full((M, 3), -1, dtype=torch.int64)
    ps = torch.zeros(M, 3, dtype=logits.dtype)
    margin, margin_x = float("inf"), float("inf")
    tset = set(int(v) for v in token_set)
    for r in range(M):
        for k in range(3):
            i = int(order[r, k])
            p = probs[r, i]
            if i in tset:
                margin = min(margin, abs(float(p) - 0.05))
            if float(p) > 0.05 and i in tset:
                ids[r, n[r]], ps[r, n[r]] = i, p
                n[r] += 1
        if V > 3 and float(probs[r, order[r, 2]]) > 0.05:
            margin_x = min(margin_x, float(logits[r, order[r, 2]] - logits[r, order[r, 3]]))
    return (n, ids, ps, margin, margin_x) if margins else (n, ids, ps)


def beam_search(n, ids, probs, deep_copy: bool = False, path_beam_size: int = 20, info: Optional[dict] = None):
    """kws_utils.py:146-229 over per-frame candidates (the frames of ONE clip). -> [(prefix, pb + pnb, nodes)] in final order.
    `info` (a dict) receives min_margin (ps against the node's prob: absolute), min_margin_rel (neighbours in each prune incl. the
    cut, pb / pnb against 1e-6: relative to the larger of the two, path scores span many decades), max_hyps (before a prune) and
    both_branches."""
    cp = (lambda nodes: copy.deepcopy(nodes)) if deep_copy else (lambda nodes: nodes.copy())
    info = {} if info is None else info
    info.update(min_margin=float("inf"), min_margin_rel=float("inf"), max_hyps=1, both_branches=False)

    def near(a, b):
        if a != b and a != 0.0:             # an exact tie or an exact zero is the same in every precision: order decides, not rounding
            info["min_margin"] = min(info["min_margin"], abs(a - b))

    def near_rel(a, b):
        if a != b and a != 0.0:
            info["min_margin_rel"] = min(info["min_margin_rel"], abs(a - b) / max(abs(a), abs(b)))

    cur_hyps = [(tuple(), (1.0, 0.0, []))]
    for t in range(len(n)):
        if int(n[t]) == 0:
            continue
        next_hyps = defaultdict(lambda: (0.0, 0.0, []))
        for k in range(int(n[t])):
            s, ps = int(ids[t][k]), float(probs[t][k])
            for prefix, (pb, pnb, cur_nodes) in cur_hyps:
                last = prefix[-1] if len(prefix) > 0 else None
                if s == 0:
                    n_pb, n_pnb, nodes = next_hyps[prefix]
                    n_pb = n_pb + pb * ps + pnb * ps
                    nodes = cp(cur_nodes)
                    next_hyps[prefix] = (n_pb, n_pnb, nodes)
                elif s == last:
                    near_rel(abs(pnb), 1e-6)
                    near_rel(abs(pb), 1e-6)
                    a = not math.isclose(pnb, 0.0, abs_tol=0.000001)
                    b = not math.isclose(pb, 0.0, abs_tol=0.000001)
                    info["both_branches"] = info["both_branches"] or (a and b)
                    if a:
                        n_pb, n_pnb, nodes = next_hyps[prefix]
                        n_pnb = n_pnb + pnb * ps
                        nodes = cp(cur_nodes)
                        near(ps, nodes[-1]['prob'])
                        if ps > nodes[-1]['prob']:
                            nodes[-1]['prob'] = ps
                            nodes[-1]['frame'] = t
                        next_hyps[prefix] = (n_pb, n_pnb, nodes)
                    if b:
                        n_prefix = prefix + (s,)
                        n_pb, n_pnb, nodes = next_hyps[n_prefix]
                        n_pnb = n_pnb + pb * ps
                        nodes = cp(cur_nodes)
                        nodes.append(dict(token=s, frame=t, prob=ps))
                        next_hyps[n_prefix] = (n_pb, n_pnb, nodes)
                else:
                    n_prefix = prefix + (s,)
                    n_pb, n_pnb, nodes = next_hyps[n_prefix]
                    if nodes:
                        near(ps, nodes[-1]['prob'])
                        if ps > nodes[-1]['prob']:
                            nodes[-1]['prob'] = ps
                            nodes[-1]['frame'] = t
                    else:
                        nodes = cp(cur_nodes)
                        nodes.append(dict(token=s, frame=t, prob=ps))
                    n_pnb = n_pnb + pb * ps + pnb * ps
                    next_hyps[n_prefix] = (n_pb, n_pnb, nodes)
        info["max_hyps"] = max(info["max_hyps"], len(next_hyps))
        next_hyps = sorted(next_hyps.items(), key=lambda x: (x[1][0] + x[1][1]), reverse=True)
        for a, b in zip(next_hyps[:path_beam_size], next_hyps[1:path_beam_size + 1]):
            near_rel(a[1][0] + a[1][1], b[1][0] + b[1][1])
        cur_hyps = next_hyps[:path_beam_size]
    return [(y[0], y[1][0] + y[1][1], y[1][2]) for y in cur_hyps]


def is_sublist(main_list, check_list):
    if len(main_list) < len(check_list):
        return -1
    if len(main_list) == len(check_list):
        return 0 if tuple(main_list) == tuple(check_list) else -1
    for i in range(len(main_list) - len(check_list) + 1):
        if tuple(main_list[i: i + len(check_list)]) == tuple(check_list):
            return i
    return -1


def decide(hyps, keywords: Sequence[Sequence[int]]):
    """_decode_inside (:267-292) -> (keyword index or -1, offset, score or None)"""
    for prefix, _, nodes in hyps:
        for w, lab in enumerate(keywords):
            off = is_sublist(prefix, lab)
            if off != -1:
                score = 1.0
                for idx in range(off, off + len(lab)):
                    score *= nodes[idx]['prob']
                return w, off, math.sqrt(score)
    return -1, -1, None
