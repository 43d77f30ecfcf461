"""Joint CTC-prefix / attention beam search over an AUTOREGRESSIVE decoder (host bookkeeping).

Mirrors `BeamSearch` (funasr/models/transformer/search.py:34-449) for the scorer set `Transformer.init_beam_search` builds
(funasr/models/transformer/model.py:464-512): `decoder` (full scorer, weight 1 - decoding_ctc_weight), `ctc` (`CTCPrefixScorer`,
partial scorer, weight decoding_ctc_weight; present when the model has a CTC head), `length_bonus` (full scorer, weight `penalty`);
`lm` / `ngram` have no scorer object there and never contribute; scorers with weight 0 are dropped (search.py:76-79). Kept as the
reference has them: the pre-beam of int(1.5 * beam) candidates on the weighted sum of the FULL scorers (pre_beam_score_key "full"),
the per-hypothesis expansion with a re-sort after every expanded hypothesis (:324-327), <eos> appended at the last position
(:430-434), `end_detect` (funasr/metrics/common.py).

What differs is where the decoder runs: the reference scores the hypotheses one at a time and recomputes the cross-attention
K / V of the whole memory in every layer at every step; here all running hypotheses of a position go through ONE `step` of a
stepper that keeps its per-hypothesis state itself:
    stepper.begin(max_len, max_hyp)            a new utterance
    stepper.reorder(parents)                   slot k takes the state of slot parents[k] of the previous position
    stepper.step(tokens, pos) -> [n, V]        log-probabilities of the next token for slot k holding tokens[k] at position pos
`funasr_amd.conformer.TransformerDecoder` is such a stepper on the device; the tests drive the same search with a CPU oracle.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .beam_search import CTCPrefixScore, end_detect


@dataclass
class Hypothesis:
    yseq: List[int]
    score: float = 0.0
    scores: Dict[str, float] = field(default_factory=dict)
    ctc_state: Optional[Tuple[float, np.ndarray]] = None     # (previous prefix score, r [T, 2])
    slot: int = 0                                            # the stepper slot that holds this hypothesis' parent state


class BeamSearchTransformer:
    def __init__(self, beam_size: int, vocab_size: int, sos: int, eos: int, ctc_weight: float = 0.0, length_bonus_weight: float = 0.0,
                 blank: int = 0, pre_beam_ratio: float = 1.5, pre_beam: bool = True):
        self.beam_size, self.n_vocab, self.sos, self.eos, self.blank = int(beam_size), int(vocab_size), sos, eos, blank
        self.w_dec, self.w_ctc, self.w_len = 1.0 - float(ctc_weight), float(ctc_weight), float(length_bonus_weight)
        self.pre_beam_size = int(pre_beam_ratio * self.beam_size)
        self.pre_beam = pre_beam

    def _beam(self, weighted: torch.Tensor, ids: torch.Tensor):
        """search.py:197-224"""
        if weighted.size(0) == ids.size(0):
            top = weighted.topk(self.beam_size)[1]
            return top, top
        tmp = weighted[ids]
        weighted[:] = -float("inf")
        weighted[ids] = tmp
        return weighted.topk(self.beam_size)[1], weighted[ids].topk(self.beam_size)[1]

    def _search(self, running: List[Hypothesis], logp: torch.Tensor, ctc: Optional[CTCPrefixScore], dtype) -> List[Hypothesis]:
        """one position (search.py:279-328); logp [len(running), V]"""
        best: List[Hypothesis] = []
        use_ctc = self.w_ctc != 0 and ctc is not None
        do_pre_beam = self.pre_beam and self.pre_beam_size < self.n_vocab and use_ctc
        part_ids = torch.arange(self.n_vocab)
        for k, hyp in enumerate(running):
            weighted = torch.zeros(self.n_vocab, dtype=dtype)
            if self.w_dec != 0:
                weighted += self.w_dec * logp[k]
            if self.w_len != 0:
                weighted += self.w_len * torch.ones(self.n_vocab, dtype=dtype)      # LengthBonus.score: 1 per token
            part_scores = new_state = None
            if use_ctc:
                if do_pre_beam:
                    part_ids = torch.topk(weighted, self.pre_beam_size)[1]
                prev_score, r_prev = hyp.ctc_state
                presub, new_r = ctc(hyp.yseq, part_ids.numpy(), r_prev)
                part_scores = torch.as_tensor(presub - prev_score, dtype=dtype)
                new_state = (presub, new_r)
                weighted[part_ids] += self.w_ctc * part_scores
            weighted += hyp.score
            for j, pj in zip(*self._beam(weighted, part_ids)):
                j, pj = int(j), int(pj)
                scores = dict(hyp.scores)
                if self.w_dec != 0:
                    scores["decoder"] = scores.get("decoder", 0.0) + float(logp[k, j])
                if self.w_len != 0:
                    scores["length_bonus"] = scores.get("length_bonus", 0.0) + 1.0
                st = None
                if part_scores is not None:
                    scores["ctc"] = scores.get("ctc", 0.0) + float(part_scores[pj])
                    st = (new_state[0][pj], new_state[1][pj])
                best.append(Hypothesis(yseq=hyp.yseq + [j], score=float(weighted[j]), scores=scores, ctc_state=st, slot=k))
            best = sorted(best, key=lambda h: h.score, reverse=True)[: min(len(best), self.beam_size)]
        return best

    def __call__(self, stepper, n_frames: int, ctc_logp: Optional[np.ndarray] = None, maxlenratio: float = 0.0,
                 minlenratio: float = 0.0, dtype=torch.float32) -> List[Hypothesis]:
        """n_frames: encoder frames of the utterance (sets the length bounds, search.py:349-355); ctc_logp [T, V] the CTC head's
        log-probabilities (host numpy) or None -> n-best, best first; yseq holds <sos> ... <eos>."""
        if maxlenratio == 0:
            maxlen = int(n_frames)
        elif maxlenratio < 0:
            maxlen = -1 * int(maxlenratio)
        else:
            maxlen = max(1, int(maxlenratio * n_frames))
        ctc = None
        init_state, init_scores = None, {}
        if self.w_ctc != 0 and ctc_logp is not None:
            ctc = CTCPrefixScore(np.asarray(ctc_logp), self.blank, self.eos)
            init_state = (0.0, ctc.initial_state())
            init_scores["ctc"] = 0.0
        if self.w_dec != 0:
            init_scores["decoder"] = 0.0
        if self.w_len != 0:
            init_scores["length_bonus"] = 0.0
        running = [Hypothesis(yseq=[self.sos], score=0.0, scores=init_scores, ctc_state=init_state, slot=0)]
        ended: List[Hypothesis] = []
        stepper.begin(maxlen, max(self.beam_size, 1))
        for i in range(maxlen):
            if i > 0:
                stepper.reorder([h.slot for h in running])
            logp = torch.as_tensor(stepper.step([h.yseq[-1] for h in running], i)).detach().to("cpu", dtype)
            best = self._search(running, logp, ctc, dtype)
            if i == maxlen - 1:                                 # search.py:430-434
                best = [Hypothesis(h.yseq + [self.eos], h.score, h.scores, h.ctc_state, h.slot) for h in best]
            running = []
            for h in best:                                      # final_score() of every scorer here is 0 (scorer_interface.py)
                (ended if h.yseq[-1] == self.eos else running).append(h)
            if maxlenratio == 0.0 and end_detect(ended, i):
                break
            if not running:
                break
        nbest = sorted(ended, key=lambda h: h.score, reverse=True)
        if not nbest and minlenratio >= 0.1:                    # search.py:380-388
            return self(stepper, n_frames, ctc_logp, maxlenratio, max(0.0, minlenratio - 0.1), dtype)
        return nbest
