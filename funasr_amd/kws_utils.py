"""Keyword parsing and the CTC keyword search of the keyword spotters (funasr/utils/kws_utils.py).

  * `split_mixed_label`, `query_token_set` (:13-87): a keyword string -> (token strings, token ids) over a token table and an
    optional word lexicon (`seg_dict`).
  * `KwsCtcPrefixDecoder` (:90-308): keywords -> token ids and the token set `{0} | all keyword ids`; `.decode(x)` takes the
    encoder output of ONE clip [T, D] (or [T, V] logits where the model has no `ctc_lo`) and returns the reference's
    `(detected, keyword | None, score | None)`. The candidate step runs on the device (`pf_kws_candidates`: 7 words per frame
    come back instead of the [T, V] posterior), the prefix search and the hit test in the library's host code (`pf_kws_search`;
    creating it needs no GPU). `decode_candidates` / `nbest` are the batched and the diagnostic forms.
"""
from __future__ import annotations

import ctypes as C
import logging
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

symbol_str = r'''[’!"#$%&'()*+,\-./:;<>=?@，。?★、…【】《》？“”‘’！\[\]\\^_`{|}~\s]+'''

SCORE_BEAM_SIZE, PATH_BEAM_SIZE = 3, 20            # beam_search's defaults, which the reference never overrides


def split_mixed_label(input_str: str) -> List[str]:
    """a run of Latin letters and `!?,<>()'` is one token, every other character its own (kws_utils.py:13-29)"""
    tokens = []
    s = input_str.lower()
    while len(s) > 0:
        match = re.match(r'[A-Za-z!?,<>()\']+', s)
        word = match.group(0) if match is not None else s[0:1]
        tokens.append(word)
        s = s.replace(word, '', 1).strip(' ')
    return tokens


def query_token_set(txt: str, symbol_table: Dict[str, int], lexicon_table: Optional[Dict[str, Sequence[str]]]):
    """keyword -> (token strings, token ids) (kws_utils.py:32-87). A lexicon of None is an empty one."""
    lexicon_table = lexicon_table or {}
    if txt in symbol_table:
        return (txt,), (symbol_table[txt],)
    tokens_str: Tuple[str, ...] = tuple()
    for part in split_mixed_label(txt):
        if part in ('!sil', '(sil)', '<sil>'):
            tokens_str += ('!sil',)
        elif part == '<blank>':
            tokens_str += ('<blank>',)
        elif part in ('(noise)', 'noise)', '(noise', '<noise>'):
            tokens_str += ('<unk>',)
        elif part in symbol_table:
            tokens_str += (part,)
        elif part in lexicon_table:
            tokens_str += tuple(lexicon_table[part])
        else:
            tokens_str += tuple(re.sub(symbol_str, '', part))
    tokens_idx: Tuple[int, ...] = tuple()
    for ch in tokens_str:
        if ch in symbol_table:
            tokens_idx += (symbol_table[ch],)
        elif ch == '!sil':
            tokens_idx += (symbol_table['sil'] if 'sil' in symbol_table else symbol_table['<blank>'],)
        elif ch == '<unk>':
            tokens_idx += (symbol_table['<unk>'] if '<unk>' in symbol_table else symbol_table['<blank>'],)
        elif '<unk>' in symbol_table:
            tokens_idx += (symbol_table['<unk>'],)
            logging.info(f'\'{ch}\' is not in token set, replace with <unk>')
        else:
            tokens_idx += (symbol_table['<blank>'],)
            logging.info(f'\'{ch}\' is not in token set, replace with <blank>')
    return tokens_str, tokens_idx


def parse_keywords(keywords: str, token_list: Sequence[str], seg_dict: Optional[dict]):
    """`KwsCtcPrefixDecoder.__init__` (:110-123): the string is split on ',' after removing spaces; a repeated keyword collapses
    (dict keys). -> ({keyword: token ids} in first-seen order, the token set {0} | all ids)"""
    if keywords is None:
        raise ValueError("keywords: a comma-separated keyword string is required (AutoModel(keywords=...) or generate(keywords=...))")
    token_table = {}
    for i, token in enumerate(token_list):
        token_table.setdefault(token, i)                 # token_list.index(token): the first occurrence
    table: Dict[str, Tuple[int, ...]] = {}
    idxset = {0}
    for keyword in str(keywords).strip().replace(' ', '').split(','):
        _, ids = query_token_set(keyword, token_table, seg_dict)
        table[keyword] = tuple(int(i) for i in ids)
        idxset.update(table[keyword])
    return table, idxset


class KwsSearch:
    """one `pf_kws_search` handle: keywords as token-id lists, the search over read-back candidates, the n-best of the last decode"""

    def __init__(self, vocab_size: int, keyword_ids: Sequence[Sequence[int]]):
        self._lib = _lib.load()
        self._h = _lib.check_handle(self._lib.pf_kws_search_create(int(vocab_size)), "pf_kws_search_create")
        self.vocab_size = int(vocab_size)
        flat = [int(i) for kw in keyword_ids for i in kw]
        offs = [0]
        for kw in keyword_ids:
            offs.append(offs[-1] + len(kw))
        _lib.check(self._lib.pf_kws_search_set_keywords(self._h, (C.c_int32 * max(1, len(flat)))(*flat), (C.c_int32 * len(offs))(*offs),
                                                        len(keyword_ids)), "pf_kws_search_set_keywords")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.pf_kws_search_destroy(h)
            except Exception:
                pass

    def token_mask(self) -> np.ndarray:
        """uint32 [ceil(V / 32)]: bit id set = blank or a keyword token"""
        n = (self.vocab_size + 31) // 32
        mask = np.zeros(n, np.uint32)
        _lib.check(self._lib.pf_kws_search_token_mask(self._h, mask.ctypes.data_as(C.POINTER(C.c_uint32)), n), "pf_kws_search_token_mask")
        return mask

    def decode(self, cand: np.ndarray, lens: Sequence[int]):
        """cand int32 [B, T, 7] (n, ids[3], fp32 bits of probs[3]) -> (hit [B] keyword index or -1, offset [B], score [B] float64)"""
        cand = np.ascontiguousarray(cand, np.int32)
        if cand.ndim != 3 or cand.shape[2] != 7:
            raise ValueError(f"candidates: expected [B, T, 7] words, got {cand.shape}")
        B, T = int(cand.shape[0]), int(cand.shape[1])
        if len(lens) != B:
            raise ValueError(f"expected {B} lengths, got {len(lens)}")
        hit, off, score = (C.c_int32 * B)(), (C.c_int32 * B)(), (C.c_double * B)()
        _lib.check(self._lib.pf_kws_search_decode(self._h, cand.ctypes.data, (C.c_int32 * B)(*[int(v) for v in lens]), B, T, hit, off, score),
                   "pf_kws_search_decode")
        return list(hit), list(off), list(score)

    def nbest(self, clip: int) -> List[dict]:
        """hypotheses of clip `clip` of the last decode in final order: prefix ids, score (pb + pnb), nodes (token, frame, prob)"""
        n = self._lib.pf_kws_search_nbest_count(self._h, int(clip))
        if n < 0:
            raise IndexError(f"no clip {clip} in the last decode")
        out = []
        for i in range(n):
            score = C.c_double()
            ln = self._lib.pf_kws_search_nbest(self._h, int(clip), i, 0, None, C.byref(score), None, None, None)
            if ln < 0:
                raise _lib.HipRuntimeError(f"pf_kws_search_nbest: {_lib.last_error()}")
            pre, tok, frm, prob = (C.c_int32 * max(1, ln))(), (C.c_int32 * max(1, ln))(), (C.c_int32 * max(1, ln))(), (C.c_double * max(1, ln))()
            self._lib.pf_kws_search_nbest(self._h, int(clip), i, ln, pre, C.byref(score), tok, frm, prob)
            out.append({"prefix": tuple(pre[:ln]), "score": float(score.value),
                        "nodes": [{"token": int(tok[j]), "frame": int(frm[j]), "prob": float(prob[j])} for j in range(ln)]})
        return out


def pack_candidates(n, ids, probs) -> np.ndarray:
    """(n [.., ], ids [.., 3], probs [.., 3] float32) -> the int32 [.., 7] words the device step writes"""
    n, ids, probs = np.asarray(n, np.int32), np.asarray(ids, np.int32), np.asarray(probs, np.float32)
    return np.concatenate([n[..., None], ids, np.ascontiguousarray(probs).view(np.int32)], axis=-1).astype(np.int32)


def candidates(logits, mask_dev, V: Optional[int] = None):
    """device logits [.., V] (last-dimension stride 1; any row stride) -> int32 [rows, 7] on the device. No sync."""
    import torch
    from .hip_module import stream_ptr

    if not logits.is_cuda or logits.dtype != torch.float32:
        raise RuntimeError("kws candidates: expected fp32 logits in GPU memory (there is no CPU path)")
    x = logits if logits.dim() == 2 and logits.stride(1) == 1 else logits.reshape(-1, logits.shape[-1]).contiguous()
    V = int(x.shape[1]) if V is None else int(V)
    M = int(x.shape[0])
    out = torch.empty(M, 7, device=x.device, dtype=torch.int32)
    if M == 0:
        return out
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().pf_kws_candidates(x.data_ptr(), int(x.stride(0)), M, V, mask_dev.data_ptr(), out.data_ptr(), stream_ptr()),
                   "pf_kws_candidates")
    return out


class KwsCtcPrefixDecoder:
    """funasr/utils/kws_utils.py KwsCtcPrefixDecoder. `ctc`: the model's CTC head (its `ctc_lo` projects the encoder output in exact
    fp32) or an object whose `ctc_lo` is None (the FSMN's output is the logits)."""

    def __init__(self, ctc, keywords: str, token_list: list, seg_dict: Optional[dict]):
        self.ctc = ctc
        self.token_list = token_list
        self.keywords_str = keywords
        table, self.keywords_idxset = parse_keywords(keywords, token_list, seg_dict)
        self.keywords_token = {k: {"token_id": v, "token_str": "".join("%s " % str(i) for i in v)} for k, v in table.items()}
        self.keywords = list(table)
        for k, v in table.items():
            if len(v) == 0:
                raise ValueError(f"keywords: {k!r} has no tokens (the reference's sub-list test indexes its first token)")
        self.search = KwsSearch(len(token_list), [table[k] for k in self.keywords])
        self._mask = {}

    def mask_on(self, device):
        import torch
        m = self._mask.get(device)
        if m is None:
            m = self._mask[device] = torch.from_numpy(self.search.token_mask().view(np.int32)).to(device)
        return m

    def logits(self, x):
        lo = getattr(self.ctc, "ctc_lo", None)
        return x if lo is None else self.ctc.logits(x)

    def decode_candidates(self, cand: np.ndarray, lens: Sequence[int]):
        """read-back candidates [B, T, 7] -> [(detected, keyword | None, score | None)] per clip"""
        hit, _, score = self.search.decode(cand, lens)
        return [(True, self.keywords[h], s) if h >= 0 else (False, None, None) for h, s in zip(hit, score)]

    def decode(self, x):
        """x [T, D] (or [T, V]) of one clip, on the device"""
        logits = self.logits(x[None])[0]
        cand = candidates(logits, self.mask_on(logits.device)).cpu().numpy()
        return self.decode_candidates(cand[None], [cand.shape[0]])[0]
