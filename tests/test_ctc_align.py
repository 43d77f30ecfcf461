"""The CPU side of the batched CTC forced alignment: the C ABI declares and binds its entry points, the ops refuse CPU tensors, and
the two halves `ctc_timestamps` was split into (targets from text, stamps from frame labels) reproduce the reference's records on
the injected log-probabilities of tests/golden/sensevoice_ts.npz."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import _lib
from funasr_amd.tokenizer import SentencepiecesTokenizer

from .test_abi import header_symbols
from .test_sensevoice_timestamps import GOLD, _gold, _model

NEW = ("pf_k_ctc_align", "pf_k_ctc_align_scratch_bytes", "pf_k_log_softmax_stats")


def test_header_declares_and_lib_binds_the_new_entry_points():
    declared = header_symbols()
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the scratch query and the argument checks answer without a GPU
    assert int(lib.pf_k_ctc_align_scratch_bytes(2, 10, 3)) >= 2 * 10 * (4 * 4 + 7)
    assert lib.pf_k_ctc_align_scratch_bytes(1, 4097, 1) < 0 and "4096" in _lib.last_error()
    assert lib.pf_k_ctc_align_scratch_bytes(1, 8, 1025) < 0 and "1024" in _lib.last_error()
    assert lib.pf_k_ctc_align_scratch_bytes(0, 8, 8) < 0


def test_ops_refuse_cpu_tensors():
    from funasr_amd import ops
    with pytest.raises(TypeError):
        ops.log_softmax_stats(torch.zeros(3, 7))
    with pytest.raises(TypeError):
        ops.ctc_forced_align(torch.zeros(1, 5, 4), torch.ones(1, 2, dtype=torch.int32), [5], [2])


def test_split_host_helpers_reproduce_the_injected_goldens():
    from funasr_amd.sense_voice import ctc_forced_align
    g = _gold()
    tok = SentencepiecesTokenizer(os.path.join(GOLD, "sv_bpe.model"))
    model = _model(g)
    cases = json.loads(str(g["injected"]))
    assert len(cases) == 16
    for ci, c in enumerate(cases):
        tokens, tg = model.timestamp_targets(c["text"], tok)
        assert tg.dtype == np.int64 and len(tg) >= len(tokens) > 0
        lp = np.array(g[f"logp_{ci}"][4:], dtype=np.float32, copy=True)
        lp[lp.argmax(-1) == model.blank_id, model.blank_id] = 0
        labels = ctc_forced_align(lp, tg, blank=model.blank_id)
        stamps, words = model.stamps_from_labels(tokens, labels.tolist())
        assert words == c["words"], (c["text"], words, c["words"])
        assert [[float(a), float(b)] for a, b in stamps] == c["timestamp"]
        assert (stamps, words) == model.ctc_timestamps(c["text"], g[f"logp_{ci}"][4:], tok)       # the unsplit form: the same records
    assert model.timestamp_targets("", tok) is None              # no pieces: no timestamp


def test_tokens2ids_of_a_list_equals_piece_by_piece():
    """the list form of SentencepiecesTokenizer.encode runs on the calling thread; the ids are those of encoding every piece alone"""
    tok = SentencepiecesTokenizer(os.path.join(GOLD, "sv_bpe.model"))
    for c in json.loads(str(_gold()["injected"])):
        pieces = tok.text2tokens(c["text"])
        assert tok.tokens2ids(pieces) == [tok.encode(p) for p in pieces] and len(pieces) > 4
