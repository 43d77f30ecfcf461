"""The Transformer decoder step (`pf_tdecoder`: begin / step / reorder) on the MI355X past the golden-size shapes: a scripted beam
history of 140 positions with up to 40 hypotheses at D = 256, 4 heads, V = 4234 against the float64 oracle (self-attention over
1 .. 140 keys, the reorder copy's second grid-stride trip from position 129, the three small-M GEMM templates), cross-attention
over 1 .. 12000 memory frames, bitwise properties (repeat, a hypothesis alone against the same hypothesis inside the beam, one
handle across utterances), the refusals of step / reorder / begin, and the beam search at beam 10.

Bars as in tests/test_conformer_gpu.py: 4 x max |oracle fp32 - oracle fp64| of the same step (the decoder step is fp32 in both
precision modes); beam scores 8 x the oracle's own fp32 - fp64 score gap."""
import pytest
import torch

from funasr_amd import _lib, synth
from funasr_amd.conformer import Conformer

from . import _conformer_oracle as O
from .test_conformer import BEAM10_TOP, BEAM10_WEIGHTS, beam10_oracle_nbest, beam10_reference_agrees_with_itself, beam10_search, beam10_setup
from .test_conformer_gpu import _check, _maxd

pytestmark = pytest.mark.gpu

V = 4234
N_POS, MAX_HYP = 140, 40
COUNTS = [1, 5, 16, 17, 32, 33, 40, 3]          # hypotheses per position, cycled: below / at / above the small-M template switches at 16 and 32


def _conf():
    return synth.conformer_conf(output_size=256, attention_heads=4, linear_units=512, enc_blocks=0, dec_blocks=2, vocab=V)


def _model(cuda, conf, seed):
    m = Conformer(**conf)
    sd = synth.conformer_state_dict(seed, m)
    m.load_state_dict(sd, strict=True)
    return m.to(cuda), sd


def long_script(seed=7):
    """(tokens, parents) per position: parents from randint(0, n_prev) -- duplicates and drops --, tokens from randint(0, V) with
    0 and V - 1 forced in"""
    g = torch.Generator().manual_seed(seed)
    tokens, parents = [], []
    for pos in range(N_POS):
        n = COUNTS[pos % len(COUNTS)]
        tokens.append(torch.randint(0, V, (n,), generator=g).tolist())
        parents.append(None if pos == 0 else torch.randint(0, len(tokens[-2]), (n,), generator=g).tolist())
    tokens[1][0], tokens[1][1], tokens[N_POS - 1][0], tokens[N_POS - 1][1] = 0, V - 1, V - 1, 0
    return tokens, parents


SHORT_TOKENS = [[1], [5, 9, 17], [30, 31, 32], [40, 41, 42], [3, 4, 5]]        # the script of the small decoder test
SHORT_PARENTS = [None, [0, 0, 0], [0, 0, 2], [2, 1, 0], [0, 1, 1]]


def run_script(stepper, tokens, parents, max_len, max_hyp):
    stepper.begin(max_len, max_hyp)
    outs = []
    for pos, (tok, par) in enumerate(zip(tokens, parents)):
        if par is not None:
            stepper.reorder(par)
        outs.append(torch.as_tensor(stepper.step(tok, pos)).detach().cpu())
    return outs


def _memory(T, D, seed=1):
    return torch.randn(T, D, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def long_run(cuda):
    """the scripted history once: the device's log-probabilities per position on a fresh model, the float64 oracle's, and the float32
    oracle's distance from it (the gap of each position)"""
    conf = _conf()
    model, sd = _model(cuda, conf, 9)
    memory = _memory(130, 256)
    tokens, parents = long_script()
    dec = model.decoder.set_memory(memory.to(cuda))
    st64 = O.DecoderStepper(O.cast(sd), conf["decoder_conf"], memory.double())
    st32 = O.DecoderStepper(O.cast(sd, torch.float32), conf["decoder_conf"], memory)
    got = run_script(dec, tokens, parents, N_POS, MAX_HYP)
    want = run_script(st64, tokens, parents, N_POS, MAX_HYP)
    gaps = [_maxd(a, b) for a, b in zip(run_script(st32, tokens, parents, N_POS, MAX_HYP), want)]
    return dict(conf=conf, model=model, sd=sd, memory=memory, tokens=tokens, parents=parents, got=got, want=want, gaps=gaps)


# ------------------------------------------------------------------------------------------------ against the oracle
def test_scripted_history_of_140_positions_against_the_oracle(long_run):
    """self-attention over 1 .. 140 keys (a lane's second and third key from 65 and 129), the ping-pong reorder at every position
    with duplicated and dropped parents (its second grid-stride trip from position 129: 129 x 512 floats > 64 x 256 float4), M = 1,
    5, 16 | 17, 32 | 33, 40 rows through the small-M GEMMs writing K / V at the slot pitch, V = 4234 (not a multiple of 16) through
    the output layer and the log-softmax. Every position, all rows, against that position's own fp32 - fp64 gap."""
    r = long_run
    assert {len(t) for t in r["tokens"]} == set(COUNTS) and max(len(t) for t in r["tokens"]) == MAX_HYP
    flat = [t for row in r["tokens"] for t in row]
    assert 0 in flat and V - 1 in flat
    assert any(len(set(p)) < len(p) for p in r["parents"][1:])                                          # duplicated parents
    assert any(len(set(p)) < len(prev) for p, prev in zip(r["parents"][1:], r["tokens"]))               # dropped ones
    failed = []
    for pos in range(N_POS):
        assert r["got"][pos].shape == (len(r["tokens"][pos]), V)
        try:
            _check(f"decoder script pos {pos} n {len(r['tokens'][pos])}", r["got"][pos], r["want"][pos], r["gaps"][pos], 4.0)
        except AssertionError as e:                  # every position is printed before the test fails
            failed.append(e.args[0])
    print(f"decoder script: worst ratio {max(_maxd(g, w) / gap for g, w, gap in zip(r['got'], r['want'], r['gaps'])):.2f}")
    assert not failed, failed


@pytest.mark.parametrize("T", [1, 63, 64, 65, 749])
def test_cross_attention_key_counts_against_the_oracle(cuda, long_run, T):
    """memory frames below / at / above the 64 lanes the keys are strided over, one frame, and a 30-s utterance's 749"""
    conf, sd = long_run["conf"], long_run["sd"]
    memory = _memory(T, 256, seed=T)
    tokens, parents = [[1, V - 1, 7], [0, 2000, 4233], [17, 18, 19]], [None, [0, 0, 2], [2, 1, 1]]
    steppers = (long_run["model"].decoder.set_memory(memory.to(cuda)), O.DecoderStepper(O.cast(sd), conf["decoder_conf"], memory.double()),
                O.DecoderStepper(O.cast(sd, torch.float32), conf["decoder_conf"], memory))
    got, want, w32 = [run_script(s, tokens, parents, 3, 3) for s in steppers]
    for pos in range(3):
        _check(f"decoder T={T} pos {pos}", got[pos], want[pos], _maxd(w32[pos], want[pos]), 4.0)


def test_cross_attention_at_the_limit_of_12000_frames(cuda):
    """the documented limit of begin(): 12000 scores of 4 bytes in the attention kernel's dynamic LDS; one frame more is refused"""
    conf = synth.conformer_conf()
    model, sd = _model(cuda, conf, 9)
    memory = _memory(12000, 128, seed=12)
    tokens, parents = [[1, 59], [0, 33]], [None, [1, 1]]
    steppers = (model.decoder.set_memory(memory.to(cuda)), O.DecoderStepper(O.cast(sd), conf["decoder_conf"], memory.double()),
                O.DecoderStepper(O.cast(sd, torch.float32), conf["decoder_conf"], memory))
    got, want, w32 = [run_script(s, tokens, parents, 2, 2) for s in steppers]
    for pos in range(2):
        _check(f"decoder T=12000 pos {pos}", got[pos], want[pos], _maxd(w32[pos], want[pos]), 4.0)
    model.decoder.set_memory(torch.zeros(12001, 128, device=cuda))
    with pytest.raises(_lib.HipRuntimeError, match="12000"):
        model.decoder.begin(2, 2)
    # the refusal left the handle as it was: the utterance above continues
    model.decoder.set_memory(memory.to(cuda))
    assert torch.equal(model.decoder.step(tokens[1], 1).cpu(), got[1])


# ------------------------------------------------------------------------------------------------ bitwise properties
def _equal_runs(tag, a, b):
    assert len(a) == len(b)
    bad = [pos for pos, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
    assert not bad, (tag, bad[:10], len(bad))


def test_scripted_history_twice_is_bitwise_equal(cuda, long_run):
    r = long_run
    dec = r["model"].decoder.set_memory(r["memory"].to(cuda))
    _equal_runs("repeat", run_script(dec, r["tokens"], r["parents"], N_POS, MAX_HYP), r["got"])


def _lineage(tokens, parents, last_pos, last_slot):
    """the slot the hypothesis in `last_slot` of position `last_pos` held at every position up to there, and its token path"""
    slots = [0] * (last_pos + 1)
    slots[-1] = last_slot
    for pos in range(last_pos, 0, -1):
        slots[pos - 1] = parents[pos][slots[pos]]
    return slots, [tokens[pos][s] for pos, s in enumerate(slots)]


def test_a_hypothesis_alone_equals_the_same_hypothesis_inside_the_beam(cuda, long_run):
    """row independence: a row's result depends on its own token path only, not on how many rows share the step (1 against up to
    40: another small-M template), on the slot it sits in, or on the reorders that moved its cache there"""
    r = long_run
    tokens, parents = r["tokens"], r["parents"]
    dec = r["model"].decoder.set_memory(r["memory"].to(cuda))
    through_duplicate = 0
    # the script collapses to one hypothesis every eighth position, so lineages share a trunk; these three end in the last slot of
    # a 17-row, a 40-row and another 40-row position and differ in the branch behind the last collapse before their end
    for last_pos, last in ((N_POS - 1, 16), (134, 39), (70, 39)):
        assert len(tokens[last_pos]) == last + 1
        slots, path = _lineage(tokens, parents, last_pos, last)
        n = last_pos + 1
        # a parent that two or more children of the next position were copied from; the lineage does not stay in slot 0
        through_duplicate += any(parents[pos].count(slots[pos - 1]) >= 2 for pos in range(1, n))
        assert max(slots) >= 16
        alone = run_script(dec, [[t] for t in path], [None] * n, N_POS, 1)
        bad = [pos for pos in range(n) if not torch.equal(alone[pos][0], r["got"][pos][slots[pos]])]
        if bad:
            pos = bad[0]
            print(f"lineage ending at position {last_pos} slot {last}: first difference at position {pos} (slot {slots[pos]} of "
                  f"{len(tokens[pos])}), max |d| {_maxd(alone[pos][0], r['got'][pos][slots[pos]]):.3e}; {len(bad)} of {n} positions differ")
        assert not bad, (last_pos, last, bad[:10], len(bad))
    assert through_duplicate >= 1


def test_one_handle_across_utterances_long_short_long(cuda, long_run):
    """begin() reuses the caches and resets `filled` / `cur`: a 5-position utterance with begin(8, 4) after the 140-position one, then
    the long one again, each bitwise what a fresh model returns"""
    r = long_run
    short_memory = _memory(45, 256, seed=2)
    fresh, _ = _model(cuda, r["conf"], 9)
    short_fresh = run_script(fresh.decoder.set_memory(short_memory.to(cuda)), SHORT_TOKENS, SHORT_PARENTS, 8, 4)
    model, _ = _model(cuda, r["conf"], 9)
    _equal_runs("long 1", run_script(model.decoder.set_memory(r["memory"].to(cuda)), r["tokens"], r["parents"], N_POS, MAX_HYP), r["got"])
    _equal_runs("short", run_script(model.decoder.set_memory(short_memory.to(cuda)), SHORT_TOKENS, SHORT_PARENTS, 8, 4), short_fresh)
    _equal_runs("long 2", run_script(model.decoder.set_memory(r["memory"].to(cuda)), r["tokens"], r["parents"], N_POS, MAX_HYP), r["got"])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_raise_and_leave_the_handle_usable(cuda, long_run):
    """host-side argument checks that return before any launch: each raises through _lib.check, and the valid step repeated after
    it returns the bits it returned before"""
    conf = long_run["conf"]
    model, _ = _model(cuda, conf, 9)
    dec = model.decoder
    with pytest.raises(_lib.HipRuntimeError, match="begin"):
        dec.step([1], 0)                                                    # a handle that never saw begin()
    dec.set_memory(_memory(45, 256, seed=2).to(cuda))
    dec.begin(8, 4)
    dec.step([1], 0)
    dec.reorder([0, 0, 0])
    before = dec.step([5, 9, 17], 1).cpu()                                  # filled = 2
    refused = [("n > max_hyp", lambda: dec.step([1, 2, 3, 4, 5], 1), "max_hyp"),
               ("pos >= max_len", lambda: dec.step([5, 9, 17], 8), "max_len"),
               ("pos > filled", lambda: dec.step([5, 9, 17], 3), "in order"),
               ("token V", lambda: dec.step([5, V, 17], 1), "vocabulary"),
               ("token -1", lambda: dec.step([5, 9, -1], 1), "vocabulary"),
               ("parent >= max_hyp", lambda: dec.reorder([0, 4, 1]), "parent"),
               ("parent < 0", lambda: dec.reorder([0, -1, 1]), "parent")]
    for tag, call, word in refused:
        with pytest.raises(_lib.HipRuntimeError, match=word):
            call()
        assert torch.equal(dec.step([5, 9, 17], 1).cpu(), before), tag


# ------------------------------------------------------------------------------------------------ beam search
def test_beam_search_at_beam_10_against_the_oracle_searches(cuda):
    """beam 10 over a 95-frame memory (seed 21): 10 running hypotheses at every position, memory and CTC log-probabilities shared by
    the three searches, so only the decoder differs. The top-3 token sequences equal the float64 oracle search's and the scores lie
    within 8 x the float32 oracle search's own distance from it (the rule of `gap_nbest_score` of the golden test); that the two
    oracle searches agree with each other is asserted first."""
    gap = beam10_reference_agrees_with_itself()
    conf, sd, memory, ctc_logp, sos, eos = beam10_setup()
    model = Conformer(**conf)
    model.load_state_dict(sd, strict=True)
    model = model.to(cuda)
    nb = beam10_oracle_nbest()
    worst = 0.0
    for w in BEAM10_WEIGHTS:
        got = beam10_search(model.decoder.set_memory(memory.to(cuda)), w, torch.float32)[:BEAM10_TOP]
        assert [h.yseq for h in got] == [h.yseq for h in nb[w, "f64"][:BEAM10_TOP]], w
        for rank, (h, h64) in enumerate(zip(got, nb[w, "f64"])):
            d = abs(h.score - h64.score)
            worst = max(worst, d / gap)
            print(f"beam 10 w={w} rank {rank}: |d score| {d:.3e}, gap {gap:.3e}, ratio {d / gap:.2f} (bar 8)")
            assert d <= 8 * gap, (w, rank, d, gap)
    print(f"beam 10 scores: worst ratio {worst:.2f}")
