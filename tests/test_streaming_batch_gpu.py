"""EVERY stream of a StreamBatch, and steps in which a stream fires no token (the fp32 step; the f16x2 step runs the same checks as
the batch cases of tests/_stream_f16x2_cases.py). The streams bring their own features at a predictor bias of -3.0 / -2.5, where most
10-frame chunks fire nothing on some streams while others decode: n_fired, dec_wp, dec_valid, the K / V rings, the decoder's FSMN
state and the CIF carry then differ between the streams of one batch, and the per-stream gate of the decoder's caches (the
reference skips the decoder when nothing fired, paraformer_streaming/model.py:589-590) is exercised in each of its forms.

References: the reference's own sparse sessions (tests/golden/streaming_sparse.npz), the reference-pinned streaming oracle run per
stream (tests/_stream_batch_common.py: inputs, their preconditions as assertions, bars), and the step against itself where the
code promises the same bits (a stream never depends on its neighbours, graph replay, reset(), re-arranged launches)."""
import pytest

from tests import _stream_batch_common as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("use_graph", [False, True])
def test_reference_sessions_with_chunks_that_fire_nothing(cuda, use_graph):
    worst, zeros = C.reference_sparse_sessions(cuda, "fp32", use_graph)
    print(f"fp32 graph={use_graph}: max |enc - reference| = {worst:.3e}, zero-fire steps = {zeros}")


@pytest.mark.parametrize("name,S", [("sparse_a", 4), ("sparse_b", 4), ("sparse_c", 4), ("sparse_d", 4), ("rows96", 2)])
def test_every_stream_matches_its_own_oracle_session(cuda, name, S):
    seeds = C.GEOMETRIES[name]["seeds"][:S]
    assert len(seeds) == S
    C.check_inputs(name, seeds)
    out, rows = C.run_batch(cuda, name, seeds, "fp32")
    if name == "rows96":
        assert rows > 48, rows                      # the 96-row instance of dec_fsmn_chunk_kernel
    worst, zeros = C.check_vs_oracle(out, name, seeds, "fp32")
    assert zeros > 0 or not C.GEOMETRIES[name]["sparse"]
    print(f"fp32 {name} S={S}: max |enc - oracle| = {worst:.3e}, zero-fire (stream, step) pairs = {zeros}, token rows = {rows}")


@pytest.mark.parametrize("name", ["sparse_a", "sparse_d"])
@pytest.mark.parametrize("ln_carry", [0, 2])
def test_every_stream_equals_its_one_stream_session_bitwise_in_any_order(cuda, ln_carry, name):
    """launch options pinned alike in both runs ("ln_carry" 1 would let one stream carry its LayerNorms in the small-M GEMMs and four
    not: another summation order): stream k of the batch == StreamBatch(model, 1) on stream k's features, ids, encoder window and
    carried CIF state bitwise; the batch with its streams reversed gives the reversed results"""
    seeds = C.GEOMETRIES[name]["seeds"][:4]
    C.check_inputs(name, seeds)
    opts = {"ln_carry": ln_carry}
    batch, _ = C.run_batch(cuda, name, seeds, "fp32", opts)
    for k, s in enumerate(seeds):
        one, _ = C.run_batch(cuda, name, [s], "fp32", opts)
        C.assert_same(one, batch, f"ln_carry {ln_carry}: stream {k} alone / in the batch", streams_b=[k])
    rev, _ = C.run_batch(cuda, name, seeds[::-1], "fp32", opts)
    C.assert_same(batch, rev, f"ln_carry {ln_carry}: streams reversed", streams_b=[3, 2, 1, 0])


@pytest.mark.parametrize("opts", [None, {"ln_carry": 1}], ids=["default", "ln_carry1"])
def test_every_stream_agrees_with_its_one_stream_session_when_options_are_not_pinned(cuda, opts):
    """default options, and "ln_carry" 1, where one stream (15 rows) takes the LayerNorm-carrying GEMMs and four (60 rows) do not -- the
    same ids and counts, encoder windows within 1e-4 (the project's bar for that reordering)"""
    name, seeds = "sparse_a", C.GEOMETRIES["sparse_a"]["seeds"][:4]
    C.check_inputs(name, seeds)
    batch, _ = C.run_batch(cuda, name, seeds, "fp32", opts)
    worst = 0.0
    for k, s in enumerate(seeds):
        one, _ = C.run_batch(cuda, name, [s], "fp32", opts)
        worst = max(worst, C.assert_same(one, batch, f"{opts}: stream {k}", streams_b=[k], enc_tol=1e-4))
    print(f"fp32 {opts}: max |enc one stream - enc in the batch| = {worst:.3e}")


@pytest.mark.parametrize("name", ["sparse_a", "sparse_d"])
def test_the_forms_of_the_zero_fire_gate_agree_on_every_stream(cuda, name):
    """the decoder's K / V append gated per stream by n_fired: one batched launch ("kv_batched" 1), or inside the cross-attention
    (app_gate) / its fallback launch ("kv_batched" 0), each with the encoder's FSMN riding in the attention launch or not: the same ids
    and the same bits of every encoder window. "ln_carry" 2 (the LayerNorm-carrying decoder on 4 x 16 token rows, more than one
    block of the carrying FSMN kernel) against 0: the same ids, windows within 1e-4, and every stream against its oracle session."""
    seeds = C.GEOMETRIES[name]["seeds"][:4]
    zeros = C.check_inputs(name, seeds)
    assert zeros >= 8
    plain, _ = C.run_batch(cuda, name, seeds, "fp32", {"ln_carry": 0, "kv_batched": 0, "fsmn_rides": 0})
    C.check_vs_oracle(plain, name, seeds, "plain launches")
    for kv, rides in ((0, 1), (1, 0), (1, 1)):
        other, _ = C.run_batch(cuda, name, seeds, "fp32", {"ln_carry": 0, "kv_batched": kv, "fsmn_rides": rides})
        C.assert_same(plain, other, f"kv_batched {kv} fsmn_rides {rides}")
    worst = 0.0
    for kv in (0, 1):
        carried, _ = C.run_batch(cuda, name, seeds, "fp32", {"ln_carry": 2, "kv_batched": kv})
        worst = max(worst, C.assert_same(plain, carried, f"ln_carry 2 kv_batched {kv}", enc_tol=1e-4))
        C.check_vs_oracle(carried, name, seeds, f"ln_carry 2 kv_batched {kv}")
    print(f"fp32 {name}: max |enc ln_carry 2 - enc ln_carry 0| = {worst:.3e}, zero-fire (stream, step) pairs = {zeros}")


def test_graph_replay_and_reset_with_diverged_streams(cuda):
    """graph replay == eager bitwise on EVERY stream; reset() after the fourth step -- the streams' dec_wp / dec_valid / n_fired differ
    there (condition (c)) -- and the whole session again == a fresh batch, bitwise on every stream"""
    name, seeds = "sparse_a", C.GEOMETRIES["sparse_a"]["seeds"][:4]
    C.check_inputs(name, seeds)
    eager, _ = C.run_batch(cuda, name, seeds, "fp32", graph=False)
    graph, _ = C.run_batch(cuda, name, seeds, "fp32", graph=True)
    C.assert_same(eager, graph, "graph replay / eager")
    again, _ = C.run_batch(cuda, name, seeds, "fp32", graph=True, reset_after=4)
    C.assert_same(graph, again, "after reset() / fresh")
