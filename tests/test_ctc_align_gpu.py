"""Batched CTC forced alignment on the device (csrc/ctc_align.hip through `ops.ctc_forced_align`) and the row statistics kernel
(`ops.log_softmax_stats`), label for label against the host restatement `funasr_amd.sense_voice.ctc_forced_align` -- itself pinned to
the reference function by tests/golden/ctc_forced_align.npz -- or against those recorded labels. Equality is exact everywhere.

The batches are built with numpy (`batches()`): without a GPU `test_batches_are_what_they_claim` still builds every
one of them with its host labels and checks the properties the GPU cases rely on (sizes at the ownership boundaries, ties, -inf,
infeasible targets).
"""
import functools
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V_EDGE = 37
# S = 2 L + 1 in {63, 65, 127, 129, 255, 257, 513}: around one wave, two waves, the workgroup's 256 threads and two states per thread
L_DENSE = (31, 32, 63, 64, 127, 128, 256)


def _log_probs(rng, *shape):
    x = (rng.standard_normal(shape) * 2).astype(np.float32)
    return torch.log_softmax(torch.from_numpy(x), -1).numpy()


def _batch(clips, blank=0, t0=0, pad_rows=1, with_pred=False):
    """clips: [(emissions [T_b + t0, V_b], targets [L_b])] -> one ragged batch. T is padded with NaN rows (and `pad_rows` more), V to
    the widest clip with NaN columns: neither may ever be read."""
    B = len(clips)
    T = max(c[0].shape[0] for c in clips) + pad_rows
    V = max(c[0].shape[1] for c in clips)
    Lm = max(len(c[1]) for c in clips)
    em = np.full((B, T, V), np.nan, dtype=np.float32)
    tg = np.full((B, Lm), blank, dtype=np.int32)
    for b, (e, y) in enumerate(clips):
        em[b, :e.shape[0], :e.shape[1]] = e
        tg[b, :len(y)] = y
    out = dict(em=em, targets=tg, in_lens=[c[0].shape[0] - t0 for c in clips], tg_lens=[len(c[1]) for c in clips], blank=blank, t0=t0,
               pred=None)
    if with_pred:                                                # the row arg-max over each clip's own columns (NaN rows: 0)
        out["pred"] = np.stack([np.concatenate([c[0].argmax(-1), np.zeros(T - c[0].shape[0], dtype=np.int64)]) for c in clips]).astype(np.int32)
    return out


def host_labels(bt):
    """the oracle: the host restatement clip by clip, on the rows from t0, the blank fix applied as the host path applies it"""
    from funasr_amd.sense_voice import ctc_forced_align
    B, T, _ = bt["em"].shape
    t0, blank = bt["t0"], bt["blank"]
    out = np.full((B, T - t0), -1, dtype=np.int32)
    for b in range(B):
        n, L = bt["in_lens"][b], bt["tg_lens"][b]
        if n == 0:
            continue
        lp = bt["em"][b, t0:t0 + n].copy()
        if bt["pred"] is not None:
            lp[bt["pred"][b, t0:t0 + n] == blank, blank] = 0
        with np.errstate(invalid="ignore"):
            out[b, :n] = ctc_forced_align(lp, bt["targets"][b, :L], blank=blank)
    return out


def _recorded():
    from oracle.make_golden_forced_align import cases
    return _batch([(lp[0].numpy(), tg[0].numpy()) for lp, tg in cases()])


def _edge_clips():
    """name -> (emissions [T, V_EDGE], targets): every edge of the issue's list as one clip"""
    rng = np.random.default_rng(7)
    distinct = lambda L: (np.arange(L) % (V_EDGE - 1) + 1).astype(np.int32)          # neighbours differ: feasible at T = L
    clips = {}
    for T in (1, 2, 3):
        clips[f"T{T}_L1"] = (_log_probs(rng, T, V_EDGE), np.array([5], dtype=np.int32))
    clips["T7_L1"] = (_log_probs(rng, 7, V_EDGE), np.array([3], dtype=np.int32))
    clips["T2_L2"] = (_log_probs(rng, 2, V_EDGE), distinct(2))
    clips["T6_L6_no_blank_fits"] = (_log_probs(rng, 6, V_EDGE), distinct(6))
    clips["T11_L5_all_equal"] = (_log_probs(rng, 11, V_EDGE), np.full(5, 9, dtype=np.int32))   # every diff false; needs 2 L - 1 frames
    clips["T40_L3_mostly_blank"] = (_log_probs(rng, 40, V_EDGE), distinct(3))
    for L in L_DENSE:                                            # T = S: more than one back-trace trip of 32 frames from L = 31 on
        clips[f"S{2 * L + 1}"] = (_log_probs(rng, 2 * L + 1, V_EDGE), rng.integers(1, V_EDGE, L).astype(np.int32))
    clips["S513_T_eq_L"] = (_log_probs(rng, 256, V_EDGE), distinct(256))
    return clips


def _ties():
    """emissions from multiples of 0.5: sums are exact, equal scores are frequent, the first-maximum order decides"""
    rng = np.random.default_rng(11)
    clips = []
    for _ in range(200):
        T, L, V = int(rng.integers(1, 25)), int(rng.integers(1, 9)), int(rng.integers(3, 7))
        clips.append(((-0.5 * rng.integers(0, 5, (T, V))).astype(np.float32), rng.integers(1, V, L).astype(np.int32)))
    return _batch(clips)


def _minus_inf():
    rng = np.random.default_rng(13)
    clips = []
    for k in range(24):
        T, L, V = int(rng.integers(2, 30)), int(rng.integers(1, 7)), 9
        e = _log_probs(rng, T, V)
        y = rng.integers(1, V, L).astype(np.int32)
        e[:, int(y[k % L])] = -np.inf                           # a banned column among the clip's own labels: no finite path
        if k % 3 == 0:
            e[T // 2:, 0] = -np.inf                             # and the blank from the middle on
        clips.append((e, y))
    for k in range(24):                                          # one label banned in SOME frames only: finite paths remain
        T, L, V = int(rng.integers(8, 30)), int(rng.integers(1, 4)), 9
        e = _log_probs(rng, T, V)
        y = rng.integers(1, V, L).astype(np.int32)
        e[rng.integers(0, T, 3), int(y[0])] = -np.inf
        clips.append((e, y))
    return _batch(clips)


def _infeasible():
    """L + repeats > T: no path through the targets exists; the recurrence still determines every label"""
    rng = np.random.default_rng(17)
    clips = []
    for T, L in ((1, 2), (1, 5), (2, 3), (3, 7), (4, 4), (5, 4), (9, 8), (20, 40), (33, 70), (64, 200)):
        y = rng.integers(1, V_EDGE, L).astype(np.int32)
        if T >= L:
            y[:] = y[0]                                          # T >= L made infeasible by repeats (each needs a blank between)
        assert L + int((y[1:] == y[:-1]).sum()) > T
        clips.append((_log_probs(rng, T, V_EDGE), y))
    return _batch(clips)


def _offset():
    """t0 = 4 with the blank fix: blank-heavy emissions so that `pred == blank` is frequent; blank = 0 and, once, blank = 2"""
    rng = np.random.default_rng(19)
    out = {}
    for blank in (0, 2):
        clips = []
        for _ in range(12):
            T, L, V = int(rng.integers(1, 40)), int(rng.integers(1, 7)), 11
            x = (rng.standard_normal((T + 4, V)) * 2).astype(np.float32)
            x[:, blank] += 3
            y = rng.integers(0, V, L).astype(np.int32)          # may hold the blank itself (an ignore id mapped to it)
            clips.append((torch.log_softmax(torch.from_numpy(x), -1).numpy(), y))
        out[blank] = _batch(clips, blank=blank, t0=4, with_pred=True)
    return out


@functools.lru_cache(maxsize=None)
def batches():
    """name -> batch, each with its host labels under "want" (computed once, never changed)"""
    edge = _edge_clips()
    out = {f"edge_{k}": _batch([v]) for k, v in edge.items()}
    out["edges_mixed"] = _batch(list(edge.values()))
    rng = np.random.default_rng(23)
    out["L1024_T2049"] = _batch([(_log_probs(rng, 2049, V_EDGE), rng.integers(1, V_EDGE, 1024).astype(np.int32))])
    out["ties"] = _ties()
    out["minus_inf"] = _minus_inf()
    out["infeasible"] = _infeasible()
    for blank, bt in _offset().items():
        out[f"offset_blank{blank}"] = bt
    out["recorded"] = _recorded()
    for bt in out.values():
        bt["want"] = host_labels(bt)
    return out


NAMES = ([f"edge_{k}" for k in _edge_clips()] +
         ["edges_mixed", "L1024_T2049", "ties", "minus_inf", "infeasible", "offset_blank0", "offset_blank2", "recorded"])


def test_batches_are_what_they_claim():
    bs = batches()
    assert sorted(bs) == sorted(NAMES)
    g = np.load(os.path.join(GOLD, "ctc_forced_align.npz"), allow_pickle=False)
    rec = bs["recorded"]
    assert rec["in_lens"] == g["lengths"].tolist() and len(rec["in_lens"]) > 150
    assert np.array_equal(np.concatenate([rec["want"][b, :n] for b, n in enumerate(rec["in_lens"])]), g["labels"])   # the reference's own labels
    assert np.isnan(rec["em"]).any() and rec["em"].shape[2] == 11
    assert sorted(2 * L + 1 for L in bs["edges_mixed"]["tg_lens"] if L >= 31)[:7] == [63, 65, 127, 129, 255, 257, 513]
    assert bs["L1024_T2049"]["tg_lens"] == [1024] and bs["L1024_T2049"]["in_lens"] == [2049]
    assert (bs["ties"]["em"][np.isfinite(bs["ties"]["em"])] % 0.5 == 0).all() and len(bs["ties"]["in_lens"]) == 200
    assert np.isneginf(bs["minus_inf"]["em"]).any()
    for name in ("offset_blank0", "offset_blank2"):
        bt = bs[name]
        on_clip = np.concatenate([bt["pred"][b, 4:4 + n] for b, n in enumerate(bt["in_lens"])])
        assert bt["t0"] == 4 and 0.2 < (on_clip == bt["blank"]).mean() < 0.9
    # a feasible clip's labels collapse to its targets
    bt = bs["edges_mixed"]
    for b, (n, L) in enumerate(zip(bt["in_lens"], bt["tg_lens"])):
        row = bt["want"][b, :n]
        keep = np.concatenate([[True], row[1:] != row[:-1]])
        assert [v for v in row[keep].tolist() if v != 0] == bt["targets"][b, :L].tolist(), b
        assert (bt["want"][b, n:] == -1).all()


def _run(bt, cuda, ld_extra=0, **kw):
    from funasr_amd import ops
    em = torch.from_numpy(bt["em"])
    if ld_extra:                                                 # a row-strided view: V columns of wider rows, NaN behind
        wide = torch.full(em.shape[:2] + (em.shape[2] + ld_extra,), float("nan"))
        wide[..., :em.shape[2]] = em
        em = wide.to(cuda)[..., :bt["em"].shape[2]]
        assert em.stride(1) == bt["em"].shape[2] + ld_extra
    else:
        em = em.to(cuda)
    pred = None if bt["pred"] is None else torch.from_numpy(bt["pred"]).to(cuda)
    got = ops.ctc_forced_align(em, torch.from_numpy(bt["targets"]).to(cuda), bt["in_lens"], bt["tg_lens"], blank=bt["blank"],
                               t0=bt["t0"], pred=pred, **kw)
    assert got.dtype == torch.int32 and tuple(got.shape) == bt["want"].shape
    return got.cpu().numpy()


def _same(got, bt):
    bad = np.argwhere(got != bt["want"])
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [(bt["in_lens"][b], bt["tg_lens"][b]) for b in sorted({int(r[0]) for r in bad[:5]})])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_labels_equal_the_host_restatement(cuda, name):
    bt = batches()[name]
    _same(_run(bt, cuda), bt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["offset_blank0", "offset_blank2", "edges_mixed"])
def test_row_strided_emissions(cuda, name):
    bt = batches()[name]
    _same(_run(bt, cuda, ld_extra=5), bt)


@pytest.mark.gpu
def test_fill_behind_the_clip_and_poisoned_scratch(cuda):
    from funasr_amd import _lib
    bs = batches()
    for name in ("edges_mixed", "offset_blank0", "minus_inf"):
        bt = bs[name]
        n = int(_lib.load().pf_k_ctc_align_scratch_bytes(len(bt["in_lens"]), max(bt["in_lens"]), max(bt["tg_lens"])))
        assert n > 0
        scratch = torch.full((n,), 0xff, dtype=torch.uint8, device=cuda)       # every float a NaN, every back-pointer 255
        got = _run(bt, cuda, scratch=scratch)
        _same(got, bt)
        for b, m in enumerate(bt["in_lens"]):
            assert (got[b, m:] == -1).all() and (got[b, :m] >= 0).all()
    # a clip without frames keeps the fill, beside one that has them
    bt = bs["edges_mixed"]
    cut = dict(bt, in_lens=[0 if b % 2 else m for b, m in enumerate(bt["in_lens"])])
    cut["want"] = host_labels(cut)
    assert (cut["want"][1] == -1).all()
    _same(_run(cut, cuda), cut)


def _stats_input(M, N, ldx):
    g = torch.Generator().manual_seed(100 * M + N)
    x = torch.full((M, ldx), float("nan"))
    x[:, :N] = torch.randn(M, N, generator=g) * 3
    if N > 1:
        x[:, N // 2] = float("-inf")                             # a banned class
    if N >= 64:                                                  # logits one ulp apart around the maximum: they may round to one
        top = x[:, :N].max(-1).values + 1                        # log-probability, and then the first column wins
        x[:, N - 2] = top
        x[:, 5] = torch.nextafter(top, top - 1)
        x[:, N - 1] = top
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 25055])
@pytest.mark.parametrize("M", [1, 5])
def test_log_softmax_stats(cuda, M, N):
    from funasr_amd import ops
    for ldx in (N, N + 3):
        x = _stats_input(M, N, ldx).to(cuda)[:, :N]
        lse, pred = ops.log_softmax_stats(x)
        assert tuple(lse.shape) == (M,) and lse.dtype == torch.float32 and tuple(pred.shape) == (M,) and pred.dtype == torch.int32
        lp = ops.log_softmax(x.contiguous())
        assert torch.equal(x - lse[:, None], lp)                 # bit for bit what log_softmax stores (-inf columns included)
        assert torch.equal(pred, ops.argmax_rows(lp))
        assert not torch.isnan(lse).any()


@pytest.mark.gpu
def test_logits_with_lse_give_the_labels_of_the_log_probabilities(cuda):
    from funasr_amd import ops
    for name in ("offset_blank0", "edges_mixed", "ties"):
        bt = batches()[name]
        B, T, V = bt["em"].shape
        g = torch.Generator().manual_seed(5)
        x = torch.from_numpy(np.nan_to_num(bt["em"], nan=0.0, neginf=-40.0)) * 1.5 + torch.randn(B, T, 1, generator=g) * 4   # logits: rows shifted
        x = x.to(cuda)
        tg = torch.from_numpy(bt["targets"]).to(cuda)
        lse, pred = ops.log_softmax_stats(x)
        lp = ops.log_softmax(x)
        assert torch.equal(pred.view(-1), ops.argmax_rows(lp.view(B * T, V)))
        a = ops.ctc_forced_align(x, tg, bt["in_lens"], bt["tg_lens"], blank=bt["blank"], t0=bt["t0"], pred=pred, lse=lse)
        b = ops.ctc_forced_align(lp, tg, bt["in_lens"], bt["tg_lens"], blank=bt["blank"], t0=bt["t0"], pred=pred)
        assert torch.equal(a, b)
        host = dict(bt, em=lp.cpu().numpy(), pred=pred.cpu().numpy())
        assert np.array_equal(a.cpu().numpy(), host_labels(host))


@pytest.mark.gpu
def test_limits_are_refused_before_any_launch(cuda):
    from funasr_amd import _lib, ops
    lib = _lib.load()
    em = torch.zeros(1, 4097, 4, device=cuda)
    tg = torch.ones(1, 1025, dtype=torch.int32, device=cuda)
    for in_len, tg_len, word in ((4097, 3, "4096"), (8, 1025, "1024"), (8, 0, "without target"), (-1, 3, "4096")):
        with pytest.raises(_lib.HipRuntimeError, match=word):
            ops.ctc_forced_align(em, tg, [in_len], [tg_len])
        assert word in _lib.last_error()
    assert lib.pf_k_ctc_align_scratch_bytes(1, 4097, 1) < 0 and lib.pf_k_ctc_align_scratch_bytes(1, 8, 1025) < 0
    assert int(lib.pf_k_ctc_align_scratch_bytes(1, 4096, 1024)) > 4096 * 2049
    # a scratch smaller than the query's answer is refused too
    with pytest.raises(_lib.HipRuntimeError, match="scratch"):
        ops.ctc_forced_align(em, tg, [8], [3], scratch=torch.empty(16, dtype=torch.uint8, device=cuda))
