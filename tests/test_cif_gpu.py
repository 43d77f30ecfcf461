"""The CIF scan / emit kernels and the row arg-max of csrc/cif.hip at their edges, on chosen weights.

The scan and emit launches are reached through `ops.cif_tail` (pf_k_cif_tail: the launches the predictor handles make after
their alpha kernel) and compared BIT-EXACTLY with the CPU oracles that restate the reference line by line:
  loop = 0  CifPredictorV2   `O.cif_frames` (cif_v1: float64 prefix sum rounded to float32, fires where floor() changes)
  loop = 1  CifPredictorV3   `bicif_oracle.cif_loop` (`cif`: sequential fp32 integrate, fires on integrate >= 1)
with the tail from `O.cif_tail`. Paths reached here and nowhere else in the suite: the long scan and the unstaged emit
(T + 1 > 4096), the last staged size, the second workgroup of the long scan, tail_mask = 0, len in {1, T - 1, T}, prefix sums
that land exactly on an integer, D that is no multiple of 256, T + 1 that is no multiple of 8, N below / above the number of
fires, an utterance that never fires, a weight above 1, and the refusal of T + 1 > 4096 by the V3 kernels.

Token counts. The reference reports floor(alphas.sum(-1)) (a float32 torch.sum), V2 here the number of fires, V3 floor of a
sequential float64 sum. On rows whose total lies within a few ulp of an integer the reference's own two numbers differ
(predictor), so every count assertion runs on inputs for which `_counts_agree` has first checked, on the CPU, that
floor(float32 sum), floor(sequential float64 sum) and the oracle's number of fires are one number -- for every row.

Without a GPU the `test_*_inputs_*` tests still build every input and reference and check these preconditions.
"""
import functools

import pytest
import torch

from funasr_amd import synth

D_EDGE = 260                     # one full block of 256 channels plus 4
T_V2 = (1, 6, 7, 8, 63, 64, 65, 4095, 4096, 4097)      # T + 1 around 8 and 64; the last staged size; the first unstaged sizes
T_V3 = tuple(t for t in T_V2 if t <= 4095)
TAIL = 0.45
TAIL_LENS = (37, 36, 1, 20)


def fires_of(peaks):
    return torch.floor(peaks) >= 1


def _fit(frames, n):
    """the oracle's frames [B, n_max, D] sliced or zero-padded to n tokens"""
    B, n_max, D = frames.shape
    if n_max >= n:
        return frames[:, :n].contiguous()
    return torch.cat([frames, torch.zeros(B, n - n_max, D)], 1)


def _counts_agree(alphas, n_fired):
    """the precondition of every count assertion (module docstring); returns the common counts"""
    f32 = torch.floor(alphas.sum(-1)).long().tolist()
    f64 = torch.floor(torch.cumsum(alphas.double(), 1)[:, -1]).long().tolist()
    assert f32 == f64 == n_fired.long().tolist(), (f32, f64, n_fired.tolist())
    return f32


def _reference(alphas, hidden, loop):
    """-> dict(frames [B, n_max, D], peaks [B, T], n_fired [B]) of the oracle of the chosen form"""
    if loop:
        from oracle import bicif_oracle as BO
        frames, peaks = BO.cif_loop(hidden, alphas)
    else:
        from oracle import paraformer_oracle as O
        frames, peaks, _ = O.cif_frames(hidden, alphas)
    n_fired = fires_of(peaks).sum(1)
    assert frames.shape[1] >= int(n_fired.max())          # the oracle's own frame count (round(sum)) holds every fire
    return dict(frames=frames, peaks=peaks, n_fired=n_fired)


# ------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def random_case(T, loop, B=3, D=D_EDGE, seed=None):
    g = torch.Generator().manual_seed(1000 + T if seed is None else seed)
    alphas = torch.rand(B, T, generator=g) * 0.6
    hidden = torch.randn(B, T, D, generator=g)
    ref = _reference(alphas, hidden, loop)
    ref.update(alphas=alphas, hidden=hidden, counts=_counts_agree(alphas, ref["n_fired"]))
    return ref


@functools.lru_cache(maxsize=None)
def dyadic_case(loop, B=8, T=200, D=12, seed=0):
    """multiples of 1/64: every prefix sum is exact in any summation order and several land exactly on an integer, where
    `floor changes` (V2) and `integrate >= 1` (V3) are decided by equality"""
    g = torch.Generator().manual_seed(seed)
    alphas = torch.randint(0, 33, (B, T), generator=g).float() / 64
    hidden = torch.randn(B, T, D, generator=g)
    ref = _reference(alphas, hidden, loop)
    assert int((ref["peaks"] == 1.0).sum()) >= 1, "no prefix sum lands on an integer: the case lost its boundary"
    ref.update(alphas=alphas, hidden=hidden, counts=_counts_agree(alphas, ref["n_fired"]))
    return ref


@functools.lru_cache(maxsize=None)
def silent_and_loud_case(loop, T=50, D=D_EDGE, seed=7):
    """row 0 never fires; row 1 holds weights above 1 (smooth_factor > 1): up to 2.5, where floor() jumps by 2 for ONE fire in
    V2 and the V3 integral stays above 1 for several frames; row 2 is ordinary. The loud frames are early, so that the V3
    integral is back below 1 at the last frame (the kernels walk one frame more than a predictor without a tail has)."""
    g = torch.Generator().manual_seed(seed)
    alphas = torch.rand(3, T, generator=g) * 0.6
    hidden = torch.randn(3, T, D, generator=g)
    alphas[0] = 0.0
    alphas[1, [5, 20, 33]] = torch.tensor([2.5, 1.7, 1.3])
    ref = _reference(alphas, hidden, loop)
    assert int(ref["n_fired"][0]) == 0 and int(ref["n_fired"][1]) > 3
    if loop:
        last = ref["peaks"][:, -1]
        assert bool((torch.where(last >= 1, last - 1, last) < 1).all())
        ref.update(counts=_counts_agree(alphas, ref["n_fired"]))
    ref.update(alphas=alphas, hidden=hidden)
    return ref


@functools.lru_cache(maxsize=None)
def tail_case(loop, tail_mask, T=37, D=D_EDGE, seed=11):
    from oracle import paraformer_oracle as O
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(TAIL_LENS)
    B = lens.numel()
    alphas = torch.rand(B, T, generator=g) * 0.6
    alphas = alphas * (torch.arange(T)[None, :] < lens[:, None]).float()        # what alpha_kernel leaves beyond len
    hidden = torch.randn(B, T, D, generator=g)
    al_t, hid_t = O.cif_tail(alphas, hidden, lens, TAIL, bool(tail_mask))
    ref = _reference(al_t, hid_t, loop)
    ref.update(alphas=alphas, hidden=hidden, lens=lens, alphas_tail=al_t, counts=_counts_agree(al_t, ref["n_fired"]))
    return ref


def _min_distance_to_integer(alphas):
    ps = torch.cumsum(alphas, dim=1, dtype=torch.float64).to(torch.float32)
    return float((ps - torch.round(ps)).abs().min())


@functools.lru_cache(maxsize=None)
def predictor_case(idim, tail_mask, T=23, seed=5):
    from oracle import paraformer_oracle as O
    cfg = dict(idim=idim, l_order=1, r_order=1, threshold=1.0, smooth_factor=1.0, noise_threshold=0.0, tail_threshold=TAIL,
               tail_mask=bool(tail_mask))
    sd = synth.predictor_state_dict(cfg, seed=seed)
    lens = torch.tensor([23, 1, 22])
    hidden = torch.randn(3, T, idim, generator=torch.Generator().manual_seed(seed + idim))
    embeds, token_num, alphas, peaks = O.cif_predictor(hidden, lens, sd, cfg)
    # 2e-6 on each weight moves a prefix sum of 24 of them by < 5e-5: with every prefix sum 1e-4 from an integer the fire
    # positions and the count are decided, whatever the order of the dot product in the alpha kernel
    assert _min_distance_to_integer(alphas) >= 1e-4
    assert int(token_num.max()) >= 2
    return dict(cfg=cfg, sd=sd, lens=lens, hidden=hidden, embeds=embeds, token_num=token_num, alphas=alphas, peaks=peaks)


# ------------------------------------------------------------------------------- CPU: every input meets its precondition
def test_v2_inputs_meet_the_count_precondition():
    for T in T_V2:
        random_case(T, 0)
    random_case(4096, 0, B=65, D=4)
    dyadic_case(0)
    silent_and_loud_case(0)
    for tm in (1, 0):
        tail_case(0, tm)


def test_v3_inputs_meet_the_count_precondition():
    for T in T_V3:
        random_case(T, 1)
    dyadic_case(1)
    silent_and_loud_case(1)
    tail_case(1, 1)


def test_oracle_cif_tail_is_the_tail_of_both_predictors():
    """given weights in, the helper puts `tail` at index len (mask) or T and appends a zero frame"""
    from oracle import paraformer_oracle as O
    c = tail_case(0, 1)
    al, hid = c["alphas_tail"], O.cif_tail(c["alphas"], c["hidden"], c["lens"], TAIL, True)[1]
    T = c["alphas"].shape[1]
    assert al.shape == (4, T + 1) and hid.shape == (4, T + 1, D_EDGE) and bool((hid[:, T] == 0).all())
    for b, n in enumerate(TAIL_LENS):
        assert float(al[b, n]) == torch.tensor(TAIL).item() and torch.equal(al[b, :n], c["alphas"][b, :n])
        assert bool((al[b, n + 1:] == 0).all())
    al0 = tail_case(0, 0)["alphas_tail"]
    assert bool((al0[:, T] == torch.tensor(TAIL)).all()) and torch.equal(al0[:, :T], c["alphas"])


def test_predictor_inputs_stay_clear_of_integer_prefix_sums():
    for idim in (256, 320):
        for tm in (1, 0):
            predictor_case(idim, tm)


# --------------------------------------------------------------------------------------------------- GPU: scan and emit
def _run(cuda, alphas, hidden, loop, n=None, lens=None, tail=0.0, tail_mask=1, ref=None):
    from funasr_amd import ops
    B, T = alphas.shape
    if n is None:
        n = max(int(ref["n_fired"].max()), 1)
    al, peaks, nf, ntok, emb = ops.cif_tail(alphas.to(cuda), hidden.to(cuda), [T] * B if lens is None else lens.tolist(), n,
                                            tail_threshold=tail, tail_mask=bool(tail_mask), loop=bool(loop))
    return dict(alphas=al.cpu(), peaks=peaks.cpu(), n_fires=nf.cpu().tolist(), n_tok=None if ntok is None else ntok.cpu().tolist(),
                embeds=emb.cpu(), n=n)


def _check_no_tail(out, ref, loop, counts=True):
    """without a tail the kernels walk T + 1 frames, the last with weight 0: it repeats the integral and cannot fire"""
    T = ref["alphas"].shape[1]
    assert torch.equal(out["alphas"][:, :T], ref["alphas"]) and bool((out["alphas"][:, T] == 0).all())
    assert torch.equal(out["peaks"][:, :T], ref["peaks"])
    assert torch.equal(fires_of(out["peaks"][:, :T]), fires_of(ref["peaks"])) and not bool(fires_of(out["peaks"][:, T]).any())
    assert out["n_fires"] == ref["n_fired"].tolist()
    assert torch.equal(out["embeds"], _fit(ref["frames"], out["n"]))
    if counts:
        assert out["n_fires"] == ref["counts"]
        if loop:
            assert out["n_tok"] == ref["counts"]


@pytest.mark.gpu
@pytest.mark.parametrize("T", T_V2)
def test_v2_scan_and_emit_bit_exact(cuda, T):
    ref = random_case(T, 0)
    _check_no_tail(_run(cuda, ref["alphas"], ref["hidden"], 0, ref=ref), ref, 0)


@pytest.mark.gpu
def test_v2_long_scan_second_workgroup(cuda):
    """B = 65 at T + 1 > 4096: one lane per utterance, the 65th in a second workgroup whose other 63 lanes must leave"""
    ref = random_case(4096, 0, B=65, D=4)
    _check_no_tail(_run(cuda, ref["alphas"], ref["hidden"], 0, ref=ref), ref, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("T", T_V3)
def test_v3_scan_and_emit_bit_exact(cuda, T):
    ref = random_case(T, 1)
    _check_no_tail(_run(cuda, ref["alphas"], ref["hidden"], 1, ref=ref), ref, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", [0, 1])
def test_prefix_sums_exactly_on_an_integer(cuda, loop):
    ref = dyadic_case(loop)
    out = _run(cuda, ref["alphas"], ref["hidden"], loop, ref=ref)
    assert int((out["peaks"] == 1.0).sum()) >= 1
    _check_no_tail(out, ref, loop)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", [0, 1])
def test_utterance_that_never_fires_and_weights_above_one(cuda, loop):
    """V2's count on the loud row is its number of fires, NOT floor(sum) (one fire per frame however far floor() jumps, as in
    the reference's cif_v1), so only the fires are compared there; V3's inputs meet the count precondition"""
    ref = silent_and_loud_case(loop)
    out = _run(cuda, ref["alphas"], ref["hidden"], loop, ref=ref)
    _check_no_tail(out, ref, loop, counts=bool(loop))
    assert out["n_fires"][0] == 0 and bool((out["embeds"][0] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("loop", [0, 1])
@pytest.mark.parametrize("extra", [-1, 0, 3])
def test_fewer_and_more_tokens_than_fires(cuda, loop, extra):
    ref = random_case(65, loop)
    n = int(ref["n_fired"].max()) + extra
    assert n >= 2
    _check_no_tail(_run(cuda, ref["alphas"], ref["hidden"], loop, n=n), ref, loop)


@pytest.mark.gpu
@pytest.mark.parametrize("loop,tail_mask", [(0, 1), (0, 0), (1, 1)])
def test_tail_at_len_and_at_T(cuda, loop, tail_mask):
    ref = tail_case(loop, tail_mask)
    out = _run(cuda, ref["alphas"], ref["hidden"], loop, lens=ref["lens"], tail=TAIL, tail_mask=tail_mask, ref=ref)
    assert torch.equal(out["alphas"], ref["alphas_tail"])
    assert torch.equal(out["peaks"], ref["peaks"])
    assert torch.equal(fires_of(out["peaks"]), fires_of(ref["peaks"]))
    assert out["n_fires"] == ref["n_fired"].tolist() == ref["counts"]
    if loop:
        assert out["n_tok"] == ref["counts"]
    assert torch.equal(out["embeds"], _fit(ref["frames"], out["n"]))


@pytest.mark.gpu
def test_v3_refuses_more_than_4095_frames_and_goes_on(cuda):
    """an error return from the launch functions' own argument check (nothing is launched), then a valid call"""
    from funasr_amd import _lib
    alphas = torch.full((1, 4096), 0.25)
    hidden = torch.zeros(1, 4096, 4)
    with pytest.raises(_lib.HipRuntimeError, match="at most 4095 encoder frames"):
        _run(cuda, alphas, hidden, 1, n=4)
    ref = random_case(7, 1)
    _check_no_tail(_run(cuda, ref["alphas"], ref["hidden"], 1, ref=ref), ref, 1)


# ------------------------------------------------------------------------------------------ GPU: the predictor module
@pytest.mark.gpu
@pytest.mark.parametrize("tail_mask", [1, 0])
@pytest.mark.parametrize("idim", [256, 320])
def test_predictor_v2_at_other_widths(cuda, idim, tail_mask):
    """alpha_kernel's channel loop makes one trip per lane at 256 channels and a second one on 16 of 64 lanes at 320"""
    from funasr_amd.cif_predictor import CifPredictorV2
    c = predictor_case(idim, tail_mask)
    p = CifPredictorV2(**c["cfg"])
    p.load_state_dict(c["sd"], strict=True)
    p = p.to(cuda)
    T = c["hidden"].shape[1]
    mask = (torch.arange(T)[None, :] < c["lens"][:, None]).float()[:, None, :]
    emb, tok, alphas, peaks = p(c["hidden"].to(cuda), None, mask.to(cuda))
    assert tok.cpu().tolist() == c["token_num"].tolist()
    assert (alphas.cpu() - c["alphas"]).abs().max().item() < 2e-6
    assert torch.equal(fires_of(peaks.cpu()), fires_of(c["peaks"]))
    assert emb.shape == c["embeds"].shape
    assert (emb.cpu() - c["embeds"]).abs().max().item() < 2e-5


# ------------------------------------------------------------------------------------------------- GPU: row arg-max
N_ARGMAX = (1, 63, 255, 256, 257, 1793, 2047, 2048, 2049, 4097, 8404)


def first_remainder_column(N):
    """the smallest column argmax_rows_kernel reads in its one-by-one loop: thread tid takes columns tid + 256 u, eight per trip
    while the eighth exists (tid + 2048 k + 1792 < N), the rest one by one. None when every column is read in full trips."""
    firsts = []
    for tid in range(256):
        j = tid
        while j + 7 * 256 < N:
            j += 8 * 256
        if j < N:
            firsts.append(j)
    return min(firsts) if firsts else None


def _argmax(cuda, x):
    from funasr_amd import ops
    return ops.argmax_rows(x.to(cuda)).cpu().long()


@pytest.mark.gpu
@pytest.mark.parametrize("N", N_ARGMAX)
def test_argmax_rows_planted_maximum(cuda, N):
    """against torch.argmax on the CPU. NaN input is out of scope: the kernel's `>` never accepts one, torch.argmax returns it."""
    x = torch.randn(5, N, generator=torch.Generator().manual_seed(N))
    rem = first_remainder_column(N)
    planted = [0, N - 1, 0 if rem is None else rem]
    for r, c in enumerate(planted):
        x[r, c] = 10.0
    ref = x.argmax(-1)
    assert ref[:3].tolist() == planted
    assert torch.equal(_argmax(cuda, x), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [257, 4097])
def test_argmax_rows_first_maximum_wins(cuda, N):
    """equal values: the smallest column, whether the copies meet in one thread (columns c, c + 256), in two lanes of a wave,
    or in two waves (with the smaller column in the LATER wave, and in the earlier one)"""
    pairs = [(0, 256), (3, 70), (65, 100), (10, 200), (200, 10 + 256)]
    if N > 2048 + 300:
        pairs += [(5, 5 + 2048), (300, 300 + 256), (1000, 2048 + 232), (2048 + 7, 2048 + 7 + 256)]
    pairs = [p for p in pairs if max(p) < N]
    x = torch.randn(len(pairs) + 1, N, generator=torch.Generator().manual_seed(N)).clamp_(-4, 4)
    for r, (a, b) in enumerate(pairs):
        x[r, a] = x[r, b] = 10.0
    x[-1] = 0.5                                        # a row of equal values
    ref = x.argmax(-1)
    assert ref.tolist() == [min(p) for p in pairs] + [0]
    assert torch.equal(_argmax(cuda, x), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [63, 2049])
def test_argmax_rows_strided_input(cuda, N):
    from funasr_amd import ops
    base = torch.randn(5, N + 3, generator=torch.Generator().manual_seed(N))
    base[:, N:] = 100.0                                # the padding holds the largest values: read it and the result is wrong
    base[2, N - 1] = 10.0
    ref = base[:, :N].argmax(-1)
    xg = base.to(cuda)[:, :N]
    assert xg.stride(0) == N + 3
    assert torch.equal(ops.argmax_rows(xg).cpu().long(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 257, 2049])
def test_argmax_rows_of_minus_infinity(cuda, N):
    """a row of -inf only gives 0 like torch.argmax (not the 0x7fffffff the search starts from: the streaming decoder uses the
    result as an embedding row); one finite value among -inf gives its column"""
    x = torch.full((3, N), float("-inf"))
    x[1, N // 2] = -5.0
    x[2, N - 1] = -1e30
    ref = x.argmax(-1)
    assert ref.tolist() == [0, N // 2, N - 1]
    assert torch.equal(_argmax(cuda, x), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 300])
def test_gemm_argmax_with_bias_of_minus_infinity(cuda, N):
    """the fused arg-max epilogue and argmax_reduce_kernel start from the same (-inf, 0x7fffffff): every logit -inf gives 0"""
    from funasr_amd import ops
    g = torch.Generator().manual_seed(N)
    a, w = torch.randn(5, 512, generator=g), torch.randn(N, 512, generator=g)
    bias = torch.full((N,), float("-inf"))
    ids = ops.gemm_argmax(a.to(cuda), w.to(cuda), bias.to(cuda)).cpu().tolist()
    assert ids == [0] * 5
    bias[N - 2] = 0.0                                   # one finite column
    ids = ops.gemm_argmax(a.to(cuda), w.to(cuda), bias.to(cuda)).cpu().tolist()
    assert ids == [N - 2] * 5
