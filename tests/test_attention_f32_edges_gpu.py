"""The three kernels of csrc/attention_f32.hip (LDS-DMA, register-staged two-source, few-query) at their tile edges, driven through
pf_k_attention_f32 / pf_k_attention_f32_two_source with every stride given explicitly.

Reference: float64 softmax attention on the CPU -- masked keys go to -inf before the softmax and to 0 after it, so an empty key
sequence gives zero rows. Bars: standard-normal inputs keep the bar of tests/test_kernels_gpu.py for the same kernels,
max |o - ref| < 2e-5. The running-maximum case is not of that distribution: the same formula is evaluated in float32 on the CPU,
gap = max |ref32 - ref64| floored at one fp32 ulp of max |ref64|, and max |o - ref64| <= 4 gap is required.
Measured ratios max |o - ref64| / gap of that case on an MI355X: 0.60 .. 1.29 (per kernel and wave in test_running_maximum_paths).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, DK = 2, 128
D = H * DK
SCALE = DK ** -0.5
BAR = 2e-5


def _ref(q, k, v, klens, dtype=torch.float64, heads=H):
    """softmax((q * scale) k^T, keys >= klens[b] at -inf) with the masked probabilities set to 0, times v; rows of k / v at or
    past klens[b] are replaced by zeros first, so nothing stored there reaches the result"""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    m = torch.arange(Tk)[None, :] >= torch.as_tensor(klens)[:, None]                    # [B, Tk]
    zero = torch.zeros((), dtype=dtype)
    kk = torch.where(m[:, :, None], zero, k.to(dtype))
    vv = torch.where(m[:, :, None], zero, v.to(dtype))
    qh = q.to(dtype).view(B, Tq, heads, DK).transpose(1, 2) * torch.tensor(SCALE, dtype=dtype)
    kh = kk.view(B, Tk, heads, DK).transpose(1, 2)
    vh = vv.view(B, Tk, heads, DK).transpose(1, 2)
    s = (qh @ kh.transpose(-1, -2)).masked_fill(m[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1).masked_fill(m[:, None, None, :], 0.0)                      # (a row of -inf only: NaN -> 0)
    return (p @ vh).transpose(1, 2).reshape(B, Tq, heads * DK)


def _rows_ok(t):
    return t.stride(2) == 1 and (t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1))


def _attn(q, k, v, klens, few=False, out=None, heads=H):
    """pf_k_attention_f32 on device views [B, T, heads * 128] of any row stride; `few` selects the few-query kernel"""
    from funasr_amd import _lib
    lib = _lib.load()
    B, Tq, _ = q.shape
    if out is None:
        out = torch.empty(B, Tq, heads * DK, device=q.device, dtype=torch.float32)
    assert all(_rows_ok(t) for t in (q, k, v, out))
    kl = torch.as_tensor(klens, dtype=torch.int32).to(q.device)
    lib.pf_set_skinny_max_m(1 << 30 if few else 0)
    try:
        _lib.check(lib.pf_k_attention_f32(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), v.data_ptr(), v.stride(1),
                                          out.data_ptr(), out.stride(1), kl.data_ptr(), B, heads, Tq, k.shape[1], SCALE,
                                          torch.cuda.current_stream().cuda_stream), "pf_k_attention_f32")
    finally:
        lib.pf_set_skinny_max_m(0)
    return out


def _attn2(q, k, v, k2, v2, n1, n2, few=False):
    """pf_k_attention_f32_two_source: keys [0, n1[b]) of (k, v), then the first n2 rows of (k2, v2)"""
    from funasr_amd import _lib
    lib = _lib.load()
    B, Tq, _ = q.shape
    out = torch.empty(B, Tq, D, device=q.device, dtype=torch.float32)
    assert all(_rows_ok(t) for t in (q, k, v, k2, v2))
    n1d = torch.as_tensor(n1, dtype=torch.int32).to(q.device)
    lib.pf_set_skinny_max_m(1 << 30 if few else 0)
    try:
        _lib.check(lib.pf_k_attention_f32_two_source(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), v.data_ptr(), v.stride(1),
                                                     k2.data_ptr(), k2.stride(1), v2.data_ptr(), v2.stride(1), out.data_ptr(), D,
                                                     n1d.data_ptr(), 1, B, H, Tq, k.shape[1], k2.shape[1], n2, SCALE,
                                                     torch.cuda.current_stream().cuda_stream), "pf_k_attention_f32_two_source")
    finally:
        lib.pf_set_skinny_max_m(0)
    return out


def _draw(seed, B, Tq, Tk, width=D):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Tq, width, generator=g), torch.randn(B, Tk, width, generator=g), torch.randn(B, Tk, width, generator=g))


def _maxd(a, b):
    return (a.double().cpu() - b.double()).abs().max().item()


# ---------------------------------------------------------------- 1. key and query edges, the LDS-DMA kernel
EDGE_KLENS = [65, 64, 63, 33, 32, 31, 1]


@pytest.mark.parametrize("Tq", [1, 31, 32, 33, 127, 128, 129])
def test_key_and_query_edges_single_source(cuda, Tq):
    """key lengths on both sides of one and two 32-key tiles (and a single key) in 65 allocated rows, query counts on both sides of
    the 32-query wave and the 128-query workgroup"""
    q, k, v = _draw(100 + Tq, len(EDGE_KLENS), Tq, 65)
    out = _attn(q.to(cuda), k.to(cuda), v.to(cuda), EDGE_KLENS)
    d = _maxd(out, _ref(q, k, v, EDGE_KLENS))
    print(f"Tq {Tq}: max |d| {d:.3e}")
    assert d < BAR


# ---------------------------------------------------------------- 2. strided operands and guard bands
@pytest.mark.parametrize("few,T", [(False, 70), (False, 129), (True, 17)])
def test_strided_operands_and_guard_bands(cuda, few, T):
    """Q, K, V as slices of one [B, T, 3 D] buffer (the engine's fused QKV projection), O into a [B, T, D + 8] buffer full of a
    sentinel: the values are bitwise those of the contiguous call, columns >= D and the row behind the last one keep the sentinel"""
    B, klens = 2, [T, T // 2 + 1]
    g = torch.Generator().manual_seed(7 * T)
    qkv = torch.randn(B, T, 3 * D, generator=g).to(cuda)
    q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    flat = torch.full((B * T + 1, D + 8), -777.0, device=cuda)
    out = flat[:B * T].view(B, T, D + 8)
    _attn(q, k, v, klens, few=few, out=out)
    plain = _attn(q.contiguous(), k.contiguous(), v.contiguous(), klens, few=few)
    assert torch.equal(out[:, :, :D], plain)
    assert (out[:, :, D:] == -777.0).all() and (flat[B * T] == -777.0).all()
    assert _maxd(plain, _ref(q.cpu(), k.cpu(), v.cpu(), klens)) < BAR


# ---------------------------------------------------------------- 3. masked rows are never read
POISON_TK, POISON_KLENS = 96, [33, 64, 1]


def _poisoned(t, lens, value=float("nan")):
    t = t.clone()
    for b, n in enumerate(lens):
        t[b, n:] = value
    return t


@pytest.mark.parametrize("few,Tq", [(False, 40), (True, 15)])
def test_masked_rows_are_never_read_single_source(cuda, few, Tq):
    """K / V rows >= klens[b] hold NaN -- for klens 33 and 1 that includes whole trailing tiles: the output is finite and bitwise the
    output with zeros there (a loader that read past its clamp would turn 0 * NaN into NaN)"""
    q, k, v = _draw(31 + Tq, 3, Tq, POISON_TK)
    outs = [_attn(q.to(cuda), _poisoned(k, POISON_KLENS, x).to(cuda), _poisoned(v, POISON_KLENS, x).to(cuda), POISON_KLENS, few=few)
            for x in (float("nan"), 0.0)]
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    assert _maxd(outs[0], _ref(q, k, v, POISON_KLENS)) < BAR


def test_masked_rows_are_never_read_two_sources(cuda):
    """the register-staged kernel: ring rows >= n1[b] and second-source rows >= n2 hold NaN"""
    Tq, T2, n2 = 40, 40, 7
    q, k, v = _draw(5, 3, Tq, POISON_TK)
    _, k2, v2 = _draw(6, 3, 1, T2)
    outs = []
    for x in (float("nan"), 0.0):
        ring = [_poisoned(t, POISON_KLENS, x).to(cuda) for t in (k, v)]
        new = [_poisoned(t, [n2] * 3, x).to(cuda) for t in (k2, v2)]
        outs.append(_attn2(q.to(cuda), ring[0], ring[1], new[0], new[1], POISON_KLENS, n2))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    cat = [torch.stack([torch.cat([a[b, :n], c[b, :n2], torch.zeros(POISON_TK - n, D)]) for b, n in enumerate(POISON_KLENS)])
           for a, c in ((k, k2), (v, v2))]
    assert _maxd(outs[0], _ref(q, cat[0], cat[1], [n + n2 for n in POISON_KLENS])) < BAR


# ---------------------------------------------------------------- 4. empty sequences
@pytest.mark.parametrize("few,Tq", [(False, 33), (True, 15)])
@pytest.mark.parametrize("klens", [[40, 0, 7], [0, 40, 7]])
def test_empty_sequence_gives_zero_rows(cuda, klens, few, Tq):
    """klens[b] == 0: that sequence's rows are exactly zero (the reference's masked_fill(0) after the softmax) -- written, not left --
    and the other sequences are bitwise what they are in a batch without it. The empty sequence's K / V rows hold NaN."""
    q, k, v = _draw(17 + Tq, 3, Tq, 40)
    kd, vd = _poisoned(k, klens).to(cuda), _poisoned(v, klens).to(cuda)
    out = torch.full((3, Tq, D), float("nan"), device=cuda)
    _attn(q.to(cuda), kd, vd, klens, few=few, out=out)
    e = klens.index(0)
    keep = [b for b in range(3) if b != e]
    assert (out[e] == 0).all()
    rest = _attn(q[keep].to(cuda), kd[keep].contiguous(), vd[keep].contiguous(), [klens[b] for b in keep], few=few)
    assert torch.equal(out[keep], rest)
    assert _maxd(out, _ref(q, k, v, klens)) < BAR


# ---------------------------------------------------------------- 5. running-maximum paths
def test_running_maximum_paths(cuda):
    """Three tiles of 32 keys. Per head, keys are a_j u1 + c_j u2 (+ a little noise) for two orthonormal directions and queries lie
    along +u1 (queries 0-31, the first wave) or -u1 (queries 32-63, the second wave), both with a small u2 part: the score of key j
    is +-a_j + ..., and a_j steps up by 40 per tile. So the tile maxima RISE by about 40 per tile for the first wave -- the rescale
    factor exp(m_old - m_new) ~ 4e-18 is far below 2^-24, everything accumulated before vanishes from the sums (it is not zero in
    fp32, that would need a step above 103) -- and FALL by about 40 for the second wave: the running maximum never moves again and
    the later tiles' probabilities exp(s - m) ~ 4e-18, 2e-35 fall below one ulp of the sums.
    Bar: 4 x gap (module docstring). Measured on an MI355X, rising / falling wave: 128-query kernel 0.84 / 1.29,
    few-query kernel 0.75 / 0.60."""
    Tq, Tk = 64, 96
    g = torch.Generator().manual_seed(23)
    a = torch.cat([torch.linspace(0.0, 1.0, 32) + 40.0 * t for t in range(3)])
    qs, ks = [], []
    for _ in range(H):
        u = torch.linalg.qr(torch.randn(DK, 2, generator=g))[0].T
        c = torch.randn(Tk, generator=g)
        ks.append(a[:, None] * u[0] + c[:, None] * u[1] + 0.02 * torch.randn(Tk, DK, generator=g))
        sign = torch.cat([torch.ones(32), -torch.ones(32)])
        w = 0.3 * torch.randn(Tq, generator=g)
        qs.append((sign[:, None] * u[0] + w[:, None] * u[1] + 0.002 * torch.randn(Tq, DK, generator=g)) / SCALE)
    q, k = torch.cat(qs, dim=1)[None], torch.cat(ks, dim=1)[None]
    v = torch.randn(1, Tk, D, generator=g)
    # the construction is what the docstring says
    for h in range(H):
        s = (q[0, :, h * DK:(h + 1) * DK].double() * SCALE) @ k[0, :, h * DK:(h + 1) * DK].double().T
        tmax = s.view(Tq, 3, 32).amax(dim=-1)
        step = tmax[:, 1:] - tmax[:, :-1]
        assert (step[:32] > 35).all() and (step[:32] < 45).all(), "first wave: the tile maxima rise by about 40"
        assert (step[32:] < -35).all() and (step[32:] > -45).all(), "second wave: the tile maxima fall by about 40"
        assert (torch.exp(-step[:32]).float() < 2.0 ** -24).all() and (torch.exp(step[32:]).float() < 2.0 ** -24).all()
    ref64, ref32 = _ref(q, k, v, [Tk]), _ref(q, k, v, [Tk], dtype=torch.float32)
    waves = (slice(0, 32), slice(32, 64))
    tile = _attn(q.to(cuda), k.to(cuda), v.to(cuda), [Tk])
    outs = [("128-query kernel", w, tile[:, w]) for w in waves]
    outs += [("few-query kernel", w, _attn(q[:, w].contiguous().to(cuda), k.to(cuda), v.to(cuda), [Tk], few=True)) for w in waves]
    for name, w, out in outs:                                          # each wave against the gap of its own rows
        m = ref64[:, w].abs().max().float()
        ulp = (torch.nextafter(m, torch.tensor(float("inf"))) - m).item()
        gap = max((ref32[:, w].double() - ref64[:, w]).abs().max().item(), ulp)
        d = _maxd(out, ref64[:, w])
        print(f"running maximum, {name} queries {w.start}-{w.stop - 1}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / gap:.2f} (bar 4)")
        assert torch.isfinite(out).all() and d <= 4 * gap, (name, w, d, gap)


# ---------------------------------------------------------------- 6. few-query kernel edges
FEWQ_KLENS = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 129]


@pytest.mark.parametrize("Tq", [1, 15, 16, 17, 31, 32])
def test_few_query_kernel_edges(cuda, Tq):
    """16 keys per wave and 64 per round: waves with no key (1, 15, 16 keys), a partly filled wave (17, 47, 49), a second and third
    round (65, 129); 16 queries per workgroup: a partly filled one, a second one. Against float64 and the 128-query kernel."""
    q, k, v = _draw(900 + Tq, len(FEWQ_KLENS), Tq, 129)
    few = _attn(q.to(cuda), k.to(cuda), v.to(cuda), FEWQ_KLENS, few=True)
    tile = _attn(q.to(cuda), k.to(cuda), v.to(cuda), FEWQ_KLENS)
    d, dt = _maxd(few, _ref(q, k, v, FEWQ_KLENS)), (few - tile).abs().max().item()
    print(f"few-query Tq {Tq}: max |d| {d:.3e}, against the 128-query kernel {dt:.3e}")
    assert d < BAR and dt < BAR


# ---------------------------------------------------------------- 7. two-source key boundary
N1 = [0, 1, 31, 32, 33]


@pytest.mark.parametrize("few,Tq", [(False, 40), (True, 15)])
@pytest.mark.parametrize("n2", [1, 31, 33])
def test_two_source_key_boundary(cuda, n2, few, Tq):
    """the boundary between the ring and the second source on both sides of the 32-key tile (and of the few-query kernel's 16-key
    waves), with no ring key at all in one sequence; ring rows >= n1[b] and a row behind each second source hold NaN. Equal to the
    single-source call on the physically concatenated keys -- bitwise for the register-staged kernel, which differs from the
    LDS-DMA kernel in how a tile reaches LDS only -- and to float64."""
    B, Tk = len(N1), 48
    q, k, v = _draw(40 * n2 + Tq, B, Tq, Tk)
    _, k2, v2 = _draw(41 * n2 + Tq, B, 1, n2 + 1)
    lens = [n + n2 for n in N1]
    cat = [torch.stack([torch.cat([a[b, :n], c[b, :n2], torch.zeros(max(lens) - n - n2, D)]) for b, n in enumerate(N1)])
           for a, c in ((k, k2), (v, v2))]
    ring = [_poisoned(t, N1).to(cuda) for t in (k, v)]
    new = [_poisoned(t, [n2] * B).to(cuda) for t in (k2, v2)]
    two = _attn2(q.to(cuda), ring[0], ring[1], new[0], new[1], N1, n2, few=few)
    one = _attn(q.to(cuda), cat[0].to(cuda), cat[1].to(cuda), lens)
    d, d1 = _maxd(two, _ref(q, cat[0], cat[1], lens)), (two - one).abs().max().item()
    print(f"two sources n2 {n2} few={few}: max |d| {d:.3e}, against one source {d1:.3e}")
    assert d < BAR and d1 < BAR
    if not few:
        assert torch.equal(two, one)


# ---------------------------------------------------------------- 8. independence and repeatability
def test_rows_and_sequences_are_independent_and_runs_repeat(cuda):
    B, Tq, Tk, klens = 2, 129, 70, [70, 33]
    q, k, v = (t.to(cuda) for t in _draw(77, B, Tq, Tk))
    full = _attn(q, k, v, klens)
    assert torch.equal(full, _attn(q, k, v, klens))
    for r in (0, 31, 32, 127, 128):
        assert torch.equal(_attn(q[:, r:r + 1].contiguous(), k, v, klens), full[:, r:r + 1]), r
    for b in range(B):
        assert torch.equal(_attn(q[b:b + 1], k[b:b + 1], v[b:b + 1], klens[b:b + 1]), full[b:b + 1]), b
    qf = q[:, :17].contiguous()
    few = _attn(qf, k, v, klens, few=True)
    assert torch.equal(few, _attn(qf, k, v, klens, few=True))
    for r in (0, 15, 16):
        assert torch.equal(_attn(qf[:, r:r + 1].contiguous(), k, v, klens, few=True), few[:, r:r + 1]), r
    for b in range(B):
        assert torch.equal(_attn(qf[b:b + 1], k[b:b + 1], v[b:b + 1], klens[b:b + 1], few=True), few[b:b + 1]), b
