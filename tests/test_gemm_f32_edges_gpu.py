"""The exact-fp32 / bf16-operand tile GEMM (csrc/gemm_f32.hip) at both block-tile heights and at every edge of its epilogues, plus the
small-M kernel (csrc/gemm_skinny.hip) on the same small shapes, through ops.gemm, ops.gemm_bf16, ops.conv1d_gemm, ops.gemm_argmax and
the raw pf_k_* calls where a stride or an unaligned pointer is needed.

Which form a shape reaches (64- or 128-row block tiles) is READ from the launcher's own rule, pf_k_gemm_f32_block_rows, and asserted
at the top of every test; nothing here recomputes the rule.

(a) exact: dense seeded integers, A in [-4, 4], W in [1, 7], bias / R1 / R2 in [-8, 8]: every product and partial sum is below 2^24
    (at most 4 * 7 * 2048 + 24), so the fp32 result is exact in any summation order and must EQUAL the float64 evaluation (computed
    with torch on the same device) cast to fp32 -- or rounded once to bf16 for the bf16-output form.
(b) guards, in the same cases: C, A, W, R1, R2 and bias live in NaN buffers, three NaN rows in front and behind, NaN pad columns
    (row strides: A / W K + 4 floats or K + 8 bf16 -- the launcher wants 16-byte operand rows --, C N + 4 and on some cases N + 1, R1
    N + 8, R2 N + 12). A load outside [0, M) x [0, K) makes the result non-finite, a store outside [0, M) x [0, N) clears a NaN.
(c) one fma chain per element, bitwise on random floats: a row does not depend on the tile height; the vector and the element-wise
    epilogue agree; each misalignment alone gives the bits of the aligned call; the gathered im2col equals the materialised one.
(d) precision on random floats: per element against float64, (K + 3) * 2^-24 * (|A||W|^T + |bias| + |R1| + |R2|), the forward-error
    bound of a K-term fp32 product sum followed by three additions in any order. Derived, not measured; not used at K = 2048, where
    it is vacuous ((a) covers long K exactly).
(e) the fused arg-max with the row maximum planted twice across its column boundaries: the lowest index wins.
(f) the launchers' refusals: an error, the output untouched, and a valid call right after is exact.

Every test prints its worst figure (mismatching elements for the exact and bitwise tests, error / bar for (d)).
"""
import pytest
import torch

from funasr_amd import _lib, ops

pytestmark = pytest.mark.gpu

GUARD = 3
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32

# name -> (bias, relu, R1, R2, which addend IS the output buffer)
MODES = {
    "none": (False, False, False, False, None),
    "bias": (True, False, False, False, None),
    "bias_relu": (True, True, False, False, None),
    "r1": (False, False, True, False, None),
    "r2": (False, False, False, True, None),
    "bias_relu_r1_r2": (True, True, True, True, None),
    "r2_is_c": (True, False, False, True, "r2"),
    "r1_is_c": (True, True, True, False, "r1"),
}
MODE_NAMES = tuple(MODES)
M64 = (1, 63, 64, 65, 129)
N64 = (1, 3, 4, 63, 64, 65, 127, 128, 129, 132)
M128 = (1921, 1985, 2048)           # sixteen row panels, the last one holding 1 / 65 / 128 rows
N128 = (3969, 3970, 4033, 4096)     # 32 column blocks, the last one holding 1 / 2 / 65 / 128 columns
KS = {"fp32": (32, 64, 96), "bf16": (64, 128, 192)}


def _block_rows(M, N):
    return int(_lib.load().pf_k_gemm_f32_block_rows(M, N))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    return 0 if t is None else t.stride(0)


def _gemm(a, w, bias=None, relu=False, r1=None, r2=None, out=None, out_bf16=False):
    """ops.gemm / ops.gemm_bf16; the raw bf16 call where the output buffer is the caller's (ops.gemm_bf16 allocates its own)"""
    if a.dtype == F32:
        return ops.gemm(a, w, bias, relu=relu, add1=r1, add2=r2, out=out)
    if out is None:
        return ops.gemm_bf16(a, w, bias, relu=relu, add1=r1, add2=r2, out_bf16=out_bf16)
    M, K = a.shape
    _lib.check(_lib.load().pf_k_gemm_bf16(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(bias), _ptr(r1), _ld(r1), _ptr(r2), _ld(r2),
                                          _ptr(out), out.stride(0), M, w.shape[0], K, int(relu), int(out.dtype == BF16), _stream()),
               "pf_k_gemm_bf16")
    return out


def _ref64(a, w, bias, relu, r1, r2):
    ref = a.double() @ w.double().T
    if bias is not None:
        ref = ref + bias.double()
    if relu:
        ref = torch.relu(ref)
    if r1 is not None:
        ref = ref + r1.double()
    if r2 is not None:
        ref = r2.double() + ref
    return ref


def _framed(t, ld):
    """t [rows, cols] inside a NaN buffer of row stride ld with GUARD NaN rows in front and behind: (buffer, view of t's place)"""
    rows, cols = t.shape
    buf = torch.full((rows + 2 * GUARD, ld), NAN, dtype=t.dtype, device=t.device)
    view = buf[GUARD:GUARD + rows, :cols]
    view.copy_(t)
    return buf, view


def _frame_intact(buf, rows, cols):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + rows:]).all()) and \
        bool(torch.isnan(buf[GUARD:GUARD + rows, cols:]).all())


def _mismatches(got, want):
    """elements of got that are not the bits' value of want (a NaN in got counts)"""
    return int((got != want).sum())


def _ints(gen, shape, lo, hi, cuda):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=cuda).float()


def _exact_case(cuda, dt, M, N, K, mode, c_pad=4):
    """(a) + (b) for one shape: returns the number of mismatching elements (asserted zero by the caller, which prints the total)"""
    has_bias, relu, has_r1, has_r2, alias = MODES[mode]
    gen = torch.Generator(device=cuda).manual_seed(1000003 * M + 1009 * N + 7 * K + MODE_NAMES.index(mode))
    a, w = _ints(gen, (M, K), -4, 4, cuda), _ints(gen, (N, K), 1, 7, cuda)
    bias = _ints(gen, (N,), -8, 8, cuda) if has_bias else None
    r1 = _ints(gen, (M, N), -8, 8, cuda) if has_r1 else None
    r2 = _ints(gen, (M, N), -8, 8, cuda) if has_r2 else None
    want = _ref64(a, w, bias, relu, r1, r2).float()
    assert float(want.abs().max()) < 2.0 ** 24
    odt = BF16 if dt == "bf16" else F32
    k_pad = 8 if dt == "bf16" else 4
    abuf, av = _framed(a.to(odt), K + k_pad)
    wbuf, wv = _framed(w.to(odt), K + k_pad)
    bv = None
    if has_bias:
        bbuf = torch.full((N + 8,), NAN, device=cuda)
        bv = bbuf[4:4 + N]
        bv.copy_(bias)
    bad = 0
    for out_dt in ((F32, BF16) if dt == "bf16" and alias is None else (F32,)):
        cbuf = torch.full((M + 2 * GUARD, N + c_pad), NAN, dtype=out_dt, device=cuda)
        cv = cbuf[GUARD:GUARD + M, :N]
        r1v = r2v = None
        if has_r1:
            if alias == "r1":
                cv.copy_(r1)
                r1v = cv
            else:
                r1buf, r1v = _framed(r1, N + 8)
        if has_r2:
            if alias == "r2":
                cv.copy_(r2)
                r2v = cv
            else:
                r2buf, r2v = _framed(r2, N + 12)
        _gemm(av, wv, bv, relu, r1v, r2v, out=cv)
        torch.cuda.synchronize()
        tag = (dt, M, N, K, mode, c_pad, out_dt)
        assert _frame_intact(cbuf, M, N), ("a store outside [0, M) x [0, N)", tag)
        assert bool(torch.isfinite(cv).all()), ("a load outside the operands reached the result", tag)
        bad += _mismatches(cv, want.to(out_dt))            # (fp32 -> bf16: one round-to-nearest-even of the exact value)
        if has_r1 and alias != "r1":
            assert torch.equal(r1v, r1) and _frame_intact(r1buf, M, N), tag
        if has_r2 and alias != "r2":
            assert torch.equal(r2v, r2) and _frame_intact(r2buf, M, N), tag
    assert torch.equal(av, a.to(odt)) and torch.equal(wv, w.to(odt)) and _frame_intact(abuf, M, K) and _frame_intact(wbuf, N, K)
    return bad


def _shapes(form, ks, mode):
    """(M, N, K, C row pad): every listed M, N and K (and K = 2048) once or more with this mode; the N + 1 output stride on a part"""
    mi = MODE_NAMES.index(mode)
    if form == 64:
        out = [(M, N, ks[(i + j + mi) % len(ks)], 1 if (i + j + mi) % 4 == 0 else 4) for i, M in enumerate(M64) for j, N in enumerate(N64)]
        out.append((129, 132, 2048, 4))
    else:
        out = [(M128[(j + mi) % 3], N, ks[(j + 2 * mi) % len(ks)], 1 if j == mi % 4 else 4) for j, N in enumerate(N128)]
        out.append((2049, 3968, ks[mi % len(ks)], 4))      # 17 panels x 31 blocks: most workgroups of the last XCD round must exit
        out.append((1985, 4033, 2048, 4))
    return out


# ------------------------------------------------------------------------------------------------ (a) + (b)
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("form", [64, 128])
def test_exact_integers_inside_nan_frames(cuda, form, dt, mode):
    shapes = _shapes(form, KS[dt], mode)
    for M, N, _, _ in shapes:
        assert _block_rows(M, N) == form, (M, N)
    assert {s[0] for s in shapes} >= set(M64 if form == 64 else M128 + (2049,))
    assert {s[1] for s in shapes} >= set(N64 if form == 64 else N128 + (3968,))
    assert {s[2] for s in shapes} >= set(KS[dt] + (2048,)) and {s[3] for s in shapes} == {1, 4}
    bad = sum(_exact_case(cuda, dt, M, N, K, mode, c_pad) for M, N, K, c_pad in shapes)
    print(f"exact {form}-row form, {dt}, {mode}: {len(shapes)} shapes, {bad} elements differ from A W^T (ratio {bad})")
    assert bad == 0


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_exact_integers_small_m_kernel(cuda, mode):
    """the 64-form matrix once more through gemm_skinny.hip, with K = 16 and K = 48 (legal there only) added"""
    shapes = _shapes(64, (32, 64, 96, 16, 48), mode)
    assert {s[2] for s in shapes} >= {16, 32, 48, 64, 96, 2048}
    lib = _lib.load()
    lib.pf_set_skinny_max_m(1 << 30)
    try:
        bad = sum(_exact_case(cuda, "fp32", M, N, K, mode, c_pad) for M, N, K, c_pad in shapes)
    finally:
        lib.pf_set_skinny_max_m(0)
    print(f"exact small-M kernel, {mode}: {len(shapes)} shapes, {bad} elements differ from A W^T (ratio {bad})")
    assert bad == 0


# ------------------------------------------------------------------------------------------------ (c)
def _floats(cuda, dt, M, N, K, seed):
    gen = torch.Generator(device=cuda).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=cuda)
    a = rnd(M, K)
    w = rnd(N, K) * K ** -0.5 * torch.linspace(0.5, 1.5, N, device=cuda)[:, None]        # asymmetric: a transposed C write shows
    if dt == "bf16":
        a, w = a.to(BF16), w.to(BF16)
    return a, w, rnd(N), rnd(M, N), rnd(M, N)


def _run_mode(a, w, bias, r1, r2, mode):
    """one contiguous call in `mode` (addends cloned where they are the output)"""
    has_bias, relu, has_r1, has_r2, alias = MODES[mode]
    r1c = r1.clone() if has_r1 else None
    r2c = r2.clone() if has_r2 else None
    out = r1c if alias == "r1" else (r2c if alias == "r2" else None)
    return _gemm(a, w, bias if has_bias else None, relu, r1c, r2c, out=out)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_rows_do_not_depend_on_the_tile_height(cuda, dt):
    """rows [0, 129) of a 128-form run are bitwise the 64-form run on those rows of A alone, in every mode"""
    K, bad, n = KS[dt][2], 0, 0
    for M, N in ((1921, 4096), (1985, 3970)):
        assert _block_rows(M, N) == 128 and _block_rows(129, N) == 64
        a, w, bias, r1, r2 = _floats(cuda, dt, M, N, K, seed=M + N)
        for mode in MODE_NAMES:
            full = _run_mode(a, w, bias, r1, r2, mode)
            part = _run_mode(a[:129].contiguous(), w, bias, r1[:129].contiguous(), r2[:129].contiguous(), mode)
            assert bool(torch.isfinite(full).all())
            bad += _mismatches(full[:129], part)
            n += 1
    print(f"tile height, {dt}: {n} pairs of runs, {bad} elements differ (ratio {bad})")
    assert bad == 0


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("form", [64, 128])
def test_vector_and_elementwise_epilogue_agree(cuda, form, dt):
    """columns [0, N) of the run at N rounded up to 128 (float4 epilogue) are bitwise the run at N (N % 4 != 0: element-wise);
    the element-wise path adds bias, ReLU, R1, R2 in the same order (gemm_f32.hip, both branches of the epilogue)"""
    M, ns = (65, (1, 3, 63, 65, 127, 129, 130)) if form == 64 else (1921, (3969, 3970, 4033))
    K, bad, n = KS[dt][1], 0, 0
    for N in ns:
        Np = (N + 127) // 128 * 128
        assert _block_rows(M, N) == form and _block_rows(M, Np) == form and N % 4 != 0
        a, w, bias, r1, r2 = _floats(cuda, dt, M, Np, K, seed=3 * M + N)
        for mode in MODE_NAMES[:6]:
            wide = _run_mode(a, w, bias, r1, r2, mode)
            narrow = _run_mode(a, w[:N], bias[:N], r1[:, :N].contiguous(), r2[:, :N].contiguous(), mode)
            assert bool(torch.isfinite(wide).all())
            bad += _mismatches(narrow, wide[:, :N])
            n += 1
    print(f"vector against element-wise epilogue, {form}-row form, {dt}: {n} pairs of runs, {bad} elements differ (ratio {bad})")
    assert bad == 0


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("form", [64, 128])
def test_each_misalignment_alone_gives_the_aligned_bits(cuda, form, dt):
    """each trigger of the element-wise epilogue, alone: bias + 1 float, C + 1 float, odd ldc, R1 + 1 float, odd ldr2"""
    M, N = (65, 132) if form == 64 else (1921, 4096)
    K = KS[dt][2]
    assert _block_rows(M, N) == form and N % 4 == 0
    a, w, bias, r1, r2 = _floats(cuda, dt, M, N, K, seed=5 * M + N)
    base = _gemm(a, w, bias, True, r1, r2, out=torch.empty(M, N, device=cuda))
    assert all(t.data_ptr() % 16 == 0 for t in (a, w, bias, r1, r2, base)) and bool(torch.isfinite(base).all())

    def shifted(t):                                      # the same values, one float further
        buf = torch.full((t.numel() + 4,), NAN, device=cuda)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    def widened(t, pad, col0=0):                         # the same values at row stride N + pad, starting at column col0
        buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, device=cuda)
        v = buf[:, col0:col0 + t.shape[1]]
        v.copy_(t)
        return buf, v

    bad = {}
    bad["bias + 1 float"] = _mismatches(_gemm(a, w, shifted(bias), True, r1, r2, out=torch.empty(M, N, device=cuda)), base)
    cbuf, cv = widened(base, 4, 1)
    cbuf.fill_(NAN)
    assert cv.data_ptr() % 16 == 4 and cv.stride(0) % 4 == 0
    bad["C + 1 float"] = _mismatches(_gemm(a, w, bias, True, r1, r2, out=cv), base)
    assert bool(torch.isnan(cbuf[:, 0]).all()) and bool(torch.isnan(cbuf[:, N + 1:]).all())
    cbuf, cv = widened(base, 1)
    cbuf.fill_(NAN)
    assert cv.data_ptr() % 16 == 0 and cv.stride(0) % 2 == 1
    bad["odd ldc"] = _mismatches(_gemm(a, w, bias, True, r1, r2, out=cv), base)
    assert bool(torch.isnan(cbuf[:, N:]).all())
    _, r1v = widened(r1, 4, 1)
    assert r1v.data_ptr() % 16 == 4 and r1v.stride(0) % 4 == 0
    bad["R1 + 1 float"] = _mismatches(_gemm(a, w, bias, True, r1v, r2, out=torch.empty(M, N, device=cuda)), base)
    _, r2v = widened(r2, 1)
    assert r2v.data_ptr() % 16 == 0 and r2v.stride(0) % 2 == 1
    bad["odd ldr2"] = _mismatches(_gemm(a, w, bias, True, r1, r2v, out=torch.empty(M, N, device=cuda)), base)
    print(f"misalignments, {form}-row form, {dt}: elements that differ from the aligned call: {bad} (ratio {sum(bad.values())})")
    assert not any(bad.values())


@pytest.mark.parametrize("form", [64, 128])
def test_gathered_im2col_is_the_materialised_gemm(cuda, form):
    """ops.conv1d_gemm == ops.gemm on the materialised column matrix at D = 32 (a K tile is one whole tap); clips so short that for
    most rows most taps lie outside the clip; odd clips are 1000 x a base clip, so a frame taken from the neighbouring clip shows"""
    D, bad, n = 32, 0, 0
    for T in (1, 2, 5):
        for ci, (taps, left) in enumerate(((3, 1), (5, 0), (5, 4), (2, 0))):
            B = 2 if form == 64 else (2050 + T - 1) // T
            N = (129, 132)[ci % 2] if form == 64 else (3969, 3972)[ci % 2]
            M, K = B * T, taps * D
            assert _block_rows(M, N) == form, (M, N)
            gen = torch.Generator(device=cuda).manual_seed(100 * T + 10 * taps + left)
            h = torch.randn(B, T, D, generator=gen, device=cuda)
            h[1::2] = 1000.0 * h[0:1]
            w = torch.randn(N, K, generator=gen, device=cuda) * K ** -0.5
            bias = torch.randn(N, generator=gen, device=cuda)
            pad = torch.nn.functional.pad(h, (0, 0, left, taps - 1 - left))
            col = torch.cat([pad[:, k:k + T] for k in range(taps)], dim=-1).reshape(M, K).contiguous()
            got = ops.conv1d_gemm(h, w, bias, left=left, relu=True)
            want = ops.gemm(col, w, bias, relu=True)
            assert bool(torch.isfinite(got).all())
            bad += _mismatches(got, want)
            n += 1
    print(f"gathered im2col, {form}-row form: {n} cases, {bad} elements differ (ratio {bad})")
    assert bad == 0


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("form", [64, 128])
def test_precision_against_float64(cuda, form, dt):
    """per element: |C - float64| <= (K + 3) 2^-24 (|A||W|^T + |bias| + |R1| + |R2|); for bf16 the reference takes the bf16-rounded
    operands, so only the fp32 accumulation differs"""
    worst = {}
    for K in KS[dt]:
        for M, N in (((129, 132), (65, 129), (1, 1)) if form == 64 else ((1985, 4033), (2048, 4096))):
            assert _block_rows(M, N) == form
            a, w, bias, r1, r2 = _floats(cuda, dt, M, N, K, seed=11 * M + N + K)
            got = _gemm(a, w, bias, False, r1, r2)
            ref = _ref64(a, w, bias, False, r1, r2)
            mag = a.double().abs() @ w.double().abs().T + bias.double().abs() + r1.double().abs() + r2.double().abs()
            ratio = float(((got.double() - ref).abs() / ((K + 3) * 2.0 ** -24 * mag)).max())
            worst[K] = max(worst.get(K, 0.0), ratio)
    print(f"precision, {form}-row form, {dt}: worst error / bar per K: " + ", ".join(f"K={k}: {v:.4f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst     # (a NaN ratio fails too)


# ------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("M,N,pairs", [
    (1, 129, ((31, 32), (63, 64), (127, 128), (5, 128))),
    (65, 129, ((31, 32), (63, 64), (127, 128), (5, 128))),
    (1, 8404, ((8351, 8352), (8383, 8384), (8319, 8320), (100, 8403), (8402, 8403))),
    (65, 8404, ((8351, 8352), (8383, 8384), (8319, 8320), (100, 8403), (8402, 8403))),
    (1921, 4096, ((31, 32), (2111, 2112), (2047, 2048), (0, 4095))),
])
def test_argmax_ties_across_column_boundaries(cuda, M, N, pairs):
    """exact integers; the row maximum sits in two columns, on either side of a 32-column MFMA tile, a 64-column wave and a
    128-column block boundary, and with the second copy in the last column: the lowest index wins. The second column alone must
    win too, or it was never looked at."""
    form = 128 if M == 1921 else 64
    assert _block_rows(M, N) == form
    K = 32
    gen = torch.Generator(device=cuda).manual_seed(M + N)
    a, w0, bias0 = _ints(gen, (M, K), -4, 4, cuda), _ints(gen, (N, K), 1, 7, cuda), _ints(gen, (N,), -8, 8, cuda)
    bad = 0
    for c1, c2 in pairs:
        assert c1 < c2 < N
        w, bias = w0.clone(), bias0.clone()
        w[c2] = w[c1]
        bias[c2] = 2000.0                                # |A W^T + bias| <= 4 * 7 * 32 + 8 elsewhere
        ids = ops.gemm_argmax(a, w, bias)
        bad += int((ids != c2).sum())
        bias[c1] = 2000.0
        ids = ops.gemm_argmax(a, w, bias)
        bad += int((ids != c1).sum())
    print(f"arg-max ties, {form}-row form, M={M} N={N}: {bad} rows with the wrong index (ratio {bad})")
    assert bad == 0


# ------------------------------------------------------------------------------------------------ (f)
def test_launcher_refusals_leave_the_output_alone(cuda):
    """argument checks that return before any launch: HipRuntimeError with the launcher's message, the NaN output untouched, and
    a valid call straight afterwards exact"""
    lib = _lib.load()
    M, N = 65, 132
    out = torch.full((M, N), NAN, device=cuda)

    def refused(match, fn):
        with pytest.raises(_lib.HipRuntimeError, match=match):
            fn(out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), match
        assert _exact_case(cuda, "fp32", M, N, 32, "bias_relu_r1_r2") == 0

    ones = lambda m, k, dt=F32: torch.ones(m, k, device=cuda, dtype=dt)
    for K in (33, 48):
        refused("gemm: K must be a multiple of 32", lambda o, K=K: ops.gemm(ones(M, K), ones(N, K), out=o))
    refused("gemm: K must be a multiple of 32", lambda o: _gemm(ones(M, 96, BF16), ones(N, 96, BF16), out=o))
    refused("gemm: operand row strides", lambda o: ops.gemm(ones(M, 33)[:, :32], ones(N, 32), out=o))
    abuf = torch.ones(M * 32 + 4, device=cuda)
    a_off = abuf[1:1 + M * 32].view(M, 32)
    assert a_off.data_ptr() % 16 == 4
    refused("gemm: operands must be 16-B aligned", lambda o: ops.gemm(a_off, ones(N, 32), out=o))
    refused("empty problem", lambda o: ops.gemm(ones(M, 32)[:0], ones(N, 32), out=o[:0]))
    hidden, zero = torch.ones(5, 13, 48, device=cuda), torch.zeros(64, device=cuda)
    refused("gemm: the im2col form needs", lambda o: _lib.check(
        lib.pf_k_conv1d_gemm_f32(_ptr(hidden), _ptr(ones(N, 96)), None, _ptr(o), 5, 13, 48, N, 2, 0, 0, _ptr(zero), _stream()), "pf_k_conv1d_gemm_f32"))
    print("refusals: 7 refused calls, 0 outputs touched (ratio 0)")
