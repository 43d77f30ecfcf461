"""The row kernels of csrc/rowwise.hip (LayerNorm, FSMN memory block, log-softmax, bf16 cast, LayerNorm constants) at their edges,
driven through the pf_k_* hooks with every stride given explicitly: both sides of every template switch and tile, strided
operands, sentinel guard bands around every output, NaN wherever the kernel has no business reading.

References are float64 evaluations on the CPU. Bars: where tests/test_kernels_gpu.py has a bar for the same kernel on the same input
distribution it is kept (LayerNorm 5e-6, FSMN with 11 taps of 0.3 randn 1e-5). Elsewhere the `4 x gap` rule of the model ports: the
same formula evaluated in float32 on the CPU, gap = max |ref32 - ref64| floored at one fp32 ulp of max |ref64|, and
max |out - ref64| <= 4 gap. Largest measured ratios max |out - ref64| / gap on an MI355X:
    LayerNorm, large-offset row      1.51 (D = 256; 0.38 .. 1.00 at the other widths)
    FSMN, 21 taps                    1.00 (every C and T: the bits of the float32 evaluation where the error is largest)
    log-softmax                      1.00 (N = 63; 0.53 .. 0.90 at the other widths)
    LayerNorm constants              1.76 (K = 512; 0.51 .. 0.84 at the other widths)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -777.0


def _lib():
    from funasr_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _gap(ref64, ref32):
    m = ref64.abs().max().float()
    ulp = (torch.nextafter(m, torch.tensor(float("inf"))) - m).item()
    return max((ref32.double() - ref64).abs().max().item(), ulp)


def _bar4(tag, got, ref64, ref32):
    """the 4 x gap rule; returns the measured ratio"""
    gap = _gap(ref64, ref32)
    d = (got.double().cpu() - ref64).abs().max().item()
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / gap:.2f} (bar 4)")
    assert d <= 4 * gap, (tag, d, gap)
    return d / gap


# ================================================================ LayerNorm
LN_WIDTHS = [4, 252, 256, 260, 508, 512, 516, 764, 768, 772, 2044, 2048]
LN_CASES = [(D, D) for D in LN_WIDTHS] + [(512, 516), (768, 772)]       # (D, Dpad); the last two pad across an instantiation
LN_CONST, LN_OFFSET = 1, 2                                                # rows of the five-row input that are not `3 randn + 0.5`


def _ln_inputs(D):
    g = torch.Generator().manual_seed(D)
    x = torch.randn(5, D, generator=g) * 3 + 0.5
    x[LN_CONST] = 3.25                                                    # sums of up to 2048 copies are exact in fp32
    x[LN_OFFSET] = 1000.0 + 0.01 * torch.randn(D, generator=g)
    return x, torch.randn(D, generator=g), torch.randn(D, generator=g)


def _ln_two_pass(x, gamma, beta, eps, dtype):
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def _ln_call(xv, gd, bd, eps, M, D, Dpad):
    """pf_k_layernorm on the first M rows of the device view xv into a sentinel-filled [M + 1, Dpad + 8] buffer"""
    L, lib = _lib()
    ybuf = torch.full((M + 1, Dpad + 8), SENT, device=xv.device)
    L.check(lib.pf_k_layernorm(xv.data_ptr(), xv.stride(0), gd.data_ptr(), bd.data_ptr(), ybuf.data_ptr(), Dpad + 8, M, D, Dpad,
                               float(eps), _stream()), "pf_k_layernorm")
    return ybuf


@pytest.mark.parametrize("D,Dpad", LN_CASES)
def test_layernorm_edges(cuda, D, Dpad):
    """both sides of every NV switch (512 / 768 columns) and of a 64-lane round, one to five rows over the four-rows-per-workgroup
    grid; the input is a column slice of a wider buffer whose other columns hold NaN, the output has ldy = Dpad + 8.
    Rows of `3 randn + 0.5`: 5e-6 against float64. A row of one repeated value: exactly beta. A row 1000 + 0.01 randn: 4 x gap
    against the float32 two-pass evaluation (a one-pass variance E[x^2] - mean^2 would lose every digit there)."""
    x, gamma, beta = _ln_inputs(D)
    wide = torch.full((5, D + 12), float("nan"))
    wide[:, 4:4 + D] = x
    xv = wide.to(cuda)[:, 4:4 + D]
    gd, bd = gamma.to(cuda), beta.to(cuda)
    plain = [r for r in range(5) if r not in (LN_CONST, LN_OFFSET)]
    worst = 0.0
    for eps in (1e-12, 1e-5):
        ref = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), eps)
        ref32 = _ln_two_pass(x, gamma, beta, eps, torch.float32)
        for M in (1, 3, 4, 5):
            ybuf = _ln_call(xv, gd, bd, eps, M, D, Dpad).cpu()
            y = ybuf[:M]
            assert (y[:, Dpad:] == SENT).all() and (ybuf[M] == SENT).all(), "guard band"
            assert (y[:, D:Dpad] == 0).all(), "padding columns"
            rows = [r for r in plain if r < M]
            d = (y[rows, :D].double() - ref[rows]).abs().max().item()
            assert d < 5e-6, (eps, M, d)
            if M > LN_CONST:
                assert torch.equal(y[LN_CONST, :D], beta)
            if M > LN_OFFSET:
                worst = max(worst, _bar4(f"layernorm D {D} eps {eps:g} M {M} offset row", y[LN_OFFSET, :D], ref[LN_OFFSET], ref32[LN_OFFSET]))
    print(f"layernorm D {D} Dpad {Dpad}: worst offset-row ratio {worst:.2f}")
    # rows are independent bitwise
    full = _ln_call(xv, gd, bd, 1e-12, 5, D, Dpad)
    for r in range(5):
        assert torch.equal(_ln_call(xv[r:r + 1], gd, bd, 1e-12, 1, D, Dpad)[0], full[r]), r


@pytest.mark.parametrize("D", [256, 512, 516, 520, 2048])
def test_layernorm_plane_output(cuda, D):
    """the two-fp16-plane output against the fp32 output of the same input: (hi + lo) 2^-e reproduces y to 2^-22 |y| + 2^-25 2^-e
    (hi = f16(y 2^e), lo = f16 of the exact remainder, to half a subnormal step at worst). D % 8 == 0 takes the paired 16-byte
    stores, D = 516 the single 8-byte stores."""
    from funasr_amd import ops
    g = torch.Generator().manual_seed(D + 1)
    x = (torch.randn(5, D, generator=g) * 3 + 0.5).to(cuda)
    gamma, beta = torch.randn(D, generator=g).to(cuda), torch.randn(D, generator=g).to(cuda)
    for e in (0, 3):
        y = ops.layernorm(x, gamma, beta, 1e-12).cpu().double()
        p = ops.layernorm_planes(x, gamma, beta, 1e-12, scale_exp=e).cpu().double()
        assert torch.isfinite(p).all()
        err = ((p[0] + p[1]) * 2.0 ** -e - y).abs()
        tol = 2.0 ** -22 * y.abs() + 2.0 ** -25 * 2.0 ** -e
        assert (err <= tol).all(), (D, e, (err - tol).max().item())
        assert torch.equal(p[0].float(), (y * 2.0 ** e).float().half().float()), "hi is the fp16 rounding of y 2^e"


# ================================================================ FSMN memory block
def _fsmn_ref(x, w, lens, left, res, dtype):
    """mask * (conv_K(pad(mask * x)) + mask * x) (+ residual), the masks taken with torch.where: NaN in a masked row stays out"""
    B, T, C = x.shape
    K = w.shape[1]
    valid = (torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None])[:, :, None]
    zero = torch.zeros((), dtype=dtype)
    xm = torch.where(valid, x.to(dtype), zero)
    xp = torch.nn.functional.pad(xm.transpose(1, 2), (left, K - 1 - left))
    conv = torch.nn.functional.conv1d(xp, w.to(dtype).view(C, 1, K), groups=C).transpose(1, 2)
    out = torch.where(valid, conv + xm, zero)
    return out if res is None else res.to(dtype) + out


def _fsmn_call(inv, w, resv, lens, K, left, expect_ok=True):
    """pf_k_fsmn on device views (input / residual [B, T, C] of any row stride) into a sentinel-filled [B T + 1, C + 4] buffer"""
    L, lib = _lib()
    B, T, C = inv.shape
    obuf = torch.full((B * T + 1, C + 4), SENT, device=inv.device)
    ld = torch.as_tensor(lens, dtype=torch.int32).to(inv.device)
    rc = lib.pf_k_fsmn(inv.data_ptr(), inv.stride(1), w.data_ptr(), _ptr(resv), resv.stride(1) if resv is not None else 0,
                       obuf.data_ptr(), C + 4, ld.data_ptr(), B, T, C, K, left, _stream())
    if expect_ok:
        L.check(rc, "pf_k_fsmn")
    return rc, obuf


def _fsmn_case(cuda, T, C, K, seed):
    lens = sorted({0, 1, max(T - 1, 0), T}, reverse=True)
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g)
    w = torch.randn(C, K, generator=g) * 0.3
    res = torch.randn(B, T, C, generator=g)
    fused = torch.full((B, T, 3 * C), float("nan"))                     # the engine's QKV buffer; the FSMN reads its last third only
    fused[:, :, 2 * C:] = x
    for b, n in enumerate(lens):
        fused[b, n:] = float("nan")                                     # rows >= lens[b]: never read
    rwide = torch.full((B, T, C + 8), float("nan"))
    rwide[:, :, 4:4 + C] = res
    return lens, x, w, res, fused.to(cuda)[:, :, 2 * C:], w.to(cuda), rwide.to(cuda)[:, :, 4:4 + C]


@pytest.mark.parametrize("C", [4, 36, 320, 1024])
@pytest.mark.parametrize("K,left", [(11, 5), (11, 10), (21, 10)])
def test_fsmn_edges(cuda, K, left, C):
    """every instantiation (offline, sanm_shfit, SeACo's 21 taps), T on both sides of one and two 8-row tiles, lens 0 / 1 / T - 1 / T
    in one batch, blocks of 1 to 256 threads; ldin = 3 C, ldr = C + 8, ldo = C + 4 with a guard band; input rows >= lens[b] (and
    every column outside the slices) hold NaN. Rows >= lens[b] of the output are exactly the residual, or zero without one."""
    worst = 0.0
    for T in (1, 7, 8, 9, 15, 16, 17, 29):
        lens, x, w, res, xd, wd, rd = _fsmn_case(cuda, T, C, K, 1000 * K + 10 * T + left)
        B = len(lens)
        for r_cpu, r_dev in ((None, None), (res, rd)):
            out = _fsmn_call(xd, wd, r_dev, lens, K, left)[1].cpu()
            o = out[:B * T, :C].view(B, T, C)
            assert (out[:B * T, C:] == SENT).all() and (out[B * T] == SENT).all(), "guard band"
            assert torch.isfinite(o).all()
            for b, n in enumerate(lens):
                assert torch.equal(o[b, n:], res[b, n:] if r_cpu is not None else torch.zeros(T - n, C)), (T, b)
            ref = _fsmn_ref(x, w, lens, left, r_cpu, torch.float64)
            if K == 11:
                d = (o.double() - ref).abs().max().item()
                assert d < 1e-5, (T, d)
            else:
                worst = max(worst, _bar4(f"fsmn K {K} C {C} T {T} res {r_cpu is not None}", o, ref,
                                         _fsmn_ref(x, w, lens, left, r_cpu, torch.float32)))
        if T == 17:                                                        # bitwise: a second run, and every sequence alone
            again = _fsmn_call(xd, wd, rd, lens, K, left)[1].cpu()
            assert torch.equal(again, out)
            for b in range(B):
                alone = _fsmn_call(xd[b:b + 1], wd, rd[b:b + 1], lens[b:b + 1], K, left)[1].cpu()
                assert torch.equal(alone[:T, :C], o[b]), b
    if K == 21:
        print(f"fsmn K 21 C {C}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("K,left,C,needle", [(11, 3, 512, "kernel_size 11"), (7, 3, 512, "kernel_size 11"),
                                             (11, 5, 1028, "<= 1024"), (11, 5, 6, "multiple of 4")])
def test_fsmn_refusals(cuda, K, left, C, needle):
    """an unbuilt (kernel_size, left padding) pair, more than 1024 channels and C % 4 != 0 are refused with a message naming the
    limit, nothing is written, and a valid call on the same stream afterwards returns the right values"""
    L, lib = _lib()
    x = torch.randn(1, 9, C, generator=torch.Generator().manual_seed(C)).to(cuda)
    w = torch.randn(C, K, generator=torch.Generator().manual_seed(K)).to(cuda)
    rc, obuf = _fsmn_call(x, w, None, [9], K, left, expect_ok=False)
    assert rc != 0 and needle in L.last_error(), L.last_error()
    assert (obuf == SENT).all()
    lens, x, w, res, xd, wd, rd = _fsmn_case(cuda, 9, 36, 11, 3)
    out = _fsmn_call(xd, wd, rd, lens, 11, 5)[1].cpu()[:len(lens) * 9, :36].view(len(lens), 9, 36)
    assert (out.double() - _fsmn_ref(x, w, lens, 5, res, torch.float64)).abs().max().item() < 1e-5


# ================================================================ log-softmax
@pytest.mark.parametrize("N", [1, 63, 64, 65, 8404])
def test_log_softmax_edges(cuda, N):
    """one to five rows over the four-rows-per-workgroup grid, N on both sides of the 64-lane sweep; row strides ldx = N + 5 and
    ldy = N + 3 with a guard band; in place equals out of place bitwise; columns at -inf (SenseVoice's banned tokens) stay -inf and
    the rest meet the bar; x - lse of pf_k_log_softmax_stats is bitwise the stored value."""
    from funasr_amd import ops
    L, lib = _lib()
    g = torch.Generator().manual_seed(N)
    x = torch.randn(5, N, generator=g) * 3
    if N > 1:
        x[0, torch.randperm(N, generator=g)[:N // 3]] = float("-inf")
        x[3, 0] = float("-inf")
    banned = torch.isinf(x)
    ref, ref32 = torch.log_softmax(x.double(), -1), torch.log_softmax(x, -1)
    fin = lambda t: torch.where(banned[:t.shape[0]], torch.zeros((), dtype=t.dtype), t)
    wide = torch.full((5, N + 5), float("nan"))
    wide[:, 2:2 + N] = x
    worst = 0.0
    for M in (1, 3, 4, 5):
        wd = wide.to(cuda)
        xv = wd[:, 2:2 + N]
        ybuf = torch.full((M + 1, N + 3), SENT, device=cuda)
        L.check(lib.pf_k_log_softmax(xv.data_ptr(), N + 5, ybuf.data_ptr(), N + 3, M, N, _stream()), "pf_k_log_softmax")
        y = ybuf.cpu()
        assert (y[:M, N:] == SENT).all() and (y[M] == SENT).all(), "guard band"
        y = y[:M, :N]
        assert torch.equal(torch.isinf(y) & (y < 0), banned[:M]) and not torch.isnan(y).any()
        worst = max(worst, _bar4(f"log_softmax N {N} M {M}", fin(y), fin(ref[:M]), fin(ref32[:M])))
        lse, _ = ops.log_softmax_stats(xv[:M])
        assert torch.equal((xv[:M] - lse[:, None]).cpu(), y)
        L.check(lib.pf_k_log_softmax(xv.data_ptr(), N + 5, xv.data_ptr(), N + 5, M, N, _stream()), "pf_k_log_softmax")   # in place
        back = wd.cpu()
        assert torch.equal(back[:M, 2:2 + N], y)
        assert torch.isnan(back[:, :2]).all() and torch.isnan(back[:, 2 + N:]).all() and torch.equal(back[M:, 2:2 + N], x[M:])
    print(f"log_softmax N {N}: worst ratio {worst:.2f}")


# ================================================================ bf16 cast
def _bits(values):
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).view(torch.float32)


def _cast(x):
    L, lib = _lib()
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    return lib.pf_k_cast_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), y


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("n", [4, 1020, 1024, 1028, 8192 * 256 * 4 + 4])
def test_cast_bf16_sizes(cuda, n):
    """bitwise torch's round-to-nearest-even cast, below and above one 256-thread block and just past the grid cap of 8192 blocks
    (the grid-stride loop); values spread over 24 binades"""
    g = torch.Generator(device=cuda).manual_seed(n % 1000)
    x = torch.randn(n, generator=g, device=cuda) * torch.pow(10.0, torch.rand(n, generator=g, device=cuda) * 12 - 6)
    rc, y = _cast(x)
    assert rc == 0
    assert _same_bits(y.cpu(), x.cpu().to(torch.bfloat16))


def test_cast_bf16_ties_and_specials(cuda):
    """every tie pattern 0x????8000 (even upper halves round down, odd ones up), subnormals, +-0, +-inf and the largest finite
    (rounds to inf) are bitwise torch's; NaNs of every payload come out NaN (the rounding add alone would turn 0x7f800001 into inf
    and 0x7fffffff into -0); n % 4 != 0 is refused"""
    L, lib = _lib()
    hi = np.arange(0x10000, dtype=np.uint32)
    hi = hi[(hi & 0x7f80) != 0x7f80]                                       # finite upper halves, even and odd
    special = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff,
               0x00000001, 0x80000001, 0x00007fff, 0x00008000, 0x00008001, 0x00018000, 0x007fffff, 0x807fffff,
               0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001]
    vals = np.concatenate([(hi << 16) | 0x8000, (hi << 16) | 0x7fff, (hi << 16) | 0x8001, np.array(special, dtype=np.uint32)])
    vals = np.concatenate([vals, np.zeros(-len(vals) % 4, dtype=np.uint32)])
    x = _bits(vals)
    rc, y = _cast(x.to(cuda))
    assert rc == 0
    want = x.to(torch.bfloat16)
    assert not torch.isnan(want.float()).any()
    assert _same_bits(y.cpu(), want)
    nan = _bits([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0xffffffff, 0xff800001, 0x7f808000, 0x7fbfffff])
    assert torch.isnan(nan).all()
    rc, y = _cast(nan.to(cuda))
    assert rc == 0 and torch.isnan(y.cpu().float()).all(), y.cpu().view(torch.int16)
    rc, _ = _cast(torch.zeros(6, device=cuda))
    assert rc != 0 and "n % 4" in L.last_error()


# ================================================================ LayerNorm constants of the small-M GEMM
@pytest.mark.parametrize("K", [4, 252, 256, 260, 512])
def test_ln_consts_edges(cuda, K):
    """c1 = W gamma, c2 = W beta + bias: K on both sides of one 256-column sweep of a wave, one to five (and 130) weight rows over the
    four-rows-per-workgroup grid, ldw = K + 4 with NaN in the padding columns, with and without bias. The hook lays c2 directly
    behind c1 (c[N .. 2 N)), so the guard band is what follows c2."""
    L, lib = _lib()
    worst = 0.0
    for N in (1, 3, 4, 5, 130):
        g = torch.Generator().manual_seed(K * 1000 + N)
        W, gamma, beta, bias = (torch.randn(N, K, generator=g), torch.randn(K, generator=g), torch.randn(K, generator=g),
                                torch.randn(N, generator=g))
        wide = torch.full((N, K + 4), float("nan"))
        wide[:, :K] = W
        wd, gd, bd = wide.to(cuda), gamma.to(cuda), beta.to(cuda)
        for bs in (None, bias):
            c = torch.full((2 * N + 8,), SENT, device=cuda)
            L.check(lib.pf_k_ln_consts(wd.data_ptr(), K + 4, N, K, gd.data_ptr(), bd.data_ptr(), _ptr(None if bs is None else bs.to(cuda)),
                                       c.data_ptr(), _stream()), "pf_k_ln_consts")
            c = c.cpu()
            assert (c[2 * N:] == SENT).all(), "guard band"

            def consts(dt):
                c2 = W.to(dt) @ beta.to(dt)
                return torch.cat([W.to(dt) @ gamma.to(dt), c2 if bs is None else c2 + bs.to(dt)])
            worst = max(worst, _bar4(f"ln_consts K {K} N {N} bias {bs is not None}", c[:2 * N], consts(torch.float64), consts(torch.float32)))
    print(f"ln_consts K {K}: worst ratio {worst:.2f}")
