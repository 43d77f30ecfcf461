"""The f16x2 GEMMs on v_mfma_f32_16x16x32_f16: lane maps, k order and every output form at the smallest shapes that can still go
wrong -- M one 16-row tile / ragged around it / ragged around one block, K one 32-deep stage / two / three -- through the same
pf_k_* hooks as tests/test_kernels_f16x2_gpu.py.

Exact layout test: small-integer planes, so every product and every partial sum is exact in fp32 and the result must EQUAL
A W^T; A has one non-zero per row at k = (7 m + 3) mod K and W holds 1 + ((n + 5 k) mod 7), so a wrong k-lane or row-lane map of
the operand fragments or of the C/D tiles cannot pass. Float64 test: the bars are those of tests/test_kernels_f16x2_gpu.py for the
same calls (4e-7 sum |a||w| + 2.5e-7 |ref| for a product sum, + 2^-22 |ref| + 2^-25 / scale for a plane output, 2e-5 for the
LayerNorm planes). Every product shape (tile ids 0 / 1 / 2 / 3 / 7 / 10) and both row heights (128 / 96) return the same bits.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

TILES = (0, 1, 2, 3, 7, 10)
ROW_HEIGHTS = (128, 96)
MS = (16, 17, 255, 257)
KS = (32, 64, 96)


def _val(p2):
    return p2[0].double() + p2[1].double()


def _check(out, ref, mag, extra=0.0, what=""):
    """the bar of tests/test_kernels_f16x2_gpu.py::_check"""
    err = (out.double() - ref).abs()
    bound = 4e-7 * mag + 2.5e-7 * ref.abs() + extra
    worst = (err / bound).max().item()
    assert worst <= 1.0, f"{what}: error {err.max().item():.3e} is {worst:.2f}x the bound"


def _exact_planes(M, N, K, which, cuda):
    """(a2, w2, A W^T): "hi" -- both operands in the hi planes (|v| <= 8); "a_lo" -- A is +-1 in its lo plane, hi zero (the lo*hi
    product alone); "w_lo" -- W is +-1 in its lo plane, hi zero (the hi*lo product alone)"""
    m = torch.arange(M)
    a = torch.zeros(M, K)
    a[m, (7 * m + 3) % K] = (1 + m % 8).float() * (1 - 2 * (m % 2)).float()
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    w = (1 + (n + 5 * k) % 7).float()
    if which == "a_lo":
        a = a.sign()
    if which == "w_lo":
        w = (1 - 2 * ((n + k) % 2)).float()
    z = torch.zeros_like
    a2 = torch.stack([z(a), a] if which == "a_lo" else [a, z(a)]).half().contiguous().to(cuda)
    w2 = torch.stack([z(w), w] if which == "w_lo" else [w, z(w)]).half().contiguous().to(cuda)
    return a2, w2, (a.double() @ w.double().T).float().to(cuda)


@pytest.mark.parametrize("which", ["hi", "a_lo", "w_lo"])
def test_exact_layout_every_tile_shape(cuda, which):
    from funasr_amd import ops
    for M in MS:
        for K in KS:
            a2, w2, want = _exact_planes(M, 256, K, which, cuda)
            for tile in TILES:
                got = ops.gemm_f16x2(a2, w2, None, scale_exp=0, tile=tile)
                assert torch.equal(got, want), f"tile {tile}, M {M}, K {K}: not A W^T"


@pytest.mark.parametrize("which", ["hi", "a_lo", "w_lo"])
def test_exact_layout_both_row_heights(cuda, which):
    from funasr_amd import ops
    for M in MS:
        for K in KS:
            a2, w2, want = _exact_planes(M, 512, K, which, cuda)
            for br in ROW_HEIGHTS:
                got, none = ops.gemm_f16x2_row(a2, w2, None, scale_exp=0, block_rows=br)
                assert none is None and torch.equal(got, want), f"block_rows {br}, M {M}, K {K}: not A W^T"


def test_exact_layout_w2_depth(cuda):
    """w_2's form once: K = 2048 at M = 256 (64 stages: the double buffer's every turn), tile shapes and row shapes"""
    from funasr_amd import ops
    a2, w2, want = _exact_planes(256, 512, 2048, "hi", cuda)
    for tile in TILES:
        assert torch.equal(ops.gemm_f16x2(a2, w2, None, scale_exp=0, tile=tile), want), f"tile {tile}"
    for br in ROW_HEIGHTS:
        assert torch.equal(ops.gemm_f16x2_row(a2, w2, None, scale_exp=0, block_rows=br)[0], want), f"block_rows {br}"


def _random(M, N, K, cuda, seed, ea=8, ew=12):
    from funasr_amd import ops
    g = torch.Generator().manual_seed(seed + 7 * M + 3 * N + K)
    a = torch.randn(M, K, generator=g).to(cuda)
    w = (torch.randn(N, K, generator=g) * K ** -0.5 * torch.linspace(0.5, 1.5, N)[:, None]).to(cuda)    # asymmetric: a transposed C write shows
    return ops.split2(a, ea), ops.split2(w, ew), ea + ew, g


def _ref(a2, w2, se, bias, relu=False, add1=None, add2=None):
    a, w = _val(a2), _val(w2)
    out = (a @ w.T) * 2.0 ** -se + bias.double()
    mag = (a.abs() @ w.abs().T) * 2.0 ** -se
    if relu:
        out = torch.relu(out)
    if add1 is not None:
        out = out + add1.double()
    if add2 is not None:
        out = out + add2.double()
    return out, mag


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_fp32_bias_two_residuals_vs_float64(cuda, M, K):
    from funasr_amd import ops
    N = 256
    a2, w2, se, g = _random(M, N, K, cuda, 1)
    bias = torch.randn(N, generator=g).to(cuda)
    r1, r2 = torch.randn(M, N, generator=g).to(cuda), torch.randn(M, N, generator=g).to(cuda)
    ref, mag = _ref(a2, w2, se, bias, add1=r1, add2=r2)
    outs = [ops.gemm_f16x2(a2, w2, bias, add1=r1, add2=r2, scale_exp=se, tile=t) for t in TILES]
    _check(outs[0], ref, mag, what="fp32 + bias + two residuals")
    for t, o in zip(TILES, outs):
        assert torch.equal(o, outs[0]), f"tile {t} differs from tile {TILES[0]}"


@pytest.mark.parametrize("M", MS)
def test_relu_planes_out_vs_float64(cuda, M):
    from funasr_amd import ops
    N, K, eo = 256, 96, 9
    a2, w2, se, g = _random(M, N, K, cuda, 2)
    bias = torch.randn(N, generator=g).to(cuda)
    ref, mag = _ref(a2, w2, se, bias, relu=True)
    outs = [ops.gemm_f16x2(a2, w2, bias, relu=True, scale_exp=se, out_planes=True, out_scale_exp=eo, tile=t) for t in TILES]
    _check(_val(outs[0]) * 2.0 ** -eo, ref, mag, extra=2.0 ** -22 * ref.abs() + 2.0 ** -25 * 2.0 ** -eo, what="plane output")
    for t, o in zip(TILES, outs):
        assert torch.equal(o, outs[0]), f"tile {t} differs from tile {TILES[0]}"


@pytest.mark.parametrize("M", [16, 272])
@pytest.mark.parametrize("kv_form", [False, True])
def test_qkv_form_vs_float64(cuda, M, kv_form):
    """Q / K planes, fp32 V and the V^T planes (the form needs M % 16 == 0: one tile, and ragged around one block)"""
    from funasr_amd import ops
    D, K = 256, 96
    nseg = 2 if kv_form else 3
    a2, w2, se, g = _random(M, nseg * D, K, cuda, 3)
    bias = torch.randn(nseg * D, generator=g).to(cuda)
    q_mul, k_mul, v_mul = 128 ** -0.5 * 2.0 ** 7, 2.0 ** 6, 2.0 ** 5
    outs = [ops.gemm_f16x2_qkv(a2, w2, bias, D, se, q_mul, k_mul, v_mul, kv_form=kv_form, tile=t) for t in (0, 2, 3, 7, 10)]
    out = outs[0]
    for t, o in zip((0, 2, 3, 7, 10), outs):
        for key in ("q2", "k2", "v", "vt"):
            assert (out[key] is None and o[key] is None) or torch.equal(out[key], o[key]), f"tile {t}: {key} differs"
    ref, mag = _ref(a2, w2, se, bias)
    segs = dict(k=0, v=1) if kv_form else dict(q=0, k=1, v=2)

    def seg(x, name):
        return x[:, segs[name] * D:(segs[name] + 1) * D]

    def check_planes(p2, name, mul):
        r, m = seg(ref, name), seg(mag, name)
        _check(_val(p2) / mul, r, m, extra=2.0 ** -22 * r.abs() + 2.0 ** -25 / mul, what=f"{name} planes")

    if not kv_form:
        check_planes(out["q2"][:, :M], "q", q_mul)
        _check(out["v"], seg(ref, "v"), seg(mag, "v"), what="fp32 v")
        assert not out["q2"][:, M:].any()
    check_planes(out["k2"][:, :M], "k", k_mul)
    assert not out["k2"][:, M:].any()
    cols = ops.vt_columns(torch.arange(M, device=cuda))
    check_planes(out["vt"][:, :, cols].transpose(1, 2), "v", v_mul)
    touched = torch.zeros(M + 64, dtype=torch.bool, device=cuda)
    touched[cols] = True
    assert not out["vt"][:, :, ~touched].any(), "V^T columns outside the row set were written"


@pytest.mark.parametrize("K", KS)
def test_row_form_fsmn_layernorm_planes(cuda, K):
    """linear_out's form: FSMN memory + residual + LayerNorm + planes, both row heights, against fsmn_kernel + the tile GEMM +
    layernorm_kernel (bits) and against float64 (M % 16 == 0: ragged slots around one block)"""
    from funasr_amd import ops
    slots, lens = [16, 112, 144], [3, 100, 144]
    M = sum(slots)
    a2, w2, se, g = _random(M, 512, K, cuda, 4)
    bias = torch.randn(512, generator=g).to(cuda)
    add2 = (torch.randn(M, 512, generator=g) * 10 + 2).to(cuda)
    gamma, beta = (torch.rand(512, generator=g) * 2 + 0.1).to(cuda), torch.randn(512, generator=g).to(cuda)
    taps = (torch.randn(512, 11, generator=g) * 0.3).to(cuda)
    v = (torch.randn(M, 512, generator=g) * 2).to(cuda)
    eps, ey = 1e-12, 7
    mem = torch.empty(M, 512, device=cuda)
    lo, hi = torch.empty(M // 16, dtype=torch.int32), torch.empty(M // 16, dtype=torch.int32)
    start = 0
    for rows, n in zip(slots, lens):
        v[start + n:start + rows] = 3.0e30
        mem[start:start + rows] = ops.fsmn(v[start:start + rows].view(1, rows, 512), taps, torch.tensor([n], dtype=torch.int32, device=cuda), 5)[0]
        lo[start // 16:(start + rows) // 16] = start
        hi[start // 16:(start + rows) // 16] = start + n
        start += rows
    c_ref = ops.gemm_f16x2(a2, w2, bias, add1=mem, add2=add2, scale_exp=se, tile=2)
    y_ref = ops.layernorm_planes(c_ref, gamma, beta, eps, scale_exp=ey)
    lo, hi = lo.to(cuda), hi.to(cuda)
    for br in ROW_HEIGHTS:
        c, y = ops.gemm_f16x2_row_fsmn(a2, w2, bias, v, taps, lo, hi, add2=add2, scale_exp=se, ln=(gamma, beta, eps), out_scale_exp=ey, block_rows=br)
        assert torch.equal(c, c_ref) and torch.equal(y, y_ref), f"block_rows {br}"
        c, y = ops.gemm_f16x2_row(a2, w2, bias, add1=mem, add2=add2, scale_exp=se, ln=(gamma, beta, eps), out_scale_exp=ey, block_rows=br)
        assert torch.equal(c, c_ref) and torch.equal(y, y_ref), f"block_rows {br}, memory as an addend"
    ref, mag = _ref(a2, w2, se, bias, add1=mem, add2=add2)
    _check(c_ref, ref, mag, what="fp32 rows")
    ln64 = torch.nn.functional.layer_norm(ref, (512,), gamma.double(), beta.double(), eps)
    assert (_val(y_ref) * 2.0 ** -ey - ln64).abs().max().item() < 2e-5 * max(1.0, ln64.abs().max().item())


@pytest.mark.parametrize("M", MS)
def test_argmax_form_index_equality(cuda, M):
    from funasr_amd import ops
    N, K = 300, 96                                  # two column blocks, the second ragged
    a2, w2, se, g = _random(M, N, K, cuda, 5)
    bias = torch.randn(N, generator=g).to(cuda)
    ids = ops.gemm_f16x2_argmax(a2, w2, bias, scale_exp=se).long()
    ref, mag = _ref(a2, w2, se, bias)
    top2 = ref.topk(2, dim=1)
    tol = 2 * (4e-7 * mag.max(dim=1).values + 2.5e-7 * top2.values[:, 0].abs())
    clear = (top2.values[:, 0] - top2.values[:, 1]) > tol
    assert clear.float().mean() > 0.99
    assert torch.equal(ids[clear], top2.indices[:, 0][clear])
    # the same index as the arg-max of the fp32 form of the same product (same bits in, lowest index on ties)
    full = ops.gemm_f16x2(a2, w2[:, :N].contiguous(), bias, scale_exp=se, tile=1) if N % 4 == 0 else None
    if full is not None:
        assert torch.equal(ids, full.argmax(dim=1))
    w2t, bt = w2.clone(), bias.clone()
    w2t[:, 270] = w2t[:, 5]
    bt[270] = bt[5] = 50.0
    assert (ops.gemm_f16x2_argmax(a2, w2t, bt, scale_exp=se) == 5).all(), "ties go to the lowest column"
