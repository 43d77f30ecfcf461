"""The Qwen3 decoder's kernels (csrc/qwen3.hip) on the MI355X, each alone through its pf_k_qwen3_* hook against the float64 oracle
(tests/_qwen3_oracle.py): RMSNorm, q/k norm + RoPE with the cache write, prefill attention, decode attention, SwiGLU.

Bars, with u = 2^-24 (the relative error of one correctly rounded fp32 operation), every bound first order plus one u for the rest:
  RMSNorm   derived, per element. The sum of D squares is a tree of non-negative terms of depth t = 3 ceil(D / 256) + 6 (per 4-column
            chunk two levels and the accumulate, then the 6-level butterfly) over rounded products: relative error (t + 1) u. Then / D,
            + eps, sqrt (which halves what came before), 1 / x, and two products: |d| <= ((t + 3) / 2 + 4 + 1) u |y|.
  q/k RoPE  derived, per element. The norm is the same with t = head_dim / 64 + 6: relative error rho = ((t + 3) / 2 + 5) u of the normed
            value; x cos +- x' sin adds one rounding per product and one for the sum: |d| <= (rho + 2 u) (|x cos| + |x' sin|).
            V rows are copies: bitwise.
  SwiGLU    derived, per element. expf within 1 ulp = 2 u; 1 + e inherits at most that and adds u; the quotient and the product add u
            each: |d| <= (5 + 1) u |y|, plus 2^-120 (1 + |up|) where exp(-gate) overflows fp32 and the kernel returns -0 for a true
            value below 90 e^-88.7 |up| < 2^-120 |up|.
  attention no bound tight enough to test anything follows from the arithmetic (a quotient of two exp-weighted K-term sums), so every
            case allows 4 x max |oracle in float32 - oracle in float64| on the same inputs, with no floor: one key is exact in the
            kernel too (p = expf(0) = 1, l = 1).
Every test prints its measured ratio.

Caches and outputs are NaN wherever the kernel under test must not read or write: beyond a sequence's length, in the slots of other
sequences, and around every output row."""
import ctypes as C

import pytest
import torch

from funasr_amd import _lib

from . import _qwen3_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
THETA = 1000000.0
TABLE_ROWS = 4096


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


U = 2.0 ** -24


def _report(tag, got, ref64, ref32):
    """max |got - ref64| within 4 x max |ref32 - ref64|"""
    assert torch.isfinite(got).all(), f"{tag}: non-finite output"
    d, bar = float((got.double().cpu() - ref64).abs().max()), 4.0 * float((ref32.double() - ref64).abs().max())
    print(f"{tag}: max |d| {d:.3e}, bar {bar:.3e}, ratio {d / max(bar, 1e-300):.3f}")
    assert d <= bar, (tag, d, bar)


def _report_elementwise(tag, got, ref64, bound):
    """|got - ref64| <= bound, element by element (a derived bound)"""
    assert torch.isfinite(got).all(), f"{tag}: non-finite output"
    d = (got.double().cpu() - ref64).abs()
    ratio = float((d / bound.clamp(min=1e-300)).max())
    print(f"{tag}: max |d| {float(d.max()):.3e}, largest |d| / bound {ratio:.3f}")
    assert bool((d <= bound).all()), (tag, float(d.max()), ratio)


def _norm_rel(depth):
    """relative error bound of x * (1 / sqrt(mean(x^2) + eps)) * w with the squares summed in a tree of `depth` levels"""
    return ((depth + 3) / 2 + 5) * U


def _tiles(G, hd):
    q, k, s = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.load().pf_k_qwen3_tiles(G, hd, C.byref(q), C.byref(k), C.byref(s)), "pf_k_qwen3_tiles")
    return q.value, k.value, s.value


# ---------------------------------------------------------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("D", [32, 96, 1024])
@pytest.mark.parametrize("M", [1, 5])
def test_rmsnorm(cuda, D, M):
    g = torch.Generator().manual_seed(D + M)
    x = torch.randn(M, D, generator=g) * 3.0
    zero_row = 3 if M > 3 else None                        # a row of zeros: rsqrt(eps) times 0
    if zero_row is not None:
        x[zero_row] = 0.0
    w = 1.0 + 0.3 * torch.randn(D, generator=g)
    ld = D + 4
    xd = torch.full((M, ld), NAN, device=cuda)
    xd[:, :D] = x.to(cuda)
    y = torch.full((M + 2, ld), NAN, device=cuda)
    wd = w.to(cuda)
    _lib.check(_lib.load().pf_k_qwen3_rmsnorm(xd.data_ptr(), ld, wd.data_ptr(), 1e-6, y[1].data_ptr(), ld, M, D, _stream()),
               "pf_k_qwen3_rmsnorm")
    assert torch.isnan(y[0]).all() and torch.isnan(y[-1]).all() and torch.isnan(y[1:-1, D:]).all()
    if zero_row is not None:
        assert (y[1 + zero_row, :D] == 0).all()
    ref = O.rmsnorm(x.double(), w.double(), 1e-6)
    _report_elementwise(f"rmsnorm M={M} D={D}", y[1:-1, :D], ref, _norm_rel(3 * ((D + 255) // 256) + 6) * ref.abs())


# ------------------------------------------------------------------------------------------------- q/k norm + RoPE + cache
@pytest.mark.parametrize("hd", [64, 128])
def test_qk_rope_and_cache_write(cuda, hd):
    Hq, Hkv, slots, cap = 4, 2, 3, TABLE_ROWS
    seq, pos = [0, 0, 2, 2, 0], [0, 1, 4095, 7, 4095]      # positions 0, 1 and the last table row, two slots, slot 1 untouched
    M, nh = len(seq), Hq + 2 * Hkv
    g = torch.Generator().manual_seed(hd)
    qkv = torch.randn(M, nh * hd, generator=g) * 2.0
    qw, kw = 1.0 + 0.3 * torch.randn(hd, generator=g), 1.0 + 0.3 * torch.randn(hd, generator=g)
    cos32, sin32 = O.rope_cos_sin(hd, THETA, range(TABLE_ROWS), torch.float32)
    qo = torch.full((M + 2, Hq * hd), NAN, device=cuda)
    kc = torch.full((slots, Hkv, cap, hd), NAN, device=cuda)
    vc = torch.full((slots, Hkv, cap, hd), NAN, device=cuda)
    qkv_d, cos_d, sin_d, qw_d, kw_d = qkv.to(cuda), cos32.to(cuda), sin32.to(cuda), qw.to(cuda), kw.to(cuda)
    _lib.check(_lib.load().pf_k_qwen3_qk_rope(qkv_d.data_ptr(), nh * hd, qw_d.data_ptr(), kw_d.data_ptr(), 1e-6,
                                              cos_d.data_ptr(), sin_d.data_ptr(), TABLE_ROWS, _i32(seq), _i32(pos), qo[1].data_ptr(), Hq * hd,
                                              kc.data_ptr(), vc.data_ptr(), slots, cap, M, Hq, Hkv, hd, _stream()), "pf_k_qwen3_qk_rope")
    assert torch.isnan(qo[0]).all() and torch.isnan(qo[-1]).all()
    x = qkv.double().reshape(M, nh, hd)
    c, s = cos32[pos].double(), sin32[pos].double()
    cc, ss = torch.cat((c, c), -1)[:, None, :], torch.cat((s, s), -1)[:, None, :]

    def ref_and_bound(heads, w):
        xn = O.rmsnorm(heads, w.double(), 1e-6)
        return O.qk_rope(heads, w.double(), 1e-6, c, s), (_norm_rel(hd // 64 + 6) + 2 * U) * ((xn * cc).abs() + (O.rotate_half(xn) * ss).abs())

    q_ref, q_bound = ref_and_bound(x[:, :Hq], qw)
    k_ref, k_bound = ref_and_bound(x[:, Hq:Hq + Hkv], kw)
    _report_elementwise(f"qk_rope q hd={hd}", qo[1:-1].reshape(M, Hq, hd), q_ref, q_bound)
    written = torch.zeros(slots, cap, dtype=torch.bool)
    for r in range(M):
        written[seq[r], pos[r]] = True
        _report_elementwise(f"qk_rope k row {r} hd={hd}", kc[seq[r], :, pos[r]], k_ref[r], k_bound[r])
        assert torch.equal(vc[seq[r], :, pos[r]].cpu(), qkv.reshape(M, nh, hd)[r, Hq + Hkv:]), "v rows are copied bit for bit"
    keep = ~written.to(cuda)[:, None, :, None].expand(slots, Hkv, cap, hd)
    assert torch.isnan(kc[keep]).all() and torch.isnan(vc[keep]).all(), "a cache row that was not written lost its poison"


# ---------------------------------------------------------------------------------------------------------- attention
def _cache(slots, Hkv, cap, hd, lens, seed, cuda):
    """K / V caches [slots, Hkv, cap, hd]: random below lens[slot], NaN at and beyond it; (device pair, host pair)"""
    g = torch.Generator().manual_seed(seed)
    k, v = torch.randn(slots, Hkv, cap, hd, generator=g), torch.randn(slots, Hkv, cap, hd, generator=g)
    for s, n in enumerate(lens):
        k[s, :, n:] = NAN
        v[s, :, n:] = NAN
    return (k.to(cuda), v.to(cuda)), (k, v)


def _prefill_case(cuda, hd, Hq, Hkv, seqs, tag):
    """seqs: (slot, rows, p0) per sequence; the cache of a slot holds p0 + rows valid rows"""
    slots, cap = max(s for s, _, _ in seqs) + 2, max(p0 + n for _, n, p0 in seqs) + 5
    lens = [0] * slots
    for s, n, p0 in seqs:
        lens[s] = p0 + n
    (kd, vd), (k, v) = _cache(slots, Hkv, cap, hd, lens, hd + Hq + len(seqs), cuda)
    M = sum(n for _, n, _ in seqs)
    q = torch.randn(M, Hq * hd, generator=torch.Generator().manual_seed(7)) * 1.5
    out = torch.full((M + 2, Hq * hd), NAN, device=cuda)
    row0, r = [], 0
    for _, n, _ in seqs:
        row0.append(r)
        r += n
    qd = q.to(cuda)
    _lib.check(_lib.load().pf_k_qwen3_prefill_attention(qd.data_ptr(), Hq * hd, kd.data_ptr(), vd.data_ptr(), slots, cap, out[1].data_ptr(),
                                                        Hq * hd, M, _i32([s for s, _, _ in seqs]), _i32(row0), _i32([n for _, n, _ in seqs]),
                                                        _i32([p for _, _, p in seqs]), len(seqs), Hq, Hkv, hd, hd ** -0.5, _stream()),
               "pf_k_qwen3_prefill_attention")
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all()
    ref = {}
    for dt in (torch.float64, torch.float32):
        parts = []
        for (s, n, p0), r0 in zip(seqs, row0):
            L = p0 + n
            parts.append(O.gqa_attention(q[r0:r0 + n].to(dt).reshape(n, Hq, hd), k[s, :, :L].to(dt).transpose(0, 1),
                                         v[s, :, :L].to(dt).transpose(0, 1), p0).reshape(n, Hq * hd))
        ref[dt] = torch.cat(parts, 0)
    _report(tag, out[1:-1], ref[torch.float64], ref[torch.float32])


@pytest.mark.parametrize("hd,Hq,Hkv", [(64, 4, 2), (64, 2, 2), (128, 4, 1), (128, 4, 2)])
def test_prefill_attention_tile_edges(cuda, hd, Hq, Hkv):
    qt, kt, _ = _tiles(Hq // Hkv, hd)
    rows = sorted({1, qt - 1, qt, qt + 1, kt - 1, kt, kt + 1} - {0})
    for n in rows:
        for p0 in (0, kt - 2):
            _prefill_case(cuda, hd, Hq, Hkv, [(0, n, p0)], f"prefill hd={hd} G={Hq // Hkv} rows={n} p0={p0}")


@pytest.mark.parametrize("hd", [64, 128])
def test_prefill_attention_two_sequences_of_different_lengths(cuda, hd):
    _, kt, _ = _tiles(2, hd)
    _prefill_case(cuda, hd, 4, 2, [(1, kt + 3, 0), (0, 5, 2 * kt + 1)], f"prefill hd={hd} B=2")


def _decode_case(cuda, hd, Hq, Hkv, rows, tag):
    """rows: (slot, length) per query row"""
    slots, cap = max(s for s, _ in rows) + 2, max(n for _, n in rows) + 3
    lens = [0] * slots
    for s, n in rows:
        lens[s] = n
    (kd, vd), (k, v) = _cache(slots, Hkv, cap, hd, lens, hd + len(rows), cuda)
    M = len(rows)
    q = torch.randn(M, Hq * hd, generator=torch.Generator().manual_seed(11)) * 1.5
    out = torch.full((M + 2, Hq * hd), NAN, device=cuda)
    qd = q.to(cuda)
    _lib.check(_lib.load().pf_k_qwen3_decode_attention(qd.data_ptr(), Hq * hd, kd.data_ptr(), vd.data_ptr(), slots, cap, out[1].data_ptr(),
                                                       Hq * hd, _i32([s for s, _ in rows]), _i32([n for _, n in rows]), M, Hq, Hkv, hd,
                                                       hd ** -0.5, _stream()), "pf_k_qwen3_decode_attention")
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all()
    ref = {}
    for dt in (torch.float64, torch.float32):
        ref[dt] = torch.cat([O.gqa_attention(q[r:r + 1].to(dt).reshape(1, Hq, hd), k[s, :, :n].to(dt).transpose(0, 1),
                                             v[s, :, :n].to(dt).transpose(0, 1), n - 1).reshape(1, Hq * hd)
                             for r, (s, n) in enumerate(rows)], 0)
    _report(tag, out[1:-1], ref[torch.float64], ref[torch.float32])


@pytest.mark.parametrize("hd,Hq,Hkv", [(64, 4, 2), (128, 4, 4), (128, 4, 1)])
def test_decode_attention_split_edges(cuda, hd, Hq, Hkv):
    _, kt, ks = _tiles(Hq // Hkv, hd)
    for L in (1, 2, kt, kt + 1, ks - 1, ks, ks + 1, 600):
        _decode_case(cuda, hd, Hq, Hkv, [(0, L)], f"decode hd={hd} G={Hq // Hkv} L={L}")


@pytest.mark.parametrize("hd", [64, 128])
def test_decode_attention_three_sequences_of_different_lengths(cuda, hd):
    _, _, ks = _tiles(2, hd)
    _decode_case(cuda, hd, 4, 2, [(2, ks + 9), (0, 3), (1, 2 * ks)], f"decode hd={hd} B=3")


# ----------------------------------------------------------------------------------------------------------------- SwiGLU
def test_swiglu(cuda):
    M, I = 3, 100                                          # 100 columns: no multiple of 4 floats x 64 lanes
    g = torch.Generator().manual_seed(5)
    gu = torch.randn(M, 2 * I, generator=g) * 4.0
    gu[0, 0], gu[0, 1], gu[1, 2], gu[1, 3] = 90.0, -90.0, 90.0, -90.0      # exp(90) overflows float32: silu -> x and -> -0
    ld = 2 * I + 4
    gd = torch.full((M, ld), NAN, device=cuda)
    gd[:, :2 * I] = gu.to(cuda)
    out = torch.full((M + 2, I + 4), NAN, device=cuda)
    _lib.check(_lib.load().pf_k_qwen3_swiglu(gd.data_ptr(), ld, out[1].data_ptr(), I + 4, M, I, _stream()), "pf_k_qwen3_swiglu")
    assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all() and torch.isnan(out[1:-1, I:]).all()
    ref = O.swiglu(gu[:, :I].double(), gu[:, I:].double())
    _report_elementwise("swiglu", out[1:-1, :I], ref, 6 * U * ref.abs() + 2.0 ** -120 * (1 + gu[:, I:].double().abs()))
    assert float(out[1, 0]) == pytest.approx(90.0 * float(gu[0, I]), rel=1e-6) and abs(float(out[1, 1])) < 1e-30
