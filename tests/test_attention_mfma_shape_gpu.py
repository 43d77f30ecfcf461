"""attention_f16x2.hip on v_mfma_f32_16x16x32_f16: the register <-> (key, query) maps at the smallest shapes that can still go wrong.

Everything goes through ops.attention_f16x2 with variant 3, the product's schedule (variants 0 / 1 as well when the measurement
library is loaded, like tests/test_kernels_f16x2_gpu.py). The bar is that test's: max |o - float64 attention| < 2e-6 max(1, max |ref|)
with plane exponents eq, ek, ev = 9, 10, 11; each test first checks on the CPU that its inputs keep |q scale| 2^eq, |k| 2^ek and
|v| 2^ev below 2^15.

What the maps are (attention_f16x2.hip's header): a wave's 32 queries are two 16-query column blocks; a query's 32 scores of a tile
sit in four lanes, 8 each, in key groups of 4 / 8 / 16; the eight probabilities of a lane are its B fragment of V^T P^T.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EQ, EK, EV = 9, 10, 11
SCALE = 128 ** -0.5
LAZY_TAU = 3.0                                                   # attention_f16x2.hip


def _variants():
    from funasr_amd import _lib
    return (0, 1, 3) if _lib.load().pf_measurement_build() else (3,)


def _ref(q, k, v, klens, H):
    """float64 attention (tests/test_kernels_f16x2_gpu.py::_attn_ref)"""
    B, Tq, D = q.shape
    Tk = k.shape[1]
    qh = q.double().view(B, Tq, H, 128).transpose(1, 2) * SCALE
    kh = k.double().view(B, Tk, H, 128).transpose(1, 2)
    vh = v.double().view(B, Tk, H, 128).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2)
    mask = torch.arange(Tk, device=q.device)[None, :] >= klens.to(q.device)[:, None]
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1).masked_fill(mask[:, None, None, :], 0.0)
    return (p @ vh).transpose(1, 2).reshape(B, Tq, D)


def _in_range(q, k, v):
    """the planes hold x 2^e in fp16: on the CPU, before anything is launched"""
    assert (q * SCALE).abs().max().item() * 2.0 ** EQ < 2.0 ** 15
    assert k.abs().max().item() * 2.0 ** EK < 2.0 ** 15
    assert v.abs().max().item() * 2.0 ** EV < 2.0 ** 15


def _run(q, k, v, klens, H, variant):
    from funasr_amd import ops
    return ops.attention_f16x2(q, k, v, klens, H, SCALE, eq=EQ, ek=EK, ev=EV, variant=variant)


def _draw(B, Tq, Tk, H, seed):
    g = torch.Generator().manual_seed(seed)
    D = 128 * H
    q, k, v = torch.randn(B, Tq, D, generator=g), torch.randn(B, Tk, D, generator=g), torch.randn(B, Tk, D, generator=g)
    _in_range(q, k, v)
    return q, k, v


def _check(o, ref, what):
    assert torch.isfinite(o).all(), what
    err = (o.double() - ref).abs().max().item()
    bar = 2e-6 * max(1.0, ref.abs().max().item())
    print(f"{what}: max |o - float64| = {err:.3e} (bar {bar:.3e})")
    assert err < bar, f"{what}: {err:.3e} >= {bar:.3e}"


def _all_variants_vs_float64(cuda, q, k, v, klens, H, what):
    q, k, v, klens = q.to(cuda), k.to(cuda), v.to(cuda), klens.to(cuda)
    ref = _ref(q, k, v, klens, H)
    outs = {}
    for variant in _variants():
        outs[variant] = _run(q, k, v, klens, H, variant)
        _check(outs[variant], ref, f"{what} variant {variant}")
    if 0 in outs:
        assert torch.equal(outs[0], outs[1]), f"{what}: the pipelined schedule is not bitwise the plain one"
    return outs, ref


KEY_LENGTHS = (1, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 20, 24, 31, 32, 33)


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("Tk", [16, 32, 48, 80])
def test_key_edges(cuda, Tk, H):
    """one sequence per key length at every boundary of the key-of-register map (groups of 4, 8, 16) and of the partly valid last tile"""
    lens = sorted({n for n in KEY_LENGTHS + (Tk,) if 1 <= n <= Tk})
    q, k, v = _draw(len(lens), 33, Tk, H, 100 * Tk + H)
    _all_variants_vs_float64(cuda, q, k, v, torch.tensor(lens, dtype=torch.int32), H, f"Tk {Tk} H {H} klens {lens}")


def test_key_permutation_localised(cuda):
    """query j points at key j (12 k_j / |k_j| sqrt(128) plus small noise), for each key of two tiles: its output is v_j, so a key order
    that differs between K Q^T and V^T P^T fails at a named key"""
    Tk = 64
    g = torch.Generator().manual_seed(7)
    k, v = torch.randn(1, Tk, 128, generator=g), torch.randn(1, Tk, 128, generator=g)
    q = 12.0 * k / k.norm(dim=-1, keepdim=True) * math.sqrt(128.0) + 0.01 * torch.randn(1, Tk, 128, generator=g)
    _in_range(q, k, v)
    outs, _ = _all_variants_vs_float64(cuda, q, k, v, torch.tensor([Tk], dtype=torch.int32), 1, "one dominant key per query")
    for variant, o in outs.items():
        d = (o[0].cpu() - v[0]).abs().amax(dim=-1)
        for j in range(Tk):
            assert d[j].item() < 1e-3 * v.abs().max().item(), f"variant {variant}: the query of key {j} did not return v[{j}] ({d[j].item():.3e})"


@pytest.mark.parametrize("Tq", [1, 15, 16, 17, 31, 32, 33, 255, 256, 257])
def test_query_edges(cuda, Tq):
    """the 16-query block inside a wave, a partly filled and an inactive wave, a second query block of the grid"""
    q, k, v = _draw(3, Tq, 48, 2, 3000 + Tq)
    _all_variants_vs_float64(cuda, q, k, v, torch.tensor([48, 31, 5], dtype=torch.int32), 2, f"Tq {Tq}")


def test_neighbour_independence_bitwise(cuda):
    """a query's bits do not depend on which other queries share its wave, its workgroup or the launch, nor on the workgroup order"""
    q, k, v = _draw(2, 257, 48, 2, 41)
    q, k, v = q.to(cuda), k.to(cuda), v.to(cuda)
    klens = torch.tensor([48, 21], dtype=torch.int32, device=cuda)
    for variant in _variants():
        o = _run(q, k, v, klens, 2, variant)
        assert torch.equal(o, _run(q, k, v, klens, 2, variant + 16)), f"variant {variant}: the workgroup order changed the result"
        for r in (0, 15, 16, 31, 32, 256):
            alone = _run(q[:, r:r + 1].contiguous(), k, v, klens, 2, variant)
            assert torch.equal(alone[:, 0], o[:, r]), f"variant {variant}: query row {r} depends on its neighbours"


def test_lazy_rescale_mixed_lanes(cuda):
    """three tiles; scores are a_i u1 + c_i u2 against the query. Queries 0-15 (u1): the tile maxima are 0, 1, 2 -- the running maximum
    creeps by less than LAZY_TAU per tile and in total, so it stays stale. Queries 16-31 (u1 + u2, same wave): + 5 on one key of tile 2,
    a jump of more than LAZY_TAU there, while their neighbours keep alpha = 1. Queries 32-47 (-u1, the next wave): the tile maxima
    fall, the maximum never moves and the wave skips the rescale."""
    Tk, Tq = 96, 48
    g = torch.Generator().manual_seed(11)
    u = torch.linalg.qr(torch.randn(128, 2, generator=g))[0].T               # two orthonormal directions
    a = torch.cat([torch.linspace(-1.0, 0.0, 32), torch.linspace(0.05, 1.0, 32), torch.linspace(1.05, 2.0, 32)])
    c = torch.zeros(Tk)
    c[64 + 13] = 5.0
    k = (a[:, None] * u[0] + c[:, None] * u[1] + 0.02 * torch.randn(Tk, 128, generator=g))[None]
    qs = torch.cat([u[0].expand(16, 128), (u[0] + u[1]).expand(16, 128), (-u[0]).expand(16, 128)])
    q = ((qs + 0.002 * torch.randn(Tq, 128, generator=g)) / SCALE)[None]
    v = torch.randn(1, Tk, 128, generator=g)
    _in_range(q, k, v)
    # the construction is what the docstring says (natural-log units, like LAZY_TAU)
    s = (q[0].double() * SCALE) @ k[0].double().T
    tmax = s.view(Tq, 3, 32).amax(dim=-1)
    run = torch.cummax(tmax, dim=1)[0]
    assert (tmax[:16, 1:] - tmax[:16, :1] < LAZY_TAU).all() and (tmax[:16, 1:] > tmax[:16, :-1]).all()
    assert (tmax[16:32, 1] - tmax[16:32, 0] < LAZY_TAU).all() and (tmax[16:32, 2] - run[16:32, 1] > LAZY_TAU).all()
    assert (tmax[32:, 1:] <= tmax[32:, :-1]).all()
    _all_variants_vs_float64(cuda, q, k, v, torch.tensor([Tk], dtype=torch.int32), 1, "lazy rescale, mixed lanes")


def test_cross_attention_small(cuda):
    """the decoder's shape in small: more keys than queries, several tiles, ragged key lengths down to one key"""
    q, k, v = _draw(3, 40, 208, 2, 5)
    _all_variants_vs_float64(cuda, q, k, v, torch.tensor([208, 1, 77], dtype=torch.int32), 2, "cross-attention 40 x 208")
