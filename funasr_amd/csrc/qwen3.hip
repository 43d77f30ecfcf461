// Row and attention kernels of the Qwen3 causal LM decoder (qwen3.h has the contracts). fp32, gfx950, 64-lane waves.
//
// The two attention kernels share one tile loop (q3_tiles). A workgroup of four waves stages a tile of KT keys -- K rows padded to hd + 1
// floats, V rows plain -- into LDS once, and every wave runs its four (query row, head) pairs against it:
//   scores   lane = (half of head_dim, key): 64 products per lane per pair, q broadcast from LDS, K conflict-free through the padding;
//            head_dim 128 adds the two halves with one cross-lane exchange
//   softmax  online over the tiles: running (m, l) per pair, one wave_max and one wave_sum per pair and tile, expf (never the fast form)
//   P V      lane = output column: p of key j comes out of lane j with a readlane, V[j] is read row-wise (conflict-free)
// All G = Hq / Hkv query heads of a K/V head are pairs of the SAME workgroup, so the cache is read once per group and tile. The math is
// plain fp32 FMA, not the matrix cores: prompts of an ASR LM are a few hundred rows and the step is bound by the weight stream of the
// GEMMs around it, not by this kernel.
#include <math.h>

#include "qwen3.h"

namespace pf {

namespace {

constexpr int Q3_THREADS = 256, Q3_WAVES = 4, Q3_PW = Q3_PAIRS / Q3_WAVES;
static_assert(Q3_PW == 4, "q3_tiles tests its four pairs by name");

// ---------------------------------------------------------------------------------------------------------------- RMSNorm
__global__ __launch_bounds__(Q3_THREADS) void q3_rmsnorm_kernel(const float* x, int ldx, const float* __restrict__ w, float eps,
                                                                float* y, int ldy, int M, int D) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * Q3_WAVES + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (size_t)row * ldx;
    float ss = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c);
        ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    ss = wave_sum(ss);
    const float r = 1.0f / sqrtf(ss / (float)D + eps);
    float* yr = y + (size_t)row * ldy;
    for (int c = lane * 4; c < D; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c), g = *reinterpret_cast<const float4*>(w + c);
        float4 o;
        o.x = v.x * r * g.x; o.y = v.y * r * g.y; o.z = v.z * r * g.z; o.w = v.w * r * g.w;
        *reinterpret_cast<float4*>(yr + c) = o;
    }
}

// --------------------------------------------------------------------------------------------- q/k RMSNorm + RoPE + cache write
template <int HD>
__global__ __launch_bounds__(Q3_THREADS) void q3_qk_rope_kernel(Q3RopeArgs a) {
#pragma clang fp contract(off)
    constexpr int NE = HD / 64, HALF = HD / 2;
    const int lane = threadIdx.x & 63, nh = a.Hq + 2 * a.Hkv;
    const long long unit = (long long)blockIdx.x * Q3_WAVES + (threadIdx.x >> 6);
    if (unit >= (long long)a.M * nh) return;
    const int row = (int)(unit / nh), head = (int)(unit % nh);
    const float* src = a.qkv + (size_t)row * a.ld + (size_t)head * HD;
    float v[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) v[i] = src[lane + 64 * i];
    const int slot = a.row_seq[row], pos = a.row_pos[row];
    if (head >= a.Hq + a.Hkv) {      // a value head: copied as it is
        float* dst = a.vc + (((size_t)slot * a.Hkv + (head - a.Hq - a.Hkv)) * a.cap + pos) * HD;
#pragma unroll
        for (int i = 0; i < NE; ++i) dst[lane + 64 * i] = v[i];
        return;
    }
    const bool is_q = head < a.Hq;
    const float* w = is_q ? a.qw : a.kw;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NE; ++i) ss += v[i] * v[i];
    ss = wave_sum(ss);
    const float r = 1.0f / sqrtf(ss / (float)HD + a.eps);
#pragma unroll
    for (int i = 0; i < NE; ++i) v[i] = v[i] * r * w[lane + 64 * i];
    float* dst = is_q ? a.q_out + (size_t)row * a.ldq + (size_t)head * HD
                      : a.kc + (((size_t)slot * a.Hkv + (head - a.Hq)) * a.cap + pos) * HD;
    const float* cr = a.cos_t + (size_t)pos * HALF;
    const float* sr = a.sin_t + (size_t)pos * HALF;
    if (HD == 64) {                  // column lane pairs with column lane ^ 32
        const float other = __shfl_xor(v[0], 32, 64);
        const float c = cr[lane & 31], s = sr[lane & 31];
        dst[lane] = lane < 32 ? v[0] * c - other * s : v[0] * c + other * s;
    } else {                         // columns lane and lane + 64 pair in the lane
        const float c = cr[lane], s = sr[lane];
        dst[lane] = v[0] * c - v[NE - 1] * s;
        dst[lane + 64] = v[NE - 1] * c + v[0] * s;
    }
}

// ------------------------------------------------------------------------------------------------------------ attention tiles
template <int HD>
struct Q3Smem {
    static constexpr int KT = HD == 64 ? 64 : 32;
    float V[KT][HD];
    float Q[Q3_PAIRS][HD];
    float K[KT][HD + 1];
};

// Keys [k0, k1) of one (slot, K/V head) against the wave's Q3_PW pairs; pair t sees keys <= lim[t] (lim < k0: none of them). k0, k1 are
// uniform over the workgroup (the loop holds its barriers); q of pair t is sm.Q[wave * Q3_PW + t], written before the call.
template <int HD>
__device__ __forceinline__ void q3_tiles(const float* __restrict__ kb, const float* __restrict__ vb, int k0, int k1, const int (&lim)[Q3_PW],
                                         float scale, float (&m)[Q3_PW], float (&l)[Q3_PW], float (&o)[Q3_PW][HD / 64], Q3Smem<HD>& sm) {
    constexpr int KT = Q3Smem<HD>::KT, NE = HD / 64, C4 = HD / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane % KT, h = lane / KT;
    for (int t0 = k0; t0 < k1; t0 += KT) {
        __syncthreads();
        for (int idx = tid; idx < KT * C4; idx += Q3_THREADS) {
            const int jj = idx / C4, c = (idx % C4) * 4, key = t0 + jj;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (key < k1) {
                kv = *reinterpret_cast<const float4*>(kb + (size_t)key * HD + c);
                vv = *reinterpret_cast<const float4*>(vb + (size_t)key * HD + c);
            }
            sm.K[jj][c] = kv.x; sm.K[jj][c + 1] = kv.y; sm.K[jj][c + 2] = kv.z; sm.K[jj][c + 3] = kv.w;
            *reinterpret_cast<float4*>(&sm.V[jj][c]) = vv;
        }
        __syncthreads();
        if (lim[Q3_PW - 1] < t0 && lim[0] < t0 && lim[1] < t0 && lim[2] < t0) continue;      // (uniform over the wave)
        float s[Q3_PW];
#pragma unroll
        for (int t = 0; t < Q3_PW; ++t) s[t] = 0.f;
        const float* kr = &sm.K[j][h * 64];
#pragma unroll 4
        for (int d = 0; d < 64; d += 4) {
            const float ka = kr[d], kb4 = kr[d + 1], kc4 = kr[d + 2], kd = kr[d + 3];
#pragma unroll
            for (int t = 0; t < Q3_PW; ++t) {
                const float4 q4 = *reinterpret_cast<const float4*>(&sm.Q[wave * Q3_PW + t][h * 64 + d]);
                s[t] = fmaf(q4.x, ka, s[t]); s[t] = fmaf(q4.y, kb4, s[t]); s[t] = fmaf(q4.z, kc4, s[t]); s[t] = fmaf(q4.w, kd, s[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < Q3_PW; ++t) {
            if (lim[t] < t0) continue;                                                       // (uniform over the wave)
            float sc = s[t];
            if (HD == 128) sc += __shfl_xor(sc, 32, 64);
            const bool live = t0 + j <= lim[t];
            sc = live ? sc * scale : -INFINITY;
            const float mn = fmaxf(m[t], wave_max(sc));                                      // finite: key t0 is live
            const float alpha = expf(m[t] - mn);
            const float p = live ? expf(sc - mn) : 0.f;
            l[t] = l[t] * alpha + wave_sum(lane < KT ? p : 0.f);
            m[t] = mn;
            float acc[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) acc[i] = o[t][i] * alpha;
#pragma unroll
            for (int jj = 0; jj < KT; ++jj) {
                const float pj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p), jj));
#pragma unroll
                for (int i = 0; i < NE; ++i) acc[i] = fmaf(pj, sm.V[jj][lane + 64 * i], acc[i]);
            }
#pragma unroll
            for (int i = 0; i < NE; ++i) o[t][i] = acc[i];
        }
    }
}

template <int HD>
__global__ __launch_bounds__(Q3_THREADS) void q3_prefill_kernel(Q3PrefillArgs a, int QT, int G, int rounds) {
    constexpr int NE = HD / 64;
    __shared__ __align__(16) Q3Smem<HD> sm;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.z, kvh = blockIdx.y, qt = blockIdx.x / rounds, round = blockIdx.x % rounds;
    const int nrows = a.nrows[i], q0 = qt * QT;
    if (q0 >= nrows) return;                                                                 // (uniform over the workgroup)
    const int slot = a.seq[i], p0 = a.p0[i], row0 = a.row0[i];
    const int rows_here = nrows - q0 < QT ? nrows - q0 : QT;
    int lim[Q3_PW], qrow[Q3_PW], head[Q3_PW];
    float m[Q3_PW], l[Q3_PW], o[Q3_PW][NE];
#pragma unroll
    for (int t = 0; t < Q3_PW; ++t) {
        const int p = round * Q3_PAIRS + wave * Q3_PW + t;
        const bool ok = p < QT * G && p / G < rows_here;
        qrow[t] = q0 + p / G; head[t] = kvh * G + p % G;
        lim[t] = ok ? p0 + qrow[t] : -1;
        m[t] = -INFINITY; l[t] = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            o[t][e] = 0.f;
            sm.Q[wave * Q3_PW + t][lane + 64 * e] = ok ? a.q[(size_t)(row0 + qrow[t]) * a.ldq + (size_t)head[t] * HD + lane + 64 * e] : 0.f;
        }
    }
    const size_t base = ((size_t)slot * a.Hkv + kvh) * a.cap * HD;
    q3_tiles<HD>(a.kc + base, a.vc + base, 0, p0 + q0 + rows_here, lim, a.scale, m, l, o, sm);
#pragma unroll
    for (int t = 0; t < Q3_PW; ++t) {
        if (lim[t] < 0) continue;
        const float inv = 1.0f / l[t];
#pragma unroll
        for (int e = 0; e < NE; ++e) a.out[(size_t)(row0 + qrow[t]) * a.ldo + (size_t)head[t] * HD + lane + 64 * e] = o[t][e] * inv;
    }
}

template <int HD>
__global__ __launch_bounds__(Q3_THREADS) void q3_decode_kernel(Q3DecodeArgs a, int G, int rounds, int nsplit) {
    constexpr int NE = HD / 64;
    __shared__ __align__(16) Q3Smem<HD> sm;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.z, kvh = blockIdx.y / rounds, round = blockIdx.y % rounds, split = blockIdx.x;
    const int len = a.row_len[r], k0 = split * Q3_KSPLIT;
    if (k0 >= len) return;                                                                   // (uniform over the workgroup)
    const int k1 = len < k0 + Q3_KSPLIT ? len : k0 + Q3_KSPLIT, slot = a.row_seq[r];
    int lim[Q3_PW], head[Q3_PW];
    float m[Q3_PW], l[Q3_PW], o[Q3_PW][NE];
#pragma unroll
    for (int t = 0; t < Q3_PW; ++t) {
        const int p = round * Q3_PAIRS + wave * Q3_PW + t;
        const bool ok = p < G;
        head[t] = kvh * G + (ok ? p : 0);
        lim[t] = ok ? len - 1 : -1;
        m[t] = -INFINITY; l[t] = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            o[t][e] = 0.f;
            sm.Q[wave * Q3_PW + t][lane + 64 * e] = ok ? a.q[(size_t)r * a.ldq + (size_t)head[t] * HD + lane + 64 * e] : 0.f;
        }
    }
    const size_t base = ((size_t)slot * a.Hkv + kvh) * a.cap * HD;
    q3_tiles<HD>(a.kc + base, a.vc + base, k0, k1, lim, a.scale, m, l, o, sm);
#pragma unroll
    for (int t = 0; t < Q3_PW; ++t) {
        if (lim[t] < 0) continue;
        float* dst = a.part + (((size_t)r * a.Hq + head[t]) * nsplit + split) * (HD + 2);
#pragma unroll
        for (int e = 0; e < NE; ++e) dst[lane + 64 * e] = o[t][e];
        if (lane == 0) { dst[HD] = m[t]; dst[HD + 1] = l[t]; }
    }
}

// one wave per (row, head): merge the splits [0, ceil(len / KSPLIT)) in split order
template <int HD>
__global__ __launch_bounds__(Q3_THREADS) void q3_decode_merge_kernel(Q3DecodeArgs a, int nsplit) {
    constexpr int NE = HD / 64;
    const int lane = threadIdx.x & 63;
    const long long unit = (long long)blockIdx.x * Q3_WAVES + (threadIdx.x >> 6);
    if (unit >= (long long)a.M * a.Hq) return;
    const int r = (int)(unit / a.Hq), head = (int)(unit % a.Hq);
    const int ns = (a.row_len[r] + Q3_KSPLIT - 1) / Q3_KSPLIT;
    const float* src = a.part + ((size_t)r * a.Hq + head) * nsplit * (HD + 2);
    float mx = -INFINITY;
    for (int s = 0; s < ns; ++s) mx = fmaxf(mx, src[(size_t)s * (HD + 2) + HD]);
    float l = 0.f, acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.f;
    for (int s = 0; s < ns; ++s) {
        const float* ps = src + (size_t)s * (HD + 2);
        const float f = expf(ps[HD] - mx);
        l = fmaf(ps[HD + 1], f, l);
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] = fmaf(ps[lane + 64 * e], f, acc[e]);
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int e = 0; e < NE; ++e) a.out[(size_t)r * a.ldo + (size_t)head * HD + lane + 64 * e] = acc[e] * inv;
}

// ---------------------------------------------------------------------------------------------------------------- SwiGLU
__global__ __launch_bounds__(Q3_THREADS) void q3_swiglu_kernel(const float* __restrict__ gu, int ld, float* __restrict__ out, int ldo, int M, int I) {
    for (int row = blockIdx.y; row < M; row += gridDim.y) {
        const float* g = gu + (size_t)row * ld;
        float* o = out + (size_t)row * ldo;
        for (int c = (blockIdx.x * Q3_THREADS + threadIdx.x) * 4; c < I; c += gridDim.x * Q3_THREADS * 4) {
            const float4 a = *reinterpret_cast<const float4*>(g + c), u = *reinterpret_cast<const float4*>(g + I + c);
            float4 v;
            v.x = a.x / (1.0f + expf(-a.x)) * u.x;
            v.y = a.y / (1.0f + expf(-a.y)) * u.y;
            v.z = a.z / (1.0f + expf(-a.z)) * u.z;
            v.w = a.w / (1.0f + expf(-a.w)) * u.w;
            *reinterpret_cast<float4*>(o + c) = v;
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_q3_rmsnorm(const float* x, int ldx, const float* w, float eps, float* y, int ldy, int M, int D, hipStream_t stream) {
    PF_REQUIRE(x && w && y && M > 0 && D > 0 && D % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= D && ldy >= D,
               "q3_rmsnorm: width and row strides must be multiples of 4 floats");
    PF_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y), "q3_rmsnorm: operands must be 16-B aligned");
    hipLaunchKernelGGL(q3_rmsnorm_kernel, dim3(ceil_div(M, Q3_WAVES)), dim3(Q3_THREADS), 0, stream, x, ldx, w, eps, y, ldy, M, D);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_q3_qk_rope(const Q3RopeArgs& a, hipStream_t stream) {
    PF_REQUIRE(q3_head_dim_ok(a.hd), "q3_qk_rope: head_dim must be 64 or 128");
    PF_REQUIRE(a.qkv && a.qw && a.kw && a.cos_t && a.sin_t && a.row_seq && a.row_pos && a.q_out && a.kc && a.vc, "q3_qk_rope: null operand");
    PF_REQUIRE(a.M > 0 && a.Hq > 0 && a.Hkv > 0 && a.cap > 0 && a.ld >= (a.Hq + 2 * a.Hkv) * a.hd && a.ldq >= a.Hq * a.hd,
               "q3_qk_rope: rows narrower than their heads");
    const long long units = (long long)a.M * (a.Hq + 2 * a.Hkv);
    PF_REQUIRE(units <= 0x7fffffffLL, "q3_qk_rope: too many rows");
    const dim3 grid((unsigned)((units + Q3_WAVES - 1) / Q3_WAVES)), block(Q3_THREADS);
    if (a.hd == 64) hipLaunchKernelGGL(q3_qk_rope_kernel<64>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(q3_qk_rope_kernel<128>, grid, block, 0, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_q3_prefill_attention(const Q3PrefillArgs& a, hipStream_t stream) {
    PF_REQUIRE(q3_head_dim_ok(a.hd), "q3_prefill_attention: head_dim must be 64 or 128");
    PF_REQUIRE(a.q && a.kc && a.vc && a.out && a.seq && a.row0 && a.nrows && a.p0, "q3_prefill_attention: null operand");
    PF_REQUIRE(a.nseq > 0 && a.nseq <= 65535 && a.max_rows > 0 && a.Hq > 0 && a.Hkv > 0 && a.Hkv <= 65535 && a.Hq % a.Hkv == 0 && a.cap > 0,
               "q3_prefill_attention: empty problem, or heads that do not group");
    PF_REQUIRE(a.ldq % 4 == 0 && a.ldo % 4 == 0 && a.ldq >= a.Hq * a.hd && a.ldo >= a.Hq * a.hd && aligned16(a.q) && aligned16(a.kc) &&
               aligned16(a.vc) && aligned16(a.out), "q3_prefill_attention: operands must be 16-B aligned");
    const int G = a.Hq / a.Hkv, QT = q3_qtile(G), rounds = ceil_div(QT * G, Q3_PAIRS);
    const dim3 grid((unsigned)(ceil_div(a.max_rows, QT) * rounds), (unsigned)a.Hkv, (unsigned)a.nseq), block(Q3_THREADS);
    if (a.hd == 64) hipLaunchKernelGGL(q3_prefill_kernel<64>, grid, block, 0, stream, a, QT, G, rounds);
    else hipLaunchKernelGGL(q3_prefill_kernel<128>, grid, block, 0, stream, a, QT, G, rounds);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_q3_decode_attention(const Q3DecodeArgs& a, hipStream_t stream) {
    PF_REQUIRE(q3_head_dim_ok(a.hd), "q3_decode_attention: head_dim must be 64 or 128");
    PF_REQUIRE(a.q && a.kc && a.vc && a.out && a.row_seq && a.row_len && a.part, "q3_decode_attention: null operand");
    PF_REQUIRE(a.M > 0 && a.M <= 65535 && a.max_len > 0 && a.max_len <= a.cap && a.Hq > 0 && a.Hkv > 0 && a.Hq % a.Hkv == 0,
               "q3_decode_attention: empty problem, lengths past the cache, or heads that do not group");
    PF_REQUIRE(a.ldq % 4 == 0 && a.ldo % 4 == 0 && a.ldq >= a.Hq * a.hd && a.ldo >= a.Hq * a.hd && aligned16(a.q) && aligned16(a.kc) &&
               aligned16(a.vc) && aligned16(a.out), "q3_decode_attention: operands must be 16-B aligned");
    const int G = a.Hq / a.Hkv, rounds = ceil_div(G, Q3_PAIRS), nsplit = ceil_div(a.max_len, Q3_KSPLIT);
    PF_REQUIRE((long long)a.Hkv * rounds <= 65535, "q3_decode_attention: too many heads");
    const dim3 grid((unsigned)nsplit, (unsigned)(a.Hkv * rounds), (unsigned)a.M), block(Q3_THREADS);
    const dim3 mgrid((unsigned)ceil_div(a.M * a.Hq, Q3_WAVES));
    if (a.hd == 64) {
        hipLaunchKernelGGL(q3_decode_kernel<64>, grid, block, 0, stream, a, G, rounds, nsplit);
        hipLaunchKernelGGL(q3_decode_merge_kernel<64>, mgrid, block, 0, stream, a, nsplit);
    } else {
        hipLaunchKernelGGL(q3_decode_kernel<128>, grid, block, 0, stream, a, G, rounds, nsplit);
        hipLaunchKernelGGL(q3_decode_merge_kernel<128>, mgrid, block, 0, stream, a, nsplit);
    }
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_q3_swiglu(const float* gu, int ld, float* out, int ldo, int M, int I, hipStream_t stream) {
    PF_REQUIRE(gu && out && M > 0 && I > 0 && I % 4 == 0 && ld % 4 == 0 && ldo % 4 == 0 && ld >= 2 * I && ldo >= I,
               "q3_swiglu: width and row strides must be multiples of 4 floats");
    PF_REQUIRE(aligned16(gu) && aligned16(out), "q3_swiglu: operands must be 16-B aligned");
    const int bx = ceil_div(I, Q3_THREADS * 4);
    hipLaunchKernelGGL(q3_swiglu_kernel, dim3((unsigned)(bx < 64 ? bx : 64), (unsigned)(M < 65535 ? M : 65535)), dim3(Q3_THREADS), 0, stream, gu, ld,
                       out, ldo, M, I);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
