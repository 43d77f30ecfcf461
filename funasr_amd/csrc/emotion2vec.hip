// emotion2vec row kernels (see emotion2vec.h): waveform statistics, conv0 + LayerNorm + GELU, LayerNorm / GELU rows, the
// grouped positional conv, token assembly + context LayerNorm, and the pooled head.
#include "emotion2vec.h"

namespace pf {
namespace {

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// last b in [0, B) with off[b] <= r (off ascending)
__device__ __forceinline__ int find_seq(const int* off, int B, int r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) e2v_wav_stats_kernel(const float* wav, const int64_t* woff, int normalize, float* stats) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!normalize) {
        if (tid == 0) { stats[2 * b] = 0.f; stats[2 * b + 1] = 1.f; }
        return;
    }
    __shared__ double red[256];
    const int64_t s0 = woff[b], n = woff[b + 1] - s0;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += 256) acc += (double)wav[s0 + i];
    red[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    const double mean = red[0] / (double)n;
    __syncthreads();
    acc = 0.0;
    for (int64_t i = tid; i < n; i += 256) {
        const double d = (double)wav[s0 + i] - mean;
        acc += d * d;
    }
    red[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) {
        stats[2 * b] = (float)mean;
        stats[2 * b + 1] = (float)(1.0 / sqrt(red[0] / (double)n + 1e-5));
    }
}

__global__ void __launch_bounds__(512) e2v_conv0_kernel(const float* wav, const int64_t* woff, const float* stats, const int* so,
                                                        const int* nfr, int B, const float* w, int k0, int s0, const float* gamma,
                                                        const float* beta, float eps, float* y) {
    const int r = blockIdx.x, c = threadIdx.x, wave = c >> 6, lane = c & 63;
    const int b = find_seq(so, B, r);
    const int t = r - so[b];
    float* out = y + (size_t)r * 512;
    if (t >= nfr[b]) { out[c] = 0.f; return; }               // uniform over the block
    __shared__ float xs[32];
    __shared__ float red[16];
    if (c < k0) xs[c] = (wav[woff[b] + (int64_t)t * s0 + c] - stats[2 * b]) * stats[2 * b + 1];
    __syncthreads();
    float acc = 0.f;
    for (int j = 0; j < k0; ++j) acc = fmaf(w[c * k0 + j], xs[j], acc);
    const float s = wave_sum(acc);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    float tot = 0.f;
    for (int i = 0; i < 8; ++i) tot += red[i];
    const float d = acc - tot / 512.f;
    const float q = wave_sum(d * d);
    if (lane == 0) red[8 + wave] = q;
    __syncthreads();
    float tq = 0.f;
    for (int i = 0; i < 8; ++i) tq += red[8 + i];
    const float rstd = 1.f / sqrtf(tq / 512.f + eps);
    out[c] = gelu_erf(d * rstd * gamma[c] + beta[c]);
}

// LayerNorm of the NC float4 chunks a lane holds (row of 256 NC values over one wave), in place
template <int NC>
__device__ __forceinline__ void wave_ln(float4 (&v)[NC], int D, const float* gamma, const float* beta, float eps, int lane) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) s += ln_sum4(v[i]);
    const float mean = ln_mean(wave_sum(s), D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) q += ln_sqdev4(v[i], mean);
    const float rstd = ln_rstd(wave_sum(q), D, eps);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = (i * 64 + lane) * 4;
        const float4 g = gamma ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 bb = beta ? *reinterpret_cast<const float4*>(beta + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[i] = ln_apply4(v[i], mean, rstd, g, bb);
    }
}

template <int NC>
__global__ void __launch_bounds__(256) e2v_rows_kernel(E2vRowArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.M) return;
    const int ir = a.in_map ? a.in_map[r] : r;
    const float* x = a.x + (size_t)ir * a.ldx;
    float4 v[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) v[i] = *reinterpret_cast<const float4*>(x + (i * 64 + lane) * 4);
    if (a.ln) wave_ln<NC>(v, a.D, a.gamma, a.beta, a.eps, lane);
    if (a.gelu) {
#pragma unroll
        for (int i = 0; i < NC; ++i) v[i] = make_float4(gelu_erf(v[i].x), gelu_erf(v[i].y), gelu_erf(v[i].z), gelu_erf(v[i].w));
    }
    float* y = a.y + (size_t)r * a.ldy;
#pragma unroll
    for (int i = 0; i < NC; ++i) *reinterpret_cast<float4*>(y + (i * 64 + lane) * 4) = v[i];
}

constexpr int PC_ROWS = 32;
__global__ void __launch_bounds__(256) e2v_posconv_kernel(const float* x, const float* wp, const float* bias, const int* foff, int B,
                                                          int F, int D, int G, int taps, float* y) {
    const int Cg = D / G, g = blockIdx.y, r0 = blockIdx.x * PC_ROWS, pad = taps / 2;
    __shared__ float xs[(PC_ROWS + 30) * 64];
    const int nrows = PC_ROWS + taps - 1;
    for (int i = threadIdx.x; i < nrows * Cg; i += 256) {
        const int rr = i / Cg, cc = i - rr * Cg, gr = r0 - pad + rr;
        xs[i] = (gr >= 0 && gr < F) ? x[(size_t)gr * D + g * Cg + cc] : 0.f;
    }
    __syncthreads();
    const int o = threadIdx.x & 63, rs = (threadIdx.x >> 6) * 8;
    if (o >= Cg) return;
    int lo[8], hi[8];
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = r0 + rs + i, rc = r < F ? r : F - 1;
        const int b = find_seq(foff, B, rc);
        lo[i] = foff[b]; hi[i] = foff[b + 1]; acc[i] = 0.f;
    }
    const float* wg = wp + (size_t)g * taps * Cg * Cg;
    for (int k = 0; k < taps; ++k)
        for (int ci = 0; ci < Cg; ++ci) {
            const float wv = wg[((size_t)k * Cg + ci) * Cg + o];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ri = r0 + rs + i + k - pad;
                const float xv = xs[(rs + i + k) * Cg + ci];
                acc[i] = fmaf(wv, (ri >= lo[i] && ri < hi[i]) ? xv : 0.f, acc[i]);
            }
        }
    const float bo = bias[g * Cg + o];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = r0 + rs + i;
        if (r < F) y[(size_t)r * D + g * Cg + o] = acc[i] + bo;
    }
}

template <int NC>
__global__ void __launch_bounds__(256) e2v_tokens_kernel(const float* xf, const float* pos, const float* extra, int E, const int* foff,
                                                         const int* toff, int B, int Ntok, int D, const float* gamma, const float* beta,
                                                         float eps, float* y) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= Ntok) return;
    const int b = find_seq(toff, B, r), t = r - toff[b];
    float4 v[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (t < E) {
            v[i] = *reinterpret_cast<const float4*>(extra + (size_t)t * D + c);
        } else {
            const size_t f = (size_t)(foff[b] + t - E) * D + c;
            const float4 a = *reinterpret_cast<const float4*>(xf + f), p = *reinterpret_cast<const float4*>(pos + f);
            v[i] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
        }
    }
    wave_ln<NC>(v, D, gamma, beta, eps, lane);
#pragma unroll
    for (int i = 0; i < NC; ++i) *reinterpret_cast<float4*>(y + (size_t)r * D + (i * 64 + lane) * 4) = v[i];
}

__global__ void __launch_bounds__(256) e2v_head_kernel(const float* x, const int* toff, int E, int D, const float* W, const float* bias,
                                                       const int* mask, int C, float* pooled, float* probs) {
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ float pl[4096];
    __shared__ float lg[1024];
    const int r0 = toff[b] + E, T = toff[b + 1] - r0;
    for (int d = tid; d < D; d += 256) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += x[(size_t)(r0 + t) * D + d];
        const float p = s / (float)T;
        pl[d] = p;
        pooled[(size_t)b * D + d] = p;
    }
    if (C <= 0) return;
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s = fmaf(W[(size_t)c * D + d], pl[d], s);
        s = wave_sum(s);
        if (lane == 0) lg[c] = s + bias[c];
    }
    __syncthreads();
    if (wave != 0) return;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) if (!mask[c]) m = fmaxf(m, lg[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) if (!mask[c]) s += expf(lg[c] - m);
    s = wave_sum(s);
    for (int c = lane; c < C; c += 64) probs[(size_t)b * C + c] = mask[c] ? 0.f : expf(lg[c] - m) / s;
}

}  // namespace

int launch_e2v_wav_stats(const float* wav, const int64_t* woff, int B, int normalize, float* stats, hipStream_t stream) {
    PF_REQUIRE(B > 0, "e2v_wav_stats: empty batch");
    hipLaunchKernelGGL(e2v_wav_stats_kernel, dim3(B), dim3(256), 0, stream, wav, woff, normalize, stats);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_e2v_conv0(const float* wav, const int64_t* woff, const float* stats, const int* so, const int* nfr, int B, int M,
                     const float* w, int k0, int s0, const float* gamma, const float* beta, float eps, float* y, hipStream_t stream) {
    PF_REQUIRE(B > 0 && M > 0 && k0 > 0 && k0 <= 32 && s0 > 0, "e2v_conv0: bad shape (k0 <= 32)");
    hipLaunchKernelGGL(e2v_conv0_kernel, dim3(M), dim3(512), 0, stream, wav, woff, stats, so, nfr, B, w, k0, s0, gamma, beta, eps, y);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

#define E2V_NC_SWITCH(NCV, LAUNCH)                                                        \
    switch (NCV) {                                                                      \
        case 1: LAUNCH(1); break;                                                       \
        case 2: LAUNCH(2); break;                                                       \
        case 3: LAUNCH(3); break;                                                       \
        case 4: LAUNCH(4); break;                                                       \
        case 8: LAUNCH(8); break;                                                       \
        case 12: LAUNCH(12); break;                                                     \
        case 16: LAUNCH(16); break;                                                     \
        default: set_error("e2v: row width must be 256 x {1, 2, 3, 4, 8, 12, 16}"); return -1; \
    }

int launch_e2v_rows(const E2vRowArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.M > 0 && a.D % 256 == 0 && a.ldx % 4 == 0 && a.ldy % 4 == 0, "e2v_rows: bad shape");
    const dim3 grid(ceil_div(a.M, 4));
#define E2V_ROWS(N) hipLaunchKernelGGL((e2v_rows_kernel<N>), grid, dim3(256), 0, stream, a)
    E2V_NC_SWITCH(a.D / 256, E2V_ROWS)
#undef E2V_ROWS
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_e2v_posconv(const float* x, const float* wp, const float* bias, const int* foff, int B, int F, int D, int groups,
                       int taps, float* y, hipStream_t stream) {
    PF_REQUIRE(F > 0 && B > 0 && groups > 0 && D % groups == 0 && D / groups <= 64 && taps % 2 == 1 && taps <= 31,
               "e2v_posconv: D / groups <= 64, odd taps <= 31");
    hipLaunchKernelGGL(e2v_posconv_kernel, dim3(ceil_div(F, PC_ROWS), groups), dim3(256), 0, stream, x, wp, bias, foff, B, F, D, groups,
                       taps, y);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_e2v_tokens(const float* xf, const float* pos, const float* extra, int n_extra, const int* foff, const int* toff, int B,
                      int Ntok, int D, const float* gamma, const float* beta, float eps, float* y, hipStream_t stream) {
    PF_REQUIRE(Ntok > 0 && B > 0 && D % 256 == 0, "e2v_tokens: bad shape");
    const dim3 grid(ceil_div(Ntok, 4));
#define E2V_TOK(N) \
    hipLaunchKernelGGL((e2v_tokens_kernel<N>), grid, dim3(256), 0, stream, xf, pos, extra, n_extra, foff, toff, B, Ntok, D, gamma, beta, eps, y)
    E2V_NC_SWITCH(D / 256, E2V_TOK)
#undef E2V_TOK
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_e2v_head(const float* x, const int* toff, int n_extra, int B, int D, const float* W, const float* bias, const int* mask,
                    int C, float* pooled, float* probs, hipStream_t stream) {
    PF_REQUIRE(B > 0 && D > 0 && D <= 4096 && C >= 0 && C <= 1024 && (C == 0 || (W && bias && mask && probs)), "e2v_head: bad shape");
    hipLaunchKernelGGL(e2v_head_kernel, dim3(B), dim3(256), 0, stream, x, toff, n_extra, D, W, bias, mask, C, pooled, probs);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
