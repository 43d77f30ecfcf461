// Row kernels of the E-Branchformer encoder block (see ebranchformer.h): the exact GELU of the cgMLP, the convolutional spatial
// gating unit (LayerNorm statistics, then normalise + depthwise conv + gate) and the depthwise branch merge. The two conv kernels
// follow cf_glu_dw_kernel of conformer.hip: one thread per channel, a tile of 32 output rows with its halo in a thread-private column
// of LDS, the taps in registers.
#include "ebranchformer.h"

namespace pf {
namespace {

// x Phi(x) with 2 Phi(x) = 1 + erf(x / sqrt(2)) = erfc(-x / sqrt(2)): the first form right of zero, the second left of it, where
// 1 + erf would cancel (the tail keeps its relative precision; -0 stays -0)
__device__ __forceinline__ float gelu_(float x) {
    const float t = 0.70710678118654752f * x;
    return 0.5f * x * (x > 0.f ? 1.f + erff(t) : erfcf(-t));
}

__global__ void __launch_bounds__(256) eb_gelu_kernel(float* x, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<float4*>(x)[i];
    v = make_float4(gelu_(v.x), gelu_(v.y), gelu_(v.z), gelu_(v.w));
    reinterpret_cast<float4*>(x)[i] = v;
}

// one wave per row: mean and 1 / sqrt(var + eps) of the C gate channels (columns C .. 2 C of the row) -> stats[row] = (mean, rstd)
__global__ void __launch_bounds__(256) eb_gate_stats_kernel(const float* h, size_t M, int C, float eps, float* stats) {
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= M) return;
    const float* row = h + r * 2 * C + C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += row[c];
    const float mean = wave_sum(s) / (float)C;
    s = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = row[c] - mean; s = fmaf(d, d, s); }
    const float rstd = 1.f / sqrtf(wave_sum(s) / (float)C + eps);
    if (lane == 0) { stats[2 * r] = mean; stats[2 * r + 1] = rstd; }
}

constexpr int EB_TT = 32;      // output rows per workgroup
__global__ void __launch_bounds__(64) eb_csgu_kernel(const float* h, const float* stats, const float* gamma, const float* beta,
                                                     const float* dw, const float* dw_bias, int T, int C, int taps, float* y) {
    const int t0 = blockIdx.x * EB_TT, c = blockIdx.y * 64 + threadIdx.x, b = blockIdx.z, pad = taps / 2;
    __shared__ float xs[(EB_TT + 30) * 64];
    if (c >= C) return;                               // (C % 64 == 32: the upper half of the last channel block; no barrier below)
    const float ga = gamma[c], be = beta[c];
    const int nrows = EB_TT + taps - 1;
    for (int r = 0; r < nrows; ++r) {
        const int t = t0 - pad + r;
        float v = 0.f;
        if (t >= 0 && t < T) {
            const size_t row = (size_t)b * T + t;
            v = (h[row * 2 * C + C + c] - stats[2 * row]) * stats[2 * row + 1] * ga + be;
        }
        xs[r * 64 + threadIdx.x] = v;
    }
    float wk[31];
#pragma unroll
    for (int k = 0; k < 31; ++k) wk[k] = k < taps ? dw[(size_t)c * taps + k] : 0.f;
    const float bb = dw_bias[c];
    for (int r = 0; r < EB_TT; ++r) {
        const int t = t0 + r;
        if (t >= T) break;
        float acc = bb;
#pragma unroll
        for (int k = 0; k < 31; ++k)
            if (k < taps) acc = fmaf(wk[k], xs[(r + k) * 64 + threadIdx.x], acc);
        const size_t row = (size_t)b * T + t;
        y[row * C + c] = h[row * 2 * C + c] * acc;
    }
}

__global__ void __launch_bounds__(64) eb_merge_kernel(const float* x1, const float* x2, const float* dw, const float* dw_bias, int T,
                                                      int D, int taps, float* y) {
    const int t0 = blockIdx.x * EB_TT, c = blockIdx.y * 64 + threadIdx.x, b = blockIdx.z, pad = taps / 2;
    __shared__ float xs[(EB_TT + 30) * 64];
    const float* src = c < D ? x1 + c : x2 + (c - D);  // channel c of the concatenation, a column of its own buffer
    const int nrows = EB_TT + taps - 1;
    for (int r = 0; r < nrows; ++r) {
        const int t = t0 - pad + r;
        xs[r * 64 + threadIdx.x] = t >= 0 && t < T ? src[((size_t)b * T + t) * D] : 0.f;
    }
    float wk[31];
#pragma unroll
    for (int k = 0; k < 31; ++k) wk[k] = k < taps ? dw[(size_t)c * taps + k] : 0.f;
    const float bb = dw_bias[c];
    for (int r = 0; r < EB_TT; ++r) {
        const int t = t0 + r;
        if (t >= T) break;
        float acc = bb;
#pragma unroll
        for (int k = 0; k < 31; ++k)
            if (k < taps) acc = fmaf(wk[k], xs[(r + k) * 64 + threadIdx.x], acc);
        y[((size_t)b * T + t) * 2 * D + c] = xs[(r + pad) * 64 + threadIdx.x] + acc;
    }
}

}  // namespace

int launch_eb_gelu(float* x, size_t n, hipStream_t stream) {
    PF_REQUIRE(x && n > 0 && n % 4 == 0 && ((uintptr_t)x & 15) == 0 && n / 4 <= (size_t)0x7fffffff * 256, "eb_gelu: n % 4, 16-B aligned");
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(eb_gelu_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, x, n4);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eb_csgu(const float* h, const float* gamma, const float* beta, float eps, const float* dw, const float* dw_bias, int B, int T,
                   int C, int taps, float* stats, float* y, hipStream_t stream) {
    PF_REQUIRE(h && gamma && beta && dw && dw_bias && stats && y && B > 0 && B <= 65535 && T > 0 && (size_t)B * T <= 0x7fffffff && C > 0 &&
                   C % 32 == 0 && C <= 8192 && taps % 2 == 1 && taps >= 1 && taps <= 31 && eps > 0.f,
               "eb_csgu: gate channels % 32 (<= 8192), odd taps <= 31");
    const size_t M = (size_t)B * T;
    hipLaunchKernelGGL(eb_gate_stats_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, h, M, C, eps, stats);
    PF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(eb_csgu_kernel, dim3(ceil_div(T, EB_TT), ceil_div(C, 64), B), dim3(64), 0, stream, h, stats, gamma, beta, dw, dw_bias,
                       T, C, taps, y);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eb_merge(const float* x1, const float* x2, const float* dw, const float* dw_bias, int B, int T, int D, int taps, float* y,
                    hipStream_t stream) {
    PF_REQUIRE(x1 && x2 && dw && dw_bias && y && B > 0 && B <= 65535 && T > 0 && D > 0 && D % 32 == 0 && taps % 2 == 1 && taps >= 1 &&
                   taps <= 31,
               "eb_merge: D % 32, odd taps <= 31");
    hipLaunchKernelGGL(eb_merge_kernel, dim3(ceil_div(T, EB_TT), 2 * D / 64, B), dim3(64), 0, stream, x1, x2, dw, dw_bias, T, D, taps, y);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
