// Paraformer-v2 posterior embedder, row kernels: row softmax + arg-max of the CTC logits, run segmentation of the greedy path,
// and the fused mean / bias / LayerNorm / ReLU / positional-encoding row kernel that writes the decoder input (ctc_merge.h).
// Plain C++ on 64-wide waves: shuffles inside a wave, LDS between the four waves of a workgroup, vector stores only.
#include "ctc_merge.h"

namespace pf {
namespace {

// ---------------------------------------------------------------------------------------- softmax + arg-max
// One workgroup per row, three passes over a row the GEMM in front has just left in L2 (8404 columns = 33 KB): max with its first
// column, exp(x - max) stored in place and summed, the division. torch.softmax's arithmetic: exp(x - max) / sum.
__global__ __launch_bounds__(256) void softmax_argmax_rows_kernel(float* __restrict__ x, int ld, int M, int V, int Vp,
                                                                  int* __restrict__ ids) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float ss[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x;
    if (row >= M) return;
    float* xr = x + (size_t)row * ld;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = threadIdx.x; j < V; j += 256) {
        const float v = xr[j];
        if (v > bv) { bv = v; bi = j; }                          // ascending columns per thread: the first maximum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    bv = sv[0]; bi = si[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
    if (threadIdx.x == 0) ids[row] = bi == 0x7fffffff ? 0 : bi;  // a row of -inf only: the first column (torch.argmax)
    float sum = 0.f;
    for (int j = threadIdx.x; j < V; j += 256) {
        const float e = expf(xr[j] - bv);
        xr[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) ss[wave] = sum;
    __syncthreads();
    const float total = (ss[0] + ss[1]) + (ss[2] + ss[3]);
    for (int j = threadIdx.x; j < Vp; j += 256) xr[j] = j < V ? xr[j] / total : 0.f;      // each thread re-reads its own columns
}

// -------------------------------------------------------------------------------------------- run scan
// One workgroup per clip, 256 frames per trip. Frame t starts a run when its label is not blank and differs from frame t - 1's (or
// t == 0), ends one when it differs from frame t + 1's (or t + 1 == len): the same label on both sides of a blank gives two runs,
// frames >= len never take part. The index of a run is the number of starts in front of it: ballot + popcount inside a wave, the
// four waves' counts through LDS, the trips' counts in a register every thread carries.
__global__ __launch_bounds__(256) void ctc_runs_kernel(const int* __restrict__ ids, const int* __restrict__ lens, int T, int blank,
                                                       int* __restrict__ counts, int* __restrict__ ranges, int ld) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int* row = ids + (size_t)b * T;
    int len = lens[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    int base = 0;
    for (int t0 = 0; t0 < len; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        const bool valid = t < len;
        const int cur = valid ? row[t] : blank;
        const int prev = (valid && t > 0) ? row[t - 1] : blank;
        const int next = (valid && t + 1 < len) ? row[t + 1] : blank;
        const bool tok = cur != blank;
        const bool start = tok && cur != prev, end = tok && cur != next;
        const unsigned long long m = __ballot(start);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int j = base + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) j += wsum[w];
        base += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (start && j < ld) ranges[((size_t)b * ld + j) * 2] = t;
        const int je = j + (start ? 1 : 0) - 1;                   // the run frame t belongs to
        if (end && je >= 0 && je < ld) ranges[((size_t)b * ld + je) * 2 + 1] = t + 1;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[b] = base;
}

// ------------------------------------------------------------------------------------ mean + LayerNorm + ReLU + PE
// One wave per token (four per workgroup): lane l holds columns 4 (l + 64 i) .. + 3 of the row in registers (D <= 2048), the
// LayerNorm statistics are the two-pass fp32 form of layernorm_kernel (common.h helpers, 64-lane butterfly). x * xscale + pe is
// rounded product, then rounded sum, as the reference's two tensor operations are.
constexpr int PE_MAX_CHUNKS = 8;
__global__ __launch_bounds__(256) void posterior_embed_kernel(const PosteriorEmbedArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long tok = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= (long)a.B * a.N) return;
    const int b = (int)(tok / a.N), j = (int)(tok % a.N);
    float* out = a.embeds + (size_t)tok * a.D;
    const int n = a.counts[b];
    const bool live = j < n && j < a.ld;
    const int s = live ? a.ranges[((size_t)b * a.ld + j) * 2] : 0, e = live ? a.ranges[((size_t)b * a.ld + j) * 2 + 1] : 0;
    if (a.ranges_out && lane == 0) *reinterpret_cast<int2*>(a.ranges_out + (size_t)tok * 2) = make_int2(s, e);
    if (!live || s < 0 || e > a.T || e <= s) {                    // (a range outside the clip cannot come from ctc_runs_kernel)
        for (int c = 4 * lane; c < a.D; c += 256) *reinterpret_cast<float4*>(out + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    float4 v[PE_MAX_CHUNKS];
#pragma unroll
    for (int i = 0; i < PE_MAX_CHUNKS; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = s; t < e; ++t) {
        const float* er = a.E + ((size_t)b * a.T + t) * a.D;
#pragma unroll
        for (int i = 0; i < PE_MAX_CHUNKS; ++i) {
            const int c = 4 * (lane + 64 * i);
            if (c < a.D) {
                const float4 x = *reinterpret_cast<const float4*>(er + c);
                v[i].x += x.x; v[i].y += x.y; v[i].z += x.z; v[i].w += x.w;
            }
        }
    }
    const float cnt = (float)(e - s);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < PE_MAX_CHUNKS; ++i) {
        const int c = 4 * (lane + 64 * i);
        if (c < a.D) {
            const float4 bb = *reinterpret_cast<const float4*>(a.bias + c);
            v[i].x = v[i].x / cnt + bb.x; v[i].y = v[i].y / cnt + bb.y; v[i].z = v[i].z / cnt + bb.z; v[i].w = v[i].w / cnt + bb.w;
            sum += ln_sum4(v[i]);
        }
    }
    const float mean = ln_mean(wave_sum(sum), a.D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < PE_MAX_CHUNKS; ++i)
        if (4 * (lane + 64 * i) < a.D) sq += ln_sqdev4(v[i], mean);
    const float rstd = ln_rstd(wave_sum(sq), a.D, a.eps);
    const float* per = a.pe + (size_t)j * a.D;
#pragma unroll
    for (int i = 0; i < PE_MAX_CHUNKS; ++i) {
        const int c = 4 * (lane + 64 * i);
        if (c < a.D) {
            const float4 y = ln_apply4(v[i], mean, rstd, *reinterpret_cast<const float4*>(a.gamma + c),
                                       *reinterpret_cast<const float4*>(a.beta + c));
            const float4 p = *reinterpret_cast<const float4*>(per + c);
            float4 o;
            o.x = fmaxf(y.x, 0.f) * a.xscale + p.x; o.y = fmaxf(y.y, 0.f) * a.xscale + p.y;
            o.z = fmaxf(y.z, 0.f) * a.xscale + p.z; o.w = fmaxf(y.w, 0.f) * a.xscale + p.w;
            *reinterpret_cast<float4*>(out + c) = o;
        }
    }
}

}  // namespace

int launch_softmax_argmax_rows(float* x, int ld, int M, int V, int Vp, int* ids, hipStream_t stream) {
    PF_REQUIRE(x && ids && M > 0 && V > 0 && Vp >= V && ld >= Vp, "softmax_argmax_rows: null/empty, or ld < Vp");
    hipLaunchKernelGGL(softmax_argmax_rows_kernel, dim3((unsigned)M), dim3(256), 0, stream, x, ld, M, V, Vp, ids);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ctc_runs(const int* ids, const int* lens, int B, int T, int blank, int* counts, int* ranges, int ld, hipStream_t stream) {
    PF_REQUIRE(ids && lens && counts && ranges && B > 0 && T > 0 && ld > 0, "ctc_runs: null/empty");
    hipLaunchKernelGGL(ctc_runs_kernel, dim3((unsigned)B), dim3(256), 0, stream, ids, lens, T, blank, counts, ranges, ld);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_posterior_embed(const PosteriorEmbedArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.E && a.counts && a.ranges && a.bias && a.gamma && a.beta && a.pe && a.embeds && a.B > 0 && a.T > 0 && a.N > 0 && a.ld > 0,
               "posterior_embed: null/empty");
    PF_REQUIRE(a.D > 0 && a.D % 4 == 0 && a.D <= 256 * PE_MAX_CHUNKS, "posterior_embed: D % 4 == 0 and D <= 2048");
    PF_REQUIRE((((uintptr_t)a.E | (uintptr_t)a.bias | (uintptr_t)a.gamma | (uintptr_t)a.beta | (uintptr_t)a.pe | (uintptr_t)a.embeds) & 15) == 0 &&
               (!a.ranges_out || ((uintptr_t)a.ranges_out & 7) == 0), "posterior_embed: operands must be 16-B aligned");
    const long tokens = (long)a.B * a.N;
    hipLaunchKernelGGL(posterior_embed_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
