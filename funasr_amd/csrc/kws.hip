// Row-wise kernels of the keyword spotters (FsmnKWS / SanmKWS): the FSMN memory block with a right context, and the per-frame
// candidate step of the CTC keyword search. Both are HBM-bound streaming kernels; the dense layers go through the GEMM kernels.
//
// Reference semantics:
//   FSMNBlock.forward          fsmn_vad_streaming/encoder.py:131-161
//       out[t] = x[t] + sum_{j < L} wl[c][j] x[t - (L-1-j) LS] + sum_{j < R} wr[c][j] x[t + (j+1) RS]; rows outside 0 .. T-1 are zero
//       (conv_left over the left-padded input, conv_right over the input shifted by RS and right-padded). T is the padded length of
//       the batch: the reference passes no lengths, so the last frames of a shorter clip read the frames behind it.
//   KwsCtcPrefixDecoder.beam_search   utils/kws_utils.py:156-171
//       softmax of the row, its three largest in descending order, each kept if p > 0.05 and the id is a keyword token (or blank)
#include "common.h"

#include <climits>

namespace pf {

namespace {

constexpr int KWS_TT = 8;            // frames per workgroup

// block = (C / 4) x KWS_TT threads: thread (c4, tt) computes 4 channels of frame t0 + tt. One accumulator per channel, the left
// taps in ascending j and then the right taps in ascending j: a fixed order, and with R = 0 the order of vad_fsmn_kernel.
__global__ __launch_bounds__(256) void kws_fsmn_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ wl,
                                                       const float* __restrict__ wr, float* __restrict__ y, int ldy, int T, int C,
                                                       int L, int LS, int R, int RS) {
    const int c4 = threadIdx.x, tt = threadIdx.y;
    const int b = blockIdx.y, t = blockIdx.x * KWS_TT + tt;
    if (t >= T || c4 * 4 >= C) return;
    const float* xb = x + (size_t)b * T * ldx;
    float4 acc = *reinterpret_cast<const float4*>(xb + (size_t)t * ldx + c4 * 4);
    const float* lp = wl + (size_t)c4 * 4 * L;
#pragma unroll 4
    for (int k = 0; k < L; ++k) {
        const int ti = t - (L - 1 - k) * LS;
        if (ti < 0) continue;
        const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)ti * ldx + c4 * 4);
        acc.x = fmaf(lp[k], v.x, acc.x);
        acc.y = fmaf(lp[L + k], v.y, acc.y);
        acc.z = fmaf(lp[2 * L + k], v.z, acc.z);
        acc.w = fmaf(lp[3 * L + k], v.w, acc.w);
    }
    const float* rp = wr + (size_t)c4 * 4 * R;          // never read when R == 0
    for (int j = 0; j < R; ++j) {
        const long ti = (long)t + (long)(j + 1) * RS;
        if (ti >= T) break;
        const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)ti * ldx + c4 * 4);
        acc.x = fmaf(rp[j], v.x, acc.x);
        acc.y = fmaf(rp[R + j], v.y, acc.y);
        acc.z = fmaf(rp[2 * R + j], v.z, acc.z);
        acc.w = fmaf(rp[3 * R + j], v.w, acc.w);
    }
    *reinterpret_cast<float4*>(y + ((size_t)b * T + t) * ldy + c4 * 4) = acc;
}

struct Top3 { float v[3]; int i[3]; };

// a ranks before b: the larger value, equal values the lower index (an empty slot is -inf at INT_MAX and ranks last)
__device__ __forceinline__ bool ranks_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

__device__ __forceinline__ void top3_insert(Top3& t, float v, int i) {
    if (!ranks_before(v, i, t.v[2], t.i[2])) return;
    if (ranks_before(v, i, t.v[0], t.i[0])) {
        t.v[2] = t.v[1]; t.i[2] = t.i[1]; t.v[1] = t.v[0]; t.i[1] = t.i[0]; t.v[0] = v; t.i[0] = i;
    } else if (ranks_before(v, i, t.v[1], t.i[1])) {
        t.v[2] = t.v[1]; t.i[2] = t.i[1]; t.v[1] = v; t.i[1] = i;
    } else {
        t.v[2] = v; t.i[2] = i;
    }
}

// One wave per row, four rows per workgroup. Lane-local top 3 over columns lane, lane + 64, ..., a butterfly merge that leaves
// the row's top 3 in every lane, then sum exp(x - max) per lane in column order and over the wave by the same butterfly: the
// same row gives the same bits. The sum is accumulated in double (the terms are fp32 expf), the three quotients are taken in
// double and rounded once to fp32. out [M, 7] words: n, ids[3] (-1 from n on), the fp32 bits of probs[3] (0 from n on): every slot
// of every row < M is written.
__global__ __launch_bounds__(256) void kws_candidates_kernel(const float* __restrict__ x, long ldx, int M, int V,
                                                             const unsigned* __restrict__ mask, int* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;                                  // whole waves leave: no shuffle below crosses a row
    const float* xr = x + (size_t)row * ldx;
    Top3 t;
#pragma unroll
    for (int k = 0; k < 3; ++k) { t.v[k] = -INFINITY; t.i[k] = INT_MAX; }
    for (int c = lane; c < V; c += 64) top3_insert(t, xr[c], c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top3 p;
#pragma unroll
        for (int k = 0; k < 3; ++k) { p.v[k] = __shfl_xor(t.v[k], o, 64); p.i[k] = __shfl_xor(t.i[k], o, 64); }
#pragma unroll
        for (int k = 0; k < 3; ++k) top3_insert(t, p.v[k], p.i[k]);
    }
    const float mx = t.v[0];
    double s = 0.0;
    for (int c = lane; c < V; c += 64) s += (double)expf(xr[c] - mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        int n = 0, ids[3] = {-1, -1, -1};
        float ps[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; ++k) {
            const int id = t.i[k];
            if (id < 0 || id >= V) continue;
            const float p = (float)(exp((double)(t.v[k] - mx)) / s);
            if (p > 0.05f && ((mask[id >> 5] >> (id & 31)) & 1u)) { ids[n] = id; ps[n] = p; ++n; }
        }
        int* o = out + (size_t)row * 7;
        o[0] = n;
        for (int k = 0; k < 3; ++k) { o[1 + k] = ids[k]; o[4 + k] = __float_as_int(ps[k]); }
    }
}

}  // namespace

int launch_kws_fsmn(const float* x, int ldx, const float* wl, const float* wr, float* y, int ldy, int B, int T, int C, int L, int LS,
                    int R, int RS, hipStream_t stream) {
    PF_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0 && C <= 128 && L >= 1 && LS >= 1 && R >= 0 && RS >= 1,
               "kws_fsmn: C % 4 == 0, C <= 128, lorder >= 1, rorder >= 0, strides >= 1");
    PF_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C, "kws_fsmn: strides % 4, >= C");
    PF_REQUIRE(x && wl && y && (R == 0 || wr) && x != y, "kws_fsmn: null argument, or in place");
    PF_REQUIRE(B <= 65535, "kws_fsmn: at most 65535 clips per launch");
    hipLaunchKernelGGL(kws_fsmn_kernel, dim3(ceil_div(T, KWS_TT), B), dim3(C / 4, KWS_TT), 0, stream, x, ldx, wl, R ? wr : wl, y, ldy,
                       T, C, L, LS, R, RS);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_kws_candidates(const float* x, long ldx, int M, int V, const unsigned* mask, int* out, hipStream_t stream) {
    PF_REQUIRE(x && mask && out && M > 0, "kws_candidates: null/empty argument");
    PF_REQUIRE(V >= 3, "kws_candidates: V < 3 (the top 3 of a row need three columns; torch.topk(3) raises there)");
    PF_REQUIRE(V <= 65536 && ldx >= V, "kws_candidates: V <= 65536, row stride >= V");
    hipLaunchKernelGGL(kws_candidates_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, stream, x, ldx, M, V, mask, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
