// Parallel integrate-and-fire, the predictor of E-Paraformer (see pif.h): funasr/models/e_paraformer/pif_predictor.py:84-130.
//
//   alphas   one wave per row of the padded batch: the depthwise conv over time (taps straight from the clip's own rows, zeros outside
//            [0, T)), + bias + the row, ReLU, the dot with cif_output over the channels (lane c, c + 64, ...; one xor butterfly), sigmoid,
//            smooth / noise, mask. Then one workgroup per clip sums the row of alphas: thread i takes t = i, i + 256, ... in float64, a
//            butterfly per wave, the four waves in order, rounded once. Neither order depends on the grid.
//   align    one wave per clip: the row scaled by fl(n / token_num) into LDS, lane 0 walks it (the recurrence is serial by
//            definition, as in cif_scan_kernel: a float64 running sum rounded to fp32 per step), coalesced write-back.
//   embed    an attention whose scores are a function of (fire position, align[t]): no K, no QK^T. A workgroup of one wave owns 16
//            fire positions x 64 channels of one sigma head of one clip and walks the clip's frames in chunks of 64: lane t of the
//            chunk computes its frame's 16 scores, the chunk's maxima and sums are butterflies, the 64 x 16 weights go through LDS,
//            and in the product every lane (now a channel) reads one h element per frame (coalesced over the channels) against 16
//            broadcast weights: 16 FMAs per 4-B load. The scores of a 64-channel block are recomputed by each of the D / (64 H)
//            blocks of a head: 16 exps per lane and chunk beside 1024 FMAs.
#include "pif.h"

namespace pf {
namespace {

__global__ __launch_bounds__(256) void pif_alpha_kernel(const float* __restrict__ h, const float* __restrict__ cw, const float* __restrict__ cb,
                                                        const float* __restrict__ ow, const float* __restrict__ ob, const int* __restrict__ lens,
                                                        int B, int T, int D, int l_order, int taps, float smooth, float noise,
                                                        float* __restrict__ a) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row % T);
    if (t >= lens[b]) {                      // masked: exactly 0, nothing read
        if (lane == 0) a[row] = 0.f;
        return;
    }
    const float* hb = h + (size_t)b * T * D;
    const int k_lo = l_order - t > 0 ? l_order - t : 0;                       // taps whose frame t + k - l_order lies in [0, T)
    const int k_hi = T - 1 - t + l_order < taps - 1 ? T - 1 - t + l_order : taps - 1;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
        float acc = cb[c];
        for (int k = k_lo; k <= k_hi; ++k) acc = fmaf(cw[(size_t)c * taps + k], hb[(size_t)(t + k - l_order) * D + c], acc);
        acc += hb[(size_t)t * D + c];
        s = fmaf(fmaxf(acc, 0.f), ow[c], s);
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float z = s + ob[0];
        const float sg = 1.0f / (1.0f + expf(-z));
        a[row] = fmaxf(__fsub_rn(__fmul_rn(sg, smooth), noise), 0.f);
    }
}

__global__ __launch_bounds__(256) void pif_sum_kernel(const float* __restrict__ a, int T, float* __restrict__ token_num) {
    __shared__ double part[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* row = a + (size_t)b * T;
    double s = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) s += (double)row[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) token_num[b] = (float)(((part[0] + part[1]) + part[2]) + part[3]);
}

__global__ __launch_bounds__(64) void pif_align_kernel(const float* a, const float* __restrict__ token_num, const int* __restrict__ n, int T,
                                                       float* an, float* __restrict__ align) {
    __shared__ float s_a[PIF_MAX_T], s_c[PIF_MAX_T];
    const int b = blockIdx.x, lane = threadIdx.x;
    const float tn = token_num[b];
    const int nb = n[b];
    const float r = tn > 0.f && nb > 0 ? __fdiv_rn((float)nb, tn) : 0.f;
    const size_t base = (size_t)b * T;
    for (int t = lane; t < T; t += 64) s_a[t] = r > 0.f ? __fmul_rn(a[base + t], r) : 0.f;
    __syncthreads();
    if (lane == 0) {
        double cs = 0.0;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            cs += (double)s_a[t];
            s_c[t] = (float)cs;
        }
    }
    __syncthreads();
    for (int t = lane; t < T; t += 64) {
        an[base + t] = s_a[t];
        align[base + t] = s_c[t];
    }
}

constexpr int PE_LT = 16, PE_TC = 64;      // fire positions per workgroup, frames per chunk

__global__ __launch_bounds__(64) void pif_embed_kernel(const float* __restrict__ align, const float* __restrict__ h,
                                                       const float* __restrict__ sigma, const int* __restrict__ lens, int T, int L, int D, int H,
                                                       float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float pw[PE_TC * PE_LT];
    const int lane = threadIdx.x, b = blockIdx.z;
    const int Dh = D / H, ncb = (Dh + 63) / 64;
    const int g = blockIdx.y / ncb, c = (blockIdx.y % ncb) * 64 + lane;
    const bool active = c < Dh;
    const int l0 = blockIdx.x * PE_LT;
    int len = lens[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    const float sg = sigma[g];
    const float* hb = h + (size_t)b * T * D + (size_t)g * Dh + (active ? c : 0);
    const float* ab = align + (size_t)b * T;

    float acc[PE_LT], m[PE_LT], ssum[PE_LT];
#pragma unroll
    for (int l = 0; l < PE_LT; ++l) { acc[l] = 0.f; m[l] = -INFINITY; ssum[l] = 0.f; }

    for (int t0 = 0; t0 < len; t0 += PE_TC) {
        const int t = t0 + lane;
        const bool valid = t < len;
        const float al = valid ? ab[t] : 0.f;
        float p[PE_LT];
#pragma unroll
        for (int l = 0; l < PE_LT; ++l) {
            const float d = __fmul_rn(__fsub_rn((float)(l0 + l) + 0.5f, al), sg);
            const float sc = valid ? -__fmul_rn(d, d) : -INFINITY;
            const float m_new = fmaxf(m[l], wave_max(sc));             // finite: lane 0's frame t0 < len is valid
            const float scale = expf(m[l] - m_new);                    // 0 at the first chunk (m = -inf)
            p[l] = valid ? expf(sc - m_new) : 0.f;                     // a far frame underflows to 0
            ssum[l] = fmaf(ssum[l], scale, wave_sum(p[l]));
            acc[l] *= scale;
            m[l] = m_new;
        }
        __syncthreads();                                               // the last chunk's weights are read
#pragma unroll
        for (int l = 0; l < PE_LT; l += 4)
            *reinterpret_cast<float4*>(&pw[lane * PE_LT + l]) = make_float4(p[l], p[l + 1], p[l + 2], p[l + 3]);
        __syncthreads();
        const int nt = len - t0 < PE_TC ? len - t0 : PE_TC;
        for (int tt = 0; tt < nt; ++tt) {
            const float hv = active ? hb[(size_t)(t0 + tt) * D] : 0.f;
#pragma unroll
            for (int l = 0; l < PE_LT; l += 4) {
                const float4 w = *reinterpret_cast<const float4*>(&pw[tt * PE_LT + l]);
                acc[l] = fmaf(w.x, hv, acc[l]);
                acc[l + 1] = fmaf(w.y, hv, acc[l + 1]);
                acc[l + 2] = fmaf(w.z, hv, acc[l + 2]);
                acc[l + 3] = fmaf(w.w, hv, acc[l + 3]);
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int l = 0; l < PE_LT; ++l) {
        if (l0 + l >= L) break;
        out[((size_t)b * L + l0 + l) * D + (size_t)g * Dh + c] = len > 0 ? acc[l] / ssum[l] : 0.f;
    }
}

__global__ __launch_bounds__(256) void pif_gather_best_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ ids, int M,
                                                              float* __restrict__ best) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < M) best[r] = x[(size_t)r * ldx + ids[r]];
}

}  // namespace

int launch_pif_alphas(const float* h, const float* conv_w, const float* conv_b, const float* out_w, const float* out_b, const int* lens, int B,
                      int T, int D, int l_order, int r_order, float smooth, float noise, float* a, float* token_num, hipStream_t stream) {
    PF_REQUIRE(h && conv_w && conv_b && out_w && out_b && lens && a && token_num, "pif_alphas: null argument");
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= PIF_MAX_T && D > 0 && D <= PIF_MAX_D && l_order >= 0 && l_order <= PIF_MAX_ORDER &&
                   r_order >= 0 && r_order <= PIF_MAX_ORDER,
               "pif_alphas: 1 .. 5000 frames, D <= 1024, l_order / r_order 0 .. 15");
    const size_t M = (size_t)B * T;
    hipLaunchKernelGGL(pif_alpha_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, h, conv_w, conv_b, out_w, out_b, lens, B, T, D,
                       l_order, l_order + r_order + 1, smooth, noise, a);
    PF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pif_sum_kernel, dim3(B), dim3(256), 0, stream, a, T, token_num);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_pif_align(const float* a, const float* token_num, const int* n, int B, int T, float* an, float* align, hipStream_t stream) {
    PF_REQUIRE(a && token_num && n && an && align, "pif_align: null argument");
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= PIF_MAX_T, "pif_align: 1 .. 5000 frames");
    hipLaunchKernelGGL(pif_align_kernel, dim3(B), dim3(64), 0, stream, a, token_num, n, T, an, align);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_pif_embed(const float* align, const float* h, const float* sigma, const int* lens, int B, int T, int L, int D, int H, float* embeds,
                     hipStream_t stream) {
    PF_REQUIRE(align && h && sigma && lens && embeds, "pif_embed: null argument");
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= PIF_MAX_T && L > 0 && L <= PIF_MAX_L && D > 0 && D <= PIF_MAX_D && H >= 1 &&
                   H <= PIF_MAX_HEADS && D % H == 0 && (D / H) % 32 == 0,
               "pif_embed: 1 .. 5000 frames, 1 .. 2048 fire positions, D <= 1024, 1 .. 8 sigma heads of a multiple of 32 channels");
    const int ncb = (D / H + 63) / 64;
    hipLaunchKernelGGL(pif_embed_kernel, dim3(ceil_div(L, PE_LT), H * ncb, B), dim3(64), 0, stream, align, h, sigma, lens, T, L, D, H, embeds);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_pif_gather_best(const float* x, int ldx, const int* ids, int M, float* best, hipStream_t stream) {
    PF_REQUIRE(x && ids && best && M > 0 && ldx > 0, "pif_gather_best: null/empty argument");
    hipLaunchKernelGGL(pif_gather_best_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, stream, x, ldx, ids, M, best);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
