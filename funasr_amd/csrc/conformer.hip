// Row kernels of the Conformer encoder and of the Transformer decoder step (see conformer.h): the first conv of Conv2dSubsampling,
// ReLU / Swish rows, the GLU + depthwise conv + BatchNorm + Swish row kernel of the convolution module, and the decoder step's
// embedding, few-query attention and cache reorder; the SAN-M decoder step's fused norm2 / FSMN window / norm3 kernel and
// few-query cross-attention for heads of 64 or 128 dims.
#include <algorithm>

#include "conformer.h"

namespace pf {
namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// one workgroup = one conv0 output time row t1 of one sequence; even t1 -> `even` row t1 / 2, odd -> `odd` row t1 / 2
__global__ void __launch_bounds__(256) cf_conv0_kernel(const float* feats, int Tin, int F, const float* w, const float* bias, int C,
                                                       int T1, int F1, int NE, int FP, float* even, float* odd) {
    const int t1 = blockIdx.x, b = blockIdx.y;
    __shared__ float xs[3][256];
    float* dst = ((t1 & 1) ? odd : even) + ((size_t)b * NE + (t1 >> 1)) * FP * C;
    const int n = FP * C;
    if (t1 >= T1) {                                   // rows the second conv's waste outputs read: zeros
        for (int i = threadIdx.x; i < n; i += 256) dst[i] = 0.f;
        return;
    }
    for (int i = threadIdx.x; i < 3 * F; i += 256) {
        const int dt = i / F, f = i - dt * F;
        xs[dt][f] = feats[((size_t)b * Tin + 2 * t1 + dt) * F + f];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int f1 = i / C, c = i - f1 * C;
        float acc = 0.f;
        if (f1 < F1) {
            acc = bias[c];
            const float* wc = w + c * 9;
#pragma unroll
            for (int dt = 0; dt < 3; ++dt)
#pragma unroll
                for (int df = 0; df < 3; ++df) acc = fmaf(wc[dt * 3 + df], xs[dt][2 * f1 + df], acc);
            acc = fmaxf(acc, 0.f);
        }
        dst[i] = acc;
    }
}

__global__ void __launch_bounds__(256) cf_act_kernel(float* x, size_t n4, int mode) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<float4*>(x)[i];
    if (mode == 0) {
        v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    } else {
        v = make_float4(v.x * sigmoidf_(v.x), v.y * sigmoidf_(v.y), v.z * sigmoidf_(v.z), v.w * sigmoidf_(v.w));
    }
    reinterpret_cast<float4*>(x)[i] = v;
}

__global__ void __launch_bounds__(256) cf_scale_rows_kernel(const float* x, int NE, float* y, int T, int D4, float scale, const float* pe,
                                                           size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / D4;
    const int c = (int)(i - row * D4);
    const int b = (int)(row / T), t = (int)(row - (size_t)b * T);
    const float4 v = reinterpret_cast<const float4*>(x)[((size_t)b * NE + t) * D4 + c];
    float4 r = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
    if (pe) {      // PositionalEncoding.forward: the product is rounded, then the table row is added (no fma)
        const float4 p = reinterpret_cast<const float4*>(pe)[(size_t)t * D4 + c];
        r = make_float4(__fadd_rn(__fmul_rn(v.x, scale), p.x), __fadd_rn(__fmul_rn(v.y, scale), p.y), __fadd_rn(__fmul_rn(v.z, scale), p.z),
                        __fadd_rn(__fmul_rn(v.w, scale), p.w));
    }
    reinterpret_cast<float4*>(y)[i] = r;
}

constexpr int DW_TT = 32;      // output rows per workgroup
__global__ void __launch_bounds__(64) cf_glu_dw_kernel(const float* g, const float* dw, const float* dw_bias, const float* bn_scale,
                                                       const float* bn_shift, int T, int D, int taps, float* y) {
    const int t0 = blockIdx.x * DW_TT, c = blockIdx.y * 64 + threadIdx.x, b = blockIdx.z, pad = taps / 2;
    __shared__ float xs[(DW_TT + 30) * 64];
    const int nrows = DW_TT + taps - 1;
    for (int r = 0; r < nrows; ++r) {
        const int t = t0 - pad + r;
        float v = 0.f;
        if (t >= 0 && t < T) {
            const float* row = g + ((size_t)b * T + t) * 2 * D;
            v = row[c] * sigmoidf_(row[D + c]);
        }
        xs[r * 64 + threadIdx.x] = v;
    }
    float wk[31];
#pragma unroll
    for (int k = 0; k < 31; ++k) wk[k] = k < taps ? dw[(size_t)c * taps + k] : 0.f;
    const float bb = dw_bias[c], sc = bn_scale[c], sh = bn_shift[c];
    for (int r = 0; r < DW_TT; ++r) {
        const int t = t0 + r;
        if (t >= T) break;
        float acc = bb;
#pragma unroll
        for (int k = 0; k < 31; ++k)
            if (k < taps) acc = fmaf(wk[k], xs[(r + k) * 64 + threadIdx.x], acc);
        const float z = acc * sc + sh;
        y[((size_t)b * T + t) * D + c] = z * sigmoidf_(z);
    }
}

__global__ void __launch_bounds__(256) td_embed_kernel(const float* table, const int* ids, const float* pe_row, float scale, float* x,
                                                       int D) {
    const int r = blockIdx.x;
    const float* e = table + (size_t)ids[r] * D;
    if (!pe_row) {                                   // the SAN-M decoder's bare embedding (scale 1)
        for (int d = threadIdx.x; d < D; d += 256) x[(size_t)r * D + d] = e[d] * scale;
        return;
    }
    for (int d = threadIdx.x; d < D; d += 256) x[(size_t)r * D + d] = e[d] * scale + pe_row[d];
}

// one wave per (query, head): lane = one of the 64 dims for the output, keys strided over the lanes for the scores
__global__ void __launch_bounds__(64) td_attention_kernel(const float* q, const float* K, const float* V, int ldkv, size_t seq_stride,
                                                          int nk, int D, float* out) {
    const int r = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    extern __shared__ float sc[];                    // nk scores
    __shared__ float qs[64];
    qs[lane] = q[(size_t)r * D + h * 64 + lane];
    __syncthreads();
    const float* Kb = K + (size_t)r * seq_stride + h * 64;
    const float* Vb = V + (size_t)r * seq_stride + h * 64;
    float mx = -INFINITY;
    for (int j = lane; j < nk; j += 64) {
        const float* kp = Kb + (size_t)j * ldkv;
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < 64; d += 4) {
            const float4 kv = *reinterpret_cast<const float4*>(kp + d);
            a = fmaf(qs[d], kv.x, a); a = fmaf(qs[d + 1], kv.y, a); a = fmaf(qs[d + 2], kv.z, a); a = fmaf(qs[d + 3], kv.w, a);
        }
        a *= 0.125f;
        sc[j] = a;
        mx = fmaxf(mx, a);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < nk; j += 64) {
        const float p = expf(sc[j] - mx);
        sc[j] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();
    float acc = 0.f;
    for (int j = 0; j < nk; ++j) acc = fmaf(sc[j], Vb[(size_t)j * ldkv + lane], acc);
    out[(size_t)r * D + h * 64 + lane] = acc / sum;
}

__global__ void __launch_bounds__(256) td_reorder_kernel(const float* src, float* dst, const int* parents, size_t layer_floats,
                                                         size_t slot_floats, size_t n4) {
    const int k = blockIdx.y, l = blockIdx.z;
    const float4* s = reinterpret_cast<const float4*>(src + (size_t)l * layer_floats + (size_t)parents[k] * slot_floats);
    float4* d = reinterpret_cast<float4*>(dst + (size_t)l * layer_floats + (size_t)k * slot_floats);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) d[i] = s[i];
}

// ---- SAN-M (FsmnDecoder) step
// the sum over the 256 threads of a workgroup in a fixed order (wave 0 + 1 + 2 + 3), the same value in every thread
__device__ __forceinline__ float fd_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                 // the previous reduction's readers are done with `red`
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

constexpr int FD_NV = 8;                             // elements per thread: D <= 256 * 8

// one workgroup = one running slot; thread t holds elements t, t + 256, ... of the row in registers through both LayerNorms
__global__ void __launch_bounds__(256) fd_fsmn_step_kernel(const float* t, const float* x, const float* g2, const float* b2, const float* w,
                                                           const float* win_in, float* win_out, const int* parents, int pos, int D, int K,
                                                           int left_pad, const float* g3, const float* b3, float eps, float* x_out,
                                                           float* xn_out) {
    __shared__ float red[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)r * D;
    float v[FD_NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < FD_NV; ++i) {
        const int d = tid + 256 * i;
        v[i] = d < D ? t[row + d] : 0.f;
        s += v[i];
    }
    float mean = fd_block_sum(s, red) / (float)D;
    s = 0.f;
#pragma unroll
    for (int i = 0; i < FD_NV; ++i)
        if (tid + 256 * i < D) { const float c = v[i] - mean; s = fmaf(c, c, s); }
    float rstd = 1.f / sqrtf(fd_block_sum(s, red) / (float)D + eps);
    const float* src = pos > 0 ? win_in + (size_t)(parents ? parents[r] : r) * K * D : nullptr;
    float* dst = win_out + (size_t)r * K * D;
    s = 0.f;
#pragma unroll
    for (int i = 0; i < FD_NV; ++i) {
        const int d = tid + 256 * i;
        if (d >= D) continue;
        const float u = (v[i] - mean) * rstd * g2[d] + b2[d];
        const float* wd = w + (size_t)d * K;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) {
            float c;
            if (pos > 0) c = k == K - 1 ? u : src[(size_t)(k + 1) * D + d];
            else c = k == left_pad ? u : 0.f;
            dst[(size_t)k * D + d] = c;
            acc = fmaf(wd[k], c, acc);
        }
        const float y = x[row + d] + (acc + u);
        x_out[row + d] = y;
        v[i] = y;
        s += y;
    }
    if (!g3) return;
    mean = fd_block_sum(s, red) / (float)D;
    s = 0.f;
#pragma unroll
    for (int i = 0; i < FD_NV; ++i)
        if (tid + 256 * i < D) { const float c = v[i] - mean; s = fmaf(c, c, s); }
    rstd = 1.f / sqrtf(fd_block_sum(s, red) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < FD_NV; ++i) {
        const int d = tid + 256 * i;
        if (d < D) xn_out[row + d] = (v[i] - mean) * rstd * g3[d] + b3[d];
    }
}

// td_attention_kernel's mapping for a head of DK = 64 or 128 dims over ONE memory: one wave per (query, head), keys strided over the
// lanes for the scores, lane = DK / 64 of the output dims
template <int DK>
__global__ void __launch_bounds__(64) fd_attention_kernel(const float* q, const float* K, const float* V, int ldkv, int nk, int D,
                                                          float* out) {
    const int r = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    extern __shared__ float sc[];                    // nk scores
    __shared__ float qs[DK];
#pragma unroll
    for (int c = 0; c < DK / 64; ++c) qs[lane + 64 * c] = q[(size_t)r * D + h * DK + lane + 64 * c];
    __syncthreads();
    const float* Kb = K + h * DK;
    const float* Vb = V + h * DK;
    const float scale = DK == 64 ? 0.125f : 0.08838834764831845f;      // 1 / sqrt(DK)
    float mx = -INFINITY;
    for (int j = lane; j < nk; j += 64) {
        const float* kp = Kb + (size_t)j * ldkv;
        float a = 0.f;
#pragma unroll 8
        for (int d = 0; d < DK; d += 4) {
            const float4 kv = *reinterpret_cast<const float4*>(kp + d);
            a = fmaf(qs[d], kv.x, a); a = fmaf(qs[d + 1], kv.y, a); a = fmaf(qs[d + 2], kv.z, a); a = fmaf(qs[d + 3], kv.w, a);
        }
        a *= scale;
        sc[j] = a;
        mx = fmaxf(mx, a);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < nk; j += 64) {
        const float p = expf(sc[j] - mx);
        sc[j] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    __syncthreads();
    float acc[DK / 64];
#pragma unroll
    for (int c = 0; c < DK / 64; ++c) acc[c] = 0.f;
    for (int j = 0; j < nk; ++j) {
        const float p = sc[j];
#pragma unroll
        for (int c = 0; c < DK / 64; ++c) acc[c] = fmaf(p, Vb[(size_t)j * ldkv + lane + 64 * c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < DK / 64; ++c) out[(size_t)r * D + h * DK + lane + 64 * c] = acc[c] / sum;
}

}  // namespace

int launch_cf_conv0(const float* feats, int B, int Tin, int F, const float* w, const float* bias, int C, int T1, int F1, int NE,
                    int FP, float* even, float* odd, hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && Tin >= 3 && F >= 3 && F <= 256 && C > 0 && T1 == (Tin - 3) / 2 + 1 && F1 == (F - 3) / 2 + 1 &&
                   F1 <= FP && NE > 0 && 2 * NE >= T1, "cf_conv0: bad shape (<= 256 input features)");
    hipLaunchKernelGGL(cf_conv0_kernel, dim3(2 * NE, B), dim3(256), 0, stream, feats, Tin, F, w, bias, C, T1, F1, NE, FP, even, odd);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cf_act(float* x, size_t n, int mode, hipStream_t stream) {
    PF_REQUIRE(n > 0 && n % 4 == 0 && ((uintptr_t)x & 15) == 0 && (mode == 0 || mode == 1), "cf_act: n % 4, aligned, mode 0 / 1");
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(cf_act_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, x, n4, mode);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cf_scale_rows(const float* x, int NE, float* y, int B, int T, int D, float scale, const float* pe, hipStream_t stream) {
    PF_REQUIRE(B > 0 && T > 0 && NE >= T && D > 0 && D % 4 == 0 && x && y && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 &&
                   ((uintptr_t)pe & 15) == 0,
               "cf_scale_rows: bad shape");
    const size_t total = (size_t)B * T * (D / 4);
    hipLaunchKernelGGL(cf_scale_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, NE, y, T, D / 4, scale, pe, total);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cf_glu_dw(const float* g, const float* dw, const float* dw_bias, const float* bn_scale, const float* bn_shift, int B,
                     int T, int D, int taps, float* y, hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && D > 0 && D % 64 == 0 && taps % 2 == 1 && taps >= 1 && taps <= 31,
               "cf_glu_dw: D % 64, odd taps <= 31");
    hipLaunchKernelGGL(cf_glu_dw_kernel, dim3(ceil_div(T, DW_TT), D / 64, B), dim3(64), 0, stream, g, dw, dw_bias, bn_scale, bn_shift, T,
                       D, taps, y);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_td_embed(const float* table, const int* ids, const float* pe_row, float scale, float* x, int n, int D, hipStream_t stream) {
    PF_REQUIRE(n > 0 && D > 0 && table && ids && x, "td_embed: bad arguments");
    hipLaunchKernelGGL(td_embed_kernel, dim3(n), dim3(256), 0, stream, table, ids, pe_row, scale, x, D);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_td_attention(const float* q, const float* K, const float* V, int ldkv, size_t seq_stride, int nk, int n, int H, float* out,
                        hipStream_t stream) {
    PF_REQUIRE(n > 0 && H > 0 && nk > 0 && nk <= 12000 && ldkv % 4 == 0 && seq_stride % 4 == 0 && ((uintptr_t)K & 15) == 0,
               "td_attention: 1 .. 12000 keys, 16-B aligned rows");
    hipLaunchKernelGGL(td_attention_kernel, dim3(n, H), dim3(64), sizeof(float) * nk, stream, q, K, V, ldkv, seq_stride, nk, H * 64, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_td_reorder(const float* src, float* dst, const int* parents, int n, int L, size_t layer_floats, size_t slot_floats,
                      int len, int row_floats, hipStream_t stream) {
    PF_REQUIRE(n > 0 && L > 0 && len > 0 && row_floats % 4 == 0 && layer_floats % 4 == 0 && slot_floats % 4 == 0 && src != dst,
               "td_reorder: bad shape");
    const size_t n4 = (size_t)len * row_floats / 4;
    const unsigned gx = (unsigned)std::min<size_t>((n4 + 255) / 256, 64);
    hipLaunchKernelGGL(td_reorder_kernel, dim3(gx, n, L), dim3(256), 0, stream, src, dst, parents, layer_floats, slot_floats, n4);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_fd_fsmn_step(const float* t, const float* x, const float* g2, const float* b2, const float* w, const float* win_in,
                        float* win_out, const int* parents, int pos, int n, int D, int K, int left_pad, const float* g3,
                        const float* b3, float eps, float* x_out, float* xn_out, hipStream_t stream) {
    PF_REQUIRE(t && x && g2 && b2 && w && win_in && win_out && x_out && win_in != win_out, "fd_fsmn_step: null argument, or one window buffer");
    PF_REQUIRE(n > 0 && n <= 65535 && D > 0 && D % 4 == 0 && D <= 256 * FD_NV && K >= 1 && K <= 32 && left_pad >= 0 && left_pad < K && pos >= 0,
               "fd_fsmn_step: D % 4 and <= 2048, 1 <= K <= 32, 0 <= left_pad < K");
    PF_REQUIRE((g3 == nullptr) == (b3 == nullptr) && (g3 == nullptr || xn_out != nullptr), "fd_fsmn_step: norm3 needs weight, bias and an output");
    hipLaunchKernelGGL(fd_fsmn_step_kernel, dim3(n), dim3(256), 0, stream, t, x, g2, b2, w, win_in, win_out, parents, pos, D, K, left_pad, g3,
                       b3, eps, x_out, xn_out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_fd_attention(const float* q, const float* K, const float* V, int ldkv, int nk, int n, int H, int dk, float* out,
                        hipStream_t stream) {
    PF_REQUIRE(q && K && V && out && n > 0 && n <= 65535 && H > 0 && H <= 65535 && nk > 0 && nk <= 12000 && (dk == 64 || dk == 128) &&
                   ldkv % 4 == 0 && ldkv >= H * dk && ((uintptr_t)K & 15) == 0,
               "fd_attention: head dim 64 or 128, 1 .. 12000 keys, 16-B aligned rows");
    if (dk == 64)
        hipLaunchKernelGGL(fd_attention_kernel<64>, dim3(n, H), dim3(64), sizeof(float) * nk, stream, q, K, V, ldkv, nk, H * dk, out);
    else
        hipLaunchKernelGGL(fd_attention_kernel<128>, dim3(n, H), dim3(64), sizeof(float) * nk, stream, q, K, V, ldkv, nk, H * dk, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
