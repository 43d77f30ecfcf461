// ALiBi self-attention of packed variable-length sequences (emotion2vec's AltAttention with its alibi bias; see emotion2vec.h).
// One workgroup = 64 queries of one (sequence, head); four lanes per query, each holding 16 of the 64 dims of q and of the output.
// K / V tiles of 64 keys are staged in LDS; a tile's 64 scores are formed first (the 4-lane partial dots summed by two xor
// shuffles, equal on all four lanes), then one online-softmax rescale per tile. The bias is computed from (i, j, head) in the
// kernel and never materialised. fp32 throughout; the key order is fixed, so a query's result depends on its own sequence only.
#include "emotion2vec.h"

namespace pf {
namespace {

constexpr int QT = 64, KT = 64, HD = 64;

// the reference's float32 bias: (slope * -|i - j|) rounded, times the clamped per-head scale, rounded
__device__ __forceinline__ float alibi_bias(float slope, float scale, int i, int j) {
#pragma clang fp contract(off)
    const float d = (float)(-(i > j ? i - j : j - i));
    return (slope * d) * scale;
}

__global__ void __launch_bounds__(256) alibi_attention_kernel(const float* qkv, const int* toff, int H, int n_alibi, int E,
                                                              const float* slope, const float* scale, float* out) {
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * QT;
    const int base = toff[b], n = toff[b + 1] - base;
    if (q0 >= n) return;
    const int D = H * HD, ld = 3 * D;
    __shared__ float Ks[KT][HD + 4];
    __shared__ float Vs[KT][HD + 4];
    const int tid = threadIdx.x, qi = tid >> 2, part = tid & 3;
    const int i = q0 + qi;
    const bool qvalid = i < n;
    float q[16], o[16];
    const float* qp = qkv + (size_t)(base + (qvalid ? i : 0)) * ld + h * HD + part * 16;
#pragma unroll
    for (int k = 0; k < 16; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(qp + k);
        q[k] = v.x * 0.125f; q[k + 1] = v.y * 0.125f; q[k + 2] = v.z * 0.125f; q[k + 3] = v.w * 0.125f;   // q * 64^-1/2 (exact)
        o[k] = o[k + 1] = o[k + 2] = o[k + 3] = 0.f;
    }
    const bool alibi = h < n_alibi;
    const float sl = alibi ? slope[h] : 0.f, sc = alibi ? scale[h] : 0.f;
    float m = -INFINITY, l = 0.f;
    for (int j0 = 0; j0 < n; j0 += KT) {
        __syncthreads();
        for (int e = tid; e < KT * 16; e += 256) {
            const int rr = e >> 4, c4 = (e & 15) * 4, j = j0 + rr;
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (j < n) {
                const float* p = qkv + (size_t)(base + j) * ld + D + h * HD + c4;
                kv = *reinterpret_cast<const float4*>(p);
                vv = *reinterpret_cast<const float4*>(p + D);
            }
            *reinterpret_cast<float4*>(&Ks[rr][c4]) = kv;
            *reinterpret_cast<float4*>(&Vs[rr][c4]) = vv;
        }
        __syncthreads();
        float s[KT];
        float tmax = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < KT; ++jj) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 16; k += 4) {
                const float4 kv = *reinterpret_cast<const float4*>(&Ks[jj][part * 16 + k]);
                a = fmaf(q[k], kv.x, a); a = fmaf(q[k + 1], kv.y, a); a = fmaf(q[k + 2], kv.z, a); a = fmaf(q[k + 3], kv.w, a);
            }
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            const int j = j0 + jj;
            if (alibi && i >= E && j >= E) a += alibi_bias(sl, sc, i, j);
            s[jj] = j < n ? a : -INFINITY;
            tmax = fmaxf(tmax, s[jj]);
        }
        const float mn = fmaxf(m, tmax);
        const float corr = expf(m - mn);
        l *= corr;
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] *= corr;
#pragma unroll
        for (int jj = 0; jj < KT; ++jj) {
            const float p = expf(s[jj] - mn);
            l += p;
#pragma unroll
            for (int k = 0; k < 16; k += 4) {
                const float4 vv = *reinterpret_cast<const float4*>(&Vs[jj][part * 16 + k]);
                o[k] = fmaf(p, vv.x, o[k]); o[k + 1] = fmaf(p, vv.y, o[k + 1]); o[k + 2] = fmaf(p, vv.z, o[k + 2]); o[k + 3] = fmaf(p, vv.w, o[k + 3]);
            }
        }
        m = mn;
    }
    if (!qvalid) return;
    const float inv = 1.f / l;
    float* op = out + (size_t)(base + i) * D + h * HD + part * 16;
#pragma unroll
    for (int k = 0; k < 16; k += 4) *reinterpret_cast<float4*>(op + k) = make_float4(o[k] * inv, o[k + 1] * inv, o[k + 2] * inv, o[k + 3] * inv);
}

}  // namespace

int launch_e2v_attention(const float* qkv, const int* toff, int B, int max_len, int H, int n_alibi, int n_extra,
                         const float* slope, const float* scale, float* out, hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && max_len > 0 && H > 0 && H <= 65535, "e2v_attention: bad shape");
    PF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0, "e2v_attention: 16-B alignment");
    hipLaunchKernelGGL(alibi_attention_kernel, dim3(ceil_div(max_len, QT), H, B), dim3(256), 0, stream, qkv, toff, H, n_alibi, n_extra,
                       slope, scale, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
