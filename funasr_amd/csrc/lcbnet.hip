// LCB-Net kernels: the audio-text cross-attention of the fusion layer (SelfSrcAttention.src_attn: the queries are audio frames, the
// keys the tokens of the OCR text) and the token rows of the text encoder (Embedding + PositionalEncoding).
//
// tf_cross_attention_kernel is the sibling of tf_attention_kernel (attention_abs.hip) on the same tile steps (attention_tile.h): a
// wave owns 32 queries, a lane ONE query (column lane & 31), and the keys of a 32-key tile run over its accumulator registers:
//     S^T[key][q] = sum_d K[key][d] q[q][d]                  A = K tile (LDS),       B = registers
//     O^T[d][q]   = sum_key V[key][d] p[q][key]               A = V tile (LDS),       B = the probabilities in the S^T registers
// What differs: the queries come from a buffer of their own (row stride ldq), K | V from a second buffer of L rows per sequence, and a
// workgroup is ONE wave of 32 queries. The work is T frames x L tokens once per utterance (L is a few tiles): 128-query workgroups
// would leave a 10-s clip (T = 248, 4 heads) at 8 workgroups for 256 compute units, 32-query ones make 32, and a K / V tile of 16 KB
// staged per wave instead of per four costs nothing that shows at this size.
// The K / V rows of a partial tile are clamped to the last valid key (their scores are masked), so no row at or past klens[b] is read.
// No atomics, one fixed order per query: a call repeats bit for bit.
#include "attention_tile.h"
#include "lcbnet.h"

namespace pf {
namespace {

constexpr int DK = 64, KT = 32, KLD = DK + 4, QT = 32;

__global__ __launch_bounds__(64) void tf_cross_attention_kernel(const float* q, int ldq, const float* kv, const int* klens, int Tq, int L,
                                                                int H, float* out) {
    __shared__ __attribute__((aligned(16))) float Ks[KT * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[KT * DK];

    const int lane = threadIdx.x;
    const int hh = lane >> 5, idx = lane & 31;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qi = blockIdx.x * QT + idx;
    const int D = H * DK, ld = 2 * D;
    int klen = klens[b];
    klen = klen > L ? L : klen;
    const int col = head * DK + hh * 32;
    if (klen < 1) {      // every key masked: the reference zeroes the probabilities -> 0
        if (qi < Tq) {
            float* op = out + ((size_t)b * Tq + qi) * D + col;
#pragma unroll
            for (int k = 0; k < 32; k += 4) *reinterpret_cast<float4*>(op + k) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }

    // this lane's query (clamped past Tq), d in [32 hh, 32 hh + 32)
    float qr[32];
    tile_load_q(q + ((size_t)b * Tq + (qi < Tq ? qi : Tq - 1)) * ldq + col, 1.0f, qr);

    floatx16 o[2];
    tile_zero(o);
    float m_run = -INFINITY, l_run = 0.f;

    const int lc4 = (lane & 15) * 4, lr = lane >> 4;
    const float* kbase = kv + (size_t)b * L * ld + head * DK + lc4;

    const int ntiles = (klen + KT - 1) / KT;
    for (int kt = 0; kt < ntiles; ++kt) {
        const int k0 = kt * KT;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = lr + 4 * i;
            int kr = k0 + r;
            kr = kr < klen ? kr : klen - 1;
            const float* src = kbase + (size_t)kr * ld;
            *reinterpret_cast<float4*>(&Ks[r * KLD + lc4]) = *reinterpret_cast<const float4*>(src);
            *reinterpret_cast<float4*>(&Vs[r * DK + lc4]) = *reinterpret_cast<const float4*>(src + D);
        }
        __syncthreads();

        const float* kp = &Ks[idx * KLD + hh * 32];
        floatx16 s = tile_kq([&](int i) { return kp + 4 * i; }, qr);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= 0.125f;
        tile_mask(s, k0, hh, klen);
        tile_softmax<2, false>(s, m_run, l_run, o);
        tile_pv(Vs, hh, idx, s, o);
    }

    if (qi < Tq) tile_store(o, l_run, hh, ((size_t)b * Tq + qi) * D + head * DK, out, nullptr, 0);
}

__global__ void __launch_bounds__(256) text_embed_rows_kernel(const float* table, const int* ids, const float* pe, float scale, float* y,
                                                             int L, int D4, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / D4;
    const int c = (int)(i - row * D4);
    const int t = (int)(row % L);
    const float4 v = reinterpret_cast<const float4*>(table)[(size_t)ids[row] * D4 + c];
    const float4 p = reinterpret_cast<const float4*>(pe)[(size_t)t * D4 + c];
    // PositionalEncoding.forward: the product is rounded, then the table row is added (no fma)
    reinterpret_cast<float4*>(y)[i] = make_float4(__fadd_rn(__fmul_rn(v.x, scale), p.x), __fadd_rn(__fmul_rn(v.y, scale), p.y),
                                                  __fadd_rn(__fmul_rn(v.z, scale), p.z), __fadd_rn(__fmul_rn(v.w, scale), p.w));
}

}  // namespace

int launch_tf_cross_attention(const float* q, int ldq, const float* kv, const int* klens, int B, int Tq, int L, int H, float* out,
                              hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && Tq > 0 && L > 0 && H > 0 && H <= 65535 && q && kv && klens && out && ldq >= H * DK,
               "tf_cross_attention: bad shape");
    PF_REQUIRE(((uintptr_t)q & 15) == 0 && ((uintptr_t)kv & 15) == 0 && ((uintptr_t)out & 15) == 0 && ldq % 4 == 0,
               "tf_cross_attention: 16-B alignment");
    hipLaunchKernelGGL(tf_cross_attention_kernel, dim3(ceil_div(Tq, QT), H, B), dim3(64), 0, stream, q, ldq, kv, klens, Tq, L, H, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_text_embed_rows(const float* table, const int* ids, const float* pe, float scale, float* y, int B, int L, int D,
                           hipStream_t stream) {
    PF_REQUIRE(B > 0 && L > 0 && D > 0 && D % 4 == 0 && table && ids && pe && y && ((uintptr_t)table & 15) == 0 && ((uintptr_t)pe & 15) == 0 &&
                   ((uintptr_t)y & 15) == 0,
               "text_embed_rows: bad shape");
    const size_t total = (size_t)B * L * (D / 4);
    hipLaunchKernelGGL(text_embed_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, table, ids, pe, scale, y, L, D / 4,
                       total);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
