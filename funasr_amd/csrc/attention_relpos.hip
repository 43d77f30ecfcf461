// Relative-position self-attention of the Conformer encoder (funasr/models/transformer/attention.py
// LegacyRelPositionMultiHeadedAttention / RelPositionMultiHeadedAttention), d_k = 64, flash-style in exact fp32 on the matrix cores.
// The reference materialises matrix_ac, matrix_bd (and its rel_shift copy) and the probabilities as [B, H, T, T]; here none exists.
//
// Mapping (attention_tile.h): one workgroup = 4 waves = 128 queries of one (sequence, head); a wave owns 32 queries, a lane ONE
// query (column lane & 31), and the keys run over its accumulator registers:
//     S^T[key][q] = sum_d K[key][d] (q + u)[q][d]            A = K tile (LDS),       B = registers
//     O^T[d][q]   = sum_key V[key][d] p[q][key]               A = V tile (LDS),       B = the probabilities in the S^T registers
// The positional term bd(i, j) = qv_i . P[c - i + j] depends on j - i: for the wave's 32 queries and a tile's 32 keys the 63 rows
// P[rb .. rb + 62], rb = c - (qs + 31) + k0, are multiplied with the 32 qv vectors on the matrix cores as well,
//     G[l][q] = sum_d P[rb + l][d] qv[q][d]                    A = rows of P (global, L2), B = registers
// and element (key kr, query q) of the tile reads G[kr - q + 31][q]: a skew inside ONE column, done through a per-wave LDS
// buffer (written [q][l] with row stride 66, read conflict-free). The legacy variant takes, right of the diagonal, the NEXT query's
// qv against P[j - i - 2] (the wrapped rows of the reference's reshape): a second G with B = qv_{q + 1} and c = -2; which of the
// two a row l of the buffer holds depends on l alone (j - i = l - 31 + k0 - qs), so one buffer serves both.
#include "attention_tile.h"
#include "conformer.h"

namespace pf {
namespace {

constexpr int DK = 64, KT = 32, KLD = DK + 4, GS = 66;

__device__ __forceinline__ floatx16 band_product(const float* P, int ldp, int row, int nP, int col, const float (&qv)[32]) {
    const int rc = row < 0 ? 0 : (row >= nP ? nP - 1 : row);      // rows outside the table feed elements nothing reads
    const float* pp = P + (size_t)rc * ldp + col;
    return tile_kq([&](int i) { return pp + 4 * i; }, qv);
}

__global__ __launch_bounds__(256) void relpos_attention_kernel(const float* qkv, const float* P, const float* ub, const float* vb,
                                                               const int* klens, int T, int H, int legacy, float* out) {
    __shared__ __attribute__((aligned(16))) float Ks[KT * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[KT * DK];
    __shared__ float Gs[4][32 * GS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, idx = lane & 31;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qs = blockIdx.x * 128 + wave * 32;
    const int qi = qs + idx;
    const int D = H * DK, ld = 3 * D;
    const int nP = legacy ? T : 2 * T - 1;
    int klen = klens[b];
    klen = klen > T ? T : klen;
    const int col = head * DK + hh * 32;
    if (klen < 1) {      // every key masked (a clip the mask rule leaves no frame): the reference zeroes the probabilities -> 0
        if (qi < T) {
            float* op = out + ((size_t)b * T + qi) * D + col;
#pragma unroll
            for (int k = 0; k < 32; k += 4) *reinterpret_cast<float4*>(op + k) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }

    // this lane's query (clamped past T), d in [32 hh, 32 hh + 32): q + u, q + v, and for legacy the next query's q + v
    float qu[32], qv[32], qn[32];
    {
        const int ic = qi < T ? qi : T - 1, in1 = qi + 1 < T ? qi + 1 : T - 1;
        const float* qp = qkv + ((size_t)b * T + ic) * ld + col;
        const float* qp1 = qkv + ((size_t)b * T + in1) * ld + col;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const float uu = ub[col + k], vv = vb[col + k];
            qu[k] = qp[k] + uu;
            qv[k] = qp[k] + vv;
            qn[k] = qp1[k] + vv;
        }
    }

    floatx16 o[2];
    tile_zero(o);
    float m_run = -INFINITY, l_run = 0.f;

    const int lc4 = (tid & 15) * 4, lr = tid >> 4;
    const float* kbase = qkv + (size_t)b * T * ld + D + head * DK + lc4;
    float* Gw = Gs[wave];

    const int ntiles = (klen + KT - 1) / KT;
    for (int kt = 0; kt < ntiles; ++kt) {
        const int k0 = kt * KT;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = lr + 16 * i;
            int kr = k0 + r;
            kr = kr < klen ? kr : klen - 1;
            const float* src = kbase + (size_t)kr * ld;
            *reinterpret_cast<float4*>(&Ks[r * KLD + lc4]) = *reinterpret_cast<const float4*>(src);
            *reinterpret_cast<float4*>(&Vs[r * DK + lc4]) = *reinterpret_cast<const float4*>(src + D);
        }
        __syncthreads();

        // ---- S^T = K (q + u)^T
        const float* kp = &Ks[idx * KLD + hh * 32];
        floatx16 s = tile_kq([&](int i) { return kp + 4 * i; }, qu);

        // ---- the band products, skewed through the wave's LDS buffer
        const int delta = k0 - qs;                   // j - i = l - 31 + delta for row l of the buffer
        const int last_lower = legacy ? 31 - delta : 63;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            floatx16 gl, gu;
#pragma unroll
            for (int r = 0; r < 16; ++r) { gl[r] = 0.f; gu[r] = 0.f; }
            if (32 * g <= last_lower) gl = band_product(P, D, T - 32 + delta + 32 * g + idx, nP, col, qv);
            if (legacy && 32 * g + 31 >= 33 - delta) gu = band_product(P, D, delta - 33 + 32 * g + idx, nP, col, qn);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int l = 32 * g + tile_key(r, hh);
                Gw[idx * GS + l] = l <= last_lower ? gl[r] : (l == last_lower + 1 ? 0.f : gu[r]);
            }
        }
        __syncthreads();

        // ---- scores, online softmax for query (lane & 31)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = (s[r] + Gw[idx * GS + tile_key(r, hh) - idx + 31]) * 0.125f;
            if (k0 + tile_key(r, hh) >= klen) s[r] = -INFINITY;
        }
        tile_softmax<2, false>(s, m_run, l_run, o);
        tile_pv(Vs, hh, idx, s, o);
    }

    if (qi < T) tile_store(o, l_run, hh, ((size_t)b * T + qi) * D + head * DK, out, nullptr, 0);
}

}  // namespace

int launch_cf_relpos_attention(const float* qkv, const float* P, const float* u, const float* v, const int* klens, int B, int T,
                               int H, int legacy, float* out, hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && H > 0 && H <= 65535 && qkv && P && u && v && klens && out, "relpos_attention: bad shape");
    PF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)P & 15) == 0 && ((uintptr_t)out & 15) == 0, "relpos_attention: 16-B alignment");
    hipLaunchKernelGGL(relpos_attention_kernel, dim3(ceil_div(T, 128), H, B), dim3(256), 0, stream, qkv, P, u, v, klens, T, H, legacy, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
