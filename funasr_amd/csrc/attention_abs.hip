// Plain masked self-attention of the Transformer encoder (funasr/models/transformer/attention.py MultiHeadedAttention), d_k = 64,
// flash-style in exact fp32 on the matrix cores: neither the scores nor the probabilities exist as [B, H, T, T].
//
// Mapping (attention_tile.h), the one of relpos_attention_kernel without its positional half: one workgroup = 4 waves = 128 queries
// of one (sequence, head); a wave owns 32 queries, a lane ONE query (column lane & 31), and the keys of a 32-key tile run over its
// accumulator registers:
//     S^T[key][q] = sum_d K[key][d] q[q][d]                  A = K tile (LDS),       B = registers
//     O^T[d][q]   = sum_key V[key][d] p[q][key]               A = V tile (LDS),       B = the probabilities in the S^T registers
// The K / V rows of a partial tile are clamped to the last valid key (their scores are masked), so no row at or past klens[b] is read.
// No atomics, one fixed order per query: a call repeats bit for bit.
#include "attention_tile.h"
#include "conformer.h"

namespace pf {
namespace {

constexpr int DK = 64, KT = 32, KLD = DK + 4;

__global__ __launch_bounds__(256) void tf_attention_kernel(const float* qkv, const int* klens, int T, int H, float* out) {
    __shared__ __attribute__((aligned(16))) float Ks[KT * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[KT * DK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, idx = lane & 31;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qi = blockIdx.x * 128 + wave * 32 + idx;
    const int D = H * DK, ld = 3 * D;
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

    // this lane's query (clamped past T), d in [32 hh, 32 hh + 32)
    float q[32];
    tile_load_q(qkv + ((size_t)b * T + (qi < T ? qi : T - 1)) * ld + col, 1.0f, q);

    floatx16 o[2];
    tile_zero(o);
    float m_run = -INFINITY, l_run = 0.f;

    const int lc4 = (tid & 15) * 4, lr = tid >> 4;
    const float* kbase = qkv + (size_t)b * T * ld + D + head * DK + lc4;

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

        const float* kp = &Ks[idx * KLD + hh * 32];
        floatx16 s = tile_kq([&](int i) { return kp + 4 * i; }, q);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= 0.125f;
        tile_mask(s, k0, hh, klen);
        tile_softmax<2, false>(s, m_run, l_run, o);
        tile_pv(Vs, hh, idx, s, o);
    }

    if (qi < T) tile_store(o, l_run, hh, ((size_t)b * T + qi) * D + head * DK, out, nullptr, 0);
}

}  // namespace

int launch_tf_attention(const float* qkv, const int* klens, int B, int T, int H, float* out, hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && H > 0 && H <= 65535 && qkv && klens && out, "tf_attention: bad shape");
    PF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 15) == 0, "tf_attention: 16-B alignment");
    hipLaunchKernelGGL(tf_attention_kernel, dim3(ceil_div(T, 128), H, B), dim3(256), 0, stream, qkv, klens, T, H, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
