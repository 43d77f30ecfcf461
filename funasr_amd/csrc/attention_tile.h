// The tile step of the swapped-MFMA attention kernels: attention_f32_kernel, attention_f32_dma_kernel, attention_bf16_kernel,
// attention_split3_kernel, relpos_attention_kernel, cc_window_attention_kernel and attention_mid_kernel.
//
// Mapping. A wave owns 32 queries and a lane owns ONE of them (q = lane & 31); both products are issued "swapped", so the keys
// of a 32-key tile and then the output channels run over the lane's accumulator registers:
//     S^T[key][q] = sum_d K[key][d] Q[q][d]          A = K tile, B = Q (registers)
//     O^T[d][q]   = sum_key V[key][d] P[q][key]      A = V tile, B = P
// Register r of half-wave h = lane >> 5 holds key tile_key(r, h) = (r & 3) + 8 (r >> 2) + 4 h. The MFMA k index is only a pairing
// between A and B, so for the second product half-wave h takes exactly the keys its own S^T registers hold: P goes from the
// accumulator straight into the B operand, the softmax row statistics are per lane (one xor-32 shuffle joins the two halves) and
// nothing is transposed through LDS. The output accumulators are ND floatx16 of 32 channels each (d_k = 32 ND).
//
// The kernels keep what is particular to them: loaders, LDS layouts, how a score is scaled / biased / masked, operand packing.
#pragma once
#include "common.h"

namespace pf {

__device__ __forceinline__ constexpr int tile_key(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

template <int ND>
__device__ __forceinline__ void tile_zero(floatx16 (&o)[ND]) {
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
}

// fp32 Q fragment: N consecutive floats of this lane's query row, pre-scaled like the reference (q * d_k^-0.5)
template <int N>
__device__ __forceinline__ void tile_load_q(const float* qp, float scale, float (&q)[N]) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
        const float4 t = *reinterpret_cast<const float4*>(qp + 4 * i);
        q[4 * i + 0] = t.x * scale;
        q[4 * i + 1] = t.y * scale;
        q[4 * i + 2] = t.z * scale;
        q[4 * i + 3] = t.w * scale;
    }
}

// fp32 A . B^T over this half-wave's N values of d: a_of(i) is the address of the lane's i-th float4 of A (an LDS row in any
// layout, or global memory), b the matching registers; four v_mfma_f32_32x32x2_f32 per float4, one chain
template <int N, class AddrOf>
__device__ __forceinline__ floatx16 tile_kq(AddrOf a_of, const float (&b)[N]) {
    floatx16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(a_of(i));
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[4 * i + 0], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[4 * i + 1], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b[4 * i + 2], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b[4 * i + 3], s, 0, 0, 0);
    }
    return s;
}

// the key mask of the tile that starts at key k0: scores of keys >= klen become -inf
__device__ __forceinline__ void tile_mask(floatx16& s, int k0, int hh, int klen) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (k0 + tile_key(r, hh) >= klen) s[r] = -INFINITY;
}

// online softmax of one score tile for query (lane & 31): s arrives scaled, biased and masked (-inf; every tile has >= 1 valid
// key, so the maximum is finite) and leaves as the probabilities against the new running maximum; l_run and o are rescaled.
// FAST_EXP: __expf instead of libm expf. S: floatx16 or float[16].
template <int ND, bool FAST_EXP, class S>
__device__ __forceinline__ void tile_softmax(S& s, float& m_run, float& l_run, floatx16 (&o)[ND]) {
    auto ex = [](float x) { return FAST_EXP ? __expf(x) : expf(x); };
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = ex(m_run - m_new);       // exp(-inf) = 0 on the first tile
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        s[r] = ex(s[r] - m_new);
        psum += s[r];
    }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
}

// tile_softmax (libm expf) for kernels whose mask can leave a query NO valid key in a tile, or in every tile so far
// (launch_cc_window_attention: a tile is taken when ANY of the workgroup's queries sees a key of it): while the running maximum is
// still -inf the exponent's reference point is 0, so a masked score gives exp(-inf) = 0 instead of exp(-inf + inf) = NaN. Where the
// new maximum is finite this is tile_softmax<ND, false> operation for operation.
template <int ND, class S>
__device__ __forceinline__ void tile_softmax_masked(S& s, float& m_run, float& l_run, floatx16 (&o)[ND]) {
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float m_ref = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = expf(m_run - m_ref);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        s[r] = expf(s[r] - m_ref);
        psum += s[r];
    }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
}

// O^T += V^T P in fp32: Vs = the V tile in LDS, [32 keys][32 ND] floats; s = the probabilities tile_softmax left
template <int ND>
__device__ __forceinline__ void tile_pv(const float* Vs, int hh, int idx, const floatx16& s, floatx16 (&o)[ND]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float* vp = Vs + tile_key(r, hh) * (32 * ND) + idx;
#pragma unroll
        for (int d = 0; d < ND; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32 * d], s[r], o[d], 0, 0, 0);
    }
}

// o / l_run -> this query's row at element offset orow: fp32 into O, or with O3 its three bf16 planes (o_plane elements apart:
// the out-projection's operand in bf16x3 mode). CH < 32 ND (a multiple of 8: attention_mid.hip) bounds the channels written:
// a lane's float4 covers channels [32 d + 8 g + 4 hh, + 4), so whole groups g fall on either side of the bound
template <int ND, int CH = 32 * ND>
__device__ __forceinline__ void tile_store(const floatx16 (&o)[ND], float l_run, int hh, size_t orow, float* O, unsigned short* O3,
                                           size_t o_plane) {
    static_assert(CH % 8 == 0 && CH <= 32 * ND, "tile_store: the channel bound is a multiple of 8");
    // l_run == 0: no tile was taken (an empty key sequence); o is still zero and the row is stored as zeros, the reference's
    // masked_fill(0) after the softmax. For l_run > 0 the quotient is the one it always was
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (d * 32 + 8 * g >= CH) continue;
            const float t[4] = {o[d][4 * g + 0] * inv, o[d][4 * g + 1] * inv, o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv};
            const size_t off = orow + d * 32 + 8 * g + 4 * hh;
            if (O3) store_split3x4(O3 + off, o_plane, t);
            else *reinterpret_cast<float4*>(O + off) = make_float4(t[0], t[1], t[2], t[3]);
        }
}

}  // namespace pf
