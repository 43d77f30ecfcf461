// Masked scaled-dot-product attention for heads of d_k = 80 and 96 (MonotonicAligner: d_model 320, 4 heads), flash-style in
// exact fp32 on the matrix cores: neither the scores nor the probabilities exist as [B, H, T, T]. Semantics of attention_f32.hip
// (funasr/models/sanm/attention.py:270-306): softmax((q * scale) . k^T, keys >= klens[b] masked) . v.
//
// Mapping (attention_tile.h), the one of tf_attention_kernel (attention_abs.hip): one workgroup = 4 waves = 128 queries of one
// (sequence, head); a wave owns 32 queries, a lane ONE query (column lane & 31), the keys of a 32-key tile run over its
// accumulator registers:
//     S^T[key][q] = sum_d K[key][d] q[q][d]        A = K tile (LDS), B = registers; half-wave h takes d in [h DK/2, (h + 1) DK/2)
//     O^T[d][q]   = sum_key V[key][d] p[q][key]     A = V tile (LDS), B = the probabilities in the S^T registers, ND = 3 blocks
// The third block of 32 output channels is only half used at DK = 80: the V tile in LDS is 96 columns wide, its columns 80..95
// are zeroed once and never loaded, and the store is bounded at DK (those channels are the next head's first 16 columns, or lie
// past the row for the last head). A 32-channel MFMA block is the finest grain the swapped product has, so 80 costs what 96 costs
// in the second product.
//
// K rows in LDS are KLD = DK + 4 floats apart. The operand fetch is one ds_read_b128 per lane at row (lane & 31); that
// instruction is served in 16-lane groups whose rows are 16 distinct values mod 16 ({0-3, 12-15, 20-27} and {4-11, 16-19,
// 28-31} per half-wave), and a lane covers one 16-byte slot of the 16 a bank row has. Row r starts at slot r KLD / 4 mod 16, so
// the fetch is conflict free iff KLD / 4 is odd: 21 (84 floats) and 25 (100 floats) are, as 33 is for d_k = 128. The V tile is
// read with ds_read_b32, 32 consecutive floats of one row per half-wave: conflict free at any row length.
//
// The K / V rows of a partial tile are clamped to the last valid key (their scores are masked), so no row at or past klens[b]
// is read. No atomics, one fixed order per query: a call repeats bit for bit.
#include "attention_tile.h"

namespace pf {
namespace {

constexpr int KT = 32, VLD = 96;

template <int DK>
__global__ __launch_bounds__(256) void attention_mid_kernel(AttnArgs p) {
    static_assert(DK % 8 == 0 && DK > 64 && DK <= VLD, "attention_mid: 64 < d_k <= 96, a multiple of 8");
    constexpr int KLD = DK + 4, HD = DK / 2, C4 = DK / 4;
    static_assert((KLD / 4) % 2 == 1, "attention_mid: the K row stride must be an odd number of 16-byte slots");
    __shared__ __attribute__((aligned(16))) float Ks[KT * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[KT * VLD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, idx = lane & 31;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qi = blockIdx.x * 128 + wave * 32 + idx;
    int klen = p.klens[b];
    klen = klen > p.Tk ? p.Tk : klen;
    if (klen < 1) {      // outside the precondition (klens[b] >= 1): read nothing, leave zeros
        if (qi < p.Tq && hh == 0) {
            float* op = p.O + ((size_t)b * p.Tq + qi) * p.ldo + head * DK;
#pragma unroll
            for (int k = 0; k < DK; k += 4) *reinterpret_cast<float4*>(op + k) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }

    // this lane's query (clamped past Tq), d in [HD hh, HD hh + HD)
    float q[HD];
    tile_load_q(p.Q + ((size_t)b * p.Tq + (qi < p.Tq ? qi : p.Tq - 1)) * p.ldq + head * DK + hh * HD, p.scale, q);

    floatx16 o[3];
    tile_zero(o);
    float m_run = -INFINITY, l_run = 0.f;

    // the padding columns of the V tile: written here only (the loop's first barrier orders this before the first read)
    if (DK < VLD)
        for (int i = tid; i < KT * (VLD - DK); i += 256) Vs[(i / (VLD - DK)) * VLD + DK + i % (VLD - DK)] = 0.f;

    const float* kbase = p.K + (size_t)b * p.Tk * p.ldk + head * DK;
    const float* vbase = p.V + (size_t)b * p.Tk * p.ldv + head * DK;

    const int ntiles = (klen + KT - 1) / KT;
    for (int kt = 0; kt < ntiles; ++kt) {
        const int k0 = kt * KT;
        __syncthreads();
        for (int i = tid; i < KT * C4; i += 256) {
            const int r = i / C4, c = 4 * (i % C4);
            int kr = k0 + r;
            kr = kr < klen ? kr : klen - 1;
            *reinterpret_cast<float4*>(&Ks[r * KLD + c]) = *reinterpret_cast<const float4*>(kbase + (size_t)kr * p.ldk + c);
            *reinterpret_cast<float4*>(&Vs[r * VLD + c]) = *reinterpret_cast<const float4*>(vbase + (size_t)kr * p.ldv + c);
        }
        __syncthreads();

        const float* kp = &Ks[idx * KLD + hh * HD];
        floatx16 s = tile_kq([&](int i) { return kp + 4 * i; }, q);
        tile_mask(s, k0, hh, klen);
        tile_softmax<3, false>(s, m_run, l_run, o);
        tile_pv(Vs, hh, idx, s, o);
    }

    if (qi < p.Tq) tile_store<3, DK>(o, l_run, hh, ((size_t)b * p.Tq + qi) * p.ldo + head * DK, p.O, nullptr, 0);
}

}  // namespace

bool attention_mid_applicable(int dk) { return dk == 80 || dk == 96; }

int launch_attention_mid(const AttnArgs& a, int dk, hipStream_t stream) {
    PF_REQUIRE(attention_mid_applicable(dk), "attention_mid: d_k is 80 or 96");
    PF_REQUIRE(a.B > 0 && a.B <= 65535 && a.H > 0 && a.H <= 65535 && a.Tq > 0 && a.Tk > 0, "attention: empty problem");
    PF_REQUIRE(a.Q && a.K && a.V && a.O && a.klens, "attention_mid: null argument");
    PF_REQUIRE(!a.K2 && !a.O3 && !a.O2 && !a.fs_in && a.mask_mode == 0 && a.app_rows == 0,
               "attention_mid: one key/value source, a key-padding mask and fp32 output only");
    PF_REQUIRE(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0, "attention_mid: strides % 4");
    PF_REQUIRE(a.ldq >= a.H * dk && a.ldk >= a.H * dk && a.ldv >= a.H * dk && a.ldo >= a.H * dk, "attention_mid: a row holds H heads of d_k columns");
    PF_REQUIRE(((uintptr_t)a.Q & 15) == 0 && ((uintptr_t)a.K & 15) == 0 && ((uintptr_t)a.V & 15) == 0 && ((uintptr_t)a.O & 15) == 0,
               "attention_mid: 16-B alignment");
    const dim3 grid(ceil_div(a.Tq, 128), a.H, a.B);
    if (dk == 80) hipLaunchKernelGGL(attention_mid_kernel<80>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(attention_mid_kernel<96>, grid, dim3(256), 0, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
