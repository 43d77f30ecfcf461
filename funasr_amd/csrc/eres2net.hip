// ERes2NetV2 speaker-embedding network on gfx950 (funasr/models/eres2net/eres2netv2.py, fusion.py).
//
// Every convolution of the network behind the stem -- the 1x1 and 3x3 convs of the Res2Net blocks, stride 1 or 2 in frequency and
// time, the two 1x1 convs of an attentional feature fusion (AFF), layer3_ds -- and the embedding layer are ONE implicit-GEMM kernel
// on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32): fp32-class results, and the order of every accumulation is fixed by the k loop
// alone, so a chunk's embedding does not depend on the batch it is launched in.
//   * K tiles are 32 wide and both operands are staged as 16-byte vectors along the channel axis: HBM -> registers (the gather of
//     the conv taps, as branch-free global loads that stay in flight under the tile being multiplied) -> the zero outside the chunk
//     and the sum with a second operand -> one ds_write_b128 per vector into row-major LDS tiles of row stride 36 floats
//     (conflict-free for the 8 x 8 lane groups of the store and the 4 x 16 groups of ds_read_b128).
//   * The MFMA takes k = lane >> 5 from its two lane halves. The half h of a lane is given the 16 CONSECUTIVE k values
//     [16 h, 16 h + 16) of the tile (A and B alike, so every product still meets its partner): a lane's operands of a K tile are four
//     ds_read_b128 per 32 rows instead of sixteen ds_read_b32.
//   * Block tile 128 x BN, four waves; BN follows N alone (32, 64: four waves stacked on M; 128: 2 x 2 waves of 64 x 64).
//   * The epilogue adds the folded-BN bias and the identity shortcut, applies ReLU / clamp(0, 20) / SiLU or the AFF combine, and
//     stores with any row stride (column slices of a wider buffer).
// The stem (1 -> C channels, K = 9) is a direct VALU kernel; the stats pool is a per-column kernel with a fixed reduction order.
#include "eres2net.h"

namespace pf {

namespace {

constexpr int BK = 32;
constexpr int LD = 36;           // LDS row stride in floats: 16-B aligned rows, 9 (odd) slots apart

// bit j set: element j of a staged vector is data (the vector is in range and its channel c + j lies below C)
__device__ __forceinline__ int keep_bits(bool ok, int c, int C) {
    const int left = C - c;
    return ok ? (left >= 4 ? 15 : (left <= 0 ? 0 : (1 << left) - 1)) : 0;
}
// (native vectors and scalar selects: v_cndmask, no memory)
__device__ __forceinline__ floatx4 mask4(floatx4 v, int bits) {
    floatx4 o;
    o.x = bits & 1 ? v.x : 0.f;
    o.y = bits & 2 ? v.y : 0.f;
    o.z = bits & 4 ? v.z : 0.f;
    o.w = bits & 8 ? v.w : 0.f;
    return o;
}

template <int WM, int WN, int MI, int NI, bool SUM>
__global__ __launch_bounds__(256) void eres_conv_kernel(EresConvArgs p) {
    constexpr int BM = 32 * WM * MI, BN = 32 * WN * NI;
    constexpr int AL = BM / 32, BL = BN / 32;            // float4 vectors each thread stages per K tile
    __shared__ __attribute__((aligned(16))) float As[BM * LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int k4 = tid & 7, srow = tid >> 3;             // the vector along k and the first row this thread stages

    const int CinP = (p.Cin + 3) & ~3;
    const int K1 = p.taps * CinP;
    const int K = K1 + (p.a2_mode == ERES_A2_CONCAT ? ((p.Cin2 + 3) & ~3) : 0);

    // per staged A row: validity and the decomposition of m the gather needs
    bool rv[AL];
    int rc[AL], rt[AL], rf[AL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        const int m = m0 + srow + i * 32;
        rv[i] = m < p.M;
        const int mm = rv[i] ? m : 0;
        const int nt = mm / p.Fo;
        rf[i] = mm - nt * p.Fo;
        rc[i] = nt / p.To;
        rt[i] = nt - rc[i] * p.To;
    }
    // Every operand pointer is a global-memory pointer: said so to the compiler, the loads are global_load (vmcnt only) and stay in
    // flight under the ds_reads of the tile being multiplied; as generic pointers they would be flat loads, which count on the LDS
    // counter too and have to be drained before the first ds_read.
    typedef const float __attribute__((address_space(1)))* gptr;
    typedef const floatx4 __attribute__((address_space(1)))* gptr4;
    const gptr gA = (gptr)p.A, gA2 = (gptr)p.A2, gW = (gptr)p.W;
    floatx4 ra[AL], ra2[SUM ? AL : 1], rb[BL];
    int ka[AL], kb[BL];
    // A load is never skipped: a vector that is out of range (padding of the conv, rows past M, columns past K) is fetched from the
    // operand's first row, so the gather has no divergent branch. What replaces it by zero (and the sum of the two operands) waits
    // until the vector is stored to LDS, one K tile later: nothing in front of the MFMAs uses a value still in flight.
    auto load = [&](int kt) {
        const int k = kt * BK + k4 * 4;
        const bool kin = k < K, first = k < K1;
        int c = k - K1, df = 0, dt = 0;
        if (first) {
            const int tap = k / CinP;
            c = k - tap * CinP;
            if (p.taps == 9) { df = tap / 3; dt = tap - 3 * df - 1; df -= 1; }
        }
        const bool second = kin && !first;                  // the K-concatenated operand
        const gptr src = second ? gA2 : gA;
        const int climit = second ? p.Cin2 : p.Cin;
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int ti = rt[i] * p.st + dt, fi = rf[i] * p.sf + df;
            const bool ok = rv[i] && kin && (second || (ti >= 0 && ti < p.Tin && fi >= 0 && fi < p.Fin));
            const size_t pos = second ? ((size_t)rc[i] * p.Tin2 + rt[i] * p.st2) * p.Fin2 + rf[i] * p.sf2
                                      : ((size_t)rc[i] * p.Tin + ti) * p.Fin + fi;
            const size_t off = ok ? pos * (second ? p.lda2 : p.lda) + c : 0;
            ra[i] = *reinterpret_cast<gptr4>(src + off);
            if constexpr (SUM) ra2[i] = *reinterpret_cast<gptr4>(gA2 + (ok ? pos * p.lda2 + c : 0));
            ka[i] = keep_bits(ok, c, climit);
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int n = n0 + srow + i * 32;
            const bool ok = kin && n < p.N;
            rb[i] = *reinterpret_cast<gptr4>(gW + (ok ? (size_t)n * p.ldw + k : 0));
            kb[i] = ok ? 15 : 0;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            floatx4 v = ra[i];
            if constexpr (SUM) v += ra2[i];
            *reinterpret_cast<floatx4*>(&As[(srow + i * 32) * LD + k4 * 4]) = mask4(v, ka[i]);
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) *reinterpret_cast<floatx4*>(&Bs[(srow + i * 32) * LD + k4 * 4]) = mask4(rb[i], kb[i]);
    };

    floatx16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const int nk = (K + BK - 1) / BK;
    const int half = lane >> 5;
    const float* ap = As + (wm * 32 * MI + (lane & 31)) * LD + half * 16;
    const float* bp = Bs + (wn * 32 * NI + (lane & 31)) * LD + half * 16;
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
        store();
        __syncthreads();
        if (kt + 1 < nk) load(kt + 1);      // global loads of the next tile in flight under this tile's MFMAs
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            floatx4 a[MI], b[NI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) a[mi] = *reinterpret_cast<const floatx4*>(ap + mi * 32 * LD + q * 4);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) b[ni] = *reinterpret_cast<const floatx4*>(bp + ni * 32 * LD + q * 4);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].x, b[ni].x, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].y, b[ni].y, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].z, b[ni].z, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].w, b[ni].w, acc[mi][ni], 0, 0, 0);
                }
        }
        __syncthreads();                    // every wave is done with the tile before the next store overwrites it
    }

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
    // The addends (shortcut, the AFF pair) of eight rows are fetched before the first of their stores: C aliases nothing the kernel
    // reads, but the compiler cannot know, and a load placed behind a store waits for it -- 64 round trips in a row per lane.
    typedef float __attribute__((address_space(1)))* gout;
    const gptr gR = (gptr)p.R, gX = (gptr)p.X, gY = (gptr)p.Y, gB = (gptr)p.bias;
    const gout gC = (gout)p.C;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int col = n0 + (wn * NI + ni) * 32 + (lane & 31);
        if (col >= p.N) continue;
        const float bias = gB ? gB[col] : 0.f;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int row0 = m0 + (wm * MI + mi) * 32 + 4 * half;
#pragma unroll
            for (int rh = 0; rh < 16; rh += 8) {             // eight rows at a time: the addends of a batch live in registers
                float rr[8], xx[8], yy[8];
#pragma unroll
                for (int r = rh; r < rh + 8; ++r) {
                    const int row = row0 + (r & 3) + 8 * (r >> 2);
                    const bool in = row < p.M;
                    rr[r - rh] = gR && in ? gR[(size_t)row * p.ldr + col] : 0.f;
                    xx[r - rh] = gX && in ? gX[(size_t)row * p.ldx + col] : 0.f;
                    yy[r - rh] = gX && in ? gY[(size_t)row * p.ldy + col] : 0.f;
                }
#pragma unroll
                for (int r = rh; r < rh + 8; ++r) {
                    const int row = row0 + (r & 3) + 8 * (r >> 2);
                    if (row >= p.M) continue;
                    float v = acc[mi][ni][r] + bias;
                    if (gR) v += rr[r - rh];
                    if (p.act == ERES_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (p.act == ERES_ACT_CLAMP20) v = fminf(fmaxf(v, 0.f), 20.f);
                    else if (p.act == ERES_ACT_SILU) v = v / (1.f + expf(-v));
                    if (gX) {
                        const float g = 1.f + tanhf(v);
                        v = xx[r - rh] * g + yy[r - rh] * (2.f - g);
                    }
                    gC[(size_t)row * p.ldc + col] = v;
                }
            }
        }
    }
}

// one thread per output element (t, f, c) of the chunk blockIdx.y: nine taps of the single input channel
__global__ __launch_bounds__(256) void eres_stem_kernel(const float* __restrict__ x, int T, int F, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int C, float* __restrict__ out) {
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x, per = (unsigned)T * F * C;
    if (idx >= per) return;
    const unsigned pos = idx / C;
    const int c = (int)(idx - pos * C), t = (int)(pos / F), f = (int)(pos - (unsigned)t * F);
    const float* xb = x + (size_t)blockIdx.y * T * F;
    float v = bias[c];
#pragma unroll
    for (int kf = 0; kf < 3; ++kf)
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
            const int fi = f + kf - 1, ti = t + kt - 1;
            if (fi >= 0 && fi < F && ti >= 0 && ti < T) v = fmaf(w[c * 9 + kf * 3 + kt], xb[(size_t)ti * F + fi], v);
        }
    out[(size_t)blockIdx.y * per + idx] = fmaxf(v, 0.f);
}

// one thread per (chunk, column): two passes over time
__global__ __launch_bounds__(256) void eres_pool_kernel(const float* __restrict__ x, int T, int S, float* __restrict__ stats) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= S) return;
    const int n = blockIdx.y;
    const float* xb = x + (size_t)n * T * S + j;
    float sum = 0.f;
    for (int t = 0; t < T; ++t) sum += xb[(size_t)t * S];
    const float mean = sum / (float)T;
    float sq = 0.f;
    for (int t = 0; t < T; ++t) {
        const float d = xb[(size_t)t * S] - mean;
        sq = fmaf(d, d, sq);
    }
    stats[(size_t)n * 2 * S + j] = mean;
    stats[(size_t)n * 2 * S + S + j] = sqrtf(sq / (float)(T - 1) + 1e-8f);
}

}  // namespace

int launch_eres_conv(const EresConvArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.M > 0 && a.N > 0 && a.A && a.W && a.C && a.Cin > 0, "eres_conv: empty problem or null operand");
    PF_REQUIRE((a.taps == 1 || a.taps == 9) && (a.st == 1 || a.st == 2) && (a.sf == 1 || a.sf == 2), "eres_conv: taps 1 / 9, strides 1 / 2");
    PF_REQUIRE(a.Tin > 0 && a.Fin > 0 && a.To == (a.Tin - 1) / a.st + 1 && a.Fo == (a.Fin - 1) / a.sf + 1 &&
               a.M % (a.To * a.Fo) == 0, "eres_conv: inconsistent conv shape");
    PF_REQUIRE(a.lda % 4 == 0 && a.lda >= eres_pad4(a.Cin) && ((uintptr_t)a.A & 15) == 0, "eres_conv: A needs a 16-B aligned base and a stride of 4 n >= pad4(Cin)");
    const int K = eres_conv_k(a);
    PF_REQUIRE(a.ldw % 4 == 0 && a.ldw >= K && ((uintptr_t)a.W & 15) == 0, "eres_conv: W needs a 16-B aligned base and a stride of 4 n >= K");
    PF_REQUIRE(a.ldc >= a.N && (!a.R || a.ldr >= a.N), "eres_conv: leading dimensions");
    PF_REQUIRE(a.act >= ERES_ACT_NONE && a.act <= ERES_ACT_SILU, "eres_conv: unknown activation");
    PF_REQUIRE((a.X == nullptr) == (a.Y == nullptr) && (!a.X || (a.ldx >= a.N && a.ldy >= a.N)), "eres_conv: the AFF combine needs both X and Y");
    if (a.a2_mode == ERES_A2_SUM) {
        PF_REQUIRE(a.A2 && a.lda2 % 4 == 0 && a.lda2 >= eres_pad4(a.Cin) && ((uintptr_t)a.A2 & 15) == 0, "eres_conv: summed second operand");
    } else if (a.a2_mode == ERES_A2_CONCAT) {
        PF_REQUIRE(a.A2 && a.Cin2 > 0 && a.lda2 % 4 == 0 && a.lda2 >= eres_pad4(a.Cin2) && ((uintptr_t)a.A2 & 15) == 0 &&
                   (a.st2 == 1 || a.st2 == 2) && (a.sf2 == 1 || a.sf2 == 2) && a.Tin2 > 0 && a.Fin2 > 0 &&
                   (a.To - 1) * a.st2 < a.Tin2 && (a.Fo - 1) * a.sf2 < a.Fin2, "eres_conv: concatenated second operand");
    } else {
        PF_REQUIRE(a.a2_mode == ERES_A2_NONE, "eres_conv: unknown second-operand mode");
    }
    const int bn = a.N <= 32 ? 32 : (a.N <= 64 ? 64 : 128);
    const dim3 grid((unsigned)ceil_div(a.M, 128), (unsigned)ceil_div(a.N, bn)), block(256);
#define PF_ERES_LAUNCH(WM_, WN_, MI_, NI_)                                                                          \
    do {                                                                                                           \
        if (sum) hipLaunchKernelGGL((eres_conv_kernel<WM_, WN_, MI_, NI_, true>), grid, block, 0, stream, a);       \
        else hipLaunchKernelGGL((eres_conv_kernel<WM_, WN_, MI_, NI_, false>), grid, block, 0, stream, a);          \
    } while (0)
    const bool sum = a.a2_mode == ERES_A2_SUM;
    if (bn == 32) PF_ERES_LAUNCH(4, 1, 1, 1);
    else if (bn == 64) PF_ERES_LAUNCH(4, 1, 1, 2);
    else PF_ERES_LAUNCH(2, 2, 2, 2);
#undef PF_ERES_LAUNCH
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eres_stem(const float* feats, int n, int T, int F, const float* w, const float* bias, int C, float* out,
                     hipStream_t stream) {
    PF_REQUIRE(feats && w && bias && out && n > 0 && T > 0 && F > 0 && C > 0, "eres_stem: bad argument");
    const size_t per = (size_t)T * F * C;
    PF_REQUIRE(n <= 65535 && per <= 0x7fffff00u, "eres_stem: at most 65535 chunks of fewer than 2^31 elements per launch");
    hipLaunchKernelGGL(eres_stem_kernel, dim3((unsigned)((per + 255) / 256), n), dim3(256), 0, stream, feats, T, F, w, bias, C, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eres_pool(const float* x, int n, int T, int S, float* stats, hipStream_t stream) {
    PF_REQUIRE(x && stats && n > 0 && n <= 65535 && T >= 2 && S > 0, "eres_pool: bad argument (T >= 2 frames, <= 65535 chunks)");
    hipLaunchKernelGGL(eres_pool_kernel, dim3(ceil_div(S, 256), n), dim3(256), 0, stream, x, T, S, stats);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
