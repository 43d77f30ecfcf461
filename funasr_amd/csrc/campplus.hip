// CAM++ speaker-embedding network on gfx950 (funasr/models/campplus/model.py, components.py).
//
// Every convolution of the network -- the 3x3 convs of the 2-D head (FCM), the stride-2 TDNN, the 1x1 bottleneck and
// transit convs and the dilated local convs of the D-TDNN layers -- is ONE implicit-GEMM kernel on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32, the instruction of gemm_f32.hip): fp32-class results, and the order of every accumulation is
// fixed by the k loop alone, so a chunk's embedding does not depend on the batch it is launched in.
//   * Operands are staged HBM -> registers -> LDS (double buffered, one barrier per 16-wide K tile); the register hop is
//     what lets the loader gather conv taps (zero outside the sequence) and apply the pre-activation BatchNorm-ReLU of a
//     dense layer / transit layer to the A operand as it is staged, instead of materialising a transformed copy.
//   * Block tile 32 WM x 32 WN with WM * WN = 4 waves, one 32 x 32 accumulator per wave; WN follows N (32: the FCM convs and
//     the 32-column local convs, 128: bottleneck / TDNN, 128 column blocks for the transits).
//   * The epilogue adds the folded-BN bias, the identity shortcut, applies ReLU or the CAM mask, and stores with any row
//     stride: the D-TDNN layers write their 32 new channels straight into the block's concat buffer.
// The CAM context (time mean + 100-frame segment means -> 128-64-32 MLP -> sigmoid) and the stats-pool head are small
// per-chunk kernels with a fixed reduction order.
#include "campplus.h"

namespace pf {

namespace {

constexpr int BK = 16;

template <bool CONV2D, int WN>
__global__ __launch_bounds__(256) void cam_gemm_kernel(CamGemmArgs p) {
    constexpr int WM = 4 / WN, BM = 32 * WM, BN = 32 * WN;
    constexpr int AL = BM * BK / 256, BL = BN * BK / 256;   // operand elements each thread stages per K tile
    constexpr int APAD = BM + 4, BPAD = BN + 4;            // row strides of the k-major LDS tiles (conflict-free stores)
    __shared__ float As[2][BK * APAD];
    __shared__ float Bs[2][BK * BPAD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kk = tid & 15;                               // the k column this thread stages (both operands)

    // per staged A row: validity and the decomposition of m the gather needs
    bool rv[AL];
    int rbase[AL], rt[AL], rf[AL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        const int m = m0 + (tid >> 4) + i * 16;
        rv[i] = m < p.M;
        const int mm = rv[i] ? m : 0;
        if constexpr (CONV2D) {
            const int nt = mm / p.Fo;                      // chunk * T + t
            rf[i] = mm - nt * p.Fo;                        // fo
            rt[i] = nt % p.T;                              // t
            rbase[i] = nt;
        } else {
            const int c = mm / p.To, to = mm - c * p.To;
            rbase[i] = c * p.Tin;
            rt[i] = to * p.stride - p.pad;
            rf[i] = 0;
        }
    }
    float ra[AL], rb[BL];
    auto load = [&](int kt) {
        const int k = kt * BK + kk;
        const bool kin = k < p.K;
        if constexpr (CONV2D) {
            const int K1 = 9 * p.Cin;
            const bool main = k < K1;
            const int tap = main ? k / p.Cin : 0, ci = main ? k - tap * p.Cin : k - K1;
            const int kf = tap / 3, ktt = tap - 3 * kf;
#pragma unroll
            for (int i = 0; i < AL; ++i) {
                float v = 0.f;
                if (rv[i] && kin) {
                    if (main) {
                        const int fi = rf[i] * p.fstride + kf - 1, ti = rt[i] + ktt - 1;
                        if (fi >= 0 && fi < p.Fin && ti >= 0 && ti < p.T)
                            v = p.A[((size_t)(rbase[i] + ktt - 1) * p.Fin + fi) * p.Cin + ci];
                    } else {
                        v = p.A2[((size_t)rbase[i] * p.Fin2 + rf[i] * p.fstride2) * p.Cin2 + ci];
                    }
                }
                ra[i] = v;
            }
        } else {
            const int tap = kin ? k / p.Cin : 0, ci = k - tap * p.Cin;
            float sc = 1.f, sh = 0.f;
            const bool pre = p.pre_scale != nullptr && kin;
            if (pre) { sc = p.pre_scale[ci]; sh = p.pre_shift[ci]; }
#pragma unroll
            for (int i = 0; i < AL; ++i) {
                float v = 0.f;
                const int ti = rt[i] + tap * p.dil;
                if (rv[i] && kin && ti >= 0 && ti < p.Tin) {
                    v = p.A[(size_t)(rbase[i] + ti) * p.lda + ci];
                    if (pre) v = fmaxf(fmaf(v, sc, sh), 0.f);
                }
                ra[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int n = n0 + (tid >> 4) + i * 16;
            rb[i] = (kin && n < p.N) ? p.W[(size_t)n * p.ldw + k] : 0.f;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AL; ++i) As[buf][kk * APAD + (tid >> 4) + i * 16] = ra[i];
#pragma unroll
        for (int i = 0; i < BL; ++i) Bs[buf][kk * BPAD + (tid >> 4) + i * 16] = rb[i];
    };

    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nk = (p.K + BK - 1) / BK;
    const int aoff = (lane >> 5) * APAD + wm * 32 + (lane & 31);
    const int boff = (lane >> 5) * BPAD + wn * 32 + (lane & 31);
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        store(buf);                     // buffer `buf` was last read in iteration kt - 2, before the barrier of kt - 1
        __syncthreads();
        if (kt + 1 < nk) load(kt + 1);  // global loads of the next tile in flight under this tile's MFMAs
        const float* a = As[buf] + aoff;
        const float* b = Bs[buf] + boff;
#pragma unroll
        for (int s = 0; s < BK / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s * APAD], b[2 * s * BPAD], acc, 0, 0, 0);
    }

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= p.N) return;
    const float bias = p.bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= p.M) continue;
        float v = acc[r] + bias;
        if (p.R) v += p.R[(size_t)row * p.ldr + col];
        if (p.relu) v = fmaxf(v, 0.f);
        if (p.mask) {
            const int c = row / p.To, to = row - c * p.To;
            v *= p.mask[((size_t)c * p.nseg + to / 100) * p.N + col];
        }
        p.C[(size_t)row * p.ldc + col] = v;
    }
}

// one workgroup per chunk, thread c = bottleneck channel (128)
__global__ __launch_bounds__(128) void cam_context_kernel(const float* __restrict__ h, int T, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, float* __restrict__ mask) {
    __shared__ float ctx[128];
    __shared__ float z[64];
    const int n = blockIdx.x, c = threadIdx.x;
    const float* hb = h + (size_t)n * T * 128 + c;
    float tot = 0.f;
    for (int t = 0; t < T; ++t) tot += hb[(size_t)t * 128];
    const float g = tot / (float)T;
    const int nseg = (T + 99) / 100;
    for (int s = 0; s < nseg; ++s) {
        const int t0 = s * 100, t1 = min(t0 + 100, T);
        float ss = 0.f;
        for (int t = t0; t < t1; ++t) ss += hb[(size_t)t * 128];
        __syncthreads();                                   // the previous segment's MLP is done with ctx / z
        ctx[c] = g + ss / (float)(t1 - t0);
        __syncthreads();
        if (c < 64) {
            float v = b1[c];
            const float* w = w1 + c * 128;
            for (int i = 0; i < 128; ++i) v = fmaf(w[i], ctx[i], v);
            z[c] = fmaxf(v, 0.f);
        }
        __syncthreads();
        if (c < 32) {
            float v = b2[c];
            const float* w = w2 + c * 64;
            for (int j = 0; j < 64; ++j) v = fmaf(w[j], z[j], v);
            mask[((size_t)n * nseg + s) * 32 + c] = 1.f / (1.f + expf(-v));
        }
    }
}

// one workgroup per chunk: out BN-ReLU, mean / unbiased std over time (two passes), dense 2C -> E, affine-free BN
__global__ __launch_bounds__(512) void cam_pool_dense_kernel(const float* __restrict__ x, int T, int C, const float* __restrict__ psc,
                                                             const float* __restrict__ psh, const float* __restrict__ wt, int E,
                                                             const float* __restrict__ osc, const float* __restrict__ osh,
                                                             float* __restrict__ emb) {
    __shared__ float st[1024];
    const int n = blockIdx.x;
    const float* xb = x + (size_t)n * T * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float sc = psc[c], sh = psh[c];
        float sum = 0.f;
        for (int t = 0; t < T; ++t) sum += fmaxf(fmaf(xb[(size_t)t * C + c], sc, sh), 0.f);
        const float mean = sum / (float)T;
        float sq = 0.f;
        for (int t = 0; t < T; ++t) {
            const float d = fmaxf(fmaf(xb[(size_t)t * C + c], sc, sh), 0.f) - mean;
            sq = fmaf(d, d, sq);
        }
        st[c] = mean;
        st[C + c] = sqrtf(sq / (float)(T - 1));
    }
    __syncthreads();
    for (int o = threadIdx.x; o < E; o += blockDim.x) {
        float v = 0.f;
        for (int k = 0; k < 2 * C; ++k) v = fmaf(wt[(size_t)k * E + o], st[k], v);
        emb[(size_t)n * E + o] = fmaf(v, osc[o], osh[o]);
    }
}

__global__ void cam_gather_chunks_kernel(const float* __restrict__ wav, int64_t n_samples, const int64_t* __restrict__ starts,
                                         const int* __restrict__ valid, int len, float* __restrict__ out) {
    const int i = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= len) return;
    const int64_t s = starts[i] + j;
    const int nv = valid ? valid[i] : len;
    out[(size_t)i * len + j] = (j < nv && s >= 0 && s < n_samples) ? wav[s] : 0.f;
}

__global__ void cam_sub_mean_kernel(float* __restrict__ f, int T, int D) {
    const int d = threadIdx.x;
    if (d >= D) return;
    float* b = f + (size_t)blockIdx.x * T * D + d;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += b[(size_t)t * D];
    const float m = s / (float)T;
    for (int t = 0; t < T; ++t) b[(size_t)t * D] -= m;
}

}  // namespace

int launch_cam_gemm(const CamGemmArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0 && a.A && a.W && a.C, "cam_gemm: empty problem or null operand");
    if (a.conv2d) {
        PF_REQUIRE(a.T > 0 && a.Fin > 0 && a.Fo > 0 && a.fstride > 0 && a.Cin > 0 && a.M % (a.T * a.Fo) == 0 &&
                   a.K == 9 * a.Cin + (a.A2 ? a.Cin2 : 0) && (a.Fo - 1) * a.fstride + 1 <= a.Fin + 1,
                   "cam_gemm: inconsistent conv2d shape");
        if (a.A2) PF_REQUIRE(a.Cin2 > 0 && a.fstride2 > 0 && (a.Fo - 1) * a.fstride2 < a.Fin2, "cam_gemm: inconsistent shortcut shape");
        PF_REQUIRE(!a.mask && !a.pre_scale, "cam_gemm: the conv2d form has no mask / prologue");
    } else {
        PF_REQUIRE(a.Tin > 0 && a.To > 0 && a.Cin > 0 && a.taps > 0 && a.stride > 0 && a.dil > 0 && a.pad >= 0 && a.M % a.To == 0 &&
                   a.K == a.taps * a.Cin && a.lda >= a.Cin, "cam_gemm: inconsistent conv1d shape");
        PF_REQUIRE(!a.pre_scale || (a.taps == 1 && a.pre_shift), "cam_gemm: the BN-ReLU prologue needs a 1x1 conv");
        PF_REQUIRE(!a.mask || (a.nseg == (a.To + 99) / 100), "cam_gemm: mask segments");
    }
    PF_REQUIRE(a.ldw >= a.K && a.ldc >= a.N && (!a.R || a.ldr >= a.N), "cam_gemm: leading dimensions");
    const int wn = a.N <= 32 ? 1 : (a.N <= 64 ? 2 : 4);
    const int bm = 32 * (4 / wn), bn = 32 * wn;
    const dim3 grid((unsigned)ceil_div(a.M, bm), (unsigned)ceil_div(a.N, bn)), block(256);
#define PF_CAM_LAUNCH(C2, WN_) hipLaunchKernelGGL((cam_gemm_kernel<C2, WN_>), grid, block, 0, stream, a)
    if (a.conv2d) {
        if (wn == 1) PF_CAM_LAUNCH(true, 1); else if (wn == 2) PF_CAM_LAUNCH(true, 2); else PF_CAM_LAUNCH(true, 4);
    } else {
        if (wn == 1) PF_CAM_LAUNCH(false, 1); else if (wn == 2) PF_CAM_LAUNCH(false, 2); else PF_CAM_LAUNCH(false, 4);
    }
#undef PF_CAM_LAUNCH
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cam_context(const float* h, int T, int n_chunks, const float* w1, const float* b1, const float* w2, const float* b2,
                       float* mask, hipStream_t stream) {
    PF_REQUIRE(h && w1 && b1 && w2 && b2 && mask && T > 0 && n_chunks > 0, "cam_context: bad argument");
    hipLaunchKernelGGL(cam_context_kernel, dim3(n_chunks), dim3(128), 0, stream, h, T, w1, b1, w2, b2, mask);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cam_pool_dense(const float* x, int T, int C, int n_chunks, const float* pre_scale, const float* pre_shift,
                          const float* wt, int E, const float* scale, const float* shift, float* emb, hipStream_t stream) {
    PF_REQUIRE(x && pre_scale && pre_shift && wt && scale && shift && emb && T >= 2 && C > 0 && C <= 512 && E > 0 && n_chunks > 0,
               "cam_pool_dense: bad argument (T >= 2 frames, C <= 512)");
    hipLaunchKernelGGL(cam_pool_dense_kernel, dim3(n_chunks), dim3(512), 0, stream, x, T, C, pre_scale, pre_shift, wt, E, scale,
                       shift, emb);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cam_gather_chunks(const float* wav, int64_t n_samples, const int64_t* starts_dev, const int* valid_dev, int n, int len,
                             float* out, hipStream_t stream) {
    PF_REQUIRE(wav && starts_dev && out && n > 0 && len > 0 && n <= 65535, "cam_gather_chunks: bad argument");
    hipLaunchKernelGGL(cam_gather_chunks_kernel, dim3(ceil_div(len, 256), n), dim3(256), 0, stream, wav, n_samples, starts_dev,
                       valid_dev, len, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cam_sub_mean(float* feats, int n, int T, int D, hipStream_t stream) {
    PF_REQUIRE(feats && n > 0 && T > 0 && D > 0 && D <= 128, "cam_sub_mean: bad argument");
    hipLaunchKernelGGL(cam_sub_mean_kernel, dim3(n), dim3(128), 0, stream, feats, T, D);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
