// Kernels of the chunk Conformer encoder (see chunk_conformer.h): the chunk-window relative-position attention, the convolution
// module's row kernel with causal padding, the StreamingConvInput front (first conv per piece, the second conv's operand gather)
// and the strided row copy.
//
// Window attention: relpos_attention_kernel's mapping (attention_tile.h: 4 waves x 32 queries, a lane = ONE query, keys over the
// accumulator registers; the positional term as band products skewed through a per-wave LDS buffer), "latest" form only. What is
// new is which tiles are taken. With a chunk mask a query sees (left + 1) * chunk keys, not T: the workgroup walks the 32-key tiles
// from the one holding start(first query) to the one holding end(last query) - 1, so the work is O(T * window), and a wave whose 32
// queries see nothing of a tile passes it (the K / V loads and the barriers stay common to the four waves). Tile starts stay
// multiples of 32 from key 0, so without a chunk mask the tiles, and the order of every sum, are the existing kernel's.
#include "attention_tile.h"
#include "chunk_conformer.h"
#include "conformer.h"

namespace pf {
namespace {

constexpr int DK = 64, KT = 32, KLD = DK + 4, GS = 66;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// rows of P outside [lo, hi] feed elements the window mask replaces; they are not read
__device__ __forceinline__ floatx16 band_product(const float* P, int ldp, int row, int lo, int hi, int col, const float (&qv)[32]) {
    const int rc = row < lo ? lo : (row > hi ? hi : row);
    const float* pp = P + (size_t)rc * ldp + col;
    return tile_kq([&](int i) { return pp + 4 * i; }, qv);
}

__global__ __launch_bounds__(256) void cc_window_attention_kernel(const float* qkv, const float* P, const float* ub, const float* vb,
                                                                  const int* klens, int T, int H, int chunk, int left, float* out) {
    __shared__ __attribute__((aligned(16))) float Ks[KT * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[KT * DK];
    __shared__ float Gs[4][32 * GS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, idx = lane & 31;
    const int b = blockIdx.z, head = blockIdx.y;
    const int q0 = blockIdx.x * 128, qs = q0 + wave * 32;
    const int qi = qs + idx;
    const int D = H * DK, ld = 3 * D;
    int klen = klens[b];
    klen = klen > T ? T : (klen < 0 ? 0 : klen);
    const int col = head * DK + hh * 32;

    // the workgroup's union of windows [lo, hi), the wave's [wlo, whi), the lane's [ms, me)
    int lo, hi, wlo = 0, whi = 0, ms = 0, me = 0, t0, t1;
    const int qlast = q0 + 127 < T ? q0 + 127 : T - 1;
    cc_window(q0, T, chunk, left, klen, &lo, &t0);
    cc_window(qlast, T, chunk, left, klen, &t1, &hi);
    const int wlast = qs + 31 < T ? qs + 31 : T - 1;
    if (qs < T) {
        cc_window(qs, T, chunk, left, klen, &wlo, &t0);
        cc_window(wlast, T, chunk, left, klen, &t1, &whi);
    }
    if (qi < T) cc_window(qi, T, chunk, left, klen, &ms, &me);
    if (hi <= lo) {      // no row of the workgroup sees a key: the reference zeroes the probabilities -> 0
        if (qi < T) {
            float* op = out + ((size_t)b * T + qi) * D + col;
#pragma unroll
            for (int k = 0; k < 32; k += 4) *reinterpret_cast<float4*>(op + k) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }

    // this lane's query (clamped past T), d in [32 hh, 32 hh + 32): q + u, q + v
    float qu[32], qv[32];
    {
        const int ic = qi < T ? qi : T - 1;
        const float* qp = qkv + ((size_t)b * T + ic) * ld + col;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            qu[k] = qp[k] + ub[col + k];
            qv[k] = qp[k] + vb[col + k];
        }
    }
    // the rows of P the wave's (query, visible key) pairs lie in
    const int plo = T - 1 - wlast + wlo, phi = T - 1 - qs + whi - 1;

    floatx16 o[2];
    tile_zero(o);
    float m_run = -INFINITY, l_run = 0.f;

    const int lc4 = (tid & 15) * 4, lr = tid >> 4;
    const float* kbase = qkv + (size_t)b * T * ld + D + head * DK + lc4;
    float* Gw = Gs[wave];

    for (int k0 = lo / KT * KT; k0 < hi; k0 += KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = lr + 16 * i;
            int kr = k0 + r;
            kr = kr < lo ? lo : (kr < hi ? kr : hi - 1);
            const float* src = kbase + (size_t)kr * ld;
            *reinterpret_cast<float4*>(&Ks[r * KLD + lc4]) = *reinterpret_cast<const float4*>(src);
            *reinterpret_cast<float4*>(&Vs[r * DK + lc4]) = *reinterpret_cast<const float4*>(src + D);
        }
        __syncthreads();

        const bool act = whi > wlo && k0 < whi && k0 + KT > wlo;      // wave-uniform
        floatx16 s;
        if (act) {
            // ---- S^T = K (q + u)^T
            const float* kp = &Ks[idx * KLD + hh * 32];
            s = tile_kq([&](int i) { return kp + 4 * i; }, qu);
            // ---- the band products, skewed through the wave's LDS buffer: j - i = l - 31 + delta for row l of the buffer
            const int delta = k0 - qs;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const floatx16 gl = band_product(P, D, T - 32 + delta + 32 * g + idx, plo, phi, col, qv);
#pragma unroll
                for (int r = 0; r < 16; ++r) Gw[idx * GS + 32 * g + tile_key(r, hh)] = gl[r];
            }
        }
        __syncthreads();
        if (act) {
            // ---- scores, the window mask, online softmax for query (lane & 31)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = k0 + tile_key(r, hh);
                s[r] = (s[r] + Gw[idx * GS + tile_key(r, hh) - idx + 31]) * 0.125f;
                if (j < ms || j >= me) s[r] = -INFINITY;
            }
            tile_softmax_masked<2>(s, m_run, l_run, o);
            tile_pv(Vs, hh, idx, s, o);
        }
    }

    if (qi < T) tile_store(o, l_run, hh, ((size_t)b * T + qi) * D + head * DK, out, nullptr, 0);
}

constexpr int DW_TT = 32;      // output rows per workgroup
__global__ void __launch_bounds__(64) cc_glu_dw_kernel(const float* g, const float* dw, const float* dw_bias, const float* bn_scale,
                                                       const float* bn_shift, int T, int D, int taps, int pad, float* y) {
    const int t0 = blockIdx.x * DW_TT, c = blockIdx.y * 64 + threadIdx.x, b = blockIdx.z;
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

// one workgroup = one output time row t1 of one piece
__global__ void __launch_bounds__(256) cc_conv0_kernel(const float* feats, int L, int F, int NC, int LC, const float* w, const float* bias,
                                                       int C, int T1, int F1, float* y) {
    const int t1 = blockIdx.x, p = blockIdx.y;
    const int b = p / NC, n = p - b * NC;
    __shared__ float xs[3][256];
    for (int i = threadIdx.x; i < 3 * F; i += 256) {
        const int dt = i / F, f = i - dt * F;
        const int r = 2 * t1 - 1 + dt;                               // frame inside the piece
        const long long fr = (long long)n * LC + r;                  // frame inside the clip
        xs[dt][f] = (r >= 0 && r < LC && fr < L) ? feats[((size_t)b * L + fr) * F + f] : 0.f;
    }
    __syncthreads();
    float* dst = y + ((size_t)p * T1 + t1) * F1 * C;
    const int nout = F1 * C;
    for (int i = threadIdx.x; i < nout; i += 256) {
        const int f1 = i / C, c = i - f1 * C;
        float acc = bias[c];
        const float* wc = w + c * 9;
#pragma unroll
        for (int dt = 0; dt < 3; ++dt)
#pragma unroll
            for (int df = 0; df < 3; ++df) acc = fmaf(wc[dt * 3 + df], xs[dt][2 * f1 + df], acc);
        dst[i] = fmaxf(acc, 0.f);
    }
}

// one workgroup = one row (p, t, f) of the operand
__global__ void __launch_bounds__(256) cc_im2col_kernel(const float* x, int T1, int F1, int C4, int k, int s, int T2, int F2, long long r0,
                                                        float* a) {
    const long long row = r0 + blockIdx.x;
    const int f = (int)(row % F2);
    const long long pt = row / F2;
    const int t = (int)(pt % T2);
    const long long p = pt / T2;
    const int pad = (k - 1) / 2, K4 = k * k * C4;
    float4* dst = reinterpret_cast<float4*>(a) + (size_t)blockIdx.x * K4;
    for (int i = threadIdx.x; i < K4; i += 256) {
        const int kk = i / C4, c4 = i - kk * C4;
        const int kt = kk / k, kf = kk - kt * k;
        const int ti = t * s + kt - pad;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ti >= 0 && ti < T1) v = reinterpret_cast<const float4*>(x)[(((size_t)p * T1 + ti) * F1 + f * s + kf) * C4 + c4];
        dst[i] = v;
    }
}

__global__ void __launch_bounds__(256) cc_copy_rows_kernel(const float* x, int Ti, int step, float* y, int To, int D4, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / D4;
    const int c = (int)(i - row * D4);
    const size_t b = row / To;
    const int t = (int)(row - b * To);
    reinterpret_cast<float4*>(y)[i] = reinterpret_cast<const float4*>(x)[(b * Ti + (size_t)t * step) * D4 + c];
}

}  // namespace

int launch_cc_window_attention(const float* qkv, const float* P, const float* u, const float* v, const int* klens, int B, int T, int H,
                               int chunk, int left, float* out, hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= (1 << 24) && H > 0 && H <= 65535 && chunk >= 0 && chunk <= (1 << 24) && qkv && P && u && v && klens && out,
               "cc_window_attention: bad shape");
    PF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)P & 15) == 0 && ((uintptr_t)out & 15) == 0, "cc_window_attention: 16-B alignment");
    // no chunk mask: every window is [0, klen), which is the existing kernel's job (same tiles, same sums, and no window logic to pay for)
    if (chunk == 0) return launch_cf_relpos_attention(qkv, P, u, v, klens, B, T, H, 0, out, stream);
    hipLaunchKernelGGL(cc_window_attention_kernel, dim3(ceil_div(T, 128), H, B), dim3(256), 0, stream, qkv, P, u, v, klens, T, H, chunk,
                       left, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cc_glu_dw(const float* g, const float* dw, const float* dw_bias, const float* bn_scale, const float* bn_shift, int B, int T,
                     int D, int taps, int causal, float* y, hipStream_t stream) {
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && D > 0 && D % 64 == 0 && taps % 2 == 1 && taps >= 1 && taps <= 31 && g && dw && dw_bias &&
                   bn_scale && bn_shift && y,
               "cc_glu_dw: D % 64, odd taps <= 31");
    hipLaunchKernelGGL(cc_glu_dw_kernel, dim3(ceil_div(T, DW_TT), D / 64, B), dim3(64), 0, stream, g, dw, dw_bias, bn_scale, bn_shift, T, D,
                       taps, causal ? taps - 1 : taps / 2, y);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cc_conv0(const float* feats, int B, int L, int F, int NC, int LC, const float* w, const float* bias, int C, float* y,
                    hipStream_t stream) {
    PF_REQUIRE(B > 0 && L > 0 && F >= 3 && F <= 256 && NC > 0 && LC > 0 && (long long)B * NC <= 65535 && C > 0 && feats && w && bias && y,
               "cc_conv0: bad shape (3 .. 256 input features, at most 65535 pieces)");
    const int T1 = (LC - 1) / 2 + 1, F1 = (F - 3) / 2 + 1;
    hipLaunchKernelGGL(cc_conv0_kernel, dim3(T1, B * NC), dim3(256), 0, stream, feats, L, F, NC, LC, w, bias, C, T1, F1, y);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cc_im2col(const float* x, int NP, int T1, int F1, int C, int k, int s, long long r0, int nrows, float* a, hipStream_t stream) {
    PF_REQUIRE(NP > 0 && T1 > 0 && C > 0 && C % 4 == 0 && k >= 1 && k % 2 == 1 && s >= 1 && F1 >= k && r0 >= 0 && nrows > 0 && x && a &&
                   ((uintptr_t)x & 15) == 0 && ((uintptr_t)a & 15) == 0,
               "cc_im2col: bad shape");
    const int T2 = (T1 - 1) / s + 1, F2 = (F1 - k) / s + 1;
    PF_REQUIRE(r0 + nrows <= (long long)NP * T2 * F2, "cc_im2col: rows past the operand");
    hipLaunchKernelGGL(cc_im2col_kernel, dim3(nrows), dim3(256), 0, stream, x, T1, F1, C / 4, k, s, T2, F2, r0, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cc_copy_rows(const float* x, int Ti, int step, float* y, int B, int To, int D, hipStream_t stream) {
    PF_REQUIRE(B > 0 && To > 0 && step >= 1 && Ti > (long long)(To - 1) * step && D > 0 && D % 4 == 0 && x && y && ((uintptr_t)x & 15) == 0 &&
                   ((uintptr_t)y & 15) == 0,
               "cc_copy_rows: bad shape");
    const size_t total = (size_t)B * To * (D / 4);
    hipLaunchKernelGGL(cc_copy_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, Ti, step, y, To, D / 4, total);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
