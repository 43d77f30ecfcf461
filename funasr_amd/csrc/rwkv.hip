// RWKV encoder on gfx950 (funasr/models/rwkv_bat): the token-shift mix behind a LayerNorm, the chunked WKV scan, and the two pointwise
// kernels of the channel mix. Everything between them is a GEMM (gemm_f32.hip) or a conv (eres2net.hip); see rwkv.h for the contracts.
//
// Row kernels: one wave per row, the row in registers as float4 per lane (D <= 1024), statistics by wave reductions in a fixed order,
// so a row's bits depend on that row (and, for the mix, the row before it in the same clip) alone.
// WKV: lane = channel, so every load and store of a wave is one contiguous 256-B segment of a row.
#include "rwkv.h"

namespace pf {

namespace {

template <int NV>
__device__ __forceinline__ void row_load(const float* __restrict__ x, int D, int lane, floatx4 (&v)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = c < D ? *reinterpret_cast<const floatx4*>(x + c) : floatx4{0.f, 0.f, 0.f, 0.f};
    }
}

// v <- (v - mean) / sqrt(var + eps) * gamma + beta (two passes over the registers; every lane of the wave takes part)
template <int NV>
__device__ __forceinline__ void row_layernorm(floatx4 (&v)[NV], int D, int lane, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);      // lanes past D hold zeros
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if ((i * 64 + lane) * 4 < D) {
            const floatx4 d = v[i] - mean;
            q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        }
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) {
            const floatx4 g = *reinterpret_cast<const floatx4*>(gamma + c), b = *reinterpret_cast<const floatx4*>(beta + c);
            v[i] = (v[i] - mean) * rstd * g + b;
        }
    }
}

template <int NV>
__global__ __launch_bounds__(256) void rwkv_mix_kernel(RwkvMixArgs p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)p.B * p.T) return;
    const int b = (int)(row / p.T), t = (int)(row - (long long)b * p.T);
    float* y = p.Y + (size_t)row * p.ldy;
    if (t >= p.lens[b]) {
        for (int j = 0; j < p.n_out; ++j)
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = (i * 64 + lane) * 4;
                if (c < p.D) *reinterpret_cast<floatx4*>(y + (size_t)j * p.D + c) = floatx4{0.f, 0.f, 0.f, 0.f};
            }
        return;
    }
    floatx4 cur[NV], prev[NV];
    const float* x = p.X + (size_t)row * p.ldx;
    row_load<NV>(x, p.D, lane, cur);
    row_layernorm<NV>(cur, p.D, lane, p.gamma, p.beta, p.eps);
    if (t > 0) {                                                                  // (uniform over the wave)
        row_load<NV>(x - p.ldx, p.D, lane, prev);
        row_layernorm<NV>(prev, p.D, lane, p.gamma, p.beta, p.eps);
    } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) prev[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    for (int j = 0; j < p.n_out; ++j) {
        const float* mu = p.mix[j];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < p.D) {
                const floatx4 m = *reinterpret_cast<const floatx4*>(mu + c);
                *reinterpret_cast<floatx4*>(y + (size_t)j * p.D + c) = cur[i] * m + prev[i] * (1.f - m);
            }
        }
    }
}

template <int NV>
__global__ __launch_bounds__(256) void rwkv_norm_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, float* __restrict__ Y, int ldy,
                                                        const int* __restrict__ lens, int B, int T, int step, int To, int D) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * To) return;
    const int b = (int)(row / To), j = (int)(row - (long long)b * To);
    const long long t = (long long)j * step;
    float* y = Y + (size_t)row * ldy;
    floatx4 v[NV];
    const bool live = t < lens[b] && t < T;
    if (live) {
        row_load<NV>(X + ((size_t)b * T + (size_t)t) * ldx, D, lane, v);
        row_layernorm<NV>(v, D, lane, gamma, beta, eps);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) *reinterpret_cast<floatx4*>(y + c) = live ? v[i] : floatx4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---------------------------------------------------------------------------------------------------------------- WKV
constexpr int L = RWKV_CHUNK;

// one state update of the recurrence (also how a chunk is summarised: from (0, 0, -1e38) the first step gives (v, 1, k))
__device__ __forceinline__ void wkv_advance(float& num, float& den, float& m, float w, float kk, float vv) {
    const float mw = m + w;
    const float ms = fmaxf(kk, mw);
    const float e1 = expf(mw - ms), e2 = expf(kk - ms);
    num = e1 * num + e2 * vv;
    den = e1 * den + e2;
    m = ms;
}

__global__ __launch_bounds__(64) void rwkv_wkv_summary_kernel(RwkvWkvArgs p) {
    const int ch = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (ch >= p.D) return;
    const int len = min(p.lens[b], p.T), t0 = c * L;
    if (t0 + L >= len) return;                                  // no chunk of this clip follows: nobody reads the summary
    const float w = p.w[ch];
    const size_t base = ((size_t)b * p.T + t0) * p.ld + ch;
    const float* __restrict__ kp = p.k + base;
    const float* __restrict__ vp = p.v + base;
    float num = 0.f, den = 0.f, m = -1e38f;
#pragma unroll 8
    for (int i = 0; i < L; ++i) wkv_advance(num, den, m, w, kp[(size_t)i * p.ld], vp[(size_t)i * p.ld]);
    float* s = p.sum + ((size_t)b * gridDim.y + c) * 3 * p.D + ch;
    s[0] = num; s[p.D] = den; s[2 * (size_t)p.D] = m;
}

__global__ __launch_bounds__(64) void rwkv_wkv_output_kernel(RwkvWkvArgs p) {
    const int ch = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (ch >= p.D) return;
    const int len = min(p.lens[b], p.T), t0 = c * L;
    const int t_end = min(t0 + L, p.T), live_end = min(t_end, len);
    float* __restrict__ op = p.out + ((size_t)b * p.T) * p.ldo + ch;
    if (t0 < len) {
        const float w = p.w[ch], u = p.u[ch], wL = w * (float)L;
        float num = 0.f, den = 0.f, m = -1e-30f;                // the reference's initial state (rwkv_encoder.py:155)
        const float* s = p.sum + (size_t)b * gridDim.y * 3 * p.D + ch;
        for (int j = 0; j < c; ++j, s += 3 * (size_t)p.D) {     // every chunk before this one is L frames long
            const float a = s[0], d = s[p.D], q = s[2 * (size_t)p.D];
            const float md = m + wL;
            const float mo = fmaxf(md, q);
            const float e1 = expf(md - mo), e2 = expf(q - mo);
            num = e1 * num + e2 * a;
            den = e1 * den + e2 * d;
            m = mo;
        }
        const size_t base = ((size_t)b * p.T) * p.ld + ch;
        const float* __restrict__ kp = p.k + base;
        const float* __restrict__ vp = p.v + base;
        const float* __restrict__ rp = p.r + base;
#pragma unroll 4
        for (int t = t0; t < live_end; ++t) {
            const float kk = kp[(size_t)t * p.ld], vv = vp[(size_t)t * p.ld], rr = rp[(size_t)t * p.ld];
            const float uk = u + kk;
            const float mo = fmaxf(m, uk);
            const float e1 = expf(m - mo), e2 = expf(uk - mo);
            const float wkv = (e1 * num + e2 * vv) / (e1 * den + e2);
            op[(size_t)t * p.ldo] = (1.f / (1.f + expf(-rr))) * wkv;
            wkv_advance(num, den, m, w, kk, vv);
        }
    }
    for (int t = max(t0, live_end); t < t_end; ++t) op[(size_t)t * p.ldo] = 0.f;
}

// ------------------------------------------------------------------------------------------------------ pointwise
enum { PW_SQRELU = 0, PW_GATE = 1 };
template <int MODE>
__global__ __launch_bounds__(256) void rwkv_pointwise_kernel(const float* x, int ldx, const float* __restrict__ r, int ldr,
                                                             const float* __restrict__ val, int ldv, float* out, int ldo,
                                                             const int* __restrict__ lens, int B, int T, int N) {
    const int n4 = N >> 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)B * T * n4) return;
    const size_t row = idx / n4;
    const int c = (int)(idx - row * n4) * 4;
    const int b = (int)(row / T), t = (int)(row - (size_t)b * T);
    floatx4 o = {0.f, 0.f, 0.f, 0.f};
    if (t < lens[b]) {
        const floatx4 a = *reinterpret_cast<const floatx4*>(x + row * ldx + c);
        if constexpr (MODE == PW_SQRELU) {
            o.x = fmaxf(a.x, 0.f); o.y = fmaxf(a.y, 0.f); o.z = fmaxf(a.z, 0.f); o.w = fmaxf(a.w, 0.f);
            o = o * o;
        } else {
            const floatx4 g = *reinterpret_cast<const floatx4*>(r + row * ldr + c), h = *reinterpret_cast<const floatx4*>(val + row * ldv + c);
            o.x = a.x + (1.f / (1.f + expf(-g.x))) * h.x;
            o.y = a.y + (1.f / (1.f + expf(-g.y))) * h.y;
            o.z = a.z + (1.f / (1.f + expf(-g.z))) * h.z;
            o.w = a.w + (1.f / (1.f + expf(-g.w))) * h.w;
        }
    }
    *reinterpret_cast<floatx4*>(out + row * ldo + c) = o;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_rwkv_mix(const RwkvMixArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.X && a.gamma && a.beta && a.Y && a.lens && a.B > 0 && a.T > 0, "rwkv_mix: null/empty argument");
    PF_REQUIRE(a.D >= 4 && a.D % 4 == 0 && a.D <= RWKV_MAX_D, "rwkv_mix: D a multiple of 4 up to 1024");
    PF_REQUIRE((a.n_out == 2 || a.n_out == 3) && a.mix[0] && a.mix[1] && (a.n_out == 2 || a.mix[2]), "rwkv_mix: 2 or 3 mixed operands");
    PF_REQUIRE(a.ldx % 4 == 0 && a.ldx >= a.D && a.ldy % 4 == 0 && a.ldy >= a.n_out * a.D, "rwkv_mix: strides of 4 n that hold the rows");
    PF_REQUIRE(aligned16(a.X) && aligned16(a.Y) && aligned16(a.gamma) && aligned16(a.beta) && aligned16(a.mix[0]) && aligned16(a.mix[1]) &&
               (a.n_out == 2 || aligned16(a.mix[2])), "rwkv_mix: operands must be 16-B aligned");
    const long long rows = (long long)a.B * a.T;
    PF_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, "rwkv_mix: too many rows");
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    if (a.D <= 512) hipLaunchKernelGGL(rwkv_mix_kernel<2>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(rwkv_mix_kernel<4>, grid, block, 0, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rwkv_norm(const float* X, int ldx, const float* gamma, const float* beta, float eps, float* Y, int ldy, const int* lens,
                     int B, int T, int step, int To, int D, hipStream_t stream) {
    PF_REQUIRE(X && gamma && beta && Y && lens && B > 0 && T > 0 && step > 0 && To > 0, "rwkv_norm: null/empty argument");
    PF_REQUIRE((long long)(To - 1) * step < T, "rwkv_norm: the last output row lies past the input");
    PF_REQUIRE(D >= 4 && D % 4 == 0 && D <= RWKV_MAX_D && ldx % 4 == 0 && ldx >= D && ldy % 4 == 0 && ldy >= D,
               "rwkv_norm: D a multiple of 4 up to 1024, strides of 4 n that hold the rows");
    PF_REQUIRE(aligned16(X) && aligned16(Y) && aligned16(gamma) && aligned16(beta), "rwkv_norm: operands must be 16-B aligned");
    const long long rows = (long long)B * To;
    PF_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, "rwkv_norm: too many rows");
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    if (D <= 512) hipLaunchKernelGGL(rwkv_norm_kernel<2>, grid, block, 0, stream, X, ldx, gamma, beta, eps, Y, ldy, lens, B, T, step, To, D);
    else hipLaunchKernelGGL(rwkv_norm_kernel<4>, grid, block, 0, stream, X, ldx, gamma, beta, eps, Y, ldy, lens, B, T, step, To, D);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rwkv_wkv(const RwkvWkvArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.k && a.v && a.r && a.w && a.u && a.lens && a.out && a.sum && a.B > 0 && a.T > 0 && a.D > 0, "rwkv_wkv: null/empty argument");
    PF_REQUIRE(a.ld >= a.D && a.ldo >= a.D, "rwkv_wkv: strides must hold the rows");
    const int nc = ceil_div(a.T, RWKV_CHUNK);
    PF_REQUIRE(a.B <= 65535 && nc <= 65535, "rwkv_wkv: at most 65535 clips of 65535 chunks per launch");
    const dim3 grid((unsigned)ceil_div(a.D, 64), (unsigned)nc, (unsigned)a.B), block(64);
    if (nc > 1) hipLaunchKernelGGL(rwkv_wkv_summary_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(rwkv_wkv_output_kernel, grid, block, 0, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

static int pointwise_check(const char* who, const void* a, int lda, const void* o, int ldo, const int* lens, int B, int T, int N) {
    PF_REQUIRE(a && o && lens && B > 0 && T > 0 && N >= 4 && N % 4 == 0, std::string(who) + ": null/empty argument, or a width that is no multiple of 4");
    PF_REQUIRE(lda % 4 == 0 && lda >= N && ldo % 4 == 0 && ldo >= N && aligned16(a) && aligned16(o),
               std::string(who) + ": 16-B aligned operands with strides of 4 n that hold the rows");
    PF_REQUIRE(((size_t)B * T * (N / 4) + 255) / 256 <= 0x7fffffffull, std::string(who) + ": too many elements");
    return 0;
}

int launch_rwkv_sqrelu(float* h, int ld, const int* lens, int B, int T, int N, hipStream_t stream) {
    if (int rc = pointwise_check("rwkv_sqrelu", h, ld, h, ld, lens, B, T, N)) return rc;
    const unsigned blocks = (unsigned)(((size_t)B * T * (N / 4) + 255) / 256);
    hipLaunchKernelGGL(rwkv_pointwise_kernel<PW_SQRELU>, dim3(blocks), dim3(256), 0, stream, h, ld, nullptr, 0, nullptr, 0, h, ld, lens, B, T, N);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rwkv_gate(const float* x, int ldx, const float* r, int ldr, const float* val, int ldv, float* x_out, int ldo, const int* lens,
                     int B, int T, int D, hipStream_t stream) {
    if (int rc = pointwise_check("rwkv_gate", x, ldx, x_out, ldo, lens, B, T, D)) return rc;
    PF_REQUIRE(r && val && ldr % 4 == 0 && ldr >= D && ldv % 4 == 0 && ldv >= D && aligned16(r) && aligned16(val),
               "rwkv_gate: 16-B aligned r / val with strides of 4 n that hold the rows");
    const unsigned blocks = (unsigned)(((size_t)B * T * (D / 4) + 255) / 256);
    hipLaunchKernelGGL(rwkv_pointwise_kernel<PW_GATE>, dim3(blocks), dim3(256), 0, stream, x, ldx, r, ldr, val, ldv, x_out, ldo, lens, B, T, D);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
