// Kernels of the UniASR two-pass model (launchers and contracts: uniasr.h). The chunk masks of overlap_chunk have block structure, so
// the kernels take the chunk geometry and work out per row which keys / rows take part; no [Tc, Tc] mask exists on the device.
#include "uniasr.h"

namespace pf {

namespace {

constexpr int CA_MAX_DK = 128;
constexpr int CA_WAVES = 4;

// One wave per (sequence, head, query row). The query's keys lie in [lo, hi): its own chunk and, for the first `stride` rows of a
// chunk, the look-back chunks in front of it, of which only the first `stride` frames per chunk are visible. Tiles of 64 keys, one
// key per lane for the scores, online softmax, then lane = output dim (lane, lane + 64) for p . V over the tile's visible keys.
__global__ __launch_bounds__(64 * CA_WAVES) void chunk_attention_kernel(AttnArgs p, int dk, ChunkGeom g) {
    __shared__ float qs[CA_WAVES][CA_MAX_DK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = blockIdx.x * CA_WAVES + wv;
    const int head = blockIdx.y, b = blockIdx.z;
    if (r >= p.Tq) return;                                   // (whole waves leave: no block-wide barrier below)
    const int period = g.chunk + g.shift;
    const int c = r / period, j = r % period - g.shift;
    float* op = p.O + ((size_t)b * p.Tq + r) * p.ldo + head * dk;
    const int klen = p.klens[b] < p.Tk ? p.klens[b] : p.Tk;
    const int own_lo = c * period + g.shift;
    int hi = own_lo + g.chunk;
    hi = hi < klen ? hi : klen;
    int lo = own_lo;
    if (j >= 0 && j < g.stride && g.look_back > 0) {
        const int c0 = c - g.look_back > 0 ? c - g.look_back : 0;
        lo = c0 * period + g.shift;
    }
    if (j < 0 || lo >= hi) {                                 // a shift row, or nothing valid in reach: zero row
        for (int d = lane; d < dk; d += 64) op[d] = 0.f;
        return;
    }
    const float* qp = p.Q + ((size_t)b * p.Tq + r) * p.ldq + head * dk;
    for (int d = lane; d < dk; d += 64) qs[wv][d] = qp[d] * p.scale;
    __builtin_amdgcn_wave_barrier();
    const float* kb = p.K + (size_t)b * p.Tk * p.ldk + head * dk;
    const float* vb = p.V + (size_t)b * p.Tk * p.ldv + head * dk;
    float m = -INFINITY, l = 0.f, acc0 = 0.f, acc1 = 0.f;
    for (int k0 = lo; k0 < hi; k0 += 64) {
        const int key = k0 + lane;
        bool vis = key < hi;
        if (vis && key < own_lo) {                           // a look-back chunk: its first `stride` frames only
            const int jj = key % period - g.shift;
            vis = jj >= 0 && jj < g.stride;
        }
        float s = -INFINITY;
        if (vis) {
            const float* kp = kb + (size_t)key * p.ldk;
            s = 0.f;
            for (int d = 0; d < dk; d += 4) {
                const float4 t = *reinterpret_cast<const float4*>(kp + d);
                s = fmaf(qs[wv][d], t.x, s); s = fmaf(qs[wv][d + 1], t.y, s);
                s = fmaf(qs[wv][d + 2], t.z, s); s = fmaf(qs[wv][d + 3], t.w, s);
            }
        }
        const float tmax = wave_max(s);
        if (tmax == -INFINITY) continue;                     // no visible key in this tile (wave-uniform)
        const float mn = fmaxf(m, tmax);
        const float alpha = m == -INFINITY ? 0.f : expf(m - mn);
        const float pr = vis ? expf(s - mn) : 0.f;
        l = l * alpha + wave_sum(pr);
        m = mn;
        acc0 *= alpha; acc1 *= alpha;
        const int nt = hi - k0 < 64 ? hi - k0 : 64;
        for (int t = 0; t < nt; ++t) {
            const float w = __shfl(pr, t, 64);
            if (w == 0.f) continue;                          // masked (or underflowed) key: its V row is not read (wave-uniform)
            const float* vp = vb + (size_t)(k0 + t) * p.ldv;
            if (lane < dk) acc0 = fmaf(w, vp[lane], acc0);
            if (lane + 64 < dk) acc1 = fmaf(w, vp[lane + 64], acc1);
        }
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;
    if (lane < dk) op[lane] = acc0 * inv;
    if (lane + 64 < dk) op[lane + 64] = acc1 * inv;
}

// one block per (row, sequence), threads over the channels
__global__ __launch_bounds__(256) void chunk_fsmn_kernel(FsmnArgs p, ChunkGeom g) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int len = p.lens[b] < p.T ? p.lens[b] : p.T;
    const int period = g.chunk + g.shift;
    const size_t base = (size_t)b * p.T;
    const bool live = t < len && t % period >= g.shift;
    for (int c = threadIdx.x; c < p.C; c += 256) {
        float o = 0.f;
        if (live) {
            float acc = 0.f;
            for (int k = 0; k < p.K; ++k) {
                const int tt = t - p.left_pad + k;
                if (tt >= 0 && tt < len && tt % period >= g.shift) acc = fmaf(p.w[(size_t)c * p.K + k], p.in[(base + tt) * p.ldin + c], acc);
            }
            o = acc + p.in[(base + t) * p.ldin + c];
        }
        p.out[(base + t) * p.ldo + c] = o;
    }
}

__global__ __launch_bounds__(256) void gather_rows_or_zero_kernel(const float* __restrict__ src, int ld, int n_src, const int* __restrict__ idx,
                                                                  float* __restrict__ out, int n, int D4) {
    const size_t total = (size_t)n * D4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / D4), c = (int)(i % D4);
        const int id = idx[r];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (id >= 0 && id < n_src) v = *reinterpret_cast<const float4*>(src + (size_t)id * ld + 4 * c);
        reinterpret_cast<float4*>(out)[i] = v;
    }
}

// One block per output row: the `taps` input rows [a | b] are staged in LDS as xs[k][ci]; one wave per output channel at a time, the
// lanes stride over the channel's contiguous weights w[co][ci][k] (flat index e = ci * taps + k).
__global__ __launch_bounds__(256) void stride_conv_kernel(const float* __restrict__ a, int Da, const float* __restrict__ b, int Db, int T,
                                                          const float* __restrict__ w, const float* __restrict__ bias, int Cout, int taps,
                                                          int stride, int pad_left, float* __restrict__ out) {
    extern __shared__ float xs[];                            // taps * (Da + Db)
    const int t = blockIdx.x, Cin = Da + Db;
    for (int i = threadIdx.x; i < taps * Cin; i += 256) {
        const int k = i / Cin, ci = i % Cin;
        const int u = t * stride + k - pad_left;
        float v = 0.f;
        if (u >= 0 && u < T) v = ci < Da ? a[(size_t)u * Da + ci] : b[(size_t)u * Db + (ci - Da)];
        xs[i] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int E = Cin * taps;
    for (int co = wv; co < Cout; co += 4) {
        const float* wp = w + (size_t)co * E;
        float acc = 0.f;
        for (int e = lane; e < E; e += 64) {
            const int ci = e / taps, k = e - ci * taps;
            acc = fmaf(wp[e], xs[k * Cin + ci], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            const float y = acc + bias[co];
            out[(size_t)t * Cout + co] = y > 0.f ? y : 0.f;
        }
    }
}

// fd_attention_kernel (conformer.hip) with a key window and a mask row: one wave per (query, head)
template <int DK>
__global__ void __launch_bounds__(64) scama_attention_kernel(const float* q, const float* K, const float* V, int ldkv, const float* mask,
                                                             int lo, int hi, int D, float* out) {
    const int r = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    extern __shared__ float sc[];                            // hi - lo probabilities
    __shared__ float qs[DK];
#pragma unroll
    for (int c = 0; c < DK / 64; ++c) qs[lane + 64 * c] = q[(size_t)r * D + h * DK + lane + 64 * c];
    __syncthreads();
    const float* Kb = K + h * DK;
    const float* Vb = V + h * DK;
    const float scale = DK == 64 ? 0.125f : 0.08838834764831845f;      // 1 / sqrt(DK)
    float mx = -INFINITY;
    for (int j = lo + lane; j < hi; j += 64) {
        float a = -INFINITY;
        if (mask == nullptr || mask[j] != 0.f) {
            const float* kp = Kb + (size_t)j * ldkv;
            a = 0.f;
#pragma unroll 8
            for (int d = 0; d < DK; d += 4) {
                const float4 kv = *reinterpret_cast<const float4*>(kp + d);
                a = fmaf(qs[d], kv.x, a); a = fmaf(qs[d + 1], kv.y, a); a = fmaf(qs[d + 2], kv.z, a); a = fmaf(qs[d + 3], kv.w, a);
            }
            a *= scale;
        }
        sc[j - lo] = a;
        mx = fmaxf(mx, a);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    if (mx != -INFINITY) {
        for (int j = lo + lane; j < hi; j += 64) {
            const float s = sc[j - lo];
            const float p = s == -INFINITY ? 0.f : expf(s - mx);
            sc[j - lo] = p;
            sum += p;
        }
    }
    sum = wave_sum(sum);
    __syncthreads();
    float acc[DK / 64];
#pragma unroll
    for (int c = 0; c < DK / 64; ++c) acc[c] = 0.f;
    if (sum > 0.f) {
        for (int j = lo; j < hi; ++j) {
            const float p = sc[j - lo];
            if (p == 0.f) continue;                          // masked key: its V row is not read (uniform over the wave)
#pragma unroll
            for (int c = 0; c < DK / 64; ++c) acc[c] = fmaf(p, Vb[(size_t)j * ldkv + lane + 64 * c], acc[c]);
        }
    }
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
    for (int c = 0; c < DK / 64; ++c) out[(size_t)r * D + h * DK + lane + 64 * c] = acc[c] * inv;
}

bool geom_ok(const ChunkGeom& g) {
    return g.chunk >= 1 && g.stride >= 1 && g.stride <= g.chunk && g.shift >= 0 && g.look_back >= 0 && g.chunk + g.shift <= (1 << 20);
}

}  // namespace

int launch_chunk_attention(const AttnArgs& a, int dk, const ChunkGeom& g, hipStream_t stream) {
    PF_REQUIRE(a.Q && a.K && a.V && a.O && a.klens && a.B > 0 && a.B <= 65535 && a.H > 0 && a.H <= 65535 && a.Tq > 0 && a.Tk == a.Tq,
               "chunk_attention: self-attention over one source (Tq == Tk)");
    PF_REQUIRE(dk >= 4 && dk <= CA_MAX_DK && dk % 4 == 0 && a.ldk % 4 == 0 && ((uintptr_t)a.K & 15) == 0 && a.K2 == nullptr && a.O3 == nullptr,
               "chunk_attention: d_k % 4 and <= 128, 16-B aligned key rows, one key/value source");
    PF_REQUIRE(geom_ok(g), "chunk_attention: chunk geometry (1 <= stride <= chunk, shift >= 0, look_back >= 0)");
    hipLaunchKernelGGL(chunk_attention_kernel, dim3(ceil_div(a.Tq, CA_WAVES), a.H, a.B), dim3(64 * CA_WAVES), 0, stream, a, dk, g);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_chunk_fsmn(const FsmnArgs& a, const ChunkGeom& g, hipStream_t stream) {
    PF_REQUIRE(a.in && a.w && a.out && a.lens && a.B > 0 && a.B <= 65535 && a.T > 0 && a.C > 0 && a.K >= 1 && a.left_pad >= 0 &&
                   a.left_pad < a.K && a.R == nullptr && a.offs == nullptr && a.in_bf16 == 0,
               "chunk_fsmn: fp32 rows, no residual, no packed layout");
    PF_REQUIRE(geom_ok(g), "chunk_fsmn: chunk geometry (1 <= stride <= chunk, shift >= 0, look_back >= 0)");
    hipLaunchKernelGGL(chunk_fsmn_kernel, dim3(a.T, a.B), dim3(256), 0, stream, a, g);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_gather_rows_or_zero(const float* src, int ld, int n_src, const int* idx, float* out, int n, int D, hipStream_t stream) {
    PF_REQUIRE(src && idx && out && n > 0 && n_src > 0 && D > 0 && D % 4 == 0 && ld % 4 == 0 && ld >= D && ((uintptr_t)src & 15) == 0 &&
                   ((uintptr_t)out & 15) == 0,
               "gather_rows_or_zero: D and ld multiples of 4, 16-B aligned rows");
    const size_t total = (size_t)n * (D / 4);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(gather_rows_or_zero_kernel, dim3(blocks), dim3(256), 0, stream, src, ld, n_src, idx, out, n, D / 4);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_stride_conv(const float* a, int Da, const float* b, int Db, int T, const float* w, const float* bias, int Cout, int taps,
                       int stride, int pad_left, int Tout, float* out, hipStream_t stream) {
    PF_REQUIRE(a && b && w && bias && out && Da > 0 && Db > 0 && T > 0 && Cout > 0 && taps >= 1 && taps <= 8 && stride >= 1 && pad_left >= 0 &&
                   Tout > 0 && Tout <= 65535 * 32,
               "stride_conv: 1 .. 8 taps, stride >= 1, pad_left >= 0");
    const size_t lds = sizeof(float) * (size_t)taps * (Da + Db);
    PF_REQUIRE(lds <= 48 * 1024, "stride_conv: taps * (Da + Db) floats must fit 48 KiB of LDS");
    hipLaunchKernelGGL(stride_conv_kernel, dim3(Tout), dim3(256), lds, stream, a, Da, b, Db, T, w, bias, Cout, taps, stride, pad_left, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_scama_attention(const float* q, const float* K, const float* V, int ldkv, int nk, const float* mask, int lo, int hi, int n,
                           int H, int dk, float* out, hipStream_t stream) {
    PF_REQUIRE(q && K && V && out && n > 0 && n <= 65535 && H > 0 && H <= 65535 && nk > 0 && nk <= 12000 && (dk == 64 || dk == 128) &&
                   ldkv % 4 == 0 && ldkv >= H * dk && ((uintptr_t)K & 15) == 0,
               "scama_attention: head dim 64 or 128, 1 .. 12000 keys, 16-B aligned rows");
    PF_REQUIRE(lo >= 0 && lo <= hi && hi <= nk, "scama_attention: key window outside 0 <= lo <= hi <= T");
    const size_t lds = sizeof(float) * (size_t)(hi - lo > 0 ? hi - lo : 1);
    if (dk == 64)
        hipLaunchKernelGGL(scama_attention_kernel<64>, dim3(n, H), dim3(64), lds, stream, q, K, V, ldkv, mask, lo, hi, H * dk, out);
    else
        hipLaunchKernelGGL(scama_attention_kernel<128>, dim3(n, H), dim3(64), lds, stream, q, K, V, ldkv, mask, lo, hi, H * dk, out);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
