// Transducer (RNN-T) search kernels: the work of ONE expansion of funasr/models/transducer/beam_search_transducer.py's
// default_beam_search. A step is a few hundred kilobytes of weights against one vector: bandwidth- and latency-bound, no matrix-core
// work, and the search's decisions must not depend on an operand split -- so everything here is plain fp32 on the VALU with 16-byte
// loads and reductions of a fixed order (per lane in index order, then the xor butterfly of wave_sum): the same inputs give the same
// bits on every call.
//
//   rnnt_cell_kernel         one LSTM layer for one vector; one wave per hidden unit (its four gate rows). Layer l + 1 reads h' of
//                            layer l, so layers are separate launches and the stream order is the synchronisation.
//   rnnt_matvec_kernel       dec_proj = lin_dec.weight . h' (no bias), written next to the state, so the joint never touches lin_dec.
//   rnnt_joint_pass1_kernel  the grid splits lin_out's rows, RNNT_ROWS per workgroup; every workgroup rebuilds
//                            z = tanh(enc_proj + dec_proj) in LDS, computes its logits and leaves a partial record: max,
//                            sum exp(x - max), the blank logit (row 0, from the workgroup that owns it) and its k best (value, row)
//                            among rows >= 1, best first, equal values by lower row.
//   rnnt_joint_pass2_kernel  one wave merges the partials: the maximum, the sum (lane-strided in workgroup order, then the
//                            butterfly), and a k-round merge of the sorted lists under the same order.
// The two passes stay two launches: the launch boundary is the only inter-workgroup hand-off.
#include <limits.h>
#include <stdint.h>

#include "common.h"
#include "transducer.h"

namespace pf {

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// sum_q w[q] . x[q] over this lane's float4 columns q = lane, lane + 64, ... (index order)
__device__ __forceinline__ float lane_dot(const float4* __restrict__ w, const float4* __restrict__ x, int n4, int lane) {
    float acc = 0.f;
    for (int q = lane; q < n4; q += 64) {
        const float4 a = w[q], b = x[q];
        acc = fmaf(a.x, b.x, acc);
        acc = fmaf(a.y, b.y, acc);
        acc = fmaf(a.z, b.z, acc);
        acc = fmaf(a.w, b.w, acc);
    }
    return acc;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// (v, i) comes before (w, j): larger value first, equal values by lower row
__device__ __forceinline__ bool rnnt_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

__global__ __launch_bounds__(256) void rnnt_cell_kernel(RnntCellArgs a) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.H) return;                                          // wave-uniform
    const float4* x4 = reinterpret_cast<const float4*>(a.x);
    const float4* h4 = reinterpret_cast<const float4*>(a.h_prev);
    const int in4 = a.in_dim >> 2, H4 = a.H >> 2;
    float gate[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const size_t row = (size_t)g * a.H + j;
        const float si = wave_sum(lane_dot(reinterpret_cast<const float4*>(a.w_ih + row * a.in_dim), x4, in4, lane));
        const float sh = wave_sum(lane_dot(reinterpret_cast<const float4*>(a.w_hh + row * a.H), h4, H4, lane));
        gate[g] = (si + a.b_ih[row]) + (sh + a.b_hh[row]);
    }
    if (lane == 0) {
        const float c = sigmoidf(gate[1]) * a.c_prev[j] + sigmoidf(gate[0]) * tanhf(gate[2]);
        a.c_out[j] = c;
        a.h_out[j] = sigmoidf(gate[3]) * tanhf(c);
    }
}

__global__ __launch_bounds__(256) void rnnt_matvec_kernel(const float* __restrict__ W, const float* __restrict__ x, float* __restrict__ y,
                                                          int rows, int cols) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                         // wave-uniform
    const float s = wave_sum(lane_dot(reinterpret_cast<const float4*>(W + (size_t)r * cols), reinterpret_cast<const float4*>(x), cols >> 2, lane));
    if (lane == 0) y[r] = s;
}

__global__ __launch_bounds__(256) void rnnt_joint_pass1_kernel(RnntJointArgs a) {
    __shared__ __attribute__((aligned(16))) float z[RNNT_MAX_DIM];
    __shared__ float logit[RNNT_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < a.J; j += 256) z[j] = tanhf(a.enc_proj[j] + a.dec_proj[j]);
    __syncthreads();
    const int r0 = blockIdx.x * RNNT_ROWS;
    const int nrows = min(RNNT_ROWS, a.V - r0);                    // >= 1 by the grid
    const int J4 = a.J >> 2;
    for (int i = wave; i < nrows; i += 4) {                        // wave-uniform
        const float s = wave_sum(lane_dot(reinterpret_cast<const float4*>(a.w_out + (size_t)(r0 + i) * a.J),
                                          reinterpret_cast<const float4*>(z), J4, lane));
        if (lane == 0) logit[i] = s + a.b_out[r0 + i];
    }
    __syncthreads();
    if (wave != 0) return;
    // one wave: lane i < nrows holds row r0 + i (RNNT_ROWS <= 64)
    const int k = a.k;
    const bool have = lane < nrows;
    const float x = have ? logit[lane] : -INFINITY;
    const float m = wave_max(x);
    const float s = wave_sum(have ? expf(x - m) : 0.f);
    const int first = r0 == 0 ? 1 : 0;                             // row 0 is the blank: never a candidate
    const int ncand = nrows - first;
    const bool cand = have && lane >= first;
    int rank = 0;                                                  // a bijection onto 0 .. ncand - 1: the order is strict
    if (cand)
        for (int o = first; o < nrows; ++o)
            if (o != lane && rnnt_before(logit[o], o, x, lane)) ++rank;
    float* P = a.partials + (size_t)blockIdx.x * (4 + 2 * k);
    int* Pi = reinterpret_cast<int*>(P);
    if (lane == 0) {
        P[0] = m;
        P[1] = s;
        P[2] = r0 == 0 ? logit[0] : 0.f;
        P[3] = 0.f;
    }
    if (cand && rank < k) {
        P[4 + rank] = x;
        Pi[4 + k + rank] = r0 + lane;
    }
    if (lane >= ncand && lane < k) {                               // fewer candidates than k: the rest of the list is empty
        P[4 + lane] = -INFINITY;
        Pi[4 + k + lane] = INT_MAX;
    }
}

constexpr int RNNT_MAX_BLOCKS = 2048;                              // workgroups of pass 1 that pass 2 keeps a list head for

__global__ __launch_bounds__(64) void rnnt_joint_pass2_kernel(RnntJointArgs a, int NB) {
    __shared__ unsigned char head[RNNT_MAX_BLOCKS];                // entries of list b already taken; touched by the owning lane only
    const int lane = threadIdx.x, k = a.k, stride = 4 + 2 * k;
    const float* P = a.partials;
    float m = -INFINITY;
    for (int b = lane; b < NB; b += 64) m = fmaxf(m, P[(size_t)b * stride]);
    const float M = wave_max(m);
    float s = 0.f;
    for (int b = lane; b < NB; b += 64) s += P[(size_t)b * stride + 1] * expf(P[(size_t)b * stride] - M);
    const float logS = logf(wave_sum(s));
    if (lane == 0) a.record[0] = (P[2] - M) - logS;
    for (int b = lane; b < NB; b += 64) head[b] = 0;
    float bv = -INFINITY;                                          // this lane's best head over its lists b = lane, lane + 64, ...
    int bi = INT_MAX, bl = -1;
    for (int b = lane; b < NB; b += 64) {
        const float v = P[(size_t)b * stride + 4];
        const int i = reinterpret_cast<const int*>(P)[(size_t)b * stride + 4 + k];
        if (bl < 0 || rnnt_before(v, i, bv, bi)) { bv = v; bi = i; bl = b; }
    }
    for (int r = 0; r < k; ++r) {
        float wv = bv;
        int wi = bi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(wv, o, 64);
            const int oi = __shfl_xor(wi, o, 64);
            if (rnnt_before(ov, oi, wv, wi)) { wv = ov; wi = oi; }
        }
        wv = __shfl(wv, 0, 64);                                    // one winner for every lane, whatever the values are
        wi = __shfl(wi, 0, 64);
        if (lane == 0) {
            a.record[1 + r] = (wv - M) - logS;
            reinterpret_cast<int*>(a.record)[1 + k + r] = wi;
        }
        if (bl >= 0 && bi == wi && wi != INT_MAX) {                // the owner takes the entry and looks at its lists again
            head[bl] = (unsigned char)(head[bl] + 1);
            bv = -INFINITY; bi = INT_MAX; bl = -1;
            for (int b = lane; b < NB; b += 64) {
                const int hd = head[b];
                if (hd >= k) continue;
                const float v = P[(size_t)b * stride + 4 + hd];
                const int i = reinterpret_cast<const int*>(P)[(size_t)b * stride + 4 + k + hd];
                if (bl < 0 || rnnt_before(v, i, bv, bi)) { bv = v; bi = i; bl = b; }
            }
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool dim_ok(int d) { return d >= 4 && d % 4 == 0 && d <= RNNT_MAX_DIM; }

}  // namespace

int launch_rnnt_cell(const RnntCellArgs& a, hipStream_t stream) {
    PF_REQUIRE(dim_ok(a.in_dim) && dim_ok(a.H), "rnnt_cell: sizes must be multiples of 4, at most 1024");
    PF_REQUIRE(a.x && a.w_ih && a.w_hh && a.b_ih && a.b_hh && a.h_prev && a.c_prev && a.h_out && a.c_out, "rnnt_cell: null");
    PF_REQUIRE(aligned16(a.x) && aligned16(a.w_ih) && aligned16(a.w_hh) && aligned16(a.h_prev), "rnnt_cell: operands must be 16-B aligned");
    PF_REQUIRE(a.h_out != a.h_prev && a.c_out != a.c_prev, "rnnt_cell: the step must write another slot than it reads");
    hipLaunchKernelGGL(rnnt_cell_kernel, dim3(ceil_div(a.H, 4)), dim3(256), 0, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rnnt_matvec(const float* W, const float* x, float* y, int rows, int cols, hipStream_t stream) {
    PF_REQUIRE(W && x && y && rows > 0 && dim_ok(cols), "rnnt_matvec: null, or a row length that is no multiple of 4 / above 1024");
    PF_REQUIRE(aligned16(W) && aligned16(x), "rnnt_matvec: operands must be 16-B aligned");
    hipLaunchKernelGGL(rnnt_matvec_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, stream, W, x, y, rows, cols);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rnnt_joint_topk(const RnntJointArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.enc_proj && a.dec_proj && a.w_out && a.b_out && a.partials && a.record, "rnnt_joint: null");
    PF_REQUIRE(dim_ok(a.J), "rnnt_joint: joint_space_size must be a multiple of 4, at most 1024");
    PF_REQUIRE(a.V >= 2 && a.V <= RNNT_MAX_BLOCKS * RNNT_ROWS, "rnnt_joint: vocabulary of 2 .. 65536 rows");
    PF_REQUIRE(a.k >= 1 && a.k <= RNNT_MAX_K && a.k <= a.V - 1, "rnnt_joint: k must be 1 .. min(16, V - 1)");
    PF_REQUIRE(aligned16(a.w_out), "rnnt_joint: lin_out.weight must be 16-B aligned");
    const int NB = rnnt_joint_blocks(a.V);
    hipLaunchKernelGGL(rnnt_joint_pass1_kernel, dim3(NB), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(rnnt_joint_pass2_kernel, dim3(1), dim3(64), 0, stream, a, NB);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
