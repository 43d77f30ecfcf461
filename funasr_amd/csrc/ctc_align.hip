// Batched CTC forced alignment on the device (ctc_align.h): a parallel gather of the emissions the recurrence reads, then one workgroup
// per clip for the Viterbi recurrence and the back-trace. Plain C++ on 64-wide waves, LDS between the four waves, vector stores only.
//
// The arithmetic is that of `ctc_forced_align` (funasr/models/sense_voice/utils/ctc_alignment.py:2-77) with 0-based states and no pad:
//   ext = [blank, y1, blank, y2, ..., blank] (S = 2 L + 1), diff[s] = s >= 2 && ext[s] != ext[s - 2]
//   best_0[0] = e(0, blank), best_0[1] = e(0, y1), -inf elsewhere
//   best_t[s] = e(t, ext[s]) + max(best[s], best[s - 1], diff[s] ? best[s - 2] : -inf)      one fp32 add; the FIRST maximum in that
//   back_t[s] = which of the three it was (all three -inf: 0)                                 order (strict > when replacing)
//   path[T - 1] = 2 L - 1 + (best[2 L] > best[2 L - 1]), path[t - 1] = path[t] - back_t[path[t]], label = ext[path]
#include "ctc_align.h"

namespace pf {
namespace {

constexpr int CA_MAX_S = 2 * CTC_ALIGN_MAX_L + 1;
constexpr int CA_SLOTS = (CA_MAX_S + 255) / 256;         // states per thread: state tid + 256 k
constexpr int CA_TRACE = 32;                             // frames per back-trace trip: the path moves down by <= 2 states per frame,
constexpr int CA_WINDOW = 64;                            // so a trip's back-pointers lie in a window of 2 * 31 + 1 = 63 states

// ------------------------------------------------------------------------------------------------ gather
// dense[b, t, 0] = e(t, blank), dense[b, t, 1 + l] = e(t, y_l): one wave per frame, four frames per workgroup. The scattered reads
// into the V-wide rows happen here, in parallel over frames, so the sequential loop below reads L + 1 contiguous floats per frame.
__global__ __launch_bounds__(256) void ctc_align_gather_kernel(const CtcAlignArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int Tb = a.lens[b], Lb = a.lens[a.B + b];
    if (t >= Tb) return;
    const size_t row = (size_t)b * a.T + a.t0 + t;
    const float* xr = a.emis + row * (size_t)a.ld;
    const float lse = a.lse ? a.lse[row] : 0.f;
    const bool blank_is_zero = a.pred && a.pred[row] == a.blank;
    const int* tg = a.targets + (size_t)b * a.ldt;
    float* d = a.dense + ((size_t)b * a.T_max + t) * (a.L_max + 1);
    for (int j = lane; j <= Lb; j += 64) {
        const int c = j == 0 ? a.blank : tg[j - 1];
        float v = -INFINITY;
        if (c >= 0 && c < a.V) {
            v = xr[c];
            if (a.lse) v = v - lse;
        }
        if (blank_is_zero && c == a.blank) v = 0.f;
        d[j] = v;
    }
}

// ------------------------------------------------------------------------------------- recurrence + back-trace
// One workgroup per clip. best is double-buffered in LDS behind two -inf pad entries (states -2 and -1), so a frame costs three LDS
// reads, one add, one LDS write and one barrier; frame t + 1's emissions are loaded before frame t's barrier. The back-trace goes in
// trips of CA_TRACE frames: all threads stage the window of back-pointers the trip can touch in LDS, one lane walks it, all threads
// write the trip's labels.
__global__ __launch_bounds__(256) void ctc_align_viterbi_kernel(const CtcAlignArgs a) {
    __shared__ float best[2][2 + CA_SLOTS * 256];
    __shared__ unsigned char win[CA_TRACE][CA_WINDOW];
    __shared__ int trip_state[CA_TRACE];
    __shared__ int next_state;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Tb = a.lens[b], Lb = a.lens[a.B + b];
    int* out = a.labels + (size_t)b * a.T_out;
    for (int t = (Tb < 0 ? 0 : Tb) + tid; t < a.T_out; t += 256) out[t] = -1;
    if (Tb <= 0) return;
    const int S = 2 * Lb + 1, nk = (S + 255) >> 8;
    const int dl = a.L_max + 1, sm = 2 * a.L_max + 1;
    const int* tg = a.targets + (size_t)b * a.ldt;
    const float* d = a.dense + (size_t)b * a.T_max * dl;
    unsigned char* bk = a.back + (size_t)b * a.T_max * sm;

    int col[CA_SLOTS];                                           // column of `dense` that holds state s's emission
    float e[CA_SLOTS];
    unsigned diff = 0;
#pragma unroll
    for (int k = 0; k < CA_SLOTS; ++k) {
        const int s = tid + 256 * k;
        col[k] = (s & 1) ? 1 + (s >> 1) : 0;
        e[k] = 0.f;
        if (k < nk && s < S) {
            if ((s & 1) && s >= 3 && tg[s >> 1] != tg[(s >> 1) - 1]) diff |= 1u << k;     // even states: blank on both sides, never
            best[0][2 + s] = s == 0 ? d[0] : (s == 1 ? d[1] : -INFINITY);
            if (Tb > 1) e[k] = d[dl + col[k]];
        }
    }
    if (tid < 2) { best[0][tid] = -INFINITY; best[1][tid] = -INFINITY; }
    __syncthreads();

    for (int t = 1; t < Tb; ++t) {
        const float* src = best[(t - 1) & 1];
        float* dst = best[t & 1];
        const bool more = t + 1 < Tb;
        const float* dn = d + (size_t)(t + 1) * dl;
        unsigned char* bt = bk + (size_t)t * sm;
#pragma unroll
        for (int k = 0; k < CA_SLOTS; ++k) {
            const int s = tid + 256 * k;
            if (k < nk && s < S) {
                const float en = more ? dn[col[k]] : 0.f;
                float m = src[2 + s];
                int idx = 0;
                const float m1 = src[1 + s], m2 = ((diff >> k) & 1u) ? src[s] : -INFINITY;
                if (m1 > m) { m = m1; idx = 1; }
                if (m2 > m) { m = m2; idx = 2; }
                dst[2 + s] = e[k] + m;
                bt[s] = (unsigned char)idx;
                e[k] = en;
            }
        }
        __syncthreads();                                         // (also orders this frame's back-pointer stores for the trace below)
    }

    if (tid == 0) {
        const float* fin = best[(Tb - 1) & 1];
        next_state = 2 * Lb - 1 + (fin[2 + 2 * Lb] > fin[2 + 2 * Lb - 1] ? 1 : 0);
    }
    __syncthreads();
    for (int top = Tb - 1; top >= 0; top -= CA_TRACE) {
        const int p = next_state;                                // the path's state at frame `top`
        const int n = top + 1 < CA_TRACE ? top + 1 : CA_TRACE;   // this trip: frames top, top - 1, ..., top - n + 1
        const int lo = p - (CA_WINDOW - 2) > 0 ? p - (CA_WINDOW - 2) : 0;
        for (int i = tid; i < n * CA_WINDOW; i += 256) {
            const int f = i / CA_WINDOW, s = lo + i % CA_WINDOW, t = top - f;
            win[f][i % CA_WINDOW] = (s <= p && t >= 1) ? bk[(size_t)t * sm + s] : (unsigned char)0;       // frame 0 has no step below it
        }
        __syncthreads();
        if (tid == 0) {
            int cur = p;
            for (int f = 0; f < n; ++f) {
                trip_state[f] = cur;
                cur -= win[f][cur - lo];
            }
            next_state = cur;
        }
        __syncthreads();
        if (tid < n) {
            const int st = trip_state[tid];
            out[top - tid] = (st & 1) ? tg[st >> 1] : a.blank;
        }
    }
}

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace

size_t ctc_align_lens_bytes(int B) { return round256(sizeof(int) * 2 * (size_t)B); }
size_t ctc_align_dense_bytes(int B, int T_max, int L_max) { return round256(sizeof(float) * (size_t)B * T_max * (L_max + 1)); }
size_t ctc_align_back_bytes(int B, int T_max, int L_max) { return (size_t)B * T_max * (2 * (size_t)L_max + 1); }

int launch_ctc_align(const CtcAlignArgs& a, hipStream_t stream) {
    PF_REQUIRE(a.emis && a.targets && a.lens && a.dense && a.back && a.labels, "ctc_align: null operand");
    PF_REQUIRE(a.B > 0 && a.B <= 65535 && a.T > 0 && a.V > 0 && a.ld >= a.V && a.t0 >= 0 && a.t0 <= a.T && a.ldt > 0 && a.T_out > 0,
               "ctc_align: bad shape");
    PF_REQUIRE(a.blank >= 0 && a.blank < a.V, "ctc_align: blank outside the vocabulary");
    PF_REQUIRE(a.T_max >= 0 && a.T_max <= CTC_ALIGN_MAX_T && a.T_max <= a.T - a.t0 && a.T_max <= a.T_out,
               "ctc_align: more than 4096 frames, or more than the emissions / the output hold");
    PF_REQUIRE(a.L_max >= 1 && a.L_max <= CTC_ALIGN_MAX_L && a.L_max <= a.ldt, "ctc_align: no target labels, more than 1024, or more than a row of `targets`");
    if (a.T_max > 0) {
        hipLaunchKernelGGL(ctc_align_gather_kernel, dim3((unsigned)ceil_div(a.T_max, 4), (unsigned)a.B), dim3(256), 0, stream, a);
        PF_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(ctc_align_viterbi_kernel, dim3((unsigned)a.B), dim3(256), 0, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace pf
