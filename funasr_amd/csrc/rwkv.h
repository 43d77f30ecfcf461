// Kernel argument blocks and launchers of the RWKV encoder's row kernels and WKV scan (rwkv.hip, engine_rwkv.hip).
// Activations are [B, T, D] rows with per-clip lengths (device int32 [B]); a row at or past its clip's length is written as zeros by
// every kernel here and never read as data. D is a multiple of 4, every operand base 16-byte aligned, every stride a multiple of 4.
#pragma once
#include "common.h"

namespace pf {

constexpr int RWKV_CHUNK = 32;       // frames per WKV chunk: fixed, so a clip's chunk boundaries never depend on T or B
constexpr int RWKV_MAX_D = 1024;     // a row of the LayerNorm kernels lives in one wave's registers (64 lanes x 4 float4)

// Y[row, j D + c] = y[c] mu_j[c] + y_prev[c] (1 - mu_j[c]) for j < n_out (2 or 3), y = LayerNorm(X[row]) and y_prev = LayerNorm of the
// row before it in the same clip, zero at the clip's frame 0 (never the previous clip's last row). One wave per row; LN(t - 1) is
// recomputed, nothing normed is staged through memory.
struct RwkvMixArgs {
    const float* X; int ldx;
    const float* gamma; const float* beta; float eps;
    const float* mix[3]; int n_out;
    float* Y; int ldy;
    const int* lens; int B, T, D;
};
int launch_rwkv_mix(const RwkvMixArgs& a, hipStream_t stream);

// Y[b, j] = LayerNorm(X[b, j step]) for j < To, live while j step < lens[b] (embed_norm: step 1; final_norm over the rows that
// survive x[:, ::step])
int launch_rwkv_norm(const float* X, int ldx, const float* gamma, const float* beta, float eps, float* Y, int ldy, const int* lens,
                     int B, int T, int step, int To, int D, hipStream_t stream);

// out[row, c] = sigmoid(r[row, c]) wkv[row, c] with the reference's recurrence per channel c (rwkv_attention.py:421-462), w = -exp(time_decay),
// u = time_first, state (num, den, m) = (0, 0, -1e-30) at a clip's frame 0:
//   mo = max(m, u + k); wkv = (e^(m - mo) num + e^(u + k - mo) v) / (e^(m - mo) den + e^(u + k - mo))
//   ms = max(k, m + w); (num, den, m) <- (e^(m + w - ms) num + e^(k - ms) v, e^(m + w - ms) den + e^(k - ms), ms)
// Chunked over time, lane = channel, two launches, no atomics:
//   1. every chunk [c L, c L + L) that has a successor in its clip is summarised from the empty state (0, 0, -1e38) into
//      sum [B, ceil(T / L), 3, D];
//   2. chunk c folds the summaries 0 .. c - 1 in order into its carry -- carry <- combine(carry decayed by w L, summary), the same max
//      trick -- starting from the reference's initial state, re-runs its frames from the carry and writes the outputs.
// The recurrence is linear in (num e^m, den e^m), so this is the sequential scan up to fp32 rounding; a frame's bits depend on its
// clip's earlier frames only.
struct RwkvWkvArgs {
    const float* k; const float* v; const float* r; int ld;
    const float* w; const float* u;
    const int* lens; int B, T, D;
    float* out; int ldo;
    float* sum;
};
static inline size_t rwkv_wkv_scratch_floats(int B, int T, int D) { return (size_t)B * ceil_div(T, RWKV_CHUNK) * 3 * D; }
int launch_rwkv_wkv(const RwkvWkvArgs& a, hipStream_t stream);

// in place: h <- relu(h)^2 over [B T, N] rows of stride ld
int launch_rwkv_sqrelu(float* h, int ld, const int* lens, int B, int T, int N, hipStream_t stream);
// x_out = x + sigmoid(r) val over [B T, D] rows (x_out may be x)
int launch_rwkv_gate(const float* x, int ldx, const float* r, int ldr, const float* val, int ldv, float* x_out, int ldo, const int* lens,
                     int B, int T, int D, hipStream_t stream);

}  // namespace pf
