// Kernel launchers of the chunk Conformer encoder (funasr/models/conformer/encoder.py ConformerChunkEncoder; chunk_conformer.hip,
// driven by engine_chunk_conformer.hip). Activations are rows of a [B * T, D] buffer, T = the batch's encoder length. Every kernel
// computes a row in a fixed order and without atomics.
#pragma once
#include "common.h"

namespace pf {

// The visible keys of query i (make_chunk_mask, nets_utils.py:614, and the source mask): [start_i, end_i) with
//   chunk > 0:  start_i = left < 0 ? 0 : max((i / chunk - left) * chunk, 0),  end_i = min((i / chunk + 1) * chunk, T)
//   chunk == 0: start_i = 0, end_i = T
// and end_i = min(end_i, klen). Both ends grow with i, so the union of the windows of rows [a, b] is [start_a, end_b).
__host__ __device__ inline void cc_window(int i, int T, int chunk, int left, int klen, int* start, int* end) {
    int s = 0, e = T;
    if (chunk > 0) {
        const int ci = i / chunk;
        s = (left < 0 || left >= ci) ? 0 : (ci - left) * chunk;
        e = (ci + 1) * chunk < T ? (ci + 1) * chunk : T;
    }
    *start = s;
    *end = e < klen ? e : klen;
}

// Chunk-window relative-position self-attention (RelPositionMultiHeadedAttentionChunk), head dim 64, flash-style in exact fp32 on the
// matrix cores: launch_cf_relpos_attention's "latest" form (qkv [B * T, 3 D], P [2 T - 1, D], u, v [H, 64];
// score(i, j) = ((q_i + u) . k_j + (q_i + v) . P[T - 1 - i + j]) / 8) where query i sees the keys of cc_window(i, T, chunk, left,
// klens[b]) only. A workgroup of 128 queries walks the 32-key tiles that meet the union of its rows' windows and masks inside them;
// a wave skips the tiles none of its 32 queries sees. K / V rows outside the workgroup's union and P rows outside
// [T - 1 - q_last + start, T - 1 - q_first + end - 1] of a wave are never read. A row without a visible key is written as zeros.
// chunk == 0 (no chunk mask) is handed to launch_cf_relpos_attention: the same tiles and sums without the window logic.
int launch_cc_window_attention(const float* qkv, const float* P, const float* u, const float* v, const int* klens, int B, int T, int H,
                               int chunk, int left, float* out, hipStream_t stream);

// launch_cf_glu_dw with the choice of CausalConvolution: causal != 0 pads taps - 1 zero rows before each sequence and none behind
// (row t reads rows t - taps + 1 .. t), causal == 0 pads taps / 2 on either side. g [B * T, 2 D] (value | gate) -> GLU -> depthwise
// Conv1d + bias -> y * bn_scale + bn_shift -> Swish -> y [B * T, D]. dw [D][taps], taps odd <= 31, D % 64 == 0.
int launch_cc_glu_dw(const float* g, const float* dw, const float* dw_bias, const float* bn_scale, const float* bn_shift, int B, int T,
                     int D, int taps, int causal, float* y, hipStream_t stream);

// First conv of StreamingConvInput: Conv2d(1 -> C, 3 x 3, stride 2, padding [1, 0]) + ReLU over feats [B, L, F] cut into NC pieces of
// LC frames per clip (frames at or past L read as zero; NC = 1, LC = L: the whole clip), each piece convolved on its own (the time
// padding falls at every piece's edges) -> y [B * NC, T1 = (LC - 1) / 2 + 1, F1 = (F - 3) / 2 + 1, C] channels-last. w [C, 9]
// (tap = dt * 3 + df). 3 <= F <= 256.
int launch_cc_conv0(const float* feats, int B, int L, int F, int NC, int LC, const float* w, const float* bias, int C, float* y,
                    hipStream_t stream);

// The operand of the second conv as a matrix: rows [r0, r0 + nrows) of the [NP * T2 * F2, k * k * C] im2col of x [NP, T1, F1, C]
// for Conv2d(C -> C, k, stride s, padding [(k - 1) / 2, 0]); column (kt * k + kf) * C + c of row (p, t, f) is
// x[p, t * s + kt - (k - 1) / 2, f * s + kf, c], zero outside [0, T1). T2 = (T1 - 1) / s + 1, F2 = (F1 - k) / s + 1. C % 4 == 0.
int launch_cc_im2col(const float* x, int NP, int T1, int F1, int C, int k, int s, long long r0, int nrows, float* a, hipStream_t stream);

// y[b * To + t] = x[b * Ti + t * step] for t < To (rows of D floats, D % 4 == 0): the cut of the chunked front's rows to the batch's
// encoder length (step 1) and x[:, ::time_reduction_factor] (Ti = T, step = the factor)
int launch_cc_copy_rows(const float* x, int Ti, int step, float* y, int B, int To, int D, hipStream_t stream);

}  // namespace pf
