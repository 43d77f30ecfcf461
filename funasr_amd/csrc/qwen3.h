// Kernel argument blocks and launchers of the Qwen3 causal LM decoder (qwen3.hip, engine_qwen3.hip): RMSNorm, per-head q/k RMSNorm +
// rotary embedding with the KV-cache write, causal grouped-query attention for prefill, key-split attention for the decode step, SwiGLU.
// fp32 throughout. Activations are rows [M, width]; every operand base is 16-byte aligned and every row stride a multiple of 4 floats.
//
// KV cache of ONE layer: K and V each [slots][Hkv][cap][hd] (slot = sequence of the batch, cap = positions the cache holds). A row of
// the cache at or past a sequence's length is never read by any kernel here.
#pragma once
#include "common.h"

namespace pf {

constexpr int Q3_PAIRS = 16;      // (query row, query head) pairs one workgroup carries in registers: 4 waves x 4
constexpr int Q3_KSPLIT = 256;    // keys per workgroup of the decode step's attention (a multiple of both key tiles)
// query rows per workgroup of the prefill attention: all G = Hq / Hkv heads of a K/V head ride in one workgroup, so K/V are staged
// once per group
static inline int q3_qtile(int G) { return G >= Q3_PAIRS ? 1 : Q3_PAIRS / G; }
// keys per LDS tile: lane = (half of head_dim, key), 64 lanes
static inline int q3_ktile(int hd) { return hd == 64 ? 64 : 32; }
static inline bool q3_head_dim_ok(int hd) { return hd == 64 || hd == 128; }

// y[row] = x[row] * (1 / sqrt(mean(x[row]^2) + eps)) * w over D columns (D % 4 == 0); one wave per row. y may be x.
int launch_q3_rmsnorm(const float* x, int ldx, const float* w, float eps, float* y, int ldy, int M, int D, hipStream_t stream);

// Row r of qkv = [q heads | k heads | v heads] (Hq + 2 Hkv heads of hd columns) belongs to cache slot row_seq[r] at position row_pos[r].
// q and k heads: RMSNorm over hd (weights qw / kw), then x cos + rotate_half(x) sin with cos / sin rows of the table [positions, hd / 2].
// Rotated q -> q_out [M, Hq hd]; rotated k and plain v -> the cache row (slot, head, position). One wave per (row, head).
struct Q3RopeArgs {
    const float* qkv; int ld;
    const float* qw; const float* kw; float eps;
    const float* cos_t; const float* sin_t;
    const int* row_seq; const int* row_pos;      // device int32 [M]
    float* q_out; int ldq;
    float* kc; float* vc; int cap;
    int M, Hq, Hkv, hd;
};
int launch_q3_qk_rope(const Q3RopeArgs& a, hipStream_t stream);

// Prefill: sequence i of the launch owns rows [row0[i], row0[i] + nrows[i]) of q / out, its row j sits at position p0[i] + j of cache
// slot seq[i] and attends to cache rows 0 .. p0[i] + j. Online softmax over key tiles, fp32.
struct Q3PrefillArgs {
    const float* q; int ldq;
    const float* kc; const float* vc; int cap;
    float* out; int ldo;
    const int* seq; const int* row0; const int* nrows; const int* p0;      // device int32 [nseq]
    int nseq, max_rows;                                                      // max_rows >= every nrows[i] (sizes the grid)
    int Hq, Hkv, hd;
    float scale;
};
int launch_q3_prefill_attention(const Q3PrefillArgs& a, hipStream_t stream);

// Decode step: row r (one query per sequence) attends to rows 0 .. row_len[r] - 1 of cache slot row_seq[r]. Workgroup (split, K/V head,
// row) covers keys [split KSPLIT, ..) and leaves (o, m, l) in part [M][Hq][nsplit][hd + 2]; a second launch merges a row's splits.
struct Q3DecodeArgs {
    const float* q; int ldq;
    const float* kc; const float* vc; int cap;
    float* out; int ldo;
    const int* row_seq; const int* row_len;      // device int32 [M]
    int M, max_len;                              // max_len >= every row_len[r] (sizes the grid)
    int Hq, Hkv, hd;
    float scale;
    float* part;                                 // q3_decode_part_floats() floats
};
static inline size_t q3_decode_part_floats(int M, int Hq, int hd, int max_len) {
    return (size_t)M * Hq * ceil_div(max_len, Q3_KSPLIT) * (hd + 2);
}
int launch_q3_decode_attention(const Q3DecodeArgs& a, hipStream_t stream);

// out[row, c] = silu(gu[row, c]) * gu[row, I + c] over I columns (I % 4 == 0): the output of one fused gate | up GEMM
int launch_q3_swiglu(const float* gu, int ld, float* out, int ldo, int M, int I, hipStream_t stream);

}  // namespace pf
