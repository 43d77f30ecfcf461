// Kernel launchers of the UniASR two-pass model (uniasr.hip; driven by engine_uniasr.hip, engine_encoder.hip and engine_conformer.hip):
// the chunk-masked SAN-M attention and FSMN memory of the offline chunked encoder (SANMEncoderChunkOpt.forward with `ind`), the row
// gathers of split_chunk / remove_chunk, the two-source strided conv1d of `stride_conv`, and the masked few-query cross-attention of
// the SCAMA decoder step. Plain fp32 FMAs, every row in a fixed order, no atomics.
#pragma once
#include "common.h"

namespace pf {

// The chunked layout of overlap_chunk (scama/chunk_utilis.py): row r of a sequence belongs to chunk r / period (period = chunk +
// shift); its first `shift` rows are the FSMN shift rows (zero input, masked everywhere), the next `chunk` rows the chunk's frames.
// chunk == 0: no chunk mask.
struct ChunkGeom {
    int chunk, stride, shift, look_back;
};

// mask_att_chunk_encoder without the [Tc, Tc] matrix: query row r = c * period + shift + j (0 <= j < chunk) sees
//   * its own chunk, keys [c period + shift, c period + shift + chunk), and
//   * when j < stride, the first `stride` frames of each of the `look_back` chunks before it: keys c' period + shift + [0, stride)
//     for max(c - look_back, 0) <= c' < c,
// both below klens[b]; a shift row (j < 0) sees nothing and its output row is zero (the reference's softmax over an all-masked
// row is zeroed by its second masked_fill). No key outside those sets is read. Q / K / V / O as AttnArgs (one source), head h at
// column h dk, dk % 4 == 0 and <= 128.
int launch_chunk_attention(const AttnArgs& a, int dk, const ChunkGeom& g, hipStream_t stream);

// FSMN memory block under mask_shfit_chunk: m(t) = t < lens[b] and t % period >= shift;
//   out[t] = m(t) * (x_m[t] + sum_k w[c][k] x_m[t - left_pad + k]),  x_m[t] = m(t) * in[t]   (FsmnArgs without R / offs / bf16)
int launch_chunk_fsmn(const FsmnArgs& a, const ChunkGeom& g, hipStream_t stream);

// out[r] = idx[r] >= 0 ? src[idx[r]] : 0 for r < n (rows of D floats, D % 4 == 0; src rows `ld` floats apart, n_src of them; every
// index is checked against n_src on the device and an index past it reads as a zero row)
int launch_gather_rows_or_zero(const float* src, int ld, int n_src, const int* idx, float* out, int n, int D, hipStream_t stream);

// Conv1dSubsampling over the concatenation [a | b] along the features WITHOUT writing the concatenation:
//   out[t][co] = relu(bias[co] + sum_{k < taps} sum_{ci < Da + Db} w[co][ci][k] * x[t * stride + k - pad_left][ci]),
//   x[u] = [a[u] | b[u]] for 0 <= u < T, zero outside; t < Tout. a [T, Da], b [T, Db] dense rows; w [Cout, Da + Db, taps].
int launch_stride_conv(const float* a, int Da, const float* b, int Db, int T, const float* w, const float* bias, int Cout, int taps,
                       int stride, int pad_left, int Tout, float* out, hipStream_t stream);

// launch_fd_attention (conformer.h) under a memory mask row shared by the n queries: key j takes part when lo <= j < hi and
// (mask == nullptr or mask[j] != 0); no other K / V row is read. No visible key: the output rows are zero
// (MultiHeadedAttentionCrossAtt.forward_attention: softmax over the filled row, then masked_fill 0).
int launch_scama_attention(const float* q, const float* K, const float* V, int ldkv, int nk, const float* mask, int lo, int hi, int n,
                           int H, int dk, float* out, hipStream_t stream);

}  // namespace pf
