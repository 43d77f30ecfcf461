// Kernel launchers of LCB-Net (lcbnet.hip; driven by engine_conformer.hip): the audio-text cross-attention of the fusion layer and the
// token rows of the text encoder. Exact fp32, every row in a fixed order, no atomics.
#pragma once
#include "common.h"

namespace pf {

// Cross-attention of many queries over a second, short sequence (lcbnet/attention.py MultiHeadedAttentionReturnWeight without its
// returned weights), head dim 64, flash-style on the tile steps of attention_tile.h: q [B * Tq, H 64] rows `ldq` floats apart (head h
// at column 64 h); kv [B * L, 2 H 64]: K in the first H 64 columns, V in the second. score(i, j) = q_i . k_j / 8, keys j >= klens[b]
// masked (klens[b] < 1: zero rows; no K / V row at or past klens[b] is read). q . k and p . v on the matrix cores in exact fp32
// (v_mfma_f32_32x32x2_f32); fp32 online softmax -> out [B * Tq, H 64]. Neither scores nor probabilities reach memory.
int launch_tf_cross_attention(const float* q, int ldq, const float* kv, const int* klens, int B, int Tq, int L, int H, float* out,
                              hipStream_t stream);

// y[b * L + t] = table[ids[b * L + t]] * scale + pe[t] (the product rounded before the sum, as PositionalEncoding.forward); ids on
// the device, every id inside the table (checked by the caller on the host). D % 4 == 0.
int launch_text_embed_rows(const float* table, const int* ids, const float* pe, float scale, float* y, int B, int L, int D,
                           hipStream_t stream);

}  // namespace pf
