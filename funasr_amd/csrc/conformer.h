// Kernel launchers of the Conformer encoder, the Transformer encoder, the Transformer decoder step and the SAN-M decoder step (conformer.hip,
// attention_relpos.hip, attention_abs.hip; driven by engine_conformer.hip). Activations are rows of a [B * T, D] buffer (T = the BATCH's encoder length: the reference computes every
// row of the zero-padded batch and so does this path). Every kernel computes a row in a fixed order and without atomics.
#pragma once
#include "common.h"

namespace pf {

// Conv2d(1 -> C, 3 x 3, stride 2) + ReLU of Conv2dSubsampling, written channels-last into TWO buffers so that the second conv
// becomes three plain GEMMs over overlapping strided views: conv0's even time rows go to `even` and its odd rows to `odd`, both
// [B][NE][FP][C] with FP = 2 * (F2 + 1) frequency columns (F1 = (F - 1) / 2 of them computed, the rest zero) and NE = T2 + 1 time
// rows (rows past conv0's T1 are zero). feats [B, Tin, F].
int launch_cf_conv0(const float* feats, int B, int Tin, int F, const float* w, const float* bias, int C, int T1, int F1, int NE,
                    int FP, float* even, float* odd, hipStream_t stream);

// in place over n floats: mode 0 = ReLU, 1 = Swish (x * sigmoid(x)); n % 4 == 0
int launch_cf_act(float* x, size_t n, int mode, hipStream_t stream);

// y[b * T + t] = x[b * NE + t] * scale for t < T (the embed linear's rows without the waste row per sequence, times sqrt(D));
// with pe [>= T, D] (the Transformer encoder's PositionalEncoding): ... + pe[t], the product rounded before the sum
int launch_cf_scale_rows(const float* x, int NE, float* y, int B, int T, int D, float scale, const float* pe, hipStream_t stream);

// The Conformer convolution module between its two pointwise convs: g [B * T, 2 D] (value | gate) -> GLU -> depthwise Conv1d over
// time (taps odd <= 31, zero padding at the edges of each sequence's T rows) + bias -> eval-mode BatchNorm as y * bn_scale +
// bn_shift -> Swish -> y [B * T, D]. dw [D][taps]. D % 64 == 0.
int launch_cf_glu_dw(const float* g, const float* dw, const float* dw_bias, const float* bn_scale, const float* bn_shift, int B,
                     int T, int D, int taps, float* y, hipStream_t stream);

// Relative-position self-attention (Transformer-XL style), head dim 64, flash-style: no [T, T] tensor reaches memory.
// qkv [B * T, 3 D] (q | k | v, head h at column 64 h of each); P [nP, D] = linear_pos(pos_emb); u, v [H, 64] = pos_bias_u / _v.
// score(i, j) = ((q_i + u) . k_j + bd(i, j)) / 8, keys j >= klens[b] masked (klens[b] == 0: zero rows), with qv_i = q_i + v and
//   legacy == 0 (nP = 2 T - 1): bd(i, j) = qv_i . P[T - 1 - i + j]
//   legacy == 1 (nP = T):       bd(i, j) = qv_i . P[T - 1 - i + j] for j <= i, 0 for j == i + 1, qv_{i + 1} . P[j - i - 2] for j >= i + 2
// (the reference's rel_shift of a [T, T] matrix wraps the next row into the upper triangle). q . k, the band products and p . v run
// on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32); fp32 online softmax -> out [B * T, D].
int launch_cf_relpos_attention(const float* qkv, const float* P, const float* u, const float* v, const int* klens, int B, int T,
                               int H, int legacy, float* out, hipStream_t stream);

// Plain masked self-attention (MultiHeadedAttention), head dim 64, flash-style, the tile mapping of the kernel above without its
// positional half: qkv [B * T, 3 D] (q | k | v, head h at column 64 h of each), score(i, j) = q_i . k_j / 8, keys j >= klens[b]
// masked (klens[b] == 0: zero rows; no K / V row at or past klens[b] is read). q . k and p . v on the matrix cores in exact fp32
// (v_mfma_f32_32x32x2_f32); fp32 online softmax -> out [B * T, D].
int launch_tf_attention(const float* qkv, const int* klens, int B, int T, int H, float* out, hipStream_t stream);

// ---- Transformer decoder step
// x[r] = table[ids[r]] * scale + pe[pos] (r < n; ids on the device); pe_row == nullptr: the scale alone (the SAN-M decoder's bare
// embedding with scale 1)
int launch_td_embed(const float* table, const int* ids, const float* pe_row, float scale, float* x, int n, int D, hipStream_t stream);

// few-query attention, head dim 64: query r (q [n, D], head h at column 64 h) over nk keys K / V rows of `ldkv` floats, the
// rows of query r starting at K + r * seq_stride (seq_stride 0: every query reads the same memory). softmax(q . k / 8) v -> out [n, D].
int launch_td_attention(const float* q, const float* K, const float* V, int ldkv, size_t seq_stride, int nk, int n, int H, float* out,
                        hipStream_t stream);

// cache reorder: dst[l][k][0 .. len) = src[l][parents[k]][0 .. len) for every layer l < L and k < n; a slot is `slot_floats` wide,
// a layer `layer_floats`, a position `row_floats`
int launch_td_reorder(const float* src, float* dst, const int* parents, int n, int L, size_t layer_floats, size_t slot_floats,
                      int len, int row_floats, hipStream_t stream);

// ---- SAN-M (FsmnDecoder) step
// The FSMN memory block of one decoder layer for the n running slots of step `pos`, one launch:
//   u = LayerNorm(t[r]; g2, b2)
//   window of slot r, K columns of D floats:  pos == 0: zeros with u at column left_pad;
//                                             pos > 0:  columns 1 .. K - 1 of win_in[parents[r]] (parents == nullptr: r), then u
//   x_out[r] = x[r] + (sum_k w[d][k] window[k][d] + u)          (the block adds its own input; no bias)
//   xn_out[r] = LayerNorm(x_out[r]; g3, b3)                     (g3 != nullptr: the layer has cross-attention)
// and the new window is written to win_out[r]. win_in / win_out [slots][K][D] must not overlap (ping-pong); every parent index is
// below the slot count of win_in (checked by the caller on the host). D % 4 == 0, D <= 2048, 1 <= K <= 32, 0 <= left_pad < K.
int launch_fd_fsmn_step(const float* t, const float* x, const float* g2, const float* b2, const float* w, const float* win_in,
                        float* win_out, const int* parents, int pos, int n, int D, int K, int left_pad, const float* g3,
                        const float* b3, float eps, float* x_out, float* xn_out, hipStream_t stream);

// few-query cross-attention for head dims 64 and 128: query r (q [n, H dk], head h at column dk h) over the SAME nk memory rows for
// every query, K / V rows of `ldkv` floats. softmax(q . k / sqrt(dk)) v -> out [n, H dk]. No mask.
int launch_fd_attention(const float* q, const float* K, const float* V, int ldkv, int nk, int n, int H, int dk, float* out,
                        hipStream_t stream);

}  // namespace pf
