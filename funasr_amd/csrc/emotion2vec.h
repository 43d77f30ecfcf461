// Kernel launchers of the emotion2vec network (emotion2vec.hip, attention_alibi.hip; driven by engine_emotion2vec.hip).
// The conv stack runs channels-last over per-utterance row slots ([rows, 512]); everything after it runs on packed rows: the
// features of utterance b are rows [foff[b], foff[b + 1]) of an [F, D] buffer, its tokens (n_extra learned rows, then the
// features) rows [toff[b], toff[b + 1]) of an [Ntok, D] buffer. Every kernel computes a row from its own utterance only, in a
// fixed order and without atomics, so an utterance's bits do not depend on the rest of the batch.
#pragma once
#include "common.h"

namespace pf {

// per utterance: mean and 1 / sqrt(var + 1e-5) of wav[woff[b] .. woff[b + 1]) in double, fixed order -> stats [B][2]
// (F.layer_norm over the whole waveform); normalize == 0 writes (0, 1)
int launch_e2v_wav_stats(const float* wav, const int64_t* woff, int B, int normalize, float* stats, hipStream_t stream);

// conv0 (1 -> 512, k0 taps, stride s0, no bias) on the normalised samples, LayerNorm(512) and exact GELU -> y [M, 512].
// Row r belongs to the slot of the last b with so[b] <= r; frame t = r - so[b] is valid for t < nfr[b], other rows are zero.
int launch_e2v_conv0(const float* wav, const int64_t* woff, const float* stats, const int* so, const int* nfr, int B, int M,
                     const float* w, int k0, int s0, const float* gamma, const float* beta, float eps, float* y, hipStream_t stream);

// y[r] = GELU?(LayerNorm?(x[in_map ? in_map[r] : r])); gamma / beta null = no affine; y may alias x when in_map is null.
// D / 256 in {1, 2, 3, 4, 8, 12, 16}.
struct E2vRowArgs {
    const float* x; int ldx; const int* in_map;
    int ln; const float* gamma; const float* beta; float eps;
    int gelu;
    float* y; int ldy;
    int M, D;
};
int launch_e2v_rows(const E2vRowArgs& a, hipStream_t stream);

// grouped Conv1d D -> D (taps odd, padding taps / 2, with bias) over packed feature rows, zero outside each utterance's rows.
// wp: weight repacked [groups][taps][Cg][Cg] (input channel, then output channel innermost); D / groups <= 64, taps <= 31.
int launch_e2v_posconv(const float* x, const float* wp, const float* bias, const int* foff, int B, int F, int D, int groups,
                       int taps, float* y, hipStream_t stream);

// token rows: toff[b] + e (e < n_extra) = extra[e], toff[b] + n_extra + t = xf[foff[b] + t] + pos[foff[b] + t]; then
// LayerNorm(gamma, beta) -> y [Ntok, D]
int launch_e2v_tokens(const float* xf, const float* pos, const float* extra, int n_extra, const int* foff, const int* toff, int B,
                      int Ntok, int D, const float* gamma, const float* beta, float eps, float* y, hipStream_t stream);

// ALiBi self-attention of packed sequences (attention_alibi.hip), head dim 64. qkv [Ntok, 3 D] (q | k | v, head h at column
// h * 64 of each). score(i, j) = (q_i / 8) . k_j + (slope[h] * -|i - j|) * scale[h] for h < n_alibi and i, j >= n_extra
// (0 otherwise); keys past the sequence are masked; fp32 online softmax -> out [Ntok, D]. max_len sizes the grid only.
int launch_e2v_attention(const float* qkv, const int* toff, int B, int max_len, int H, int n_alibi, int n_extra,
                         const float* slope, const float* scale, float* out, hipStream_t stream);

// per utterance: mean of its feature rows (toff[b] + n_extra ..) in a fixed order -> pooled [B, D]; C > 0: logits = W pooled +
// bias (W [C, D]), classes with mask[c] != 0 at -inf, softmax -> probs [B, C]. D <= 4096, C <= 1024.
int launch_e2v_head(const float* x, const int* toff, int n_extra, int B, int D, const float* W, const float* bias, const int* mask,
                    int C, float* pooled, float* probs, hipStream_t stream);

}  // namespace pf
