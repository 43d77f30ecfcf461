// Kernel argument blocks and launchers of the ERes2NetV2 speaker-embedding network (eres2net.hip, engine_eres2net.hip).
// Activations are channels-last [chunk, t, f, c]; the channel stride of every buffer is a multiple of 4 floats, so a lane stages
// 16 bytes along c. Channels between a tensor's count and its stride ("pad channels") are never used as data: the loader
// replaces them by zero, and the matching weight columns are zero.
#pragma once
#include "common.h"

namespace pf {

enum { ERES_ACT_NONE = 0, ERES_ACT_RELU = 1, ERES_ACT_CLAMP20 = 2, ERES_ACT_SILU = 3 };
enum { ERES_A2_NONE = 0, ERES_A2_SUM = 1, ERES_A2_CONCAT = 2 };

static inline int eres_pad4(int c) { return (c + 3) / 4 * 4; }

// One implicit GEMM on the exact-f32 MFMA: C[m, n] = epilogue(sum_k A[m, k] * W[n, k]), row m = ((chunk * To + to) * Fo + fo).
// The A operand is gathered by the loader (never materialised as an im2col copy):
//   k = tap * pad4(Cin) + c, tap = kf * 3 + kt (taps == 9, padding 1) or the centre alone (taps == 1), reads
//   A[((chunk * Tin + to * st + kt - 1) * Fin + fo * sf + kf - 1) * lda + c], zero outside [0, Tin) x [0, Fin) of the row's chunk
//   and for c >= Cin.
// Second operand A2:
//   ERES_A2_SUM     the loader adds A2 (same geometry, own stride lda2) to A before the product;
//   ERES_A2_CONCAT  k in [taps * pad4(Cin), + pad4(Cin2)) continues with a 1x1 conv of A2 [chunk, Tin2, Fin2, lda2] sampled at
//                   (to * st2, fo * sf2): cat(x, y) of AFF's first conv, or the projection shortcut inside conv3's product.
// Epilogue: v = acc + bias[n]; v += R[m, n]; activation; or (X != null) the AFF combine with a = v:
//   C = X[m, n] * (1 + tanh a) + Y[m, n] * (1 - tanh a).
// A, A2, W must be 16-byte aligned with strides that are multiples of 4; C, R, X, Y take any stride (column slices).
// The k order of every output element is fixed by K alone and the tile shape by N alone: no atomics, a chunk's rows have
// the same bits whatever else is in the launch.
struct EresConvArgs {
    int M, N;
    const float* W; int ldw;
    float* C; int ldc;
    const float* bias;
    const float* R; int ldr;
    int act;
    const float* X; int ldx;
    const float* Y; int ldy;
    const float* A; int lda; int Cin;
    int taps;
    int Tin, Fin, To, Fo, st, sf;
    int a2_mode;
    const float* A2; int lda2; int Cin2;
    int Tin2, Fin2, st2, sf2;
};
static inline int eres_conv_k(const EresConvArgs& a) {
    return a.taps * eres_pad4(a.Cin) + (a.a2_mode == ERES_A2_CONCAT ? eres_pad4(a.Cin2) : 0);
}
int launch_eres_conv(const EresConvArgs& a, hipStream_t stream);

// the stem: 3x3 conv 1 -> C (padding 1, folded BN, ReLU) of feats [n, T, F] -> out [n, T, F, C]; w [C, 9] (tap = kf * 3 + kt)
int launch_eres_stem(const float* feats, int n, int T, int F, const float* w, const float* bias, int C, float* out,
                     hipStream_t stream);

// TSTP: x [n, T, S] (S = F' * C columns) -> stats [n, 2 S]: the mean over t, then sqrt(unbiased variance + 1e-8). T >= 2.
int launch_eres_pool(const float* x, int n, int T, int S, float* stats, hipStream_t stream);

}  // namespace pf
