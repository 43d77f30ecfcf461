// Kernel argument blocks and launchers of the CAM++ speaker-embedding network (campplus.hip, engine_campplus.hip).
// Activations are channels-last: 1-D layers [chunks * frames, channels], the 2-D head [chunks * frames * freq, channels].
#pragma once
#include "common.h"

namespace pf {

// One implicit GEMM on the exact-f32 MFMA: C[m, n] = epilogue(sum_k A[m, k] * W[n, k]).
// The A operand is gathered by the loader (never materialised as an im2col copy):
//   conv1d  (conv2d == 0): row m = (chunk, to), k = tap * Cin + ci, reads A[(chunk * Tin + to * stride + tap * dil - pad) * lda + ci]
//           (zero outside [0, Tin)); with pre_scale / pre_shift (taps == 1 only) the value is max(a * scale[ci] + shift[ci], 0):
//           the BatchNorm-ReLU in front of a 1x1 conv, applied to the operand as it is staged.
//   conv2d  (conv2d != 0): 3x3 conv over (freq, time), stride (fstride, 1), padding 1; row m = ((chunk * T + t) * Fo + fo),
//           k = (kf * 3 + kt) * Cin + ci reads A[((chunk * T + t + kt - 1) * Fin + fo * fstride + kf - 1) * Cin + ci];
//           k in [9 Cin, 9 Cin + Cin2) continues with the 1x1 stride-(fstride2, 1) shortcut conv of A2 [.., Fin2, Cin2]
//           (concatenated K: the main conv and the projection shortcut are one product).
// Epilogue: + bias[n], + R[m, n] (identity shortcut), ReLU, or (mask != null) * mask[(chunk * nseg + to / 100) * N + n]
// (the context-aware mask of a CAM layer; rows of one chunk are To apart).
struct CamGemmArgs {
    int M, N, K;
    const float* W; int ldw;           // [N, ldw], k contiguous
    float* C; int ldc;
    const float* bias;
    const float* R; int ldr;
    int relu;
    const float* mask; int nseg;
    const float* A; int lda;
    int conv2d;
    int Tin, To, Cin, taps, stride, dil, pad;          // conv1d
    const float* pre_scale; const float* pre_shift;
    int T, Fin, Fo, fstride;                           // conv2d
    const float* A2; int Cin2, Fin2, fstride2;
};
int launch_cam_gemm(const CamGemmArgs& a, hipStream_t stream);

// CAM layer context: per chunk, the mask sigmoid(W2 relu(W1 (mean_t h + segmean_s h) + b1) + b2) for every 100-frame segment s
// (avg_pool1d(100, ceil_mode): the last segment divides by its true length). h: [n_chunks * T, 128]; mask: [n_chunks, nseg, 32].
int launch_cam_context(const float* h, int T, int n_chunks, const float* w1, const float* b1, const float* w2, const float* b2,
                       float* mask, hipStream_t stream);

// out BN-ReLU, mean and unbiased std over time, dense 2C -> E (weight transposed [2C, E]), affine-free BN folded to
// y * scale + shift. x: [n_chunks * T, C]; emb: [n_chunks, E].
int launch_cam_pool_dense(const float* x, int T, int C, int n_chunks, const float* pre_scale, const float* pre_shift,
                          const float* wt, int E, const float* scale, const float* shift, float* emb, hipStream_t stream);

// chunks of a device waveform: out[i, j] = wav[start[i] + j] for j < valid[i] (and inside the waveform), 0 otherwise
int launch_cam_gather_chunks(const float* wav, int64_t n_samples, const int64_t* starts_dev, const int* valid_dev, int n, int len,
                             float* out, hipStream_t stream);

// feats [n, T, D] -= mean over T (per chunk and bin), in place
int launch_cam_sub_mean(float* feats, int n, int T, int D, hipStream_t stream);

}  // namespace pf
