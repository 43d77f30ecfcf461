// Batched CTC forced alignment (ctc_align.hip): the Viterbi path of each clip's target labels through its emissions, the arithmetic of
// `ctc_forced_align` (funasr/models/sense_voice/utils/ctc_alignment.py:2-77) comparison by comparison, so the labels are bit-determined.
#pragma once
#include "common.h"

namespace pf {

constexpr int CTC_ALIGN_MAX_T = 4096;    // frames of one clip (back-pointers: one byte per frame and state in the caller's scratch)
constexpr int CTC_ALIGN_MAX_L = 1024;    // target labels of one clip (2 L + 1 states, double-buffered in LDS)

// A ragged batch of B clips over emissions [B, T, V] (row stride ld): clip b reads rows b * T + t0 + t, t < T_b, and its L_b labels
// targets[b * ldt + l] (values outside [0, V) count as an emission of -inf). lens (device int32 [2 B]) holds T_0 .. T_{B-1} and then
// L_0 .. L_{B-1}; the host has checked T_b <= min(T - t0, T_max, T_out), 1 <= L_b <= min(ldt, L_max) before the launch.
//   lse  (nullable, [B * T]): the emissions are logits and e(t, c) = fl(x[t][c] - lse[t]), the value log_softmax would have stored
//   pred (nullable, [B * T]): e(t, blank) = 0 on the rows with pred == blank (the reference's `logits[pred == blank, blank] = 0`)
// dense [B, T_max, L_max + 1] and back [B, T_max, 2 L_max + 1] are scratch; every entry that is read has been written by the same call.
// labels [B, T_out]: ext[path[t]] for t < T_b, -1 behind.
struct CtcAlignArgs {
    const float* emis; int ld, T, V, t0;
    const float* lse; const int* pred;
    const int* targets; int ldt;
    const int* lens;
    int blank, B, T_max, L_max;
    float* dense; unsigned char* back;
    int* labels; int T_out;
};
size_t ctc_align_lens_bytes(int B);                            // the head of the scratch buffer: lens, rounded up to 256 bytes
size_t ctc_align_dense_bytes(int B, int T_max, int L_max);     // rounded up to 256 bytes
size_t ctc_align_back_bytes(int B, int T_max, int L_max);
int launch_ctc_align(const CtcAlignArgs& a, hipStream_t stream);

}  // namespace pf
