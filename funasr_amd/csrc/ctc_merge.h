// Row kernels of the Paraformer-v2 posterior embedder (ctc_merge.hip): the decoder input made from the CTC head's posteriors
// (funasr/models/paraformer_v2_community/model.py:451-482, decoder.py:318-325) instead of a CIF predictor.
#pragma once
#include "common.h"

namespace pf {

// x[row, 0 .. V) (row stride ld >= Vp) -> softmax over the V columns IN PLACE, columns V .. Vp-1 written as zero (they are the
// zero K-padding of the GEMM that reads the probabilities), ids[row] = first column of the row's largest logit (torch.argmax)
int launch_softmax_argmax_rows(float* x, int ld, int M, int V, int Vp, int* ids, hipStream_t stream);

// Run segmentation of the greedy paths ids [B, T] (device int32): per clip b over its first lens[b] frames (device int32, clamped
// to [0, T]) the maximal stretches of one label that is not `blank`, in order. counts[b] = their number n_b; ranges[(b * ld + j) * 2
// + {0, 1}] = first frame and one-past-last frame of run j < min(n_b, ld). Entries of runs j >= n_b are not written.
int launch_ctc_runs(const int* ids, const int* lens, int B, int T, int blank, int* counts, int* ranges, int ld, hipStream_t stream);

// embeds[b, j, :] = pe[j] + xscale * relu(LayerNorm_eps(mean_{t in run j of clip b} E[b, t, :] + bias; gamma, beta)) for j < counts[b],
// zero rows behind. E [B, T, D] holds the frame-wise products probs . W^T (the first layer of `embed` is linear and a run's weights
// sum to one, so Linear(mean p) = mean(p W^T) + bias). ranges_out (optional, int32 [B, N, 2]): the runs' frame ranges, zero behind.
struct PosteriorEmbedArgs {
    const float* E; const int* counts; const int* ranges; int ld;
    const float* bias; const float* gamma; const float* beta; const float* pe;
    float xscale, eps;
    float* embeds; int* ranges_out;
    int B, T, D, N;
};
int launch_posterior_embed(const PosteriorEmbedArgs& a, hipStream_t stream);

}  // namespace pf
