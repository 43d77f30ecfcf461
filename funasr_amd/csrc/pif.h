// Kernel launchers of the E-Paraformer predictor (pif.hip; driven by engine_conformer.hip): parallel integrate-and-fire,
// funasr/models/e_paraformer/pif_predictor.py PifPredictor.forward (inference path). Activations are rows of a [B * T, D] buffer, T =
// the BATCH's encoder length. Exact fp32, every output element in a fixed summation order, no atomics: a call repeats bit for bit.
#pragma once
#include "common.h"

namespace pf {

constexpr int PIF_MAX_T = 5000, PIF_MAX_L = 2048, PIF_MAX_D = 1024, PIF_MAX_ORDER = 15, PIF_MAX_HEADS = 8;

// a[b, t] = relu(sigmoid(dot(relu(dwconv(h)[b, t] + conv_b + h[b, t]), out_w) + out_b) * smooth - noise) for t < lens[b], else 0;
// token_num[b] = sum_t a[b, t]. The depthwise conv (conv_w [D][l_order + r_order + 1]) runs over time within ONE clip's T rows of the
// padded batch and reads zeros outside [0, T); it is NOT masked by lens (the reference's is not): the frames near a shorter clip's end
// read the rows behind it. Two launches: one wave per row, then one workgroup per clip that sums its T alphas (thread i takes
// t = i, i + 256, ..., then a fixed tree; float64 partials, rounded once).
int launch_pif_alphas(const float* h, const float* conv_w, const float* conv_b, const float* out_w, const float* out_b, const int* lens, int B,
                      int T, int D, int l_order, int r_order, float smooth, float noise, float* a, float* token_num, hipStream_t stream);

// an[b, t] = a[b, t] * (n[b] / token_num[b]) (the quotient rounded to fp32 first, as the reference's tensor ops do; 0 where
// token_num[b] == 0 or n[b] <= 0: no division, no NaN) and align[b, t] = its inclusive prefix sum in sequential order (a float64
// running sum rounded to fp32 per step: ATen's CPU cumsum). One wave per clip, the row staged in LDS; `an` may alias `a`.
int launch_pif_align(const float* a, const float* token_num, const int* n, int B, int T, float* an, float* align, hipStream_t stream);

// embeds[b, l, g Dh + d] = sum_t softmax_t(-((l + 0.5 - align[b, t]) sigma[g])^2)[t] h[b, t, g Dh + d] over t < lens[b], Dh = D / H, for
// ALL l < L of every clip (rows at or past a clip's own count are what the reference computes there). Flash form: one pass over the
// frames in chunks of 64 with a running maximum and sum; a workgroup (one wave) owns 16 fire positions x 64 channels of one head.
// Frames t >= lens[b] are never read (neither h nor align); a clip with lens[b] == 0 gets zero rows.
int launch_pif_embed(const float* align, const float* h, const float* sigma, const int* lens, int B, int T, int L, int D, int H, float* embeds,
                     hipStream_t stream);

// best[r] = x[r, ids[r]] (the log-probability of a row's arg-max)
int launch_pif_gather_best(const float* x, int ldx, const int* ids, int M, float* best, hipStream_t stream);

}  // namespace pf
