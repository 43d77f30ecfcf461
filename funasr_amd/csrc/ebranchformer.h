// Kernel launchers of the E-Branchformer encoder block (ebranchformer.hip; driven by engine_conformer.hip): the exact GELU of the cgMLP,
// its convolutional spatial gating unit and the depthwise branch merge. Activations are rows of a [B * T, width] buffer (T = the
// BATCH's encoder length: the reference runs both depthwise convs over the zero-padded batch without masking and so does this path).
// Exact fp32, every row in a fixed order, no atomics.
#pragma once
#include "common.h"

namespace pf {

// in place over n floats: x = 0.5 x (1 + erf(x / sqrt(2))), the exact (erf) GELU of torch.nn.GELU(); n % 4 == 0, x 16-B aligned
int launch_eb_gelu(float* x, size_t n, hipStream_t stream);

// ConvolutionalSpatialGatingUnit (gate_activation identity, no linear after the conv): h [B * T, 2 C] = x_r | x_g, already through
// GELU -> y [B * T, C] = x_r * (dwconv(LayerNorm_C(x_g; gamma, beta)) + bias). The LayerNorm is per row over the C gate channels; the
// depthwise Conv1d (dw [C][taps], taps odd <= 31) runs over time within one sequence's T rows and reads zeros outside [0, T).
// Two launches: the rows' mean / rstd into `stats` [B * T, 2] (workspace of the caller), then normalise + conv + gate over tiles of
// 32 rows x 64 channels, the halo rows normalised from their stats. C % 32 == 0, C <= 8192.
int launch_eb_csgu(const float* h, const float* gamma, const float* beta, float eps, const float* dw, const float* dw_bias, int B, int T,
                   int C, int taps, float* stats, float* y, hipStream_t stream);

// The branch merge up to its projection: c = [x1 | x2] (x1, x2 [B * T, D], each read from its own buffer; no concatenated copy is
// made) -> y [B * T, 2 D] = c + dwconv(c) + bias, the operand of merge_proj. dw [2 D][taps], taps odd <= 31, zeros outside [0, T).
// D % 32 == 0.
int launch_eb_merge(const float* x1, const float* x2, const float* dw, const float* dw_bias, int B, int T, int D, int taps, float* y,
                    hipStream_t stream);

}  // namespace pf
