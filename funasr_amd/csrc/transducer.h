// Transducer (RNN-T) search kernels (transducer.hip): one prediction-network step and the two-launch joint step. Exact fp32, VALU.
#pragma once
#include <hip/hip_runtime.h>

namespace pf {

constexpr int RNNT_MAX_DIM = 1024;     // embed / hidden / joint sizes (multiples of 4: 16-byte rows)
constexpr int RNNT_MAX_K = 16;         // beam
constexpr int RNNT_ROWS = 32;          // output rows of lin_out per workgroup of the joint's first pass

// one LSTM cell for one vector: gates = W_ih x + b_ih + W_hh h + b_hh (i, f, g, o), c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c')
struct RnntCellArgs {
    const float* x;          // device [in_dim]: the embedding row of the label (layer 0) or h' of the layer below
    const float* w_ih;       // device [4 H][in_dim]
    const float* w_hh;       // device [4 H][H]
    const float* b_ih;       // device [4 H]
    const float* b_hh;       // device [4 H]
    const float* h_prev;     // device [H] (slot src)
    const float* c_prev;     // device [H]
    float* h_out;            // device [H] (slot dst; must not alias h_prev: every workgroup reads all of h_prev)
    float* c_out;            // device [H]
    int in_dim, H;
};
int launch_rnnt_cell(const RnntCellArgs& a, hipStream_t stream);

// y[r] = W[r, :] . x for r < rows (no bias): dec_proj = lin_dec.weight . h'
int launch_rnnt_matvec(const float* W, const float* x, float* y, int rows, int cols, hipStream_t stream);

// floats of the joint's scratch: per workgroup b < ceil(V / RNNT_ROWS) the record [max, sum exp(x - max), blank logit, pad,
// k values, k rows (int32 bits)]
static inline int rnnt_joint_blocks(int V) { return (V + RNNT_ROWS - 1) / RNNT_ROWS; }
static inline size_t rnnt_joint_partial_floats(int V, int k) { return (size_t)rnnt_joint_blocks(V) * (4 + 2 * k); }

struct RnntJointArgs {
    const float* enc_proj;   // device [J]: lin_enc(enc[t]) with its bias
    const float* dec_proj;   // device [J]: lin_dec . h' of the slot
    const float* w_out;      // device [V][J]
    const float* b_out;      // device [V]
    float* partials;         // device, rnnt_joint_partial_floats(V, k)
    float* record;           // device [1 + 2 k] words: logp of row 0, k best logp of rows >= 1, their rows (int32 bits)
    int V, J, k;
};
// pass 1 (the grid splits the rows) and pass 2 (one wave merges the partials in workgroup order) on `stream`
int launch_rnnt_joint_topk(const RnntJointArgs& a, hipStream_t stream);

}  // namespace pf
