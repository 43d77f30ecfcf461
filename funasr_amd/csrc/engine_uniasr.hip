// C-ABI layer, UniASR two-pass ASR (funasr/models/uniasr/model.py): what the model needs beside the handles it shares with the other
// SAN-M families. The chunked encoder is pf_encoder_* with pf_encoder_set_chunk_mask (engine_encoder.hip), the SCAMA decoder step is
// pf_scamadecoder_* (engine_conformer.hip, beside the SAN-M stepper it extends); here are the stateless calls between them -- the row
// gathers of split_chunk / remove_chunk and the two-source `stride_conv` -- and the single-kernel hooks of the tests. Kernels: uniasr.hip.
#include "engine_internal.h"
#include "uniasr.h"

using namespace pf;

extern "C" {

int pf_uniasr_gather_rows(const float* src, int32_t ld_src, int32_t n_src, const int32_t* idx_dev, float* out, int32_t n, int32_t D,
                          void* stream) {
    if (check_device()) return -1;
    return launch_gather_rows_or_zero(src, ld_src, n_src, idx_dev, out, n, D, reinterpret_cast<hipStream_t>(stream));
}

int pf_uniasr_stride_conv(const float* a, int32_t Da, const float* b, int32_t Db, int32_t T, const float* w, const float* bias, int32_t Cout,
                          int32_t taps, int32_t stride, int32_t pad_left, int32_t pad_right, float* out, int32_t Tout, void* stream) {
    if (check_device()) return -1;
    PF_REQUIRE(T > 0 && taps >= 1 && stride >= 1 && pad_left >= 0 && pad_right >= 0, "uniasr_stride_conv: bad shape");
    // the rows the convolution yields over the padded input; the caller may ask for fewer (the reference keeps (T - 1) / stride + 1)
    const int full = T + pad_left + pad_right >= taps ? (T + pad_left + pad_right - taps) / stride + 1 : 0;
    PF_REQUIRE(Tout >= 1 && Tout <= full, "uniasr_stride_conv: Tout above what the padded input yields ((T + pad - taps) / stride + 1)");
    return launch_stride_conv(a, Da, b, Db, T, w, bias, Cout, taps, stride, pad_left, Tout, out, reinterpret_cast<hipStream_t>(stream));
}

// single-kernel hooks (tests)
int pf_k_chunk_attention(const float* qkv, const int32_t* klens_dev, int32_t B, int32_t T, int32_t H, int32_t dk, int32_t chunk, int32_t stride,
                         int32_t shift, int32_t look_back, float* out, void* stream) {
    PF_REQUIRE(qkv && out && H > 0 && dk > 0, "chunk_attention: null argument");
    const int D = H * dk;
    AttnArgs a{};
    a.Q = qkv; a.ldq = 3 * D; a.K = qkv + D; a.ldk = 3 * D; a.V = qkv + 2 * D; a.ldv = 3 * D; a.O = out; a.ldo = D;
    a.klens = klens_dev; a.B = B; a.H = H; a.Tq = T; a.Tk = T; a.scale = powf((float)dk, -0.5f);
    return launch_chunk_attention(a, dk, ChunkGeom{chunk, stride, shift, look_back}, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_chunk_fsmn(const float* in, int32_t ldin, const float* w, const int32_t* lens_dev, int32_t B, int32_t T, int32_t C, int32_t K,
                    int32_t left_pad, int32_t chunk, int32_t stride, int32_t shift, float* out, void* stream) {
    FsmnArgs f{};
    f.in = in; f.ldin = ldin; f.w = w; f.out = out; f.ldo = C; f.lens = lens_dev; f.B = B; f.T = T; f.C = C; f.K = K; f.left_pad = left_pad;
    return launch_chunk_fsmn(f, ChunkGeom{chunk, stride, shift, 0}, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_scama_attention(const float* q, const float* kv, int32_t T, const float* mask_row_dev, int32_t key_lo, int32_t key_hi, int32_t n,
                         int32_t H, int32_t dk, float* out, void* stream) {
    PF_REQUIRE(kv && H > 0 && (dk == 64 || dk == 128), "scama_attention: head dim 64 or 128");
    return launch_scama_attention(q, kv, kv + H * dk, 2 * H * dk, T, mask_row_dev, key_lo, key_hi, n, H, dk, out,
                                  reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
