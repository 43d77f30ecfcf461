// C-ABI layer, Conformer / Transformer / SANM ASR: pf_conformer_* and pf_tfencoder_* (the two encoders over one Conv2dSubsampling front),
// pf_tdecoder_* (the autoregressive Transformer decoder step) and pf_fsmndecoder_* (the SAN-M decoder step); kernels in conformer.hip, attention_relpos.hip and
// attention_abs.hip, GEMMs through the shared launchers.
//
// Host structure: what two handles have in common is written once. SubEnc is the base of both encoders: their state, the prologue of
// a forward (front()), the GEMM / LayerNorm pair of the block loops and the a-priori exponent pair of prepare(); enc_forward,
// enc_set_precision and enc_num_frames are the entry points of both, worded by the family. Stepper is the base of both decoder
// steppers: their state, the named Linear / LayerNorm of a step (lin / norm), the cross-attention sub-block and the output tail;
// begin_common, step_common_checks and reorder_common are the argument checks of both. Cf, Tf, Td and Fd add what is their own: the
// block loops, the K / V cache with its device reorder, the FSMN windows with their position rule. The LCB-Net handles (pf_textencoder_*,
// pf_fusion_*; kernels in lcbnet.hip) sit on the same base: the text encoder is the Transformer encoder's block loop (SubEnc::tf_blocks)
// behind token rows instead of the subsampling, the fusion layer that block with a cross-attention between its two halves. The
// E-Branchformer encoder (pf_ebranchformer_*, struct Eb; kernels in ebranchformer.hip) is a third block loop behind the same front.
// E-Paraformer's one-pass decoder (pf_sandecoder_*, struct Sd) is the fusion layer's block n_blocks times on that base, and its
// predictor (pf_pif_*, struct Pif; kernels in pif.hip) a handle of two calls.
//
// Encoder forward over the zero-padded batch [B, Tin, F] (the reference runs Conv2dSubsampling and the convolution module over
// the padded tensor without masking, so every row of the batch is computed and a clip's frames depend on the batch's length):
//   conv0 + ReLU into the even / odd time-row buffers -> conv1 as THREE accumulating GEMMs over overlapping strided views
//   (element r = t (F2 + 1) + f of the output reads the contiguous 3 C floats at 2 C r of even[t], odd[t], even[t + 1]: lda = 2 C,
//   K = 3 C, no im2col; one output column in F2 + 1 is waste) + ReLU -> the output linear over rows of (F2 + 1) C floats (weight
//   permuted, zero for the waste column; K in slices of 1024, gemm_f32_ksliced) -> x sqrt(D) into [B T, D] rows -> blocks: [macaron FFN] -> LayerNorm, q / k / v and
//   linear_pos GEMMs, relative-position attention, linear_out (+ residual) -> LayerNorm, pointwise-1, GLU + depthwise + BatchNorm
//   + Swish, pointwise-2 (+ residual) -> FFN -> norm_final; after_norm.
// ff_scale = 0.5 of the macaron pair is folded into w_2 and its bias at load (an exact scaling), so the residual rides in the GEMM.
// precision 3 (f16x2): the block GEMMs take two-plane fp16 operands with exponents from a-priori bounds of the weights (LayerNorm
// outputs: sqrt(D) max|gamma| + max|beta|; hidden / value / conv-module rows: row-L1 bounds). The subsampling GEMMs (their input is
// the caller's features, for which no bound exists) and linear_pos stay exact-fp32 MFMA GEMMs in both modes.
//
// Decoder: begin() computes the cross-attention K / V of every layer once per utterance; step() runs all running hypotheses of a
// beam through the layers (M = n_hyp rows: the small-M weight-streaming GEMMs, fp32 in both modes), appending each layer's
// self-attention K / V at `pos` of the hypothesis' slot; reorder() gathers the surviving hypotheses' parent slots on the device.
//
// SAN-M decoder (pf_fsmndecoder_*, FsmnDecoder.forward_one_step): the same three calls. begin() projects K | V of every cross-attention
// layer through linear_k_v and zeroes the FSMN windows; step() runs FFN -> fused norm2 / FSMN window / norm3 kernel -> cross-attention per
// layer; reorder() only records the parents: the FSMN kernel of the next step reads the parent's window of one buffer and writes its own
// into the other.
#include <algorithm>
#include <cmath>

#include "engine_internal.h"
#include "conformer.h"
#include "uniasr.h"
#include "lcbnet.h"
#include "ebranchformer.h"
#include "cif.h"
#include "pif.h"

using namespace pf;

namespace {

constexpr int LIN_K_SLICE = 1024;      // K extent of one launch of the subsampling's output linear (a multiple of the GEMM's 32)

// Conv2dSubsampling up to its output linear, shared by the Conformer and the Transformer encoder handles: the buffers, what is
// derived from the weights at prepare(), and the launches.
struct CfSub {
    DevBuf even, odd, ya, yb, lin, lin2;
    static int F1(int F) { return (F - 3) / 2 + 1; }
    static int F2(int F) { return (F1(F) - 3) / 2 + 1; }
    static int sub(int L, int n) { const int m = std::min(L, n - 2); return m <= 0 ? 0 : (m + 1) / 2; }
    // encoder frames of a length-L clip inside a batch padded to n frames (the mask rule x_mask[:, :, :-2:2][:, :, :-2:2])
    static int out_len(int L, int n) { const int n1 = sub(n, n); return sub(sub(L, n), n1); }
    static int prepare(TensorTable& tt, int C, int D, int f2, const char* who);
    // feats [B, Tin, F] -> *rows: [B, NE = T + 1, D] rows of the output linear (row T of each sequence is waste)
    int forward(TensorTable& tt, DevBuf& planes, const float* feats, int B, int Tin, int F, int C, int D, const float** rows, hipStream_t s);
};

int CfSub::prepare(TensorTable& tt, int C, int D, int f2, const char* who) {
    // conv1 [C, C, 3, 3] -> per time tap dt the [C, 3 C] matrix W_dt[co][df C + ci]
    std::vector<float> w = tt.host("embed.conv.2.weight");
    if (w.empty()) { set_error(std::string(who) + ": weight copy failed"); return -2; }
    for (int dt = 0; dt < 3; ++dt) {
        std::vector<float> m((size_t)C * 3 * C);
        for (int co = 0; co < C; ++co)
            for (int df = 0; df < 3; ++df)
                for (int ci = 0; ci < C; ++ci) m[((size_t)co * 3 + df) * C + ci] = w[(((size_t)co * C + ci) * 3 + dt) * 3 + df];
        if (tt.put_derived("#conv1.tap" + std::to_string(dt), m)) return -2;
    }
    // output linear [D, C F2] (feature c F2 + f) -> [D, (F2 + 1) C] (feature f C + c, zero for the waste column)
    std::vector<float> l = tt.host("embed.out.0.weight");
    std::vector<float> m((size_t)D * (f2 + 1) * C, 0.f);
    for (int d = 0; d < D; ++d)
        for (int c = 0; c < C; ++c)
            for (int f = 0; f < f2; ++f) m[((size_t)d * (f2 + 1) + f) * C + c] = l[((size_t)d * C + c) * f2 + f];
    return tt.put_derived("#embed.out", m) ? -2 : 0;
}

int CfSub::forward(TensorTable& tt, DevBuf& planes, const float* feats, int B, int Tin, int F, int C, int D, const float** rows,
                   hipStream_t s) {
    const int f1 = F1(F), f2 = F2(F), FP = 2 * (f2 + 1);
    const int T1 = (Tin - 3) / 2 + 1, T = (T1 - 3) / 2 + 1, NE = T + 1;
    const size_t Mc = (size_t)B * NE * (f2 + 1), EO = (size_t)B * NE * FP * C, SL = (size_t)2 * FP * C;
    if (even.ensure(sizeof(float) * (EO + SL)) || odd.ensure(sizeof(float) * (EO + SL)) || ya.ensure(sizeof(float) * Mc * C) ||
        yb.ensure(sizeof(float) * Mc * C) || lin.ensure(sizeof(float) * (size_t)B * NE * D) || lin2.ensure(sizeof(float) * (size_t)B * NE * D))
        return -2;
    int rc;
    // C[M, N] = A[M, K] (row stride lda = 2 C, K = 3 C: overlapping views) W^T + bias (+ R1); fp32 only
    auto gm = [&](const float* A, const std::string& w, const float* bias, const float* R1, float* Cc) {
        return gemm_two_mode(tt, planes, false, A, 3 * C, Mc, 2 * C, (int)Mc, 3 * C, w, C, bias, R1, Cc, C, 0, 0, s);
    };
    float *ev = even.as<float>(), *od = odd.as<float>(), *a = ya.as<float>(), *b = yb.as<float>();
    PF_HIP_TRY(hipMemsetAsync(ev + EO, 0, sizeof(float) * SL, s));
    PF_HIP_TRY(hipMemsetAsync(od + EO, 0, sizeof(float) * SL, s));
    if ((rc = launch_cf_conv0(feats, B, Tin, F, tt.get("embed.conv.0.weight"), tt.get("embed.conv.0.bias"), C, T1, f1, NE, FP, ev, od, s)))
        return rc;
    if ((rc = gm(ev, "#conv1.tap0", tt.get("embed.conv.2.bias"), nullptr, a))) return rc;
    if ((rc = gm(od, "#conv1.tap1", nullptr, a, b))) return rc;
    if ((rc = gm(ev + (size_t)FP * C, "#conv1.tap2", nullptr, b, a))) return rc;
    if ((rc = launch_cf_act(a, Mc * C, 0, s))) return rc;
    // the output linear sums (F2 + 1) C terms per element (2560 at 80 features and C = 128, 8192 at 256 features): K in slices
    const int Kl = (f2 + 1) * C;
    return gemm_f32_ksliced(a, Kl, tt.get("#embed.out"), Kl, tt.get("embed.out.0.bias"), B * NE, D, Kl, LIN_K_SLICE, lin.as<float>(),
                            lin2.as<float>(), rows, nullptr, s);
}

std::string blk(int i) { return "encoders." + std::to_string(i) + "."; }

// set_tensor / missing of the four handles (`null_msg`: the family's refusal of a null argument)
template <class H> int table_set(H* h, const char* null_msg, const char* name, const float* data, int64_t numel) {
    PF_REQUIRE(h && name && data, null_msg);
    return h->tt.set(name, data, numel);
}
template <class H> int table_missing(const H* h) { return h ? h->tt.missing() : -1; }

// the a-priori plane exponents of one Transformer encoder block (precision 3)
struct TfBlockX { int e_mha_in = 0, e_att = 0, e_ff_in = 0, e_ff_h = 0; };

// What the encoders of the family share: the two over the Conv2dSubsampling front, and the LCB-Net handles, whose rows come from
// token ids (text encoder) or from the caller (fusion layer). Cfg: pf_conformer_config / pf_tfencoder_config / LcbCfg (the fields
// read here carry the same names in all).
template <class Cfg> struct SubEnc {
    Cfg cfg;
    TensorTable tt;
    unsigned long long prepared = ~0ull;
    CfSub sub_;
    DevBuf xa, xb, xn, qkv, att, hid, planes, klens;
    int T = 0, Mi = 0;                     // the forward in flight (front()): encoder frames per clip, rows of the block loop, its stream
    hipStream_t s = nullptr;

    // prepare(): the a-priori plane exponents of LayerNorm `norm` -> Linear `lin` (its first `rows` rows): *e_in for the LayerNorm's
    // output rows, *e_out for the linear's, whose bound goes to *out_bound where asked for
    int ln_lin_exps(const std::string& norm, const std::string& lin, int rows, int* e_in, int* e_out, hipStream_t ps, float* out_bound = nullptr) {
        const int D = cfg.d_model;
        float nb, hb;
        if (TensorTable::dev_ln_bound(tt.get(norm + "weight"), tt.get(norm + "bias"), D, &nb, ps)) return -2;
        *e_in = exp_for_bound(nb);
        if (TensorTable::dev_linear_bound(tt.get(lin + "weight"), rows, D, D, tt.get(lin + "bias"), nb, &hb, ps)) return -2;
        *e_out = exp_for_bound(hb);
        if (out_bound) *out_bound = hb;
        return 0;
    }
    // What every front begins with: B sequences of T_ rows are in flight on fs; the buffers (hid: hid_w floats per row), the valid
    // rows kl [B] into klens.
    int rows(int B, int T_, int hid_w, const int32_t* kl, hipStream_t fs) {
        const int D = cfg.d_model;
        T = T_; Mi = B * T; s = fs;
        const size_t M = (size_t)Mi;
        if (xa.ensure(sizeof(float) * M * D) || xb.ensure(sizeof(float) * M * D) || xn.ensure(sizeof(float) * M * D) ||
            qkv.ensure(sizeof(float) * M * 3 * D) || att.ensure(sizeof(float) * M * D) || hid.ensure(sizeof(float) * M * hid_w) ||
            klens.ensure(sizeof(int32_t) * B))
            return -2;
        return upload_h2d(klens.p, kl, sizeof(int32_t) * B, s) ? -2 : 0;
    }
    // The prologue of a forward behind the subsampling: frame counts, the clips' encoder frames into klens (and olens), the buffers,
    // the subsampling, and its rows x sqrt(D) (+ pe) as the [B T, D] rows of xa.
    int front(const float* feats, const int32_t* lens, int B, int Tin, int hid_w, const float* pe, int32_t* olens, hipStream_t fs) {
        const int D = cfg.d_model;
        const int T1 = (Tin - 3) / 2 + 1;
        std::vector<int32_t> kl(B);
        for (int b = 0; b < B; ++b) {
            kl[b] = CfSub::out_len(lens[b], Tin);
            if (olens) olens[b] = kl[b];
        }
        if (int rc = rows(B, (T1 - 3) / 2 + 1, hid_w, kl.data(), fs)) return rc;
        const float* rows;
        if (int rc = sub_.forward(tt, planes, feats, B, Tin, cfg.input_dim, D, D, &rows, s)) return rc;
        return launch_cf_scale_rows(rows, T + 1, xa.as<float>(), B, T, D, sqrtf((float)D), pe, s);
    }
    // C[M, N] = A[M, K] W^T + bias (+ R1); x2: from two-plane fp16 operands, A's at the a-priori exponent e_a
    int gm(bool x2, const float* A, int M, int K, const std::string& w, const float* bias, int N, const float* R1, float* C, int ldc, int e_a) {
        return gemm_two_mode(tt, planes, x2, A, K, (size_t)M, K, M, K, w, N, bias, R1, C, ldc, e_a, 0, s);
    }
    // the Linear named `p` (its tensors carry `sfx`) over the forward's rows, in the handle's precision
    int lin(const float* A, int K, const std::string& p, int N, const float* R1, float* C, int ldc, int e_a, const char* sfx = "") {
        return gm(cfg.precision == 3, A, Mi, K, p + "weight" + sfx, tt.get(p + "bias" + sfx), N, R1, C, ldc, e_a);
    }
    int ln(const std::string& p, const float* in, float* o) {
        const int D = cfg.d_model;
        return layernorm(in, D, tt.get(p + "weight"), tt.get(p + "bias"), o, D, Mi, D, D, cfg.ln_eps, s);
    }
    // The block loop of the Transformer encoders behind either front (the subsampling of the audio encoder, the token rows of the
    // LCB-Net text encoder), over the rows the front left in xa: per block `encoders.i.` x += linear_out(attention(LN1 x)), keys at or
    // past klens masked; x += w_2(relu(w_1(LN2 x))); then after_norm -> out [B T, D].
    int tf_blocks(const std::vector<TfBlockX>& bx, int B, float* out) {
        const int D = cfg.d_model, FF = cfg.ffn_dim;
        float *x = xa.as<float>(), *y = xb.as<float>(), *xn_ = xn.as<float>(), *qkv_ = qkv.as<float>(), *att_ = att.as<float>(),
              *hid_ = hid.as<float>();
        int rc;
        for (int i = 0; i < cfg.n_blocks; ++i) {
            const std::string p = blk(i);
            const TfBlockX& e = bx[i];
            if ((rc = ln(p + "norm1.", x, xn_))) return rc;
            const char* names[3] = {"self_attn.linear_q.", "self_attn.linear_k.", "self_attn.linear_v."};
            for (int j = 0; j < 3; ++j)
                if ((rc = lin(xn_, D, p + names[j], D, nullptr, qkv_ + (size_t)j * D, 3 * D, e.e_mha_in))) return rc;
            if ((rc = launch_tf_attention(qkv_, klens.as<int>(), B, T, cfg.n_heads, att_, s))) return rc;
            if ((rc = lin(att_, D, p + "self_attn.linear_out.", D, x, y, D, e.e_att))) return rc;
            std::swap(x, y);
            if ((rc = ln(p + "norm2.", x, xn_))) return rc;
            if ((rc = lin(xn_, D, p + "feed_forward.w_1.", FF, nullptr, hid_, FF, e.e_ff_in))) return rc;
            if ((rc = launch_cf_act(hid_, (size_t)Mi * FF, 0, s))) return rc;
            if ((rc = lin(hid_, FF, p + "feed_forward.w_2.", D, x, y, D, e.e_ff_h))) return rc;
            std::swap(x, y);
        }
        return ln("after_norm.", x, out);
    }
};

// The entry points of both encoders. `who`: the family word of every message ("conformer" / "tfencoder"); `table`: the family's words
// for its positional table(s) in the one message that has them.
template <class H>
int enc_forward(H* h, const std::string& who, const char* table, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin,
                float* out, int32_t* out_lens_host, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && feats && lens_host && out && B > 0, who + "_forward: null/empty argument");
    if (Tin < 7) { set_error(who + ": has " + std::to_string(Tin) + " frames and is too short for subsampling (it needs more than 7 frames)"); return -1; }
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= Tin, who + "_forward: a length exceeds the padded length");
    const int T = CfSub::out_len(Tin, Tin);
    if (T > 5000) { set_error(who + ": " + std::to_string(T) + " encoder frames; the positional " + table + " 5000 (200 s)"); return -1; }
    int rc;
    if ((rc = h->tt.require_all(who.c_str()))) return rc;
    if (h->prepared != h->tt.version && (rc = h->prepare(s))) return rc;
    return h->forward(feats, lens_host, B, Tin, out, out_lens_host, s);
}
template <class H> int enc_set_precision(H* h, const std::string& who, int32_t precision) {
    PF_REQUIRE(h && (precision == 0 || precision == 3), who + "_set_precision: 0 (fp32) or 3 (f16x2)");
    if (h->cfg.precision != precision) { h->cfg.precision = precision; h->prepared = ~0ull; }
    return 0;
}
int32_t enc_num_frames(const void* h, int32_t n_frames, int32_t padded_frames) {
    if (!h || padded_frames < 7 || n_frames > padded_frames) return -1;
    return CfSub::out_len(n_frames, padded_frames);
}

// ================================================================================================ Conformer encoder
struct CfBlockX { int e_ffm_in = 0, e_ffm_h = 0, e_mha_in = 0, e_att = 0, e_conv_in = 0, e_cm = 0, e_ff_in = 0, e_ff_h = 0; };

struct Cf : SubEnc<pf_conformer_config> {
    std::vector<CfBlockX> bx;
    DevBuf P;
    int F2() const { return CfSub::F2(cfg.input_dim); }
    int pos_rows() const { return cfg.legacy ? 5000 : 9999; }
    int prepare(hipStream_t s);
    int forward(const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s);
};

int Cf::prepare(hipStream_t s) {
    const int D = cfg.d_model, NB = cfg.n_blocks, K = cfg.kernel_size, FF = cfg.ffn_dim;
    if (CfSub::prepare(tt, D, D, F2(), "conformer")) return -2;
    std::vector<float> bnv((size_t)NB * 2 * D);
    bx.assign(NB, CfBlockX());
    if (cfg.precision == 3) tt.drop_bf16();
    for (int i = 0; i < NB; ++i) {
        const std::string p = blk(i);
        std::vector<double> sc, sh;
        if (!tt.bn_fold(p + "conv_module.norm.", true, 1e-5, sc, sh)) { set_error("conformer: weight copy failed"); return -2; }
        for (int c = 0; c < D; ++c) {
            bnv[((size_t)i * 2) * D + c] = (float)sc[c];
            bnv[((size_t)i * 2 + 1) * D + c] = (float)sh[c];
        }
        for (const char* ff : {"feed_forward.", "feed_forward_macaron."}) {
            if (!cfg.macaron) break;
            std::vector<float> w = tt.host(p + ff + "w_2.weight"), bb = tt.host(p + ff + "w_2.bias");
            for (float& v : w) v *= 0.5f;
            for (float& v : bb) v *= 0.5f;
            if (tt.put_derived(p + ff + "w_2.weight#half", w) || tt.put_derived(p + ff + "w_2.bias#half", bb)) return -2;
        }
        if (cfg.precision != 3) continue;
        CfBlockX& x = bx[i];
        float hb;
        int e_glu;                          // (the GLU's value half: its bound goes into the conv module's below, not into a plane)
        if (cfg.macaron && ln_lin_exps(p + "norm_ff_macaron.", p + "feed_forward_macaron.w_1.", FF, &x.e_ffm_in, &x.e_ffm_h, s)) return -2;
        if (ln_lin_exps(p + "norm_ff.", p + "feed_forward.w_1.", FF, &x.e_ff_in, &x.e_ff_h, s)) return -2;
        if (ln_lin_exps(p + "norm_mha.", p + "self_attn.linear_v.", D, &x.e_mha_in, &x.e_att, s)) return -2;
        if (ln_lin_exps(p + "norm_conv.", p + "conv_module.pointwise_conv1.", D, &x.e_conv_in, &e_glu, s, &hb)) return -2;
        std::vector<float> dw = tt.host(p + "conv_module.depthwise_conv.weight"), db = tt.host(p + "conv_module.depthwise_conv.bias");
        float zb = 0.f;
        for (int c = 0; c < D; ++c) {
            float l1 = 0.f;
            for (int k = 0; k < K; ++k) l1 += fabsf(dw[(size_t)c * K + k]);
            zb = fmaxf(zb, (hb * l1 + fabsf(db[c])) * fabsf(bnv[((size_t)i * 2) * D + c]) + fabsf(bnv[((size_t)i * 2 + 1) * D + c]));
        }
        x.e_cm = exp_for_bound(zb);
    }
    if (NB > 0 && tt.put_derived("#bn", bnv)) return -2;
    prepared = tt.version;
    return 0;
}

int Cf::forward(const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s) {
    const pf_conformer_config& c = cfg;
    const int D = c.d_model, FF = c.ffn_dim;
    int rc;
    if ((rc = front(feats, lens, B, Tin, std::max(FF, 2 * D), nullptr, olens, s))) return rc;
    const int nP = c.legacy ? T : 2 * T - 1;
    if (P.ensure(sizeof(float) * (size_t)nP * D)) return -2;
    const size_t M = (size_t)Mi;
    const float* pos = tt.get("pos_table") + (c.legacy ? (size_t)0 : (size_t)(5000 - T) * D);
    float *x = xa.as<float>(), *y = xb.as<float>(), *xn = this->xn.as<float>(), *qkv = this->qkv.as<float>(), *Pm = P.as<float>(),
          *att = this->att.as<float>(), *hid = this->hid.as<float>();
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        const CfBlockX& e = bx[i];
        const char* half = c.macaron ? "#half" : "";
        auto ffn = [&](const std::string& f, const std::string& norm, int e_in, int e_h) {
            int r;
            if ((r = ln(p + norm, x, xn))) return r;
            if ((r = lin(xn, D, p + f + "w_1.", FF, nullptr, hid, FF, e_in))) return r;
            if ((r = launch_cf_act(hid, M * FF, 1, s))) return r;
            if ((r = lin(hid, FF, p + f + "w_2.", D, x, y, D, e_h, half))) return r;
            std::swap(x, y);
            return 0;
        };
        if (c.macaron && (rc = ffn("feed_forward_macaron.", "norm_ff_macaron.", e.e_ffm_in, e.e_ffm_h))) return rc;
        // relative-position self-attention
        if ((rc = ln(p + "norm_mha.", x, xn))) return rc;
        const char* names[3] = {"self_attn.linear_q.", "self_attn.linear_k.", "self_attn.linear_v."};
        for (int j = 0; j < 3; ++j)
            if ((rc = lin(xn, D, p + names[j], D, nullptr, qkv + (size_t)j * D, 3 * D, e.e_mha_in))) return rc;
        if ((rc = gm(false, pos, nP, D, p + "self_attn.linear_pos.weight", nullptr, D, nullptr, Pm, D, 0))) return rc;
        if ((rc = launch_cf_relpos_attention(qkv, Pm, tt.get(p + "self_attn.pos_bias_u"), tt.get(p + "self_attn.pos_bias_v"),
                                             klens.as<int>(), B, T, c.n_heads, c.legacy, att, s)))
            return rc;
        if ((rc = lin(att, D, p + "self_attn.linear_out.", D, x, y, D, e.e_att))) return rc;
        std::swap(x, y);
        // convolution module
        if ((rc = ln(p + "norm_conv.", x, xn))) return rc;
        if ((rc = lin(xn, D, p + "conv_module.pointwise_conv1.", 2 * D, nullptr, hid, 2 * D, e.e_conv_in))) return rc;
        const float* bnp = tt.get("#bn") + (size_t)i * 2 * D;
        if ((rc = launch_cf_glu_dw(hid, tt.get(p + "conv_module.depthwise_conv.weight"), tt.get(p + "conv_module.depthwise_conv.bias"),
                                   bnp, bnp + D, B, T, D, c.kernel_size, att, s)))
            return rc;
        if ((rc = lin(att, D, p + "conv_module.pointwise_conv2.", D, x, y, D, e.e_cm))) return rc;
        std::swap(x, y);
        if ((rc = ffn("feed_forward.", "norm_ff.", e.e_ff_in, e.e_ff_h))) return rc;
        if ((rc = ln(p + "norm_final.", x, y))) return rc;
        std::swap(x, y);
    }
    return ln("after_norm.", x, out);
}

// ================================================================================================ Transformer encoder
// funasr/models/transformer/encoder.py TransformerEncoder (input_layer conv2d, normalize_before): the shared subsampling ->
// x sqrt(D) + pe -> blocks: LayerNorm(norm1), q / k / v GEMMs, plain masked attention, linear_out (+ residual) -> LayerNorm(norm2),
// w_1, ReLU, w_2 (+ residual); after_norm. precision 3: the block GEMMs from two-plane fp16 operands, exponents from a-priori
// bounds: the LayerNorm bounds for the q / k / v and w_1 operands, the row-L1 bound of linear_v for the attention output (a convex
// combination of value rows) and the row-L1 bound of w_1 for the hidden rows (ReLU does not enlarge it).
struct Tf : SubEnc<pf_tfencoder_config> {
    std::vector<TfBlockX> bx;
    int prepare(hipStream_t s);
    int forward(const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s);
};

int Tf::prepare(hipStream_t s) {
    const int D = cfg.d_model, NB = cfg.n_blocks;
    if (CfSub::prepare(tt, D, D, CfSub::F2(cfg.input_dim), "tfencoder")) return -2;
    bx.assign(NB, TfBlockX());
    if (cfg.precision == 3) tt.drop_bf16();
    for (int i = 0; i < NB && cfg.precision == 3; ++i) {
        const std::string p = blk(i);
        TfBlockX& x = bx[i];
        if (ln_lin_exps(p + "norm1.", p + "self_attn.linear_v.", D, &x.e_mha_in, &x.e_att, s)) return -2;
        if (ln_lin_exps(p + "norm2.", p + "feed_forward.w_1.", cfg.ffn_dim, &x.e_ff_in, &x.e_ff_h, s)) return -2;
    }
    prepared = tt.version;
    return 0;
}

int Tf::forward(const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s) {
    if (int rc = front(feats, lens, B, Tin, cfg.ffn_dim, tt.get("pos_table"), olens, s)) return rc;
    return tf_blocks(bx, B, out);
}

// ================================================================================================ E-Branchformer encoder
// funasr/models/e_branchformer/encoder.py EBranchformerEncoder (input_layer conv2d, rel_selfattn): the shared subsampling -> x sqrt(D)
// -> blocks `encoders.i.`:
//   [x += 0.5 ffm(norm_ff_macaron x)]                                        (use_ffn and macaron; Swish, 0.5 folded into w_2#half)
//   x1 = attn(norm_mha x)                                                    (the Conformer's relative-position attention + linear_out)
//   x2 = channel_proj2(csgu(GELU(channel_proj1(norm_mlp x))))                (cgMLP; launch_eb_gelu, launch_eb_csgu)
//   x += merge_proj([x1 | x2] + depthwise_conv_fusion([x1 | x2]))            (launch_eb_merge reads x1 and x2 from their own buffers)
//   [x += ff_scale ff(norm_ff x)]                                            (use_ffn)
//   x = norm_final x
// -> after_norm. Neither depthwise conv is masked: every row of the padded batch is computed in every block.
// Launches per block in fp32: 16 without feed-forwards (8 GEMMs: q, k, v, linear_pos, linear_out, channel_proj1, channel_proj2,
// merge_proj; 5 row kernels: norm_mha, norm_mlp, GELU, merge, norm_final; 2 for the gating unit: row statistics, then normalise +
// conv + gate; 1 attention), + 4 per feed-forward (LayerNorm, w_1, Swish, w_2): 24 at the template's macaron pair.
// precision 3: the block GEMMs from two-plane fp16 operands, exponents from a-priori bounds of the weights: the LayerNorm bounds for
// q / k / v, channel_proj1 and w_1; the row-L1 bound of linear_v for linear_out's operand and of w_1 for w_2's; for channel_proj2's
// operand x_r * g the product of the row-L1 bound of channel_proj1's first U / 2 rows (|GELU(v)| <= |v|) and of the gate's bound
// (csgu.norm's LayerNorm bound times the tap L1, plus |bias|). merge_proj STAYS EXACT FP32 in this mode: the bound of its operand
// ((1 + tap L1) times the row-L1 bounds of linear_out and of channel_proj2 over the product bound above, plus |bias|) compounds to
// 2^20 times the rows' size at the test fixture's weights and further at the template's widths, past the 2^17 within which a two-plane
// operand keeps its 22 bits, and with it the template-size encoder was 18 x the reference's fp32 - fp64 gap from the float64 oracle
// (DESIGN 3.16). linear_pos and the subsampling stay exact fp32 too.
struct EbBlockX { int e_ffm_in = 0, e_ffm_h = 0, e_mha_in = 0, e_att = 0, e_mlp_in = 0, e_gate = 0, e_ff_in = 0, e_ff_h = 0; };

struct Eb : SubEnc<pf_ebranchformer_config> {
    std::vector<EbBlockX> bx;
    DevBuf P, b1, b2, gate, cat, stats;
    int pos_rows() const { return cfg.legacy ? 5000 : 9999; }
    bool ffn() const { return cfg.use_ffn != 0; }
    bool macaron() const { return cfg.use_ffn != 0 && cfg.macaron != 0; }
    int prepare(hipStream_t s);
    int forward(const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s);
};

// max over the C channels of a depthwise conv (w [C][K], bias [C]) of in_bound * sum_k |w[c][k]| + |bias[c]|: an a-priori bound on
// |conv(x) + bias| for |x| <= in_bound
float dw_bound(const std::vector<float>& w, const std::vector<float>& bias, int K, int C, float in_bound) {
    float m = 0.f;
    for (int c = 0; c < C; ++c) {
        float l1 = 0.f;
        for (int k = 0; k < K; ++k) l1 += fabsf(w[(size_t)c * K + k]);
        m = fmaxf(m, in_bound * l1 + fabsf(bias[c]));
    }
    return m;
}

int Eb::prepare(hipStream_t s) {
    const int D = cfg.d_model, NB = cfg.n_blocks, FF = cfg.ffn_dim, U = cfg.cgmlp_units, C = U / 2;
    if (CfSub::prepare(tt, D, D, CfSub::F2(cfg.input_dim), "ebranchformer")) return -2;
    bx.assign(NB, EbBlockX());
    if (cfg.precision == 3) tt.drop_bf16();
    for (int i = 0; i < NB; ++i) {
        const std::string p = blk(i);
        for (const char* ff : {"feed_forward.", "feed_forward_macaron."}) {
            if (!macaron()) break;
            std::vector<float> w = tt.host(p + ff + "w_2.weight"), bb = tt.host(p + ff + "w_2.bias");
            if (w.empty() || bb.empty()) { set_error("ebranchformer: weight copy failed"); return -2; }
            for (float& v : w) v *= 0.5f;
            for (float& v : bb) v *= 0.5f;
            if (tt.put_derived(p + ff + "w_2.weight#half", w) || tt.put_derived(p + ff + "w_2.bias#half", bb)) return -2;
        }
        if (cfg.precision != 3) continue;
        EbBlockX& x = bx[i];
        if (macaron() && ln_lin_exps(p + "norm_ff_macaron.", p + "feed_forward_macaron.w_1.", FF, &x.e_ffm_in, &x.e_ffm_h, s)) return -2;
        if (ffn() && ln_lin_exps(p + "norm_ff.", p + "feed_forward.w_1.", FF, &x.e_ff_in, &x.e_ff_h, s)) return -2;
        float rb, nb;
        if (ln_lin_exps(p + "norm_mha.", p + "attn.linear_v.", D, &x.e_mha_in, &x.e_att, s)) return -2;
        int e_r;                            // (x_r alone reaches no GEMM: its bound goes into the gated product's)
        if (ln_lin_exps(p + "norm_mlp.", p + "cgmlp.channel_proj1.0.", C, &x.e_mlp_in, &e_r, s, &rb)) return -2;
        if (TensorTable::dev_ln_bound(tt.get(p + "cgmlp.csgu.norm.weight"), tt.get(p + "cgmlp.csgu.norm.bias"), C, &nb, s)) return -2;
        std::vector<float> gw = tt.host(p + "cgmlp.csgu.conv.weight"), gb = tt.host(p + "cgmlp.csgu.conv.bias");
        if (gw.empty() || gb.empty()) { set_error("ebranchformer: weight copy failed"); return -2; }
        x.e_gate = exp_for_bound(rb * dw_bound(gw, gb, cfg.cgmlp_kernel, C, nb));
    }
    prepared = tt.version;
    return 0;
}

int Eb::forward(const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s) {
    const pf_ebranchformer_config& c = cfg;
    const int D = c.d_model, FF = c.ffn_dim, U = c.cgmlp_units, C = U / 2;
    int rc;
    if ((rc = front(feats, lens, B, Tin, std::max(ffn() ? FF : 0, U), nullptr, olens, s))) return rc;
    const int nP = c.legacy ? T : 2 * T - 1;
    const size_t M = (size_t)Mi;
    if (P.ensure(sizeof(float) * (size_t)nP * D) || b1.ensure(sizeof(float) * M * D) || b2.ensure(sizeof(float) * M * D) ||
        gate.ensure(sizeof(float) * M * C) || cat.ensure(sizeof(float) * M * 2 * D) || stats.ensure(sizeof(float) * M * 2))
        return -2;
    const float* pos = tt.get("pos_table") + (c.legacy ? (size_t)0 : (size_t)(5000 - T) * D);
    float *x = xa.as<float>(), *y = xb.as<float>(), *xn = this->xn.as<float>(), *qkv = this->qkv.as<float>(), *Pm = P.as<float>(),
          *att = this->att.as<float>(), *hid = this->hid.as<float>(), *x1 = b1.as<float>(), *x2 = b2.as<float>(), *g = gate.as<float>(),
          *cc = cat.as<float>();
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        const EbBlockX& e = bx[i];
        const char* half = macaron() ? "#half" : "";
        auto ff = [&](const std::string& f, const std::string& norm, int e_in, int e_h) {
            int r;
            if ((r = ln(p + norm, x, xn))) return r;
            if ((r = lin(xn, D, p + f + "w_1.", FF, nullptr, hid, FF, e_in))) return r;
            if ((r = launch_cf_act(hid, M * FF, 1, s))) return r;
            if ((r = lin(hid, FF, p + f + "w_2.", D, x, y, D, e_h, half))) return r;
            std::swap(x, y);
            return 0;
        };
        if (macaron() && (rc = ff("feed_forward_macaron.", "norm_ff_macaron.", e.e_ffm_in, e.e_ffm_h))) return rc;
        // branch 1: relative-position self-attention -> x1
        if ((rc = ln(p + "norm_mha.", x, xn))) return rc;
        const char* names[3] = {"attn.linear_q.", "attn.linear_k.", "attn.linear_v."};
        for (int j = 0; j < 3; ++j)
            if ((rc = lin(xn, D, p + names[j], D, nullptr, qkv + (size_t)j * D, 3 * D, e.e_mha_in))) return rc;
        if ((rc = gm(false, pos, nP, D, p + "attn.linear_pos.weight", nullptr, D, nullptr, Pm, D, 0))) return rc;
        if ((rc = launch_cf_relpos_attention(qkv, Pm, tt.get(p + "attn.pos_bias_u"), tt.get(p + "attn.pos_bias_v"), klens.as<int>(), B, T,
                                             c.n_heads, c.legacy, att, s)))
            return rc;
        if ((rc = lin(att, D, p + "attn.linear_out.", D, nullptr, x1, D, e.e_att))) return rc;
        // branch 2: cgMLP -> x2
        if ((rc = ln(p + "norm_mlp.", x, xn))) return rc;
        if ((rc = lin(xn, D, p + "cgmlp.channel_proj1.0.", U, nullptr, hid, U, e.e_mlp_in))) return rc;
        if ((rc = launch_eb_gelu(hid, M * U, s))) return rc;
        if ((rc = launch_eb_csgu(hid, tt.get(p + "cgmlp.csgu.norm.weight"), tt.get(p + "cgmlp.csgu.norm.bias"), c.ln_eps,
                                 tt.get(p + "cgmlp.csgu.conv.weight"), tt.get(p + "cgmlp.csgu.conv.bias"), B, T, C, c.cgmlp_kernel,
                                 stats.as<float>(), g, s)))
            return rc;
        if ((rc = lin(g, C, p + "cgmlp.channel_proj2.", D, nullptr, x2, D, e.e_gate))) return rc;
        // merge
        if ((rc = launch_eb_merge(x1, x2, tt.get(p + "depthwise_conv_fusion.weight"), tt.get(p + "depthwise_conv_fusion.bias"), B, T, D,
                                  c.merge_kernel, cc, s)))
            return rc;
        if ((rc = gm(false, cc, Mi, 2 * D, p + "merge_proj.weight", tt.get(p + "merge_proj.bias"), D, x, y, D, 0))) return rc;   // fp32 in both modes
        std::swap(x, y);
        if (ffn() && (rc = ff("feed_forward.", "norm_ff.", e.e_ff_in, e.e_ff_h))) return rc;
        if ((rc = ln(p + "norm_final.", x, y))) return rc;
        std::swap(x, y);
    }
    return ln("after_norm.", x, out);
}

// ================================================================================================ LCB-Net: text encoder, fusion layer
// funasr/models/lcbnet/encoder.py. TransformerTextEncoder: Embedding x sqrt(D) + pe -> the block loop of the Transformer encoder ->
// after_norm; its front is the token rows instead of the subsampling. FusionSANEncoder (SelfSrcAttention), ONE layer over the audio
// encoder's rows x and the text encoder's rows mem: the block above with a cross-attention between its two halves,
//   x += self_attn(norm1 x); x += src_attn(norm2 x, mem, mem); x += ffn(norm3 x).
// Both handles run exact-fp32 GEMMs (precision 0 of the shared helpers): no a-priori bound crosses the handles (the text encoder's
// after_norm feeds the fusion layer's K / V projections), and the rows are few and run once per utterance.
struct LcbCfg { int vocab_size = 0, d_model = 0, n_heads = 0, ffn_dim = 0, n_blocks = 0, precision = 0, input_dim = 0; float ln_eps = 0.f; };

struct Te : SubEnc<LcbCfg> {
    std::vector<TfBlockX> bx;
    DevBuf ids;
};

struct Fu : SubEnc<LcbCfg> {
    DevBuf kv, mlens;
};

bool lcb_shape_ok(int d_model, int n_heads, int ffn_dim, float ln_eps) {
    return d_model > 0 && d_model <= 2048 && n_heads > 0 && d_model == 64 * n_heads && ffn_dim > 0 && ffn_dim % 32 == 0 && ln_eps > 0.f;
}

// the tensors of one block of plain attention + feed-forward: `attns` attention groups, `norms` LayerNorms
int add_tf_block(TensorTable& tt, const std::string& p, std::initializer_list<const char*> attns, std::initializer_list<const char*> norms,
                 int D, int FF) {
    int rc = 0;
    for (const char* a : attns)
        for (const char* n : {"linear_q.", "linear_k.", "linear_v.", "linear_out."}) rc |= tt.add_linear(p + a + n, D, D);
    rc |= tt.add_linear(p + "feed_forward.w_1.", FF, D);
    rc |= tt.add_linear(p + "feed_forward.w_2.", D, FF);
    for (const char* n : norms) rc |= tt.add_linear(p + n, D, 1);
    return rc;
}

// ================================================================================================ decoder steppers
// What the Transformer and the SAN-M decoder steppers share. Cfg: pf_tdecoder_config / pf_fsmndecoder_config (the fields read here
// carry the same names in both).
template <class Cfg> struct Stepper {
    Cfg cfg;
    TensorTable tt;
    DevBuf ckv, x, y, xn, q, a, hid, logits, ids, par;
    int T = 0, max_len = 0, max_hyp = 0, filled = 0, cur = 0;
    int n = 0;                             // the step in flight (step_common_checks): its hypotheses, its stream
    hipStream_t s = nullptr;

    // the Linear named `p` over the step's rows: out[n, N] (row stride ldc) = in[n, K] W^T (+ bias) (ReLU) (+ residual [n, d_model])
    int lin(const std::string& p, const float* in, int K, float* out, int ldc, int N, bool relu = false, const float* residual = nullptr,
            bool bias = true) {
        return gemm_simple(in, K, tt.get(p + "weight"), K, bias ? tt.get(p + "bias") : nullptr, out, ldc, n, N, K, relu, residual,
                           residual ? cfg.d_model : 0, nullptr, 0, s);
    }
    // the LayerNorm named `p` over the step's rows of W floats
    int norm(const std::string& p, const float* in, float* out, int W) {
        return layernorm(in, W, tt.get(p + "weight"), tt.get(p + "bias"), out, W, n, W, W, cfg.ln_eps, s);
    }
    // src_attn of the layer `p`: y = x + linear_out(attention(linear_q(xn))); `attn`: the family's launch from q into a
    template <class Attn> int cross_attention(const std::string& p, const float* xn_, const float* x_, float* y_, Attn attn) {
        const int D = cfg.d_model;
        int rc;
        if ((rc = lin(p + "src_attn.linear_q.", xn_, D, q.as<float>(), D, D))) return rc;
        if ((rc = attn())) return rc;
        return lin(p + "src_attn.linear_out.", a.as<float>(), D, y_, D, D, false, x_);
    }
    // logp [n, V] = log_softmax(output_layer(after_norm(x)))
    int output_tail(const float* x_, float* logp) {
        const int D = cfg.d_model, V = cfg.vocab_size;
        int rc;
        if ((rc = norm("after_norm.", x_, xn.as<float>(), D))) return rc;
        if ((rc = lin("output_layer.", xn.as<float>(), D, logits.as<float>(), V, V))) return rc;
        return launch_log_softmax(logits.as<float>(), V, logp, V, n, V, s);
    }
};

// The argument checks of both steppers; `who`: the family word ("tdecoder" / "fsmndecoder"). A family's own rule comes in as
// `rule` (returns 0, or a refusal's code after set_error) and runs where it always stood, so the refusals keep their order.
// begin(): the range check in the family's words (`ranges_msg`), the state reset, the buffers both hold (ckv: K | V of n_cross layers)
template <class H>
int begin_common(H* h, const char* who, const char* ranges_msg, const float* memory, int T, int max_len, int max_hyp, int n_cross) {
    PF_REQUIRE(h && memory && T > 0 && T <= 12000 && max_len > 0 && max_len <= 5000 && max_hyp > 0 && max_hyp <= 256, ranges_msg);
    if (h->tt.require_all(who)) return -3;
    h->T = T; h->max_len = max_len; h->max_hyp = max_hyp; h->filled = 0; h->cur = 0;
    const size_t n = (size_t)max_hyp, D = h->cfg.d_model;
    if (h->ckv.ensure(sizeof(float) * (size_t)n_cross * T * 2 * D) || h->x.ensure(sizeof(float) * n * D) || h->y.ensure(sizeof(float) * n * D) ||
        h->xn.ensure(sizeof(float) * n * D) || h->q.ensure(sizeof(float) * n * D) || h->a.ensure(sizeof(float) * n * D) ||
        h->hid.ensure(sizeof(float) * n * h->cfg.ffn_dim) || h->logits.ensure(sizeof(float) * n * h->cfg.vocab_size) ||
        h->ids.ensure(sizeof(int32_t) * n) || h->par.ensure(sizeof(int32_t) * n))
        return -2;
    return 0;
}
// step(): arguments, the family's rule for `pos` and `n`, the token ids; then the ids go up and the step is in flight
template <class H, class Rule>
int step_common_checks(H* h, const std::string& who, const int32_t* tokens_host, const float* logp, int n, Rule rule, hipStream_t s) {
    PF_REQUIRE(h && tokens_host && logp && h->max_len > 0, who + "_step: null argument or no begin()");
    if (int rc = rule()) return rc;
    for (int i = 0; i < n; ++i)
        PF_REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < h->cfg.vocab_size, who + "_step: token id outside the vocabulary");
    if (upload_h2d(h->ids.p, tokens_host, sizeof(int32_t) * n, s)) return -2;
    h->n = n; h->s = s;
    return 0;
}
// reorder(): arguments, parents; 1 when no position is filled yet (nothing to do); else the family's rule, then the parents go up
template <class H, class Rule>
int reorder_common(H* h, const std::string& who, const int32_t* parents_host, int n, Rule rule, hipStream_t s) {
    PF_REQUIRE(h && parents_host && h->max_len > 0 && n > 0 && n <= h->max_hyp, who + "_reorder: null argument, no begin() or n_hyp > max_hyp");
    for (int i = 0; i < n; ++i) PF_REQUIRE(parents_host[i] >= 0 && parents_host[i] < h->max_hyp, who + "_reorder: parent slot out of range");
    if (h->filled == 0) return 1;
    if (int rc = rule()) return rc;
    return upload_h2d(h->par.p, parents_host, sizeof(int32_t) * n, s) ? -2 : 0;
}

struct Td : Stepper<pf_tdecoder_config> {
    DevBuf cache;
    size_t slot() const { return (size_t)max_len * 2 * cfg.d_model; }
    size_t layer() const { return slot() * max_hyp; }
    float* cache_of(int which, int l) { return cache.as<float>() + ((size_t)which * cfg.n_blocks + l) * layer(); }
};

std::string dl(int i) { return "decoders." + std::to_string(i) + "."; }

// ================================================================================================ E-Paraformer: PIF predictor, SAN decoder
// funasr/models/e_paraformer. The predictor (pf_pif_*, kernels in pif.hip) is two calls around ONE host read of the B token sums, as
// the CIF predictor's: alphas() -> the caller rounds the sums (half to even) -> embeds() with the counts. Exact fp32 in every mode.
struct Pif {
    pf_pif_config cfg;
    TensorTable tt;
    DevBuf lens, counts;
};

// The decoder (pf_sandecoder_*; ParaformerSANDecoder.forward, decoder.py:1201-1251) runs ONCE over all B x L token rows: the rows are
// the predictor's embeddings (no lookup, no positional row), per layer `decoders.i.`
//   x += linear_out(attention(norm1 x))                  keys at or past the clip's token count masked, NOT causal (launch_tf_attention)
//   x += linear_out(attention(norm2 x, memory))          keys at or past the clip's encoder length masked (launch_tf_cross_attention)
//   x += w_2(relu(w_1(norm3 x)))
// then after_norm, output_layer, log-softmax, row arg-max. It is the LCB-Net fusion layer's block n_blocks times on the same base.
// Launches per forward: 18 per layer (3 LayerNorms, 10 GEMMs, 2 attentions, ReLU; K and V of the memory are two GEMMs into one
// [B T, 2 D] buffer) + 5 (after_norm, output_layer, log-softmax, arg-max, its log-probability).
// precision 3: from two-plane fp16 operands run the GEMMs whose operand has an a-priori bound -- self_attn q / k / v (norm1's
// LayerNorm bound), self_attn.linear_out (the row-L1 bound of linear_v: the attention output is a convex combination of value rows,
// or zero), src_attn.linear_q (norm2's bound), w_1 (norm3's bound) and w_2 (the row-L1 bound of w_1; ReLU does not enlarge it).
// Exact fp32 in both modes: src_attn.linear_k / linear_v (their operand is the CALLER's memory, for which no bound exists inside this
// handle), src_attn.linear_out (its operand is bounded only through that memory) and output_layer (V = 4234 is no multiple of 4, and
// the arg-max of its rows is the result).
struct SdBlockX { int e_sa_in = 0, e_sa = 0, e_ca_in = 0, e_ff_in = 0, e_ff_h = 0; };

struct Sd : SubEnc<LcbCfg> {
    std::vector<SdBlockX> bx;
    DevBuf kv, mlens, logits;
    int prepare(hipStream_t ps) {
        const int D = cfg.d_model;
        bx.assign(cfg.n_blocks, SdBlockX());
        for (int i = 0; i < cfg.n_blocks && cfg.precision == 3; ++i) {
            const std::string p = dl(i);
            SdBlockX& x = bx[i];
            int unused;
            if (ln_lin_exps(p + "norm1.", p + "self_attn.linear_v.", D, &x.e_sa_in, &x.e_sa, ps)) return -2;
            if (ln_lin_exps(p + "norm2.", p + "src_attn.linear_q.", D, &x.e_ca_in, &unused, ps)) return -2;
            if (ln_lin_exps(p + "norm3.", p + "feed_forward.w_1.", cfg.ffn_dim, &x.e_ff_in, &x.e_ff_h, ps)) return -2;
        }
        prepared = tt.version;
        return 0;
    }
};

// ================================================================================================ SAN-M (FsmnDecoder) step
// One layer table for the three groups of the reference's module: `decoders` (FFN, FSMN memory, cross-attention), `decoders2` (FFN,
// FSMN memory) and the one FFN-only layer of `decoders3`.
struct FdLayer { std::string p; bool fsmn, cross; };

struct Fd : Stepper<pf_fsmndecoder_config> {
    std::vector<FdLayer> layers;
    DevBuf win, t, hidn;
    int n_prev = 0, n_par = 0;
    int n_fsmn() const { return cfg.n_blocks; }
    int left_pad() const { return (cfg.kernel_size - 1) / 2 + (cfg.sanm_shift > 0 ? cfg.sanm_shift : 0); }
    size_t slot() const { return (size_t)cfg.kernel_size * cfg.d_model; }            // the window of one (layer, slot): K columns
    size_t layer() const { return slot() * max_hyp; }
    float* win_of(int which, int l) { return win.as<float>() + ((size_t)which * n_fsmn() + l) * layer(); }
};

// the limits of the handle, one message per field; nullptr = accepted
const char* fd_refusal(const pf_fsmndecoder_config& c) {
    if (c.vocab_size < 1) return "fsmndecoder: vocab_size must be positive";
    if (c.n_heads < 1 || (c.d_model != 64 * c.n_heads && c.d_model != 128 * c.n_heads))
        return "fsmndecoder: n_heads with d_model: only a head dim of 64 or 128 is built";
    if (c.d_model > 2048) return "fsmndecoder: d_model above 2048";
    if (c.ffn_dim < 32 || c.ffn_dim % 32 != 0 || c.ffn_dim > 2048) return "fsmndecoder: ffn_dim must be a multiple of 32 up to 2048";
    if (c.kernel_size < 1 || c.kernel_size > 32) return "fsmndecoder: kernel_size outside 1 .. 32";
    if (c.sanm_shift < 0 || (c.kernel_size - 1) / 2 + c.sanm_shift > c.kernel_size - 1)
        return "fsmndecoder: sanm_shift leaves a negative right padding (kernel_size - 1 - (kernel_size - 1) / 2 - sanm_shift < 0)";
    if (c.n_blocks < 1 || c.att_layer_num < 1 || c.att_layer_num > c.n_blocks) return "fsmndecoder: att_layer_num outside 1 .. n_blocks";
    if (!(c.ln_eps > 0.f)) return "fsmndecoder: ln_eps must be positive";
    return nullptr;
}

}  // namespace

extern "C" {

pf_conformer* pf_conformer_create(const pf_conformer_config* cfg) {
    if (!cfg) { set_error("conformer: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_conformer_config& c = *cfg;
    const bool ok = c.input_dim >= 7 && c.input_dim <= 256 && c.d_model > 0 && c.d_model % 64 == 0 && c.d_model <= 2048 &&
                    c.n_heads > 0 && c.d_model == 64 * c.n_heads && c.ffn_dim > 0 && c.ffn_dim % 32 == 0 && c.n_blocks >= 0 &&
                    c.kernel_size % 2 == 1 && c.kernel_size >= 1 && c.kernel_size <= 31 && (c.macaron == 0 || c.macaron == 1) &&
                    (c.legacy == 0 || c.legacy == 1) && (c.precision == 0 || c.precision == 3) && c.ln_eps > 0.f;
    if (!ok) {
        set_error("conformer: unsupported config (7 .. 256 input features, head dim 64, d_model % 64, ffn_dim % 32, odd kernel <= 31, "
                  "precision 0 or 3)");
        return nullptr;
    }
    std::unique_ptr<Cf> h(new Cf());
    h->cfg = c;
    TensorTable& tt = h->tt;
    const int D = c.d_model, C = c.d_model, FF = c.ffn_dim, K = c.kernel_size;
    int rc = 0;
    rc |= tt.add_linear("embed.conv.0.", C, 9);
    rc |= tt.add_linear("embed.conv.2.", C, (int64_t)C * 9);
    rc |= tt.add_linear("embed.out.0.", D, (int64_t)C * h->F2());
    rc |= tt.add("pos_table", (int64_t)h->pos_rows() * D);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        for (const char* n : {"linear_q.", "linear_k.", "linear_v.", "linear_out."}) rc |= tt.add_linear(p + "self_attn." + n, D, D);
        rc |= tt.add_linear(p + "self_attn.linear_pos.", D, D, false);
        rc |= tt.add(p + "self_attn.pos_bias_u", D);
        rc |= tt.add(p + "self_attn.pos_bias_v", D);
        rc |= tt.add_linear(p + "feed_forward.w_1.", FF, D);
        rc |= tt.add_linear(p + "feed_forward.w_2.", D, FF);
        if (c.macaron) {
            rc |= tt.add_linear(p + "feed_forward_macaron.w_1.", FF, D);
            rc |= tt.add_linear(p + "feed_forward_macaron.w_2.", D, FF);
            rc |= tt.add_linear(p + "norm_ff_macaron.", D, 1);
        }
        rc |= tt.add_linear(p + "conv_module.pointwise_conv1.", 2 * D, D);
        rc |= tt.add_linear(p + "conv_module.depthwise_conv.", D, K);
        rc |= tt.add_linear(p + "conv_module.norm.", D, 1);
        rc |= tt.add(p + "conv_module.norm.running_mean", D);
        rc |= tt.add(p + "conv_module.norm.running_var", D);
        rc |= tt.add_linear(p + "conv_module.pointwise_conv2.", D, D);
        for (const char* n : {"norm_ff.", "norm_mha.", "norm_conv.", "norm_final."}) rc |= tt.add_linear(p + n, D, 1);
    }
    rc |= tt.add_linear("after_norm.", D, 1);
    if (rc) return nullptr;
    return reinterpret_cast<pf_conformer*>(h.release());
}
void pf_conformer_destroy(pf_conformer* h) { delete reinterpret_cast<Cf*>(h); }
int pf_conformer_set_tensor(pf_conformer* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Cf*>(h), "conformer_set_tensor: null", name, data, numel);
}
int pf_conformer_missing(const pf_conformer* h) { return table_missing(reinterpret_cast<const Cf*>(h)); }
int pf_conformer_set_precision(pf_conformer* h, int32_t precision) { return enc_set_precision(reinterpret_cast<Cf*>(h), "conformer", precision); }
int32_t pf_conformer_num_frames(const pf_conformer* h, int32_t n_frames, int32_t padded_frames) { return enc_num_frames(h, n_frames, padded_frames); }
int pf_conformer_forward(pf_conformer* h, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, float* out,
                         int32_t* out_lens_host, void* stream) {
    return enc_forward(reinterpret_cast<Cf*>(h), "conformer", "tables hold", feats, lens_host, B, Tin, out, out_lens_host, stream);
}

pf_tfencoder* pf_tfencoder_create(const pf_tfencoder_config* cfg) {
    if (!cfg) { set_error("tfencoder: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_tfencoder_config& c = *cfg;
    const bool ok = c.input_dim >= 7 && c.input_dim <= 256 && c.d_model > 0 && c.d_model % 64 == 0 && c.d_model <= 2048 &&
                    c.n_heads > 0 && c.d_model == 64 * c.n_heads && c.ffn_dim > 0 && c.ffn_dim % 32 == 0 && c.n_blocks >= 0 &&
                    (c.precision == 0 || c.precision == 3) && c.ln_eps > 0.f;
    if (!ok) {
        set_error("tfencoder: unsupported config (7 .. 256 input features, head dim 64, d_model % 64, ffn_dim % 32, precision 0 or 3)");
        return nullptr;
    }
    std::unique_ptr<Tf> h(new Tf());
    h->cfg = c;
    TensorTable& tt = h->tt;
    const int D = c.d_model, FF = c.ffn_dim;
    int rc = 0;
    rc |= tt.add_linear("embed.conv.0.", D, 9);
    rc |= tt.add_linear("embed.conv.2.", D, (int64_t)D * 9);
    rc |= tt.add_linear("embed.out.0.", D, (int64_t)D * CfSub::F2(c.input_dim));
    rc |= tt.add("pos_table", (int64_t)5000 * D);
    for (int i = 0; i < c.n_blocks; ++i) rc |= add_tf_block(tt, blk(i), {"self_attn."}, {"norm1.", "norm2."}, D, FF);
    rc |= tt.add_linear("after_norm.", D, 1);
    if (rc) return nullptr;
    return reinterpret_cast<pf_tfencoder*>(h.release());
}
void pf_tfencoder_destroy(pf_tfencoder* h) { delete reinterpret_cast<Tf*>(h); }
int pf_tfencoder_set_tensor(pf_tfencoder* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Tf*>(h), "tfencoder_set_tensor: null", name, data, numel);
}
int pf_tfencoder_missing(const pf_tfencoder* h) { return table_missing(reinterpret_cast<const Tf*>(h)); }
int pf_tfencoder_set_precision(pf_tfencoder* h, int32_t precision) { return enc_set_precision(reinterpret_cast<Tf*>(h), "tfencoder", precision); }
int32_t pf_tfencoder_num_frames(const pf_tfencoder* h, int32_t n_frames, int32_t padded_frames) { return enc_num_frames(h, n_frames, padded_frames); }
int pf_tfencoder_forward(pf_tfencoder* h, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, float* out,
                         int32_t* out_lens_host, void* stream) {
    return enc_forward(reinterpret_cast<Tf*>(h), "tfencoder", "table holds", feats, lens_host, B, Tin, out, out_lens_host, stream);
}

pf_ebranchformer* pf_ebranchformer_create(const pf_ebranchformer_config* cfg) {
    if (!cfg) { set_error("ebranchformer: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_ebranchformer_config& c = *cfg;
    auto odd31 = [](int k) { return k % 2 == 1 && k >= 1 && k <= 31; };
    auto flag = [](int v) { return v == 0 || v == 1; };
    const bool ok = c.input_dim >= 7 && c.input_dim <= 256 && c.d_model > 0 && c.d_model % 64 == 0 && c.d_model <= 2048 && c.n_heads > 0 &&
                    c.d_model == 64 * c.n_heads && c.n_blocks >= 0 && c.cgmlp_units > 0 && c.cgmlp_units % 64 == 0 && c.cgmlp_units <= 16384 &&
                    odd31(c.cgmlp_kernel) && odd31(c.merge_kernel) && flag(c.use_ffn) && flag(c.macaron) && flag(c.legacy) &&
                    (!c.use_ffn || (c.ffn_dim > 0 && c.ffn_dim % 32 == 0)) && (c.precision == 0 || c.precision == 3) && c.ln_eps > 0.f;
    if (!ok) {
        set_error("ebranchformer: unsupported config (7 .. 256 input features, head dim 64, d_model % 64, cgmlp_units % 64 (gate channels "
                  "% 32), ffn_dim % 32, odd conv kernels <= 31, precision 0 or 3)");
        return nullptr;
    }
    std::unique_ptr<Eb> h(new Eb());
    h->cfg = c;
    TensorTable& tt = h->tt;
    const int D = c.d_model, FF = c.ffn_dim, U = c.cgmlp_units;
    int rc = 0;
    rc |= tt.add_linear("embed.conv.0.", D, 9);
    rc |= tt.add_linear("embed.conv.2.", D, (int64_t)D * 9);
    rc |= tt.add_linear("embed.out.0.", D, (int64_t)D * CfSub::F2(c.input_dim));
    rc |= tt.add("pos_table", (int64_t)h->pos_rows() * D);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        for (const char* n : {"linear_q.", "linear_k.", "linear_v.", "linear_out."}) rc |= tt.add_linear(p + "attn." + n, D, D);
        rc |= tt.add_linear(p + "attn.linear_pos.", D, D, false);
        rc |= tt.add(p + "attn.pos_bias_u", D);
        rc |= tt.add(p + "attn.pos_bias_v", D);
        rc |= tt.add_linear(p + "cgmlp.channel_proj1.0.", U, D);
        rc |= tt.add_linear(p + "cgmlp.csgu.norm.", U / 2, 1);
        rc |= tt.add_linear(p + "cgmlp.csgu.conv.", U / 2, c.cgmlp_kernel);
        rc |= tt.add_linear(p + "cgmlp.channel_proj2.", D, U / 2);
        rc |= tt.add_linear(p + "depthwise_conv_fusion.", 2 * D, c.merge_kernel);
        rc |= tt.add_linear(p + "merge_proj.", D, 2 * D);
        if (h->ffn()) {
            rc |= tt.add_linear(p + "feed_forward.w_1.", FF, D);
            rc |= tt.add_linear(p + "feed_forward.w_2.", D, FF);
            rc |= tt.add_linear(p + "norm_ff.", D, 1);
        }
        if (h->macaron()) {
            rc |= tt.add_linear(p + "feed_forward_macaron.w_1.", FF, D);
            rc |= tt.add_linear(p + "feed_forward_macaron.w_2.", D, FF);
            rc |= tt.add_linear(p + "norm_ff_macaron.", D, 1);
        }
        for (const char* n : {"norm_mha.", "norm_mlp.", "norm_final."}) rc |= tt.add_linear(p + n, D, 1);
    }
    rc |= tt.add_linear("after_norm.", D, 1);
    if (rc) return nullptr;
    return reinterpret_cast<pf_ebranchformer*>(h.release());
}
void pf_ebranchformer_destroy(pf_ebranchformer* h) { delete reinterpret_cast<Eb*>(h); }
int pf_ebranchformer_set_tensor(pf_ebranchformer* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Eb*>(h), "ebranchformer_set_tensor: null", name, data, numel);
}
int pf_ebranchformer_missing(const pf_ebranchformer* h) { return table_missing(reinterpret_cast<const Eb*>(h)); }
int pf_ebranchformer_set_precision(pf_ebranchformer* h, int32_t precision) {
    return enc_set_precision(reinterpret_cast<Eb*>(h), "ebranchformer", precision);
}
int32_t pf_ebranchformer_num_frames(const pf_ebranchformer* h, int32_t n_frames, int32_t padded_frames) {
    return enc_num_frames(h, n_frames, padded_frames);
}
int pf_ebranchformer_forward(pf_ebranchformer* h, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, float* out,
                             int32_t* out_lens_host, void* stream) {
    return enc_forward(reinterpret_cast<Eb*>(h), "ebranchformer", "tables hold", feats, lens_host, B, Tin, out, out_lens_host, stream);
}

pf_tdecoder* pf_tdecoder_create(const pf_tdecoder_config* cfg) {
    if (!cfg) { set_error("tdecoder: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_tdecoder_config& c = *cfg;
    if (!(c.vocab_size > 0 && c.d_model > 0 && c.d_model % 64 == 0 && c.d_model <= 2048 && c.n_heads > 0 && c.d_model == 64 * c.n_heads &&
          c.ffn_dim > 0 && c.ffn_dim % 32 == 0 && c.n_blocks > 0 && c.ln_eps > 0.f)) {
        set_error("tdecoder: unsupported config (head dim 64, d_model % 64, ffn_dim % 32)");
        return nullptr;
    }
    std::unique_ptr<Td> h(new Td());
    h->cfg = c;
    TensorTable& tt = h->tt;
    const int D = c.d_model, FF = c.ffn_dim, V = c.vocab_size;
    int rc = 0;
    rc |= tt.add("embed.0.weight", (int64_t)V * D);
    rc |= tt.add("pos_table", (int64_t)5000 * D);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = dl(i);
        for (const char* a : {"self_attn.", "src_attn."})
            for (const char* n : {"linear_q.", "linear_k.", "linear_v.", "linear_out."}) rc |= tt.add_linear(p + a + n, D, D);
        rc |= tt.add_linear(p + "feed_forward.w_1.", FF, D);
        rc |= tt.add_linear(p + "feed_forward.w_2.", D, FF);
        for (const char* n : {"norm1.", "norm2.", "norm3."}) rc |= tt.add_linear(p + n, D, 1);
    }
    rc |= tt.add_linear("after_norm.", D, 1);
    rc |= tt.add_linear("output_layer.", V, D);
    if (rc) return nullptr;
    return reinterpret_cast<pf_tdecoder*>(h.release());
}
void pf_tdecoder_destroy(pf_tdecoder* h) { delete reinterpret_cast<Td*>(h); }
int pf_tdecoder_set_tensor(pf_tdecoder* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Td*>(h), "tdecoder_set_tensor: null", name, data, numel);
}
int pf_tdecoder_missing(const pf_tdecoder* h) { return table_missing(reinterpret_cast<const Td*>(h)); }
int pf_tdecoder_begin(pf_tdecoder* hh, const float* memory, int32_t T, int32_t max_len, int32_t max_hyp, void* stream) {
    Td* h = reinterpret_cast<Td*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if ((rc = begin_common(h, "tdecoder", "tdecoder_begin: 1 .. 12000 memory rows, 1 .. 5000 positions, 1 .. 256 hypotheses", memory, T, max_len,
                           max_hyp, h ? h->cfg.n_blocks : 0)))
        return rc;
    const int D = h->cfg.d_model, L = h->cfg.n_blocks;
    if (h->cache.ensure(sizeof(float) * 2 * L * h->layer())) return -2;
    for (int l = 0; l < L; ++l) {
        const std::string p = dl(l) + "src_attn.";
        float* kv = h->ckv.as<float>() + (size_t)l * T * 2 * D;
        GemmArgs g{};
        g.A = memory; g.lda = D; g.ldw = D; g.ldc = 2 * D; g.M = T; g.N = D; g.K = D;
        g.W = h->tt.get(p + "linear_k.weight"); g.bias = h->tt.get(p + "linear_k.bias"); g.C = kv;
        if ((rc = launch_gemm_f32(g, s))) return rc;
        g.W = h->tt.get(p + "linear_v.weight"); g.bias = h->tt.get(p + "linear_v.bias"); g.C = kv + D;
        if ((rc = launch_gemm_f32(g, s))) return rc;
    }
    return 0;
}
int pf_tdecoder_step(pf_tdecoder* hh, const int32_t* tokens_host, int32_t pos, int32_t n, float* logp, void* stream) {
    Td* h = reinterpret_cast<Td*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if ((rc = step_common_checks(h, "tdecoder", tokens_host, logp, n, [&] {
             PF_REQUIRE(n > 0 && n <= h->max_hyp && pos >= 0 && pos < h->max_len && pos <= h->filled,
                        "tdecoder_step: n_hyp <= max_hyp, positions appended in order below max_len");
             return 0;
         }, s)))
        return rc;
    const pf_tdecoder_config& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim, H = c.n_heads, T = h->T;
    StreamModeScope small_m;                         // every GEMM of the step has M = n_hyp rows: the weight-streaming kernel
    float *x = h->x.as<float>(), *y = h->y.as<float>(), *xn = h->xn.as<float>(), *q = h->q.as<float>(), *a = h->a.as<float>(),
          *hid = h->hid.as<float>();
    if ((rc = launch_td_embed(h->tt.get("embed.0.weight"), h->ids.as<int>(), h->tt.get("pos_table") + (size_t)pos * D, sqrtf((float)D), x, n,
                              D, s)))
        return rc;
    const int ldslot = (int)h->slot();
    for (int l = 0; l < c.n_blocks; ++l) {
        const std::string p = dl(l);
        float* cache = h->cache_of(h->cur, l);
        float* at_pos = cache + (size_t)pos * 2 * D;             // K | V of this position, one row per hypothesis slot
        if ((rc = h->norm(p + "norm1.", x, xn, D))) return rc;
        if ((rc = h->lin(p + "self_attn.linear_q.", xn, D, q, D, D))) return rc;
        if ((rc = h->lin(p + "self_attn.linear_k.", xn, D, at_pos, ldslot, D))) return rc;
        if ((rc = h->lin(p + "self_attn.linear_v.", xn, D, at_pos + D, ldslot, D))) return rc;
        if ((rc = launch_td_attention(q, cache, cache + D, 2 * D, h->slot(), pos + 1, n, H, a, s))) return rc;
        if ((rc = h->lin(p + "self_attn.linear_out.", a, D, y, D, D, false, x))) return rc;
        std::swap(x, y);
        if ((rc = h->norm(p + "norm2.", x, xn, D))) return rc;
        const float* kv = h->ckv.as<float>() + (size_t)l * T * 2 * D;
        if ((rc = h->cross_attention(p, xn, x, y, [&] { return launch_td_attention(q, kv, kv + D, 2 * D, 0, T, n, H, a, s); }))) return rc;
        std::swap(x, y);
        if ((rc = h->norm(p + "norm3.", x, xn, D))) return rc;
        if ((rc = h->lin(p + "feed_forward.w_1.", xn, D, hid, FF, FF, true))) return rc;
        if ((rc = h->lin(p + "feed_forward.w_2.", hid, FF, y, D, D, false, x))) return rc;
        std::swap(x, y);
    }
    if ((rc = h->output_tail(x, logp))) return rc;
    h->filled = std::max(h->filled, pos + 1);
    return 0;
}
int pf_tdecoder_reorder(pf_tdecoder* hh, const int32_t* parents_host, int32_t n, void* stream) {
    Td* h = reinterpret_cast<Td*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if ((rc = reorder_common(h, "tdecoder", parents_host, n, [] { return 0; }, s))) return rc < 0 ? rc : 0;
    if ((rc = launch_td_reorder(h->cache_of(h->cur, 0), h->cache_of(h->cur ^ 1, 0), h->par.as<int>(), n, h->cfg.n_blocks, h->layer(), h->slot(),
                                h->filled, 2 * h->cfg.d_model, s)))
        return rc;
    h->cur ^= 1;
    return 0;
}

pf_fsmndecoder* pf_fsmndecoder_create(const pf_fsmndecoder_config* cfg) {
    if (!cfg) { set_error("fsmndecoder: null config"); return nullptr; }
    if (const char* why = fd_refusal(*cfg)) { set_error(why); return nullptr; }     // (before any device call)
    if (check_device()) return nullptr;
    const pf_fsmndecoder_config& c = *cfg;
    std::unique_ptr<Fd> h(new Fd());
    h->cfg = c;
    TensorTable& tt = h->tt;
    const int D = c.d_model, FF = c.ffn_dim, V = c.vocab_size, K = c.kernel_size;
    for (int i = 0; i < c.att_layer_num; ++i) h->layers.push_back({dl(i), true, true});
    for (int i = 0; i < c.n_blocks - c.att_layer_num; ++i) h->layers.push_back({"decoders2." + std::to_string(i) + ".", true, false});
    h->layers.push_back({"decoders3.0.", false, false});
    int rc = 0;
    rc |= tt.add("embed.0.weight", (int64_t)V * D);
    for (const FdLayer& l : h->layers) {
        rc |= tt.add_linear(l.p + "norm1.", D, 1);
        rc |= tt.add_linear(l.p + "feed_forward.w_1.", FF, D);
        rc |= tt.add_linear(l.p + "feed_forward.norm.", FF, 1);
        rc |= tt.add_linear(l.p + "feed_forward.w_2.", D, FF, false);
        if (l.fsmn) {
            rc |= tt.add_linear(l.p + "norm2.", D, 1);
            rc |= tt.add(l.p + "self_attn.fsmn_block.weight", (int64_t)D * K);
        }
        if (l.cross) {
            rc |= tt.add_linear(l.p + "norm3.", D, 1);
            rc |= tt.add_linear(l.p + "src_attn.linear_q.", D, D);
            rc |= tt.add_linear(l.p + "src_attn.linear_k_v.", 2 * D, D);
            rc |= tt.add_linear(l.p + "src_attn.linear_out.", D, D);
        }
    }
    rc |= tt.add_linear("after_norm.", D, 1);
    rc |= tt.add_linear("output_layer.", V, D);
    if (rc) return nullptr;
    return reinterpret_cast<pf_fsmndecoder*>(h.release());
}
void pf_fsmndecoder_destroy(pf_fsmndecoder* h) { delete reinterpret_cast<Fd*>(h); }
int pf_fsmndecoder_set_tensor(pf_fsmndecoder* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Fd*>(h), "fsmndecoder_set_tensor: null", name, data, numel);
}
int pf_fsmndecoder_missing(const pf_fsmndecoder* h) { return table_missing(reinterpret_cast<const Fd*>(h)); }
int pf_fsmndecoder_begin(pf_fsmndecoder* hh, const float* memory, int32_t T, int32_t max_len, int32_t max_hyp, void* stream) {
    Fd* h = reinterpret_cast<Fd*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if ((rc = begin_common(h, "fsmndecoder",
                           "fsmndecoder_begin: 1 .. 12000 memory rows, 1 .. 5000 positions (max_len), 1 .. 256 hypotheses (max_hyp)", memory, T,
                           max_len, max_hyp, h ? h->cfg.att_layer_num : 0)))
        return rc;
    const int D = h->cfg.d_model, LA = h->cfg.att_layer_num;
    h->n_prev = 0; h->n_par = 0;
    const size_t n = (size_t)max_hyp, wbytes = sizeof(float) * 2 * h->n_fsmn() * h->layer();
    if (h->win.ensure(wbytes) || h->t.ensure(sizeof(float) * n * D) || h->hidn.ensure(sizeof(float) * n * h->cfg.ffn_dim)) return -2;
    PF_HIP_TRY(hipMemsetAsync(h->win.p, 0, wbytes, s));
    for (int l = 0; l < LA; ++l) {                   // K | V of the whole memory, once per utterance: one GEMM through linear_k_v
        const std::string p = h->layers[l].p + "src_attn.linear_k_v.";
        GemmArgs g{};
        g.A = memory; g.lda = D; g.ldw = D; g.ldc = 2 * D; g.M = T; g.N = 2 * D; g.K = D;
        g.W = h->tt.get(p + "weight"); g.bias = h->tt.get(p + "bias"); g.C = h->ckv.as<float>() + (size_t)l * T * 2 * D;
        if ((rc = launch_gemm_f32(g, s))) return rc;
    }
    return 0;
}
// The step of both SAN-M steppers. `win` == nullptr: pf_fsmndecoder_step, every cross-attention over the whole memory. Otherwise
// pf_scamadecoder_step: the cross-attention of every `decoders` layer restricted to the keys of the window that the mask row admits.
struct FdWindow { const float* mask; int lo, hi; };
static int fd_step(Fd* h, const int32_t* tokens_host, int32_t pos, int32_t n, float* logp, const FdWindow* win, hipStream_t s) {
    int rc;
    if ((rc = step_common_checks(h, "fsmndecoder", tokens_host, logp, n, [&] {
             PF_REQUIRE(n > 0 && n <= h->max_hyp && pos >= 0 && pos < h->max_len && pos == h->filled,
                        "fsmndecoder_step: n_hyp <= max_hyp, every position once and in order below max_len");
             // whose window a slot continues: the parents of the last reorder(), else its own (then it must have run at the last position)
             PF_REQUIRE(pos == 0 || (h->n_par ? n == h->n_par : n <= h->n_prev),
                        "fsmndecoder_step: n_hyp differs from the last reorder(), or a slot without a parent");
             return 0;
         }, s)))
        return rc;
    const pf_fsmndecoder_config& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim, H = c.n_heads, T = h->T, K = c.kernel_size;
    StreamModeScope small_m;                         // every GEMM of the step has M = n_hyp rows: the weight-streaming kernel
    float *x = h->x.as<float>(), *y = h->y.as<float>(), *xn = h->xn.as<float>(), *t = h->t.as<float>(), *q = h->q.as<float>(),
          *a = h->a.as<float>(), *hid = h->hid.as<float>(), *hidn = h->hidn.as<float>();
    if ((rc = launch_td_embed(h->tt.get("embed.0.weight"), h->ids.as<int>(), nullptr, 1.f, x, n, D, s))) return rc;      // bare: no positional row
    auto W = [&](const std::string& nme) { return h->tt.get(nme); };
    const int* parents = pos > 0 && h->n_par ? h->par.as<int>() : nullptr;
    int lf = 0, lc = 0;
    for (const FdLayer& l : h->layers) {
        const std::string& p = l.p;
        // t = w_2(LayerNorm_FF(relu(w_1(norm1(x)))))
        if ((rc = h->norm(p + "norm1.", x, xn, D))) return rc;
        if ((rc = h->lin(p + "feed_forward.w_1.", xn, D, hid, FF, FF, true))) return rc;
        if ((rc = h->norm(p + "feed_forward.norm.", hid, hidn, FF))) return rc;
        if ((rc = h->lin(p + "feed_forward.w_2.", hidn, FF, l.fsmn ? t : y, D, D, false, nullptr, false))) return rc;
        if (!l.fsmn) { std::swap(x, y); continue; }  // decoders3: no residual
        // y = x + fsmn(norm2(t)), xn = norm3(y)
        if ((rc = launch_fd_fsmn_step(t, x, W(p + "norm2.weight"), W(p + "norm2.bias"), W(p + "self_attn.fsmn_block.weight"),
                                      h->win_of(h->cur, lf), h->win_of(h->cur ^ 1, lf), parents, pos, n, D, K, h->left_pad(),
                                      l.cross ? W(p + "norm3.weight") : nullptr, l.cross ? W(p + "norm3.bias") : nullptr, c.ln_eps, y,
                                      l.cross ? xn : nullptr, s)))
            return rc;
        ++lf;
        std::swap(x, y);
        if (!l.cross) continue;
        const float* kv = h->ckv.as<float>() + (size_t)lc * T * 2 * D;
        ++lc;
        if ((rc = h->cross_attention(p, xn, x, y, [&] {
                 return win ? launch_scama_attention(q, kv, kv + D, 2 * D, T, win->mask, win->lo, win->hi, n, H, D / H, a, s)
                            : launch_fd_attention(q, kv, kv + D, 2 * D, T, n, H, D / H, a, s);
             })))
            return rc;
        std::swap(x, y);
    }
    if ((rc = h->output_tail(x, logp))) return rc;
    h->filled = pos + 1; h->cur ^= 1; h->n_prev = n; h->n_par = 0;
    return 0;
}
int pf_fsmndecoder_step(pf_fsmndecoder* hh, const int32_t* tokens_host, int32_t pos, int32_t n, float* logp, void* stream) {
    return fd_step(reinterpret_cast<Fd*>(hh), tokens_host, pos, n, logp, nullptr, reinterpret_cast<hipStream_t>(stream));
}
int pf_fsmndecoder_reorder(pf_fsmndecoder* hh, const int32_t* parents_host, int32_t n, void* stream) {
    Fd* h = reinterpret_cast<Fd*>(hh);
    // no launch: the FSMN kernel of the next step reads window parents[k] of the buffer the last step wrote and writes window k of
    // the other one, so a parent may repeat or be dropped and nothing is overwritten before it is read
    const int rc = reorder_common(h, "fsmndecoder", parents_host, n, [&] {
        for (int i = 0; i < n; ++i) PF_REQUIRE(parents_host[i] < h->n_prev, "fsmndecoder_reorder: parent slot did not run at the last position");
        return 0;
    }, reinterpret_cast<hipStream_t>(stream));
    if (rc) return rc < 0 ? rc : 0;
    h->n_par = n;
    return 0;
}

// ---- SCAMA decoder step (FsmnDecoderSCAMAOpt.forward_one_step, scama/decoder.py:455-524): the SAN-M stepper above behind entry points
// of its own; the step takes the memory mask of its position
pf_scamadecoder* pf_scamadecoder_create(const pf_fsmndecoder_config* cfg) { return reinterpret_cast<pf_scamadecoder*>(pf_fsmndecoder_create(cfg)); }
void pf_scamadecoder_destroy(pf_scamadecoder* h) { pf_fsmndecoder_destroy(reinterpret_cast<pf_fsmndecoder*>(h)); }
int pf_scamadecoder_set_tensor(pf_scamadecoder* h, const char* name, const float* data, int64_t numel) {
    return pf_fsmndecoder_set_tensor(reinterpret_cast<pf_fsmndecoder*>(h), name, data, numel);
}
int pf_scamadecoder_missing(const pf_scamadecoder* h) { return pf_fsmndecoder_missing(reinterpret_cast<const pf_fsmndecoder*>(h)); }
int pf_scamadecoder_begin(pf_scamadecoder* h, const float* memory, int32_t T, int32_t max_len, int32_t max_hyp, void* stream) {
    return pf_fsmndecoder_begin(reinterpret_cast<pf_fsmndecoder*>(h), memory, T, max_len, max_hyp, stream);
}
int pf_scamadecoder_step(pf_scamadecoder* hh, const int32_t* tokens_host, int32_t pos, int32_t n, const float* mask_row_dev, int32_t key_lo,
                         int32_t key_hi, float* logp, void* stream) {
    Fd* h = reinterpret_cast<Fd*>(hh);
    PF_REQUIRE(h && h->max_len > 0, "scamadecoder_step: null handle or no begin()");
    PF_REQUIRE(key_lo >= 0 && key_lo <= key_hi && key_hi <= h->T, "scamadecoder_step: key window outside 0 <= key_lo <= key_hi <= T");
    const FdWindow win{mask_row_dev, key_lo, key_hi};
    return fd_step(h, tokens_host, pos, n, logp, &win, reinterpret_cast<hipStream_t>(stream));
}
int pf_scamadecoder_reorder(pf_scamadecoder* h, const int32_t* parents_host, int32_t n, void* stream) {
    return pf_fsmndecoder_reorder(reinterpret_cast<pf_fsmndecoder*>(h), parents_host, n, stream);
}

// ---- LCB-Net (funasr/models/lcbnet): the text encoder over token ids and the audio-text fusion layer
pf_textencoder* pf_textencoder_create(const pf_textencoder_config* cfg) {
    if (!cfg) { set_error("textencoder: null config"); return nullptr; }
    if (!(cfg->vocab_size > 0 && cfg->n_blocks >= 0 && lcb_shape_ok(cfg->d_model, cfg->n_heads, cfg->ffn_dim, cfg->ln_eps))) {
        set_error("textencoder: unsupported config (vocab_size > 0, head dim 64, d_model <= 2048, ffn_dim % 32)");
        return nullptr;
    }
    if (check_device()) return nullptr;
    std::unique_ptr<Te> h(new Te());
    LcbCfg& c = h->cfg;
    c.vocab_size = cfg->vocab_size; c.d_model = cfg->d_model; c.n_heads = cfg->n_heads; c.ffn_dim = cfg->ffn_dim; c.n_blocks = cfg->n_blocks;
    c.ln_eps = cfg->ln_eps;
    h->bx.assign(c.n_blocks, TfBlockX());
    TensorTable& tt = h->tt;
    int rc = 0;
    rc |= tt.add("embed.0.weight", (int64_t)c.vocab_size * c.d_model);
    rc |= tt.add("pos_table", (int64_t)5000 * c.d_model);
    for (int i = 0; i < c.n_blocks; ++i) rc |= add_tf_block(tt, blk(i), {"self_attn."}, {"norm1.", "norm2."}, c.d_model, c.ffn_dim);
    rc |= tt.add_linear("after_norm.", c.d_model, 1);
    if (rc) return nullptr;
    return reinterpret_cast<pf_textencoder*>(h.release());
}
void pf_textencoder_destroy(pf_textencoder* h) { delete reinterpret_cast<Te*>(h); }
int pf_textencoder_set_tensor(pf_textencoder* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Te*>(h), "textencoder_set_tensor: null", name, data, numel);
}
int pf_textencoder_missing(const pf_textencoder* h) { return table_missing(reinterpret_cast<const Te*>(h)); }
int pf_textencoder_forward(pf_textencoder* hh, const int32_t* ids_host, const int32_t* lens_host, int32_t B, int32_t L, float* out,
                           void* stream) {
    Te* h = reinterpret_cast<Te*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && ids_host && lens_host && out && B > 0 && B <= 65535, "textencoder_forward: null/empty argument");
    if (L < 1 || L > 5000) { set_error("textencoder: " + std::to_string(L) + " tokens; 1 .. 5000 (the positional table holds 5000)"); return -1; }
    const LcbCfg& c = h->cfg;
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= L, "textencoder_forward: a length exceeds the padded length");
    for (size_t i = 0; i < (size_t)B * L; ++i)
        if (ids_host[i] < 0 || ids_host[i] >= c.vocab_size) {
            set_error("textencoder: token id " + std::to_string(ids_host[i]) + " outside the vocabulary of " + std::to_string(c.vocab_size));
            return -1;
        }
    int rc;
    if ((rc = h->tt.require_all("textencoder"))) return rc;
    if ((rc = h->rows(B, L, c.ffn_dim, lens_host, s))) return rc;
    if (h->ids.ensure(sizeof(int32_t) * (size_t)B * L) || upload_h2d(h->ids.p, ids_host, sizeof(int32_t) * (size_t)B * L, s)) return -2;
    if ((rc = launch_text_embed_rows(h->tt.get("embed.0.weight"), h->ids.as<int>(), h->tt.get("pos_table"), sqrtf((float)c.d_model),
                                     h->xa.as<float>(), B, L, c.d_model, s)))
        return rc;
    return h->tf_blocks(h->bx, B, out);
}

pf_fusion* pf_fusion_create(const pf_fusion_config* cfg) {
    if (!cfg) { set_error("fusion: null config"); return nullptr; }
    if (!lcb_shape_ok(cfg->d_model, cfg->n_heads, cfg->ffn_dim, cfg->ln_eps)) {
        set_error("fusion: unsupported config (head dim 64, d_model <= 2048, ffn_dim % 32)");
        return nullptr;
    }
    if (check_device()) return nullptr;
    std::unique_ptr<Fu> h(new Fu());
    LcbCfg& c = h->cfg;
    c.d_model = cfg->d_model; c.n_heads = cfg->n_heads; c.ffn_dim = cfg->ffn_dim; c.ln_eps = cfg->ln_eps;
    if (add_tf_block(h->tt, "", {"self_attn.", "src_attn."}, {"norm1.", "norm2.", "norm3."}, c.d_model, c.ffn_dim)) return nullptr;
    return reinterpret_cast<pf_fusion*>(h.release());
}
void pf_fusion_destroy(pf_fusion* h) { delete reinterpret_cast<Fu*>(h); }
int pf_fusion_set_tensor(pf_fusion* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Fu*>(h), "fusion_set_tensor: null", name, data, numel);
}
int pf_fusion_missing(const pf_fusion* h) { return table_missing(reinterpret_cast<const Fu*>(h)); }
int pf_fusion_forward(pf_fusion* hh, const float* x_in, const int32_t* x_lens_host, const float* mem, const int32_t* mem_lens_host, int32_t B,
                      int32_t T, int32_t L, int32_t add_input, float* out, void* stream) {
    Fu* h = reinterpret_cast<Fu*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && x_in && mem && out && x_in != out && B > 0 && B <= 65535, "fusion_forward: null/empty argument");
    PF_REQUIRE(T >= 1 && T <= 12000 && L >= 1 && L <= 5000, "fusion_forward: 1 .. 12000 rows, 1 .. 5000 memory rows");
    PF_REQUIRE(((uintptr_t)x_in & 15) == 0 && ((uintptr_t)mem & 15) == 0 && ((uintptr_t)out & 15) == 0, "fusion_forward: 16-B alignment");
    std::vector<int32_t> xl(B, T), ml(B, L);               // NULL lengths: every row and every key
    for (int b = 0; b < B; ++b) {
        if (x_lens_host) xl[b] = x_lens_host[b];
        if (mem_lens_host) ml[b] = mem_lens_host[b];
        PF_REQUIRE(xl[b] >= 0 && xl[b] <= T && ml[b] >= 0 && ml[b] <= L, "fusion_forward: a length exceeds the padded length");
    }
    const LcbCfg& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim;
    int rc;
    if ((rc = h->tt.require_all("fusion"))) return rc;
    if ((rc = h->rows(B, T, FF, xl.data(), s))) return rc;
    if (h->kv.ensure(sizeof(float) * (size_t)B * L * 2 * D) || h->mlens.ensure(sizeof(int32_t) * B) ||
        upload_h2d(h->mlens.p, ml.data(), sizeof(int32_t) * B, s))
        return -2;
    float *x = h->xa.as<float>(), *xn = h->xn.as<float>(), *q = h->qkv.as<float>(), *att = h->att.as<float>(), *hid = h->hid.as<float>(),
          *kv = h->kv.as<float>();
    // x1 = x + self_attn(norm1 x)
    if ((rc = h->ln("norm1.", x_in, xn))) return rc;
    const char* names[3] = {"self_attn.linear_q.", "self_attn.linear_k.", "self_attn.linear_v."};
    for (int j = 0; j < 3; ++j)
        if ((rc = h->lin(xn, D, names[j], D, nullptr, q + (size_t)j * D, 3 * D, 0))) return rc;
    if ((rc = launch_tf_attention(q, h->klens.as<int>(), B, T, c.n_heads, att, s))) return rc;
    if ((rc = h->lin(att, D, "self_attn.linear_out.", D, x_in, x, D, 0))) return rc;
    // x2 = x1 + src_attn(norm2 x1, mem, mem): q [B T, D] into the q | k | v buffer (row stride D), K | V of the memory rows by two
    // GEMMs with ldc = 2 D
    float* x2 = h->xb.as<float>();
    if ((rc = h->ln("norm2.", x, xn))) return rc;
    if ((rc = h->lin(xn, D, "src_attn.linear_q.", D, nullptr, q, D, 0))) return rc;
    if ((rc = h->gm(false, mem, B * L, D, "src_attn.linear_k.weight", h->tt.get("src_attn.linear_k.bias"), D, nullptr, kv, 2 * D, 0))) return rc;
    if ((rc = h->gm(false, mem, B * L, D, "src_attn.linear_v.weight", h->tt.get("src_attn.linear_v.bias"), D, nullptr, kv + D, 2 * D, 0))) return rc;
    if ((rc = launch_tf_cross_attention(q, D, kv, h->mlens.as<int>(), B, T, L, c.n_heads, att, s))) return rc;
    if ((rc = h->lin(att, D, "src_attn.linear_out.", D, x, x2, D, 0))) return rc;
    // out = (x +) x2 + ffn(norm3 x2): both addends ride in the last GEMM
    if ((rc = h->ln("norm3.", x2, xn))) return rc;
    if ((rc = h->lin(xn, D, "feed_forward.w_1.", FF, nullptr, hid, FF, 0))) return rc;
    if ((rc = launch_cf_act(hid, (size_t)h->Mi * FF, 0, s))) return rc;
    GemmArgs g{};
    g.A = hid; g.lda = FF; g.W = h->tt.get("feed_forward.w_2.weight"); g.ldw = FF; g.bias = h->tt.get("feed_forward.w_2.bias");
    g.R1 = x2; g.ldr1 = D; g.R2 = add_input ? x_in : nullptr; g.ldr2 = D; g.C = out; g.ldc = D; g.M = h->Mi; g.N = D; g.K = FF;
    return launch_gemm_f32(g, s);
}

// ---- E-Paraformer (funasr/models/e_paraformer): the PIF predictor's two calls and the one-pass SAN decoder
pf_pif* pf_pif_create(const pf_pif_config* cfg) {
    if (!cfg) { set_error("pif: null config"); return nullptr; }
    const pf_pif_config& c = *cfg;
    if (!(c.d_model > 0 && c.d_model <= PIF_MAX_D && c.sigma_heads >= 1 && c.sigma_heads <= PIF_MAX_HEADS && c.d_model % c.sigma_heads == 0 &&
          (c.d_model / c.sigma_heads) % 32 == 0 && c.l_order >= 0 && c.l_order <= PIF_MAX_ORDER && c.r_order >= 0 && c.r_order <= PIF_MAX_ORDER)) {
        set_error("pif: unsupported config (d_model <= 1024, 1 .. 8 sigma heads of a multiple of 32 channels, l_order / r_order 0 .. 15)");
        return nullptr;
    }
    if (check_device()) return nullptr;
    std::unique_ptr<Pif> h(new Pif());
    h->cfg = c;
    TensorTable& tt = h->tt;
    int rc = 0;
    rc |= tt.add_linear("cif_conv1d.", c.d_model, c.l_order + c.r_order + 1);
    rc |= tt.add_linear("cif_output.", 1, c.d_model);
    rc |= tt.add("sigma", c.sigma_heads);
    rc |= tt.add("bias", c.sigma_heads);                 // constant over the frames: it cancels in the softmax and is never read
    if (rc) return nullptr;
    return reinterpret_cast<pf_pif*>(h.release());
}
void pf_pif_destroy(pf_pif* h) { delete reinterpret_cast<Pif*>(h); }
int pf_pif_set_tensor(pf_pif* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Pif*>(h), "pif_set_tensor: null", name, data, numel);
}
int pf_pif_missing(const pf_pif* h) { return table_missing(reinterpret_cast<const Pif*>(h)); }
static int pif_lens(Pif* h, const char* who, const int32_t* lens_host, int B, int T, hipStream_t s) {
    PF_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= PIF_MAX_T, std::string(who) + ": 1 .. 65535 clips of 1 .. 5000 frames");
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= T, std::string(who) + ": a length exceeds the padded length");
    if (h->tt.require_all("pif")) return -3;
    return upload_lens(h->lens, lens_host, B, s) ? -2 : 0;
}
int pf_pif_alphas(pf_pif* hh, const float* x, const int32_t* lens_host, int32_t B, int32_t T, float* alphas, float* token_num, void* stream) {
    Pif* h = reinterpret_cast<Pif*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && x && lens_host && alphas && token_num, "pif_alphas: null argument");
    if (int rc = pif_lens(h, "pif_alphas", lens_host, B, T, s)) return rc;
    const pf_pif_config& c = h->cfg;
    return launch_pif_alphas(x, h->tt.get("cif_conv1d.weight"), h->tt.get("cif_conv1d.bias"), h->tt.get("cif_output.weight"),
                             h->tt.get("cif_output.bias"), h->lens.as<int>(), B, T, c.d_model, c.l_order, c.r_order, c.smooth_factor,
                             c.noise_threshold, alphas, token_num, s);
}
int pf_pif_embeds(pf_pif* hh, const float* x, float* alphas, const float* token_num, const int32_t* counts_host, const int32_t* lens_host,
                  int32_t B, int32_t T, int32_t Lmax, float* align, float* embeds, void* stream) {
    Pif* h = reinterpret_cast<Pif*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && x && alphas && token_num && counts_host && lens_host && align && embeds, "pif_embeds: null argument");
    PF_REQUIRE(Lmax >= 1 && Lmax <= PIF_MAX_L, "pif_embeds: 1 .. 2048 fire positions");
    if (int rc = pif_lens(h, "pif_embeds", lens_host, B, T, s)) return rc;
    for (int b = 0; b < B; ++b) PF_REQUIRE(counts_host[b] >= 0 && counts_host[b] <= Lmax, "pif_embeds: a token count outside 0 .. Lmax");
    if (upload_lens(h->counts, counts_host, B, s)) return -2;
    int rc;
    if ((rc = launch_pif_align(alphas, token_num, h->counts.as<int>(), B, T, alphas, align, s))) return rc;
    return launch_pif_embed(align, x, h->tt.get("sigma"), h->lens.as<int>(), B, T, Lmax, h->cfg.d_model, h->cfg.sigma_heads, embeds, s);
}

pf_sandecoder* pf_sandecoder_create(const pf_sandecoder_config* cfg) {
    if (!cfg) { set_error("sandecoder: null config"); return nullptr; }
    if (!(cfg->vocab_size > 0 && cfg->n_blocks >= 1 && (cfg->precision == 0 || cfg->precision == 3) &&
          lcb_shape_ok(cfg->d_model, cfg->n_heads, cfg->ffn_dim, cfg->ln_eps))) {
        set_error("sandecoder: unsupported config (vocab_size > 0, head dim 64, d_model <= 2048, ffn_dim % 32, precision 0 or 3)");
        return nullptr;
    }
    if (check_device()) return nullptr;
    std::unique_ptr<Sd> h(new Sd());
    LcbCfg& c = h->cfg;
    c.vocab_size = cfg->vocab_size; c.d_model = cfg->d_model; c.n_heads = cfg->n_heads; c.ffn_dim = cfg->ffn_dim; c.n_blocks = cfg->n_blocks;
    c.precision = cfg->precision; c.ln_eps = cfg->ln_eps;
    TensorTable& tt = h->tt;
    int rc = 0;
    for (int i = 0; i < c.n_blocks; ++i) rc |= add_tf_block(tt, dl(i), {"self_attn.", "src_attn."}, {"norm1.", "norm2.", "norm3."}, c.d_model, c.ffn_dim);
    rc |= tt.add_linear("after_norm.", c.d_model, 1);
    rc |= tt.add_linear("output_layer.", c.vocab_size, c.d_model);
    if (rc) return nullptr;
    return reinterpret_cast<pf_sandecoder*>(h.release());
}
void pf_sandecoder_destroy(pf_sandecoder* h) { delete reinterpret_cast<Sd*>(h); }
int pf_sandecoder_set_tensor(pf_sandecoder* h, const char* name, const float* data, int64_t numel) {
    return table_set(reinterpret_cast<Sd*>(h), "sandecoder_set_tensor: null", name, data, numel);
}
int pf_sandecoder_missing(const pf_sandecoder* h) { return table_missing(reinterpret_cast<const Sd*>(h)); }
int pf_sandecoder_set_precision(pf_sandecoder* h, int32_t precision) { return enc_set_precision(reinterpret_cast<Sd*>(h), "sandecoder", precision); }
int pf_sandecoder_forward(pf_sandecoder* hh, const float* memory, const int32_t* mem_lens_host, const float* embeds, const int32_t* tok_lens_host,
                          int32_t B, int32_t T, int32_t L, float* logp, int32_t* ids, float* best, void* stream) {
    Sd* h = reinterpret_cast<Sd*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && memory && mem_lens_host && embeds && tok_lens_host && ids && best && B > 0 && B <= 65535,
               "sandecoder_forward: null/empty argument");
    PF_REQUIRE(T >= 1 && T <= 12000 && L >= 1 && L <= PIF_MAX_L, "sandecoder_forward: 1 .. 12000 memory rows, 1 .. 2048 token rows");
    PF_REQUIRE(((uintptr_t)memory & 15) == 0 && ((uintptr_t)embeds & 15) == 0, "sandecoder_forward: 16-B alignment");
    for (int b = 0; b < B; ++b)
        PF_REQUIRE(mem_lens_host[b] >= 0 && mem_lens_host[b] <= T && tok_lens_host[b] >= 0 && tok_lens_host[b] <= L,
                   "sandecoder_forward: a length exceeds the padded length");
    const LcbCfg& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim, V = c.vocab_size;
    int rc;
    if ((rc = h->tt.require_all("sandecoder"))) return rc;
    if (h->prepared != h->tt.version && (rc = h->prepare(s))) return rc;
    if ((rc = h->rows(B, L, FF, tok_lens_host, s))) return rc;
    const size_t M = (size_t)h->Mi;
    if (h->kv.ensure(sizeof(float) * (size_t)B * T * 2 * D) || h->logits.ensure(sizeof(float) * M * V) || upload_lens(h->mlens, mem_lens_host, B, s))
        return -2;
    float *bufs[2] = {h->xa.as<float>(), h->xb.as<float>()}, *xn = h->xn.as<float>(), *q = h->qkv.as<float>(), *att = h->att.as<float>(),
          *hid = h->hid.as<float>(), *kv = h->kv.as<float>();
    const float* x = embeds;                       // the rows of the block in flight: the caller's, then the two buffers in turn
    int cur = 0;
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = dl(i);
        const SdBlockX& e = h->bx[i];
        if ((rc = h->ln(p + "norm1.", x, xn))) return rc;
        const char* names[3] = {"self_attn.linear_q.", "self_attn.linear_k.", "self_attn.linear_v."};
        for (int j = 0; j < 3; ++j)
            if ((rc = h->lin(xn, D, p + names[j], D, nullptr, q + (size_t)j * D, 3 * D, e.e_sa_in))) return rc;
        if ((rc = launch_tf_attention(q, h->klens.as<int>(), B, L, c.n_heads, att, s))) return rc;     // no key of a clip without tokens: zeros
        if ((rc = h->lin(att, D, p + "self_attn.linear_out.", D, x, bufs[cur], D, e.e_sa))) return rc;
        x = bufs[cur]; cur ^= 1;
        if ((rc = h->ln(p + "norm2.", x, xn))) return rc;
        if ((rc = h->lin(xn, D, p + "src_attn.linear_q.", D, nullptr, q, D, e.e_ca_in))) return rc;
        if ((rc = h->gm(false, memory, B * T, D, p + "src_attn.linear_k.weight", h->tt.get(p + "src_attn.linear_k.bias"), D, nullptr, kv, 2 * D, 0))) return rc;
        if ((rc = h->gm(false, memory, B * T, D, p + "src_attn.linear_v.weight", h->tt.get(p + "src_attn.linear_v.bias"), D, nullptr, kv + D, 2 * D, 0))) return rc;
        if ((rc = launch_tf_cross_attention(q, D, kv, h->mlens.as<int>(), B, L, T, c.n_heads, att, s))) return rc;
        if ((rc = h->gm(false, att, h->Mi, D, p + "src_attn.linear_out.weight", h->tt.get(p + "src_attn.linear_out.bias"), D, x, bufs[cur], D, 0))) return rc;
        x = bufs[cur]; cur ^= 1;
        if ((rc = h->ln(p + "norm3.", x, xn))) return rc;
        if ((rc = h->lin(xn, D, p + "feed_forward.w_1.", FF, nullptr, hid, FF, e.e_ff_in))) return rc;
        if ((rc = launch_cf_act(hid, M * FF, 0, s))) return rc;
        if ((rc = h->lin(hid, FF, p + "feed_forward.w_2.", D, x, bufs[cur], D, e.e_ff_h))) return rc;
        x = bufs[cur]; cur ^= 1;
    }
    if ((rc = h->ln("after_norm.", x, xn))) return rc;
    float* logits = h->logits.as<float>();
    if ((rc = h->gm(false, xn, h->Mi, D, "output_layer.weight", h->tt.get("output_layer.bias"), V, nullptr, logits, V, 0))) return rc;
    float* lp = logp ? logp : logits;
    if ((rc = launch_log_softmax(logits, V, lp, V, h->Mi, V, s))) return rc;
    if ((rc = launch_argmax_rows(lp, V, h->Mi, V, ids, s))) return rc;
    return launch_pif_gather_best(lp, V, ids, h->Mi, best, s);
}

// single-kernel hooks (tests)
int pf_k_pif_alphas(const float* h, const float* conv_w, const float* conv_b, const float* out_w, const float* out_b, const int32_t* lens_dev,
                    int32_t B, int32_t T, int32_t D, int32_t l_order, int32_t r_order, float smooth, float noise, float* a, float* token_num,
                    void* stream) {
    return launch_pif_alphas(h, conv_w, conv_b, out_w, out_b, lens_dev, B, T, D, l_order, r_order, smooth, noise, a, token_num,
                             reinterpret_cast<hipStream_t>(stream));
}
int pf_k_pif_align(const float* a, const float* token_num, const int32_t* n_dev, int32_t B, int32_t T, float* an, float* align, void* stream) {
    return launch_pif_align(a, token_num, n_dev, B, T, an, align, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_pif_embed(const float* align, const float* h, const float* sigma, const int32_t* lens_dev, int32_t B, int32_t T, int32_t L, int32_t D,
                   int32_t H, float* embeds, void* stream) {
    return launch_pif_embed(align, h, sigma, lens_dev, B, T, L, D, H, embeds, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_fsmn_step(const float* t, const float* x, const float* g2, const float* b2, const float* w, const float* win_in, float* win_out,
                   const int32_t* parents_dev, int32_t pos, int32_t n, int32_t D, int32_t K, int32_t left_pad, const float* g3, const float* b3,
                   float eps, float* x_out, float* xn_out, void* stream) {
    return launch_fd_fsmn_step(t, x, g2, b2, w, win_in, win_out, parents_dev, pos, n, D, K, left_pad, g3, b3, eps, x_out, xn_out,
                               reinterpret_cast<hipStream_t>(stream));
}
int pf_k_cross_attention_step(const float* q, const float* kv, int32_t T, int32_t n, int32_t H, int32_t dk, float* out, void* stream) {
    PF_REQUIRE(kv && H > 0 && (dk == 64 || dk == 128), "cross_attention_step: head dim 64 or 128");
    return launch_fd_attention(q, kv, kv + H * dk, 2 * H * dk, T, n, H, dk, out, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_relpos_attention(const float* qkv, const float* P, const float* u, const float* v, const int32_t* klens_dev, int32_t B, int32_t T,
                          int32_t H, int32_t legacy, float* out, void* stream) {
    return launch_cf_relpos_attention(qkv, P, u, v, klens_dev, B, T, H, legacy, out, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_tf_attention(const float* qkv, const int32_t* klens_dev, int32_t B, int32_t T, int32_t H, float* out, void* stream) {
    return launch_tf_attention(qkv, klens_dev, B, T, H, out, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_tf_embed_rows(const float* x, int32_t NE, const float* pe, int32_t B, int32_t T, int32_t D, float scale, float* y, void* stream) {
    return launch_cf_scale_rows(x, NE, y, B, T, D, scale, pe, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_tf_cross_attention(const float* q, int32_t ldq, const float* kv, const int32_t* klens_dev, int32_t B, int32_t Tq, int32_t L, int32_t H,
                            float* out, void* stream) {
    return launch_tf_cross_attention(q, ldq, kv, klens_dev, B, Tq, L, H, out, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_text_embed_rows(const float* table, const int32_t* ids_dev, const float* pe, int32_t B, int32_t L, int32_t D, float scale, float* y,
                         void* stream) {
    return launch_text_embed_rows(table, ids_dev, pe, scale, y, B, L, D, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_conformer_glu_dw(const float* g,const float* dw, const float* dw_bias, const float* bn_scale, const float* bn_shift, int32_t B,
                          int32_t T, int32_t D, int32_t taps, float* y, void* stream) {
    return launch_cf_glu_dw(g, dw, dw_bias, bn_scale, bn_shift, B, T, D, taps, y, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_eb_gelu(float* x, int64_t n, void* stream) {
    PF_REQUIRE(n > 0, "eb_gelu: n > 0");
    return launch_eb_gelu(x, (size_t)n, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_eb_csgu(const float* h, const float* gamma, const float* beta, float eps, const float* dw, const float* dw_bias, int32_t B, int32_t T,
                 int32_t C, int32_t taps, float* stats, float* y, void* stream) {
    return launch_eb_csgu(h, gamma, beta, eps, dw, dw_bias, B, T, C, taps, stats, y, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_eb_merge(const float* x1, const float* x2, const float* dw, const float* dw_bias, int32_t B, int32_t T, int32_t D, int32_t taps,
                  float* y, void* stream) {
    return launch_eb_merge(x1, x2, dw, dw_bias, B, T, D, taps, y, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
