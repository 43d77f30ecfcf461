// C-ABI layer, Conformer / Transformer / SANM ASR: pf_conformer_* and pf_tfencoder_* (the two encoders over one Conv2dSubsampling front),
// pf_tdecoder_* (the autoregressive Transformer decoder step) and pf_fsmndecoder_* (the SAN-M decoder step); kernels in conformer.hip, attention_relpos.hip and
// attention_abs.hip, GEMMs through the shared launchers.
//
// Encoder forward over the zero-padded batch [B, Tin, F] (the reference runs Conv2dSubsampling and the convolution module over
// the padded tensor without masking, so every row of the batch is computed and a clip's frames depend on the batch's length):
//   conv0 + ReLU into the even / odd time-row buffers -> conv1 as THREE accumulating GEMMs over overlapping strided views
//   (element r = t (F2 + 1) + f of the output reads the contiguous 3 C floats at 2 C r of even[t], odd[t], even[t + 1]: lda = 2 C,
//   K = 3 C, no im2col; one output column in F2 + 1 is waste) + ReLU -> the output linear over rows of (F2 + 1) C floats (weight
//   permuted, zero for the waste column; K in slices of 1024, see cf_forward) -> x sqrt(D) into [B T, D] rows -> blocks: [macaron FFN] -> LayerNorm, q / k / v and
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

using namespace pf;

namespace {

constexpr int LIN_K_SLICE = 1024;      // K extent of one launch of the subsampling's output linear (a multiple of the GEMM's 32)

// Conv2dSubsampling up to its output linear, shared by the Conformer and the Transformer encoder handles: the buffers, what is
// derived from the weights at prepare(), and the launches.
struct CfSub {
    DevBuf even, odd, ya, yb, lin, lin2;
    static int F1(int F) { return (F - 3) / 2 + 1; }
    static int F2(int F) { return (F1(F) - 3) / 2 + 1; }
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
    // The output linear sums (F2 + 1) C terms per element (2560 at 80 features and C = 128, 8192 at 256 features). One fp32 fma chain of
    // that length drifts several times further from the exact sum than a blocked CPU GEMM does, so K goes in slices of 1024: a
    // slice's chain starts at zero and the running sum rides in as the addend of the next launch (ping-pong, no in-place addend).
    float *l = lin.as<float>(), *l_prev = lin2.as<float>();
    const int Kl = (f2 + 1) * C;
    for (int k0 = 0; k0 < Kl; k0 += LIN_K_SLICE) {
        GemmArgs g{};
        g.A = a + k0; g.lda = Kl; g.W = tt.get("#embed.out") + k0; g.ldw = Kl;
        g.bias = k0 == 0 ? tt.get("embed.out.0.bias") : nullptr;
        g.R1 = k0 == 0 ? nullptr : l_prev; g.ldr1 = D;
        g.C = l; g.ldc = D; g.M = B * NE; g.N = D; g.K = std::min(LIN_K_SLICE, Kl - k0);
        if ((rc = launch_gemm_f32(g, s))) return rc;
        std::swap(l, l_prev);
    }
    *rows = l_prev;
    return 0;
}

struct CfBlockX { int e_ffm_in = 0, e_ffm_h = 0, e_mha_in = 0, e_att = 0, e_conv_in = 0, e_cm = 0, e_ff_in = 0, e_ff_h = 0; };

struct Cf {
    pf_conformer_config cfg;
    TensorTable tt;
    unsigned long long prepared = ~0ull;
    std::vector<CfBlockX> bx;
    CfSub sub_;
    DevBuf xa, xb, xn, qkv, P, att, hid, planes, klens;

    int F2() const { return CfSub::F2(cfg.input_dim); }
    int pos_rows() const { return cfg.legacy ? 5000 : 9999; }
    static int sub(int L, int n) { const int m = std::min(L, n - 2); return m <= 0 ? 0 : (m + 1) / 2; }
    // encoder frames of a length-L clip inside a batch padded to n frames (the mask rule x_mask[:, :, :-2:2][:, :, :-2:2])
    static int out_len(int L, int n) { const int n1 = sub(n, n); return sub(sub(L, n), n1); }
    int ln_bound(const std::string& p, float* out, hipStream_t s) {
        return TensorTable::dev_ln_bound(tt.get(p + "weight"), tt.get(p + "bias"), cfg.d_model, out, s);
    }
    int prepare(hipStream_t s);
};

std::string blk(int i) { return "encoders." + std::to_string(i) + "."; }

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
        float hb = 0.f, mb, cb;
        auto ffn = [&](const std::string& f, const std::string& norm, int* e_in, int* e_h) {
            float nb;
            if (ln_bound(p + norm, &nb, s)) return -2;
            *e_in = exp_for_bound(nb);
            if (TensorTable::dev_linear_bound(tt.get(p + f + "w_1.weight"), FF, D, D, tt.get(p + f + "w_1.bias"), nb, &hb, s)) return -2;
            *e_h = exp_for_bound(hb);
            return 0;
        };
        if (cfg.macaron && ffn("feed_forward_macaron.", "norm_ff_macaron.", &x.e_ffm_in, &x.e_ffm_h)) return -2;
        if (ffn("feed_forward.", "norm_ff.", &x.e_ff_in, &x.e_ff_h)) return -2;
        if (ln_bound(p + "norm_mha.", &mb, s)) return -2;
        x.e_mha_in = exp_for_bound(mb);
        if (TensorTable::dev_linear_bound(tt.get(p + "self_attn.linear_v.weight"), D, D, D, tt.get(p + "self_attn.linear_v.bias"), mb, &hb, s))
            return -2;
        x.e_att = exp_for_bound(hb);
        if (ln_bound(p + "norm_conv.", &cb, s)) return -2;
        x.e_conv_in = exp_for_bound(cb);
        if (TensorTable::dev_linear_bound(tt.get(p + "conv_module.pointwise_conv1.weight"), D, D, D,
                                          tt.get(p + "conv_module.pointwise_conv1.bias"), cb, &hb, s))
            return -2;
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

int cf_forward(Cf* h, const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s) {
    const pf_conformer_config& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim;
    const int T1 = (Tin - 3) / 2 + 1, T = (T1 - 3) / 2 + 1, NE = T + 1;
    const bool x2 = c.precision == 3;
    const float eps = c.ln_eps;
    std::vector<int32_t> kl(B);
    for (int b = 0; b < B; ++b) {
        kl[b] = Cf::out_len(lens[b], Tin);
        if (olens) olens[b] = kl[b];
    }
    const size_t M = (size_t)B * T;
    const int nP = c.legacy ? T : 2 * T - 1;
    if (h->xa.ensure(sizeof(float) * M * D) || h->xb.ensure(sizeof(float) * M * D) || h->xn.ensure(sizeof(float) * M * D) ||
        h->qkv.ensure(sizeof(float) * M * 3 * D) || h->P.ensure(sizeof(float) * (size_t)nP * D) || h->att.ensure(sizeof(float) * M * D) ||
        h->hid.ensure(sizeof(float) * M * std::max(FF, 2 * D)) || h->klens.ensure(sizeof(int32_t) * B))
        return -2;
    if (upload_h2d(h->klens.p, kl.data(), sizeof(int32_t) * B, s)) return -2;
    int rc;
    // C[M, N] = A[M, K] (row stride lda) W^T + bias (+ R1)
    auto gm = [&](bool x2_, const float* A, int lda, int M_, int K, const std::string& w, int N, const float* bias, const float* R1, float* Cc,
                  int ldc, int e_a) {
        return gemm_two_mode(h->tt, h->planes, x2_, A, K, (size_t)M_, lda, M_, K, w, N, bias, R1, Cc, ldc, e_a, 0, s);
    };
    const float* lin_prev;
    if ((rc = h->sub_.forward(h->tt, h->planes, feats, B, Tin, c.input_dim, D, D, &lin_prev, s))) return rc;
    float* x = h->xa.as<float>();
    float* y = h->xb.as<float>();
    if ((rc = launch_cf_scale_rows(lin_prev, NE, x, B, T, D, sqrtf((float)D), nullptr, s))) return rc;
    const float* pos = h->tt.get("pos_table") + (c.legacy ? (size_t)0 : (size_t)(5000 - T) * D);
    float *xn = h->xn.as<float>(), *qkv = h->qkv.as<float>(), *Pm = h->P.as<float>(), *att = h->att.as<float>(), *hid = h->hid.as<float>();
    const int Mi = (int)M;
    auto ln = [&](const std::string& p, const float* in, float* o) {
        return layernorm(in, D, h->tt.get(p + "weight"), h->tt.get(p + "bias"), o, D, Mi, D, D, eps, s);
    };
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        const CfBlockX& e = h->bx[i];
        const std::string half = c.macaron ? "#half" : "";
        auto ffn = [&](const std::string& f, const std::string& norm, int e_in, int e_h) {
            int r;
            if ((r = ln(p + norm, x, xn))) return r;
            if ((r = gm(x2, xn, D, Mi, D, p + f + "w_1.weight", FF, h->tt.get(p + f + "w_1.bias"), nullptr, hid, FF, e_in))) return r;
            if ((r = launch_cf_act(hid, M * FF, 1, s))) return r;
            if ((r = gm(x2, hid, FF, Mi, FF, p + f + "w_2.weight" + half, D, h->tt.get(p + f + "w_2.bias" + half), x, y, D, e_h)))
                return r;
            std::swap(x, y);
            return 0;
        };
        if (c.macaron && (rc = ffn("feed_forward_macaron.", "norm_ff_macaron.", e.e_ffm_in, e.e_ffm_h))) return rc;
        // relative-position self-attention
        if ((rc = ln(p + "norm_mha.", x, xn))) return rc;
        const char* names[3] = {"self_attn.linear_q.", "self_attn.linear_k.", "self_attn.linear_v."};
        for (int j = 0; j < 3; ++j)
            if ((rc = gm(x2, xn, D, Mi, D, p + names[j] + "weight", D, h->tt.get(p + names[j] + "bias"), nullptr, qkv + (size_t)j * D,
                              3 * D, e.e_mha_in)))
                return rc;
        if ((rc = gm(false, pos, D, nP, D, p + "self_attn.linear_pos.weight", D, nullptr, nullptr, Pm, D, 0))) return rc;
        if ((rc = launch_cf_relpos_attention(qkv, Pm, h->tt.get(p + "self_attn.pos_bias_u"), h->tt.get(p + "self_attn.pos_bias_v"),
                                             h->klens.as<int>(), B, T, c.n_heads, c.legacy, att, s)))
            return rc;
        if ((rc = gm(x2, att, D, Mi, D, p + "self_attn.linear_out.weight", D, h->tt.get(p + "self_attn.linear_out.bias"), x, y, D,
                          e.e_att)))
            return rc;
        std::swap(x, y);
        // convolution module
        if ((rc = ln(p + "norm_conv.", x, xn))) return rc;
        if ((rc = gm(x2, xn, D, Mi, D, p + "conv_module.pointwise_conv1.weight", 2 * D, h->tt.get(p + "conv_module.pointwise_conv1.bias"),
                          nullptr, hid, 2 * D, e.e_conv_in)))
            return rc;
        const float* bnp = h->tt.get("#bn") + (size_t)i * 2 * D;
        if ((rc = launch_cf_glu_dw(hid, h->tt.get(p + "conv_module.depthwise_conv.weight"), h->tt.get(p + "conv_module.depthwise_conv.bias"),
                                   bnp, bnp + D, B, T, D, c.kernel_size, att, s)))
            return rc;
        if ((rc = gm(x2, att, D, Mi, D, p + "conv_module.pointwise_conv2.weight", D, h->tt.get(p + "conv_module.pointwise_conv2.bias"),
                          x, y, D, e.e_cm)))
            return rc;
        std::swap(x, y);
        if ((rc = ffn("feed_forward.", "norm_ff.", e.e_ff_in, e.e_ff_h))) return rc;
        if ((rc = ln(p + "norm_final.", x, y))) return rc;
        std::swap(x, y);
    }
    return layernorm(x, D, h->tt.get("after_norm.weight"), h->tt.get("after_norm.bias"), out, D, Mi, D, D, eps, s);
}

// ================================================================================================ Transformer encoder
// funasr/models/transformer/encoder.py TransformerEncoder (input_layer conv2d, normalize_before): the shared subsampling ->
// x sqrt(D) + pe -> blocks: LayerNorm(norm1), q / k / v GEMMs, plain masked attention, linear_out (+ residual) -> LayerNorm(norm2),
// w_1, ReLU, w_2 (+ residual); after_norm. precision 3: the block GEMMs from two-plane fp16 operands, exponents from a-priori
// bounds: the LayerNorm bounds for the q / k / v and w_1 operands, the row-L1 bound of linear_v for the attention output (a convex
// combination of value rows) and the row-L1 bound of w_1 for the hidden rows (ReLU does not enlarge it).
struct TfBlockX { int e_mha_in = 0, e_att = 0, e_ff_in = 0, e_ff_h = 0; };

struct Tf {
    pf_tfencoder_config cfg;
    TensorTable tt;
    unsigned long long prepared = ~0ull;
    std::vector<TfBlockX> bx;
    CfSub sub_;
    DevBuf xa, xb, xn, qkv, att, hid, planes, klens;
    int prepare(hipStream_t s);
};

int Tf::prepare(hipStream_t s) {
    const int D = cfg.d_model, NB = cfg.n_blocks, FF = cfg.ffn_dim;
    if (CfSub::prepare(tt, D, D, CfSub::F2(cfg.input_dim), "tfencoder")) return -2;
    bx.assign(NB, TfBlockX());
    if (cfg.precision == 3) tt.drop_bf16();
    for (int i = 0; i < NB && cfg.precision == 3; ++i) {
        const std::string p = blk(i);
        TfBlockX& x = bx[i];
        float nb, hb;
        if (TensorTable::dev_ln_bound(tt.get(p + "norm1.weight"), tt.get(p + "norm1.bias"), D, &nb, s)) return -2;
        x.e_mha_in = exp_for_bound(nb);
        if (TensorTable::dev_linear_bound(tt.get(p + "self_attn.linear_v.weight"), D, D, D, tt.get(p + "self_attn.linear_v.bias"), nb, &hb, s))
            return -2;
        x.e_att = exp_for_bound(hb);
        if (TensorTable::dev_ln_bound(tt.get(p + "norm2.weight"), tt.get(p + "norm2.bias"), D, &nb, s)) return -2;
        x.e_ff_in = exp_for_bound(nb);
        if (TensorTable::dev_linear_bound(tt.get(p + "feed_forward.w_1.weight"), FF, D, D, tt.get(p + "feed_forward.w_1.bias"), nb, &hb, s))
            return -2;
        x.e_ff_h = exp_for_bound(hb);
    }
    prepared = tt.version;
    return 0;
}

int tf_forward(Tf* h, const float* feats, const int32_t* lens, int B, int Tin, float* out, int32_t* olens, hipStream_t s) {
    const pf_tfencoder_config& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim;
    const int T1 = (Tin - 3) / 2 + 1, T = (T1 - 3) / 2 + 1, NE = T + 1;
    const bool x2 = c.precision == 3;
    std::vector<int32_t> kl(B);
    for (int b = 0; b < B; ++b) {
        kl[b] = Cf::out_len(lens[b], Tin);
        if (olens) olens[b] = kl[b];
    }
    const size_t M = (size_t)B * T;
    if (h->xa.ensure(sizeof(float) * M * D) || h->xb.ensure(sizeof(float) * M * D) || h->xn.ensure(sizeof(float) * M * D) ||
        h->qkv.ensure(sizeof(float) * M * 3 * D) || h->att.ensure(sizeof(float) * M * D) || h->hid.ensure(sizeof(float) * M * FF) ||
        h->klens.ensure(sizeof(int32_t) * B))
        return -2;
    if (upload_h2d(h->klens.p, kl.data(), sizeof(int32_t) * B, s)) return -2;
    int rc;
    const float* rows;
    if ((rc = h->sub_.forward(h->tt, h->planes, feats, B, Tin, c.input_dim, D, D, &rows, s))) return rc;
    float *x = h->xa.as<float>(), *y = h->xb.as<float>(), *xn = h->xn.as<float>(), *qkv = h->qkv.as<float>(), *att = h->att.as<float>(),
          *hid = h->hid.as<float>();
    if ((rc = launch_cf_scale_rows(rows, NE, x, B, T, D, sqrtf((float)D), h->tt.get("pos_table"), s))) return rc;
    const int Mi = (int)M;
    // C[M, N] = A[M, K] W^T + bias (+ R1)
    auto gm = [&](const float* A, int K, const std::string& w, int N, const float* R1, float* Cc, int ldc, int e_a) {
        return gemm_two_mode(h->tt, h->planes, x2, A, K, M, K, Mi, K, w + "weight", N, h->tt.get(w + "bias"), R1, Cc, ldc, e_a, 0, s);
    };
    auto ln = [&](const std::string& p, const float* in, float* o) {
        return layernorm(in, D, h->tt.get(p + "weight"), h->tt.get(p + "bias"), o, D, Mi, D, D, c.ln_eps, s);
    };
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        const TfBlockX& e = h->bx[i];
        if ((rc = ln(p + "norm1.", x, xn))) return rc;
        const char* names[3] = {"self_attn.linear_q.", "self_attn.linear_k.", "self_attn.linear_v."};
        for (int j = 0; j < 3; ++j)
            if ((rc = gm(xn, D, p + names[j], D, nullptr, qkv + (size_t)j * D, 3 * D, e.e_mha_in))) return rc;
        if ((rc = launch_tf_attention(qkv, h->klens.as<int>(), B, T, c.n_heads, att, s))) return rc;
        if ((rc = gm(att, D, p + "self_attn.linear_out.", D, x, y, D, e.e_att))) return rc;
        std::swap(x, y);
        if ((rc = ln(p + "norm2.", x, xn))) return rc;
        if ((rc = gm(xn, D, p + "feed_forward.w_1.", FF, nullptr, hid, FF, e.e_ff_in))) return rc;
        if ((rc = launch_cf_act(hid, M * FF, 0, s))) return rc;
        if ((rc = gm(hid, FF, p + "feed_forward.w_2.", D, x, y, D, e.e_ff_h))) return rc;
        std::swap(x, y);
    }
    return ln("after_norm.", x, out);
}

// ================================================================================================ decoder
struct Td {
    pf_tdecoder_config cfg;
    TensorTable tt;
    DevBuf ckv, cache, x, y, xn, q, a, hid, logits, ids, par;
    int T = 0, max_len = 0, max_hyp = 0, filled = 0, cur = 0;
    size_t slot() const { return (size_t)max_len * 2 * cfg.d_model; }
    size_t layer() const { return slot() * max_hyp; }
    float* cache_of(int which, int l) { return cache.as<float>() + ((size_t)which * cfg.n_blocks + l) * layer(); }
};

std::string dl(int i) { return "decoders." + std::to_string(i) + "."; }

// ================================================================================================ SAN-M (FsmnDecoder) step
// One layer table for the three groups of the reference's module: `decoders` (FFN, FSMN memory, cross-attention), `decoders2` (FFN,
// FSMN memory) and the one FFN-only layer of `decoders3`.
struct FdLayer { std::string p; bool fsmn, cross; };

struct Fd {
    pf_fsmndecoder_config cfg;
    TensorTable tt;
    std::vector<FdLayer> layers;
    DevBuf ckv, win, x, y, xn, t, q, a, hid, hidn, logits, ids, par;
    int T = 0, max_len = 0, max_hyp = 0, filled = 0, cur = 0, n_prev = 0, n_par = 0;
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
    const int D = c.d_model, C = c.d_model, FF = c.ffn_dim, K = c.kernel_size;
    int rc = 0;
    rc |= h->tt.add("embed.conv.0.weight", (int64_t)C * 9);
    rc |= h->tt.add("embed.conv.0.bias", C);
    rc |= h->tt.add("embed.conv.2.weight", (int64_t)C * C * 9);
    rc |= h->tt.add("embed.conv.2.bias", C);
    rc |= h->tt.add("embed.out.0.weight", (int64_t)D * C * h->F2());
    rc |= h->tt.add("embed.out.0.bias", D);
    rc |= h->tt.add("pos_table", (int64_t)h->pos_rows() * D);
    auto lin = [&](const std::string& n, int o, int i, bool bias = true) {
        rc |= h->tt.add(n + "weight", (int64_t)o * i);
        if (bias) rc |= h->tt.add(n + "bias", o);
    };
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        for (const char* n : {"linear_q.", "linear_k.", "linear_v.", "linear_out."}) lin(p + "self_attn." + n, D, D);
        lin(p + "self_attn.linear_pos.", D, D, false);
        rc |= h->tt.add(p + "self_attn.pos_bias_u", D);
        rc |= h->tt.add(p + "self_attn.pos_bias_v", D);
        lin(p + "feed_forward.w_1.", FF, D);
        lin(p + "feed_forward.w_2.", D, FF);
        if (c.macaron) {
            lin(p + "feed_forward_macaron.w_1.", FF, D);
            lin(p + "feed_forward_macaron.w_2.", D, FF);
            lin(p + "norm_ff_macaron.", D, 1);
        }
        lin(p + "conv_module.pointwise_conv1.", 2 * D, D);
        lin(p + "conv_module.depthwise_conv.", D, K);
        lin(p + "conv_module.norm.", D, 1);
        rc |= h->tt.add(p + "conv_module.norm.running_mean", D);
        rc |= h->tt.add(p + "conv_module.norm.running_var", D);
        lin(p + "conv_module.pointwise_conv2.", D, D);
        for (const char* n : {"norm_ff.", "norm_mha.", "norm_conv.", "norm_final."}) lin(p + n, D, 1);
    }
    lin("after_norm.", D, 1);
    if (rc) return nullptr;
    return reinterpret_cast<pf_conformer*>(h.release());
}
void pf_conformer_destroy(pf_conformer* h) { delete reinterpret_cast<Cf*>(h); }
int pf_conformer_set_tensor(pf_conformer* hh, const char* name, const float* data, int64_t numel) {
    Cf* h = reinterpret_cast<Cf*>(hh);
    PF_REQUIRE(h && name && data, "conformer_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_conformer_missing(const pf_conformer* hh) {
    const Cf* h = reinterpret_cast<const Cf*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_conformer_set_precision(pf_conformer* hh, int32_t precision) {
    Cf* h = reinterpret_cast<Cf*>(hh);
    PF_REQUIRE(h && (precision == 0 || precision == 3), "conformer_set_precision: 0 (fp32) or 3 (f16x2)");
    if (h->cfg.precision != precision) { h->cfg.precision = precision; h->prepared = ~0ull; }
    return 0;
}
int32_t pf_conformer_num_frames(const pf_conformer* hh, int32_t n_frames, int32_t padded_frames) {
    if (!hh || padded_frames < 7 || n_frames > padded_frames) return -1;
    return Cf::out_len(n_frames, padded_frames);
}
int pf_conformer_forward(pf_conformer* hh, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, float* out,
                         int32_t* out_lens_host, void* stream) {
    Cf* h = reinterpret_cast<Cf*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && feats && lens_host && out && B > 0, "conformer_forward: null/empty argument");
    if (Tin < 7) { set_error("conformer: has " + std::to_string(Tin) + " frames and is too short for subsampling (it needs more than 7 frames)"); return -1; }
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= Tin, "conformer_forward: a length exceeds the padded length");
    const int T = Cf::out_len(Tin, Tin);
    if (T > 5000) { set_error("conformer: " + std::to_string(T) + " encoder frames; the positional tables hold 5000 (200 s)"); return -1; }
    int rc;
    if ((rc = h->tt.require_all("conformer"))) return rc;
    if (h->prepared != h->tt.version && (rc = h->prepare(s))) return rc;
    return cf_forward(h, feats, lens_host, B, Tin, out, out_lens_host, s);
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
    const int D = c.d_model, FF = c.ffn_dim;
    int rc = 0;
    auto lin = [&](const std::string& n, int o, int i) {
        rc |= h->tt.add(n + "weight", (int64_t)o * i);
        rc |= h->tt.add(n + "bias", o);
    };
    lin("embed.conv.0.", D, 9);
    lin("embed.conv.2.", D, D * 9);
    lin("embed.out.0.", D, D * CfSub::F2(c.input_dim));
    rc |= h->tt.add("pos_table", (int64_t)5000 * D);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        for (const char* n : {"linear_q.", "linear_k.", "linear_v.", "linear_out."}) lin(p + "self_attn." + n, D, D);
        lin(p + "feed_forward.w_1.", FF, D);
        lin(p + "feed_forward.w_2.", D, FF);
        for (const char* n : {"norm1.", "norm2."}) lin(p + n, D, 1);
    }
    lin("after_norm.", D, 1);
    if (rc) return nullptr;
    return reinterpret_cast<pf_tfencoder*>(h.release());
}
void pf_tfencoder_destroy(pf_tfencoder* h) { delete reinterpret_cast<Tf*>(h); }
int pf_tfencoder_set_tensor(pf_tfencoder* hh, const char* name, const float* data, int64_t numel) {
    Tf* h = reinterpret_cast<Tf*>(hh);
    PF_REQUIRE(h && name && data, "tfencoder_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_tfencoder_missing(const pf_tfencoder* hh) {
    const Tf* h = reinterpret_cast<const Tf*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_tfencoder_set_precision(pf_tfencoder* hh, int32_t precision) {
    Tf* h = reinterpret_cast<Tf*>(hh);
    PF_REQUIRE(h && (precision == 0 || precision == 3), "tfencoder_set_precision: 0 (fp32) or 3 (f16x2)");
    if (h->cfg.precision != precision) { h->cfg.precision = precision; h->prepared = ~0ull; }
    return 0;
}
int32_t pf_tfencoder_num_frames(const pf_tfencoder* hh, int32_t n_frames, int32_t padded_frames) {
    if (!hh || padded_frames < 7 || n_frames > padded_frames) return -1;
    return Cf::out_len(n_frames, padded_frames);
}
int pf_tfencoder_forward(pf_tfencoder* hh, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, float* out,
                         int32_t* out_lens_host, void* stream) {
    Tf* h = reinterpret_cast<Tf*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && feats && lens_host && out && B > 0, "tfencoder_forward: null/empty argument");
    if (Tin < 7) { set_error("tfencoder: has " + std::to_string(Tin) + " frames and is too short for subsampling (it needs more than 7 frames)"); return -1; }
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= Tin, "tfencoder_forward: a length exceeds the padded length");
    const int T = Cf::out_len(Tin, Tin);
    if (T > 5000) { set_error("tfencoder: " + std::to_string(T) + " encoder frames; the positional table holds 5000 (200 s)"); return -1; }
    int rc;
    if ((rc = h->tt.require_all("tfencoder"))) return rc;
    if (h->prepared != h->tt.version && (rc = h->prepare(s))) return rc;
    return tf_forward(h, feats, lens_host, B, Tin, out, out_lens_host, s);
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
    const int D = c.d_model, FF = c.ffn_dim, V = c.vocab_size;
    int rc = 0;
    auto lin = [&](const std::string& n, int o, int i) {
        rc |= h->tt.add(n + "weight", (int64_t)o * i);
        rc |= h->tt.add(n + "bias", o);
    };
    rc |= h->tt.add("embed.0.weight", (int64_t)V * D);
    rc |= h->tt.add("pos_table", (int64_t)5000 * D);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = dl(i);
        for (const char* a : {"self_attn.", "src_attn."})
            for (const char* n : {"linear_q.", "linear_k.", "linear_v.", "linear_out."}) lin(p + a + n, D, D);
        lin(p + "feed_forward.w_1.", FF, D);
        lin(p + "feed_forward.w_2.", D, FF);
        for (const char* n : {"norm1.", "norm2.", "norm3."}) lin(p + n, D, 1);
    }
    lin("after_norm.", D, 1);
    lin("output_layer.", V, D);
    if (rc) return nullptr;
    return reinterpret_cast<pf_tdecoder*>(h.release());
}
void pf_tdecoder_destroy(pf_tdecoder* h) { delete reinterpret_cast<Td*>(h); }
int pf_tdecoder_set_tensor(pf_tdecoder* hh, const char* name, const float* data, int64_t numel) {
    Td* h = reinterpret_cast<Td*>(hh);
    PF_REQUIRE(h && name && data, "tdecoder_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_tdecoder_missing(const pf_tdecoder* hh) {
    const Td* h = reinterpret_cast<const Td*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_tdecoder_begin(pf_tdecoder* hh, const float* memory, int32_t T, int32_t max_len, int32_t max_hyp, void* stream) {
    Td* h = reinterpret_cast<Td*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && memory && T > 0 && T <= 12000 && max_len > 0 && max_len <= 5000 && max_hyp > 0 && max_hyp <= 256,
               "tdecoder_begin: 1 .. 12000 memory rows, 1 .. 5000 positions, 1 .. 256 hypotheses");
    if (h->tt.require_all("tdecoder")) return -3;
    const int D = h->cfg.d_model, L = h->cfg.n_blocks;
    h->T = T; h->max_len = max_len; h->max_hyp = max_hyp; h->filled = 0; h->cur = 0;
    const size_t n = (size_t)max_hyp;
    if (h->ckv.ensure(sizeof(float) * (size_t)L * T * 2 * D) || h->cache.ensure(sizeof(float) * 2 * L * h->layer()) ||
        h->x.ensure(sizeof(float) * n * D) || h->y.ensure(sizeof(float) * n * D) || h->xn.ensure(sizeof(float) * n * D) ||
        h->q.ensure(sizeof(float) * n * D) || h->a.ensure(sizeof(float) * n * D) || h->hid.ensure(sizeof(float) * n * h->cfg.ffn_dim) ||
        h->logits.ensure(sizeof(float) * n * h->cfg.vocab_size) || h->ids.ensure(sizeof(int32_t) * n) || h->par.ensure(sizeof(int32_t) * n))
        return -2;
    int rc;
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
    PF_REQUIRE(h && tokens_host && logp && h->max_len > 0, "tdecoder_step: null argument or no begin()");
    PF_REQUIRE(n > 0 && n <= h->max_hyp && pos >= 0 && pos < h->max_len && pos <= h->filled,
               "tdecoder_step: n_hyp <= max_hyp, positions appended in order below max_len");
    const pf_tdecoder_config& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim, V = c.vocab_size, H = c.n_heads, T = h->T;
    for (int i = 0; i < n; ++i) PF_REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < V, "tdecoder_step: token id outside the vocabulary");
    if (upload_h2d(h->ids.p, tokens_host, sizeof(int32_t) * n, s)) return -2;
    int rc;
    StreamModeScope small_m;                         // every GEMM of the step has M = n_hyp rows: the weight-streaming kernel
    float *x = h->x.as<float>(), *y = h->y.as<float>(), *xn = h->xn.as<float>(), *q = h->q.as<float>(), *a = h->a.as<float>(),
          *hid = h->hid.as<float>();
    if ((rc = launch_td_embed(h->tt.get("embed.0.weight"), h->ids.as<int>(), h->tt.get("pos_table") + (size_t)pos * D, sqrtf((float)D), x, n,
                              D, s)))
        return rc;
    auto W = [&](const std::string& nme) { return h->tt.get(nme); };
    const int ldslot = (int)h->slot();
    for (int l = 0; l < c.n_blocks; ++l) {
        const std::string p = dl(l);
        float* cache = h->cache_of(h->cur, l);
        if ((rc = layernorm(x, D, W(p + "norm1.weight"), W(p + "norm1.bias"), xn, D, n, D, D, c.ln_eps, s))) return rc;
        if ((rc = gemm_simple(xn, D, W(p + "self_attn.linear_q.weight"), D, W(p + "self_attn.linear_q.bias"), q, D, n, D, D, 0, nullptr, 0,
                              nullptr, 0, s)))
            return rc;
        if ((rc = gemm_simple(xn, D, W(p + "self_attn.linear_k.weight"), D, W(p + "self_attn.linear_k.bias"), cache + (size_t)pos * 2 * D, ldslot,
                              n, D, D, 0, nullptr, 0, nullptr, 0, s)))
            return rc;
        if ((rc = gemm_simple(xn, D, W(p + "self_attn.linear_v.weight"), D, W(p + "self_attn.linear_v.bias"), cache + (size_t)pos * 2 * D + D,
                              ldslot, n, D, D, 0, nullptr, 0, nullptr, 0, s)))
            return rc;
        if ((rc = launch_td_attention(q, cache, cache + D, 2 * D, h->slot(), pos + 1, n, H, a, s))) return rc;
        if ((rc = gemm_simple(a, D, W(p + "self_attn.linear_out.weight"), D, W(p + "self_attn.linear_out.bias"), y, D, n, D, D, 0, x, D,
                              nullptr, 0, s)))
            return rc;
        std::swap(x, y);
        if ((rc = layernorm(x, D, W(p + "norm2.weight"), W(p + "norm2.bias"), xn, D, n, D, D, c.ln_eps, s))) return rc;
        if ((rc = gemm_simple(xn, D, W(p + "src_attn.linear_q.weight"), D, W(p + "src_attn.linear_q.bias"), q, D, n, D, D, 0, nullptr, 0,
                              nullptr, 0, s)))
            return rc;
        const float* kv = h->ckv.as<float>() + (size_t)l * T * 2 * D;
        if ((rc = launch_td_attention(q, kv, kv + D, 2 * D, 0, T, n, H, a, s))) return rc;
        if ((rc = gemm_simple(a, D, W(p + "src_attn.linear_out.weight"), D, W(p + "src_attn.linear_out.bias"), y, D, n, D, D, 0, x, D,
                              nullptr, 0, s)))
            return rc;
        std::swap(x, y);
        if ((rc = layernorm(x, D, W(p + "norm3.weight"), W(p + "norm3.bias"), xn, D, n, D, D, c.ln_eps, s))) return rc;
        if ((rc = gemm_simple(xn, D, W(p + "feed_forward.w_1.weight"), D, W(p + "feed_forward.w_1.bias"), hid, FF, n, FF, D, 1, nullptr, 0,
                              nullptr, 0, s)))
            return rc;
        if ((rc = gemm_simple(hid, FF, W(p + "feed_forward.w_2.weight"), FF, W(p + "feed_forward.w_2.bias"), y, D, n, D, FF, 0, x, D, nullptr,
                              0, s)))
            return rc;
        std::swap(x, y);
    }
    if ((rc = layernorm(x, D, W("after_norm.weight"), W("after_norm.bias"), xn, D, n, D, D, c.ln_eps, s))) return rc;
    if ((rc = gemm_simple(xn, D, W("output_layer.weight"), D, W("output_layer.bias"), h->logits.as<float>(), V, n, V, D, 0, nullptr, 0, nullptr,
                          0, s)))
        return rc;
    if ((rc = launch_log_softmax(h->logits.as<float>(), V, logp, V, n, V, s))) return rc;
    h->filled = std::max(h->filled, pos + 1);
    return 0;
}
int pf_tdecoder_reorder(pf_tdecoder* hh, const int32_t* parents_host, int32_t n, void* stream) {
    Td* h = reinterpret_cast<Td*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && parents_host && h->max_len > 0 && n > 0 && n <= h->max_hyp, "tdecoder_reorder: null argument, no begin() or n_hyp > max_hyp");
    for (int i = 0; i < n; ++i) PF_REQUIRE(parents_host[i] >= 0 && parents_host[i] < h->max_hyp, "tdecoder_reorder: parent slot out of range");
    if (h->filled == 0) return 0;
    if (upload_h2d(h->par.p, parents_host, sizeof(int32_t) * n, s)) return -2;
    int rc;
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
    const int D = c.d_model, FF = c.ffn_dim, V = c.vocab_size, K = c.kernel_size;
    for (int i = 0; i < c.att_layer_num; ++i) h->layers.push_back({dl(i), true, true});
    for (int i = 0; i < c.n_blocks - c.att_layer_num; ++i) h->layers.push_back({"decoders2." + std::to_string(i) + ".", true, false});
    h->layers.push_back({"decoders3.0.", false, false});
    int rc = 0;
    auto lin = [&](const std::string& n, int o, int i, bool bias = true) {
        rc |= h->tt.add(n + "weight", (int64_t)o * i);
        if (bias) rc |= h->tt.add(n + "bias", o);
    };
    rc |= h->tt.add("embed.0.weight", (int64_t)V * D);
    for (const FdLayer& l : h->layers) {
        lin(l.p + "norm1.", D, 1);
        lin(l.p + "feed_forward.w_1.", FF, D);
        lin(l.p + "feed_forward.norm.", FF, 1);
        lin(l.p + "feed_forward.w_2.", D, FF, false);
        if (l.fsmn) {
            lin(l.p + "norm2.", D, 1);
            rc |= h->tt.add(l.p + "self_attn.fsmn_block.weight", (int64_t)D * K);
        }
        if (l.cross) {
            lin(l.p + "norm3.", D, 1);
            lin(l.p + "src_attn.linear_q.", D, D);
            lin(l.p + "src_attn.linear_k_v.", 2 * D, D);
            lin(l.p + "src_attn.linear_out.", D, D);
        }
    }
    lin("after_norm.", D, 1);
    lin("output_layer.", V, D);
    if (rc) return nullptr;
    return reinterpret_cast<pf_fsmndecoder*>(h.release());
}
void pf_fsmndecoder_destroy(pf_fsmndecoder* h) { delete reinterpret_cast<Fd*>(h); }
int pf_fsmndecoder_set_tensor(pf_fsmndecoder* hh, const char* name, const float* data, int64_t numel) {
    Fd* h = reinterpret_cast<Fd*>(hh);
    PF_REQUIRE(h && name && data, "fsmndecoder_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_fsmndecoder_missing(const pf_fsmndecoder* hh) {
    const Fd* h = reinterpret_cast<const Fd*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_fsmndecoder_begin(pf_fsmndecoder* hh, const float* memory, int32_t T, int32_t max_len, int32_t max_hyp, void* stream) {
    Fd* h = reinterpret_cast<Fd*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && memory && T > 0 && T <= 12000 && max_len > 0 && max_len <= 5000 && max_hyp > 0 && max_hyp <= 256,
               "fsmndecoder_begin: 1 .. 12000 memory rows, 1 .. 5000 positions (max_len), 1 .. 256 hypotheses (max_hyp)");
    if (h->tt.require_all("fsmndecoder")) return -3;
    const int D = h->cfg.d_model, LA = h->cfg.att_layer_num;
    h->T = T; h->max_len = max_len; h->max_hyp = max_hyp; h->filled = 0; h->cur = 0; h->n_prev = 0; h->n_par = 0;
    const size_t n = (size_t)max_hyp, wbytes = sizeof(float) * 2 * h->n_fsmn() * h->layer();
    if (h->ckv.ensure(sizeof(float) * (size_t)LA * T * 2 * D) || h->win.ensure(wbytes) || h->x.ensure(sizeof(float) * n * D) ||
        h->y.ensure(sizeof(float) * n * D) || h->xn.ensure(sizeof(float) * n * D) || h->t.ensure(sizeof(float) * n * D) ||
        h->q.ensure(sizeof(float) * n * D) || h->a.ensure(sizeof(float) * n * D) || h->hid.ensure(sizeof(float) * n * h->cfg.ffn_dim) ||
        h->hidn.ensure(sizeof(float) * n * h->cfg.ffn_dim) || h->logits.ensure(sizeof(float) * n * h->cfg.vocab_size) ||
        h->ids.ensure(sizeof(int32_t) * n) || h->par.ensure(sizeof(int32_t) * n))
        return -2;
    PF_HIP_TRY(hipMemsetAsync(h->win.p, 0, wbytes, s));
    int rc;
    for (int l = 0; l < LA; ++l) {                   // K | V of the whole memory, once per utterance: one GEMM through linear_k_v
        const std::string p = h->layers[l].p + "src_attn.linear_k_v.";
        GemmArgs g{};
        g.A = memory; g.lda = D; g.ldw = D; g.ldc = 2 * D; g.M = T; g.N = 2 * D; g.K = D;
        g.W = h->tt.get(p + "weight"); g.bias = h->tt.get(p + "bias"); g.C = h->ckv.as<float>() + (size_t)l * T * 2 * D;
        if ((rc = launch_gemm_f32(g, s))) return rc;
    }
    return 0;
}
int pf_fsmndecoder_step(pf_fsmndecoder* hh, const int32_t* tokens_host, int32_t pos, int32_t n, float* logp, void* stream) {
    Fd* h = reinterpret_cast<Fd*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && tokens_host && logp && h->max_len > 0, "fsmndecoder_step: null argument or no begin()");
    PF_REQUIRE(n > 0 && n <= h->max_hyp && pos >= 0 && pos < h->max_len && pos == h->filled,
               "fsmndecoder_step: n_hyp <= max_hyp, every position once and in order below max_len");
    // whose window a slot continues: the parents of the last reorder(), else its own (then it must have run at the last position)
    PF_REQUIRE(pos == 0 || (h->n_par ? n == h->n_par : n <= h->n_prev),
               "fsmndecoder_step: n_hyp differs from the last reorder(), or a slot without a parent");
    const pf_fsmndecoder_config& c = h->cfg;
    const int D = c.d_model, FF = c.ffn_dim, V = c.vocab_size, H = c.n_heads, T = h->T, K = c.kernel_size;
    for (int i = 0; i < n; ++i) PF_REQUIRE(tokens_host[i] >= 0 && tokens_host[i] < V, "fsmndecoder_step: token id outside the vocabulary");
    if (upload_h2d(h->ids.p, tokens_host, sizeof(int32_t) * n, s)) return -2;
    int rc;
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
        if ((rc = layernorm(x, D, W(p + "norm1.weight"), W(p + "norm1.bias"), xn, D, n, D, D, c.ln_eps, s))) return rc;
        if ((rc = gemm_simple(xn, D, W(p + "feed_forward.w_1.weight"), D, W(p + "feed_forward.w_1.bias"), hid, FF, n, FF, D, 1, nullptr, 0,
                              nullptr, 0, s)))
            return rc;
        if ((rc = layernorm(hid, FF, W(p + "feed_forward.norm.weight"), W(p + "feed_forward.norm.bias"), hidn, FF, n, FF, FF, c.ln_eps, s)))
            return rc;
        if ((rc = gemm_simple(hidn, FF, W(p + "feed_forward.w_2.weight"), FF, nullptr, l.fsmn ? t : y, D, n, D, FF, 0, nullptr, 0, nullptr, 0, s)))
            return rc;
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
        if ((rc = gemm_simple(xn, D, W(p + "src_attn.linear_q.weight"), D, W(p + "src_attn.linear_q.bias"), q, D, n, D, D, 0, nullptr, 0,
                              nullptr, 0, s)))
            return rc;
        const float* kv = h->ckv.as<float>() + (size_t)lc * T * 2 * D;
        ++lc;
        if ((rc = launch_fd_attention(q, kv, kv + D, 2 * D, T, n, H, D / H, a, s))) return rc;
        if ((rc = gemm_simple(a, D, W(p + "src_attn.linear_out.weight"), D, W(p + "src_attn.linear_out.bias"), y, D, n, D, D, 0, x, D,
                              nullptr, 0, s)))
            return rc;
        std::swap(x, y);
    }
    if ((rc = layernorm(x, D, W("after_norm.weight"), W("after_norm.bias"), xn, D, n, D, D, c.ln_eps, s))) return rc;
    if ((rc = gemm_simple(xn, D, W("output_layer.weight"), D, W("output_layer.bias"), h->logits.as<float>(), V, n, V, D, 0, nullptr, 0, nullptr,
                          0, s)))
        return rc;
    if ((rc = launch_log_softmax(h->logits.as<float>(), V, logp, V, n, V, s))) return rc;
    h->filled = pos + 1; h->cur ^= 1; h->n_prev = n; h->n_par = 0;
    return 0;
}
int pf_fsmndecoder_reorder(pf_fsmndecoder* hh, const int32_t* parents_host, int32_t n, void* stream) {
    Fd* h = reinterpret_cast<Fd*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && parents_host && h->max_len > 0 && n > 0 && n <= h->max_hyp, "fsmndecoder_reorder: null argument, no begin() or n_hyp > max_hyp");
    for (int i = 0; i < n; ++i) PF_REQUIRE(parents_host[i] >= 0 && parents_host[i] < h->max_hyp, "fsmndecoder_reorder: parent slot out of range");
    if (h->filled == 0) return 0;
    for (int i = 0; i < n; ++i) PF_REQUIRE(parents_host[i] < h->n_prev, "fsmndecoder_reorder: parent slot did not run at the last position");
    // no launch: the FSMN kernel of the next step reads window parents[k] of the buffer the last step wrote and writes window k of
    // the other one, so a parent may repeat or be dropped and nothing is overwritten before it is read
    if (upload_h2d(h->par.p, parents_host, sizeof(int32_t) * n, s)) return -2;
    h->n_par = n;
    return 0;
}

// single-kernel hooks (tests)
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
int pf_k_conformer_glu_dw(const float* g,const float* dw, const float* dw_bias, const float* bn_scale, const float* bn_shift, int32_t B,
                          int32_t T, int32_t D, int32_t taps, float* y, void* stream) {
    return launch_cf_glu_dw(g, dw, dw_bias, bn_scale, bn_shift, B, T, D, taps, y, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
