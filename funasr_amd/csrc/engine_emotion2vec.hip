// C-ABI layer, emotion2vec: pf_emotion2vec_* (kernels in emotion2vec.hip and attention_alibi.hip).
//
// One forward, per sub-batch of whole utterances (workspace bounded by max_samples):
//   waveform statistics -> conv0 + LN + GELU into per-utterance row slots -> conv1.. as plain GEMMs over an OVERLAPPING strided view
//   of the previous layer (output row t of a (k, s) conv reads the contiguous K = k * 512 run at row s * t: lda = s * 512; the weight
//   is permuted to [512, k * 512] at load) + LN + GELU rows. Slots are multiples of the product of the later strides, so every layer
//   halves (divides) them exactly and one launch covers the ragged batch; rows past an utterance's frames are computed and never
//   read by a valid row.
//   -> project_features (LN rows gathered into packed feature rows, GEMM) -> positional conv x depth (grouped conv, LN without
//   affine, GELU) -> tokens (extra tokens + features + positions, context LN) -> blocks: QKV GEMM, ALiBi attention, proj GEMM
//   (+ residual), LN1, fc1 GEMM, GELU, fc2 GEMM (+ LN1 output), LN2 -> frames / pooled head.
// precision 3 (f16x2): each GEMM's A operand is split into two fp16 planes (launch_split2) with an exponent from an a-priori bound
// that depends on the weights only (LayerNorm outputs: sqrt(D) max|gamma| + max|beta|; attention outputs: the row-L1 bound of the
// value projection; GELU(fc1): that of fc1), never on the batch.
#include <algorithm>
#include <cmath>
#include <functional>

#include "engine_internal.h"
#include "emotion2vec.h"

using namespace pf;

namespace {

const char* kA = "modality_encoders.AUDIO.";

struct E2v {
    pf_emotion2vec_config cfg;
    TensorTable tt;
    int64_t max_samples = (int64_t)8 << 20;
    unsigned long long prepared = ~0ull;
    std::vector<std::string> blocks;                  // prefixes of the prenet and main blocks, in order
    DevBuf mask;
    bool mask_set = false;
    // f16x2: exponents of the GEMM A operands
    std::vector<int> e_conv;                          // input of conv layer l (l >= 1)
    int e_pf = 0;
    std::vector<int> e_x, e_attn, e_x1, e_hid;        // per block
    DevBuf stats, woff, so, nfr, inmap, foff, toff, convA, convB, feat, xf, posA, posB, x, qkv, attn, y1, x1, hid, planes, zero;

    int D() const { return cfg.embed_dim; }
    int C() const { return cfg.vocab_size; }
    int ln_bound(const std::string& p, int D, float* out, hipStream_t s) {
        return TensorTable::dev_ln_bound(tt.get(p + "weight"), tt.get(p + "bias"), D, out, s);
    }
    int prepare(hipStream_t s);
    // frames after conv layer l of an utterance of n samples (0: too short)
    int64_t frames(int64_t n, int upto) const {
        int64_t L = n;
        for (int l = 0; l <= upto; ++l) {
            if (L < cfg.conv_kernel[l]) return 0;
            L = (L - cfg.conv_kernel[l]) / cfg.conv_stride[l] + 1;
        }
        return L;
    }
};

const std::string conv_name(int l, const char* what) {
    return std::string(kA) + "local_encoder.conv_layers." + std::to_string(l) + what;
}

int E2v::prepare(hipStream_t s) {
    const int D = cfg.embed_dim, H = cfg.num_heads, G = cfg.conv_pos_groups, Cg = D / G, K = cfg.conv_pos_kernel;
    // positional conv weights [D, Cg, K] -> [G][K][Cg (in)][Cg (out)]
    std::vector<float> wp((size_t)cfg.conv_pos_depth * D * Cg * K);
    for (int l = 0; l < cfg.conv_pos_depth; ++l) {
        std::vector<float> w = tt.host(std::string(kA) + "relative_positional_encoder." + std::to_string(l + 1) + ".0.weight");
        if (w.empty()) { set_error("emotion2vec: weight copy failed"); return -2; }
        float* dst = wp.data() + (size_t)l * D * Cg * K;
        for (int g = 0; g < G; ++g)
            for (int o = 0; o < Cg; ++o)
                for (int ci = 0; ci < Cg; ++ci)
                    for (int k = 0; k < K; ++k)
                        dst[(((size_t)g * K + k) * Cg + ci) * Cg + o] = w[(((size_t)(g * Cg + o)) * Cg + ci) * K + k];
    }
    if (!wp.empty() && tt.put_derived("#posw", wp)) return -2;
    // ALiBi slopes (get_slopes of the reference) and per-block scales clamp_min(alibi_scale, 0)
    const int NA = cfg.num_alibi_heads, NB = (int)blocks.size();
    std::vector<double> sl;
    std::function<void(int)> slopes = [&](int n) {
        auto pow2 = [](int n) {
            std::vector<double> v;
            const double start = std::pow(2.0, -std::pow(2.0, -(std::log2((double)n) - 3)));
            for (int i = 0; i < n; ++i) v.push_back(start * std::pow(start, i));
            return v;
        };
        const double lg = std::log2((double)n);
        if (lg == std::floor(lg)) { sl = pow2(n); return; }
        const int cp = 1 << (int)std::floor(lg);
        std::vector<double> a = pow2(cp);
        slopes(2 * cp);
        std::vector<double> b = sl;
        for (int i = 0; i < n - cp; ++i) a.push_back(b[2 * i]);
        sl = a;
    };
    slopes(NA);
    std::vector<float> sc = tt.host(std::string(kA) + "alibi_scale");
    if (sc.empty()) { set_error("emotion2vec: weight copy failed"); return -2; }
    std::vector<float> h_slope((size_t)NB * H, 0.f), h_scale((size_t)NB * H, 0.f);     // per block: [H] slopes and clamped scales
    for (int i = 0; i < NB; ++i)
        for (int h = 0; h < NA; ++h) {
            const int row = cfg.alibi_scale_layers > 1 ? i : 0, col = cfg.alibi_scale_heads > 1 ? h : 0;
            h_slope[(size_t)i * H + h] = (float)sl[h];
            h_scale[(size_t)i * H + h] = fmaxf(sc[(size_t)row * cfg.alibi_scale_heads + col], 0.f);
        }
    if (NB > 0 && (tt.put_derived("#slope", h_slope) || tt.put_derived("#scale", h_scale))) return -2;
    if (!mask_set && C() > 0) {
        std::vector<int32_t> z((size_t)C(), 0);
        if (mask.ensure(sizeof(int32_t) * z.size())) return -2;
        PF_HIP_TRY(hipMemcpy(mask.p, z.data(), sizeof(int32_t) * z.size(), hipMemcpyHostToDevice));
    }
    if (zero.ensure(256)) return -2;
    PF_HIP_TRY(hipMemset(zero.p, 0, 256));
    if (cfg.precision == 3) {
        tt.drop_bf16();
        e_conv.assign(cfg.n_conv, 0);
        float xb;
        for (int l = 1; l < cfg.n_conv; ++l) {
            if (ln_bound(conv_name(l - 1, ".2.1."), 512, &xb, s)) return -2;
            e_conv[l] = exp_for_bound(xb);
        }
        if (ln_bound(std::string(kA) + "project_features.1.", 512, &xb, s)) return -2;
        e_pf = exp_for_bound(xb);
        e_x.assign(NB, 0); e_attn.assign(NB, 0); e_x1.assign(NB, 0); e_hid.assign(NB, 0);
        if (ln_bound(std::string(kA) + "context_encoder.norm.", D, &xb, s)) return -2;
        for (int i = 0; i < NB; ++i) {
            const std::string& p = blocks[i];
            e_x[i] = exp_for_bound(xb);
            float vb = 0.f, hb = 0.f, b1;
            if (TensorTable::dev_linear_bound(tt.get(p + "attn.qkv.weight") + (size_t)2 * D * D, D, D, D, tt.get(p + "attn.qkv.bias") + 2 * D,
                                              xb, &vb, s))
                return -2;
            e_attn[i] = exp_for_bound(vb);
            if (ln_bound(p + "norm1.", D, &b1, s)) return -2;
            e_x1[i] = exp_for_bound(b1);
            if (TensorTable::dev_linear_bound(tt.get(p + "mlp.fc1.weight"), cfg.ffn_dim, D, D, tt.get(p + "mlp.fc1.bias"), b1, &hb, s))
                return -2;
            e_hid[i] = exp_for_bound(hb);
            if (ln_bound(p + "norm2.", D, &xb, s)) return -2;
        }
    }
    prepared = tt.version;
    return 0;
}

int e2v_rows(const float* x, int ldx, const int* in_map, const float* g, const float* b, int ln, int gelu, float eps, float* y, int M,
             int D, hipStream_t s) {
    E2vRowArgs a{};
    a.x = x; a.ldx = ldx; a.in_map = in_map; a.ln = ln; a.gamma = g; a.beta = b; a.eps = eps; a.gelu = gelu;
    a.y = y; a.ldy = D; a.M = M; a.D = D;
    return launch_e2v_rows(a, s);
}

// one sub-batch: utterances with sample counts n[0..B) at wav (back to back)
int run(E2v* h, const float* wav, const int64_t* n, int B, float* feats, float* pooled, float* probs, hipStream_t s) {
    const pf_emotion2vec_config& c = h->cfg;
    const int D = c.embed_dim, E = c.num_extra_tokens, FF = c.ffn_dim, NL = c.n_conv;
    const float eps = c.norm_eps;
    int P = 1;
    for (int l = 1; l < NL; ++l) P *= c.conv_stride[l];
    std::vector<int64_t> woff(B + 1, 0);
    std::vector<int32_t> so(B + 1, 0), nfr(B), foff(B + 1, 0), toff(B + 1, 0), Tl(B);
    for (int b = 0; b < B; ++b) {
        woff[b + 1] = woff[b] + n[b];
        const int64_t L0 = h->frames(n[b], 0);
        nfr[b] = (int32_t)L0;
        so[b + 1] = so[b] + (int32_t)((L0 + P - 1) / P * P);
        Tl[b] = (int32_t)h->frames(n[b], NL - 1);
        foff[b + 1] = foff[b] + Tl[b];
        toff[b + 1] = toff[b] + E + Tl[b];
    }
    const int M0 = so[B], F = foff[B], Ntok = toff[B];
    int maxlen = 0;
    for (int b = 0; b < B; ++b) maxlen = std::max(maxlen, E + Tl[b]);
    std::vector<int32_t> inmap(F);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < Tl[b]; ++t) inmap[foff[b] + t] = so[b] / P + t;
    const size_t SL = 8;           // slack rows behind every conv activation: the last row's overlapping K-run
    if (h->stats.ensure(sizeof(float) * 2 * B) || h->woff.ensure(sizeof(int64_t) * (B + 1)) || h->so.ensure(sizeof(int32_t) * (B + 1)) ||
        h->nfr.ensure(sizeof(int32_t) * B) || h->inmap.ensure(sizeof(int32_t) * F) || h->foff.ensure(sizeof(int32_t) * (B + 1)) ||
        h->toff.ensure(sizeof(int32_t) * (B + 1)) || h->convA.ensure(sizeof(float) * ((size_t)M0 + SL) * 512) ||
        h->convB.ensure(sizeof(float) * ((size_t)M0 / 2 + SL) * 512) || h->feat.ensure(sizeof(float) * (size_t)F * 512) ||
        h->xf.ensure(sizeof(float) * (size_t)F * D) || h->posA.ensure(sizeof(float) * (size_t)F * D) ||
        h->posB.ensure(sizeof(float) * (size_t)F * D) || h->x.ensure(sizeof(float) * (size_t)Ntok * D) ||
        h->qkv.ensure(sizeof(float) * (size_t)Ntok * 3 * D) || h->attn.ensure(sizeof(float) * (size_t)Ntok * D) ||
        h->y1.ensure(sizeof(float) * (size_t)Ntok * D) || h->x1.ensure(sizeof(float) * (size_t)Ntok * D) ||
        h->hid.ensure(sizeof(float) * (size_t)Ntok * FF))
        return -2;
    if (upload_h2d(h->woff.p, woff.data(), sizeof(int64_t) * (B + 1), s) || upload_h2d(h->so.p, so.data(), sizeof(int32_t) * (B + 1), s) ||
        upload_h2d(h->nfr.p, nfr.data(), sizeof(int32_t) * B, s) || upload_h2d(h->inmap.p, inmap.data(), sizeof(int32_t) * F, s) ||
        upload_h2d(h->foff.p, foff.data(), sizeof(int32_t) * (B + 1), s) || upload_h2d(h->toff.p, toff.data(), sizeof(int32_t) * (B + 1), s))
        return -2;
    int rc;
    const bool x2 = c.precision == 3;
    // C[M, N] = A (a_rows physical rows of `width` floats, viewed at row stride lda with K columns) W^T + bias (+ R1)
    auto gm = [&](const float* A, int width, size_t a_rows, int lda, int M_, int K, const std::string& w, int N, const float* bias,
                  const float* R1, float* C, int e_a) {
        return gemm_two_mode(h->tt, h->planes, x2, A, width, a_rows, lda, M_, K, w, N, bias, R1, C, N, e_a, 0, s);
    };
    const int *d_so = h->so.as<int>(), *d_foff = h->foff.as<int>(), *d_toff = h->toff.as<int>();
    if ((rc = launch_e2v_wav_stats(wav, h->woff.as<int64_t>(), B, c.normalize, h->stats.as<float>(), s))) return rc;
    float* cur = h->convA.as<float>();
    float* nxt = h->convB.as<float>();
    if ((rc = launch_e2v_conv0(wav, h->woff.as<int64_t>(), h->stats.as<float>(), d_so, h->nfr.as<int>(), B, M0,
                               h->tt.get(conv_name(0, ".0.weight")), c.conv_kernel[0], c.conv_stride[0], h->tt.get(conv_name(0, ".2.1.weight")),
                               h->tt.get(conv_name(0, ".2.1.bias")), eps, cur, s)))
        return rc;
    int M = M0;
    for (int l = 1; l < NL; ++l) {
        const int k = c.conv_kernel[l], st = c.conv_stride[l], Mo = M / st;
        PF_HIP_TRY(hipMemsetAsync(cur + (size_t)M * 512, 0, sizeof(float) * SL * 512, s));
        if ((rc = gm(cur, 512, (size_t)M + SL, st * 512, Mo, k * 512, conv_name(l, ".0.weight"), 512, nullptr, nullptr, nxt,
                           x2 ? h->e_conv[l] : 0)))
            return rc;
        if ((rc = e2v_rows(nxt, 512, nullptr, h->tt.get(conv_name(l, ".2.1.weight")), h->tt.get(conv_name(l, ".2.1.bias")), 1, 1, eps, nxt,
                           Mo, 512, s)))
            return rc;
        std::swap(cur, nxt);
        M = Mo;
    }
    // project_features: LayerNorm(512) of the valid frames, gathered into packed rows, then Linear(512 -> D)
    const std::string pf = std::string(kA) + "project_features.";
    if ((rc = e2v_rows(cur, 512, h->inmap.as<int>(), h->tt.get(pf + "1.weight"), h->tt.get(pf + "1.bias"), 1, 0, eps, h->feat.as<float>(), F,
                       512, s)))
        return rc;
    if ((rc = gm(h->feat.as<float>(), 512, F, 512, F, 512, pf + "2.weight", D, h->tt.get(pf + "2.bias"), nullptr, h->xf.as<float>(),
                       h->e_pf)))
        return rc;
    // relative positional encoder
    const float* pin = h->xf.as<float>();
    float* pa = h->posA.as<float>();
    float* pb = h->posB.as<float>();
    const int Cg = D / c.conv_pos_groups;
    for (int l = 0; l < c.conv_pos_depth; ++l) {
        const std::string p = std::string(kA) + "relative_positional_encoder." + std::to_string(l + 1) + ".0.";
        if ((rc = launch_e2v_posconv(pin, h->tt.get("#posw") + (size_t)l * D * Cg * c.conv_pos_kernel, h->tt.get(p + "bias"), d_foff, B, F,
                                     D, c.conv_pos_groups, c.conv_pos_kernel, pa, s)))
            return rc;
        if ((rc = e2v_rows(pa, D, nullptr, nullptr, nullptr, 1, 1, eps, pa, F, D, s))) return rc;
        pin = pa;
        std::swap(pa, pb);
    }
    float* x = h->x.as<float>();
    if ((rc = launch_e2v_tokens(h->xf.as<float>(), pin, h->tt.get(std::string(kA) + "extra_tokens"), E, d_foff, d_toff, B, Ntok, D,
                                h->tt.get(std::string(kA) + "context_encoder.norm.weight"),
                                h->tt.get(std::string(kA) + "context_encoder.norm.bias"), eps, x, s)))
        return rc;
    for (size_t i = 0; i < h->blocks.size(); ++i) {
        const std::string& p = h->blocks[i];
        float *qkv = h->qkv.as<float>(), *at = h->attn.as<float>(), *y1 = h->y1.as<float>(), *x1 = h->x1.as<float>(), *hd = h->hid.as<float>();
        if ((rc = gm(x, D, Ntok, D, Ntok, D, p + "attn.qkv.weight", 3 * D, h->tt.get(p + "attn.qkv.bias"), nullptr, qkv,
                           x2 ? h->e_x[i] : 0)))
            return rc;
        if ((rc = launch_e2v_attention(qkv, d_toff, B, maxlen, c.num_heads, c.num_alibi_heads, E, h->tt.get("#slope") + i * c.num_heads,
                                       h->tt.get("#scale") + i * c.num_heads, at, s)))
            return rc;
        if ((rc = gm(at, D, Ntok, D, Ntok, D, p + "attn.proj.weight", D, h->tt.get(p + "attn.proj.bias"), x, y1,
                           x2 ? h->e_attn[i] : 0)))
            return rc;
        if ((rc = e2v_rows(y1, D, nullptr, h->tt.get(p + "norm1.weight"), h->tt.get(p + "norm1.bias"), 1, 0, eps, x1, Ntok, D, s))) return rc;
        if ((rc = gm(x1, D, Ntok, D, Ntok, D, p + "mlp.fc1.weight", FF, h->tt.get(p + "mlp.fc1.bias"), nullptr, hd,
                           x2 ? h->e_x1[i] : 0)))
            return rc;
        if ((rc = e2v_rows(hd, FF, nullptr, nullptr, nullptr, 0, 1, eps, hd, Ntok, FF, s))) return rc;
        if ((rc = gm(hd, FF, Ntok, FF, Ntok, FF, p + "mlp.fc2.weight", D, h->tt.get(p + "mlp.fc2.bias"), x1, y1,
                           x2 ? h->e_hid[i] : 0)))
            return rc;
        if ((rc = e2v_rows(y1, D, nullptr, h->tt.get(p + "norm2.weight"), h->tt.get(p + "norm2.bias"), 1, 0, eps, x, Ntok, D, s))) return rc;
    }
    if (feats)
        for (int b = 0; b < B; ++b)
            if (Tl[b] > 0)
                PF_HIP_TRY(hipMemcpyAsync(feats + (size_t)foff[b] * D, x + (size_t)(toff[b] + E) * D, sizeof(float) * (size_t)Tl[b] * D,
                                          hipMemcpyDeviceToDevice, s));
    if (pooled || probs) {
        if (!pooled) {
            if (h->y1.ensure(sizeof(float) * (size_t)B * D)) return -2;     // (y1 is free here)
            pooled = h->y1.as<float>();
        }
        const int Cc = probs ? c.vocab_size : 0;
        if ((rc = launch_e2v_head(x, d_toff, E, B, D, Cc ? h->tt.get("proj.weight") : nullptr, Cc ? h->tt.get("proj.bias") : nullptr,
                                  Cc ? h->mask.as<int>() : nullptr, Cc, pooled, probs, s)))
            return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

pf_emotion2vec* pf_emotion2vec_create(const pf_emotion2vec_config* cfg) {
    if (!cfg) { set_error("emotion2vec: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_emotion2vec_config& c = *cfg;
    bool ok = c.embed_dim > 0 && c.num_heads > 0 && c.embed_dim == 64 * c.num_heads && c.embed_dim % 256 == 0 && c.ffn_dim % 256 == 0 &&
              c.prenet_depth >= 0 && c.depth >= 0 && c.num_extra_tokens >= 0 && c.num_alibi_heads >= 0 && c.num_alibi_heads <= c.num_heads &&
              (c.alibi_scale_layers == 1 || c.alibi_scale_layers == c.prenet_depth + c.depth) &&
              (c.alibi_scale_heads == 1 || c.alibi_scale_heads == c.num_alibi_heads) && c.n_conv >= 1 && c.n_conv <= 8 &&
              c.conv_pos_depth >= 0 && c.conv_pos_groups > 0 && c.embed_dim % c.conv_pos_groups == 0 &&
              c.embed_dim / c.conv_pos_groups <= 64 && c.conv_pos_kernel % 2 == 1 && c.conv_pos_kernel <= 31 && c.vocab_size >= 0 &&
              c.vocab_size <= 1024 && (c.precision == 0 || c.precision == 3) && c.norm_eps > 0.f;
    for (int l = 0; ok && l < c.n_conv; ++l)
        ok = c.conv_kernel[l] > 0 && c.conv_stride[l] > 0 && c.conv_kernel[l] >= c.conv_stride[l] && (l > 0 || c.conv_kernel[0] <= 32);
    const int fw = c.embed_dim / 256, hw = c.ffn_dim / 256;
    auto width_ok = [](int w) { return w == 1 || w == 2 || w == 3 || w == 4 || w == 8 || w == 12 || w == 16; };
    if (!ok || !width_ok(fw) || !width_ok(hw)) {
        set_error("emotion2vec: unsupported config (head dim 64, embed_dim and ffn_dim 256 x {1, 2, 3, 4, 8, 12, 16}, <= 8 conv layers, "
                  "positional groups of <= 64 channels, odd kernel <= 31, precision 0 or 3)");
        return nullptr;
    }
    std::unique_ptr<E2v> h(new E2v());
    h->cfg = c;
    const int D = c.embed_dim;
    int rc = 0;
    const std::string A = kA;
    rc |= h->tt.add(A + "extra_tokens", (int64_t)c.num_extra_tokens * D);
    rc |= h->tt.add(A + "alibi_scale", (int64_t)c.alibi_scale_layers * c.alibi_scale_heads);
    for (int l = 0; l < c.n_conv; ++l) {
        if (l == 0) rc |= h->tt.add(conv_name(0, ".0.weight"), (int64_t)512 * c.conv_kernel[0]);
        else rc |= h->tt.add_conv(conv_name(l, ".0.weight"), 512, 512, c.conv_kernel[l]);
        rc |= h->tt.add_linear(conv_name(l, ".2.1."), 512, 1);
    }
    rc |= h->tt.add_linear(A + "project_features.1.", 512, 1);
    rc |= h->tt.add_linear(A + "project_features.2.", D, 512);
    for (int l = 0; l < c.conv_pos_depth; ++l)
        rc |= h->tt.add_linear(A + "relative_positional_encoder." + std::to_string(l + 1) + ".0.", D, (int64_t)(D / c.conv_pos_groups) * c.conv_pos_kernel);
    rc |= h->tt.add_linear(A + "context_encoder.norm.", D, 1);
    for (int i = 0; i < c.prenet_depth; ++i) h->blocks.push_back(A + "context_encoder.blocks." + std::to_string(i) + ".");
    for (int i = 0; i < c.depth; ++i) h->blocks.push_back("blocks." + std::to_string(i) + ".");
    for (const std::string& p : h->blocks) {
        for (const char* nm : {"norm1.", "norm2."}) rc |= h->tt.add_linear(p + nm, D, 1);
        rc |= h->tt.add_linear(p + "attn.qkv.", 3 * D, D);
        rc |= h->tt.add_linear(p + "attn.proj.", D, D);
        rc |= h->tt.add_linear(p + "mlp.fc1.", c.ffn_dim, D);
        rc |= h->tt.add_linear(p + "mlp.fc2.", D, c.ffn_dim);
    }
    if (c.vocab_size > 0) rc |= h->tt.add_linear("proj.", c.vocab_size, D);
    if (rc) return nullptr;
    return reinterpret_cast<pf_emotion2vec*>(h.release());
}
void pf_emotion2vec_destroy(pf_emotion2vec* h) { delete reinterpret_cast<E2v*>(h); }
int pf_emotion2vec_set_tensor(pf_emotion2vec* hh, const char* name, const float* data, int64_t numel) {
    E2v* h = reinterpret_cast<E2v*>(hh);
    PF_REQUIRE(h && name && data, "emotion2vec_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_emotion2vec_missing(const pf_emotion2vec* hh) {
    const E2v* h = reinterpret_cast<const E2v*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_emotion2vec_set_label_mask(pf_emotion2vec* hh, const int32_t* mask_host, int32_t n) {
    E2v* h = reinterpret_cast<E2v*>(hh);
    PF_REQUIRE(h && mask_host && n == h->cfg.vocab_size && n > 0, "emotion2vec_set_label_mask: one entry per class");
    if (h->mask.ensure(sizeof(int32_t) * n)) return -2;
    PF_HIP_TRY(hipMemcpy(h->mask.p, mask_host, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    h->mask_set = true;
    return 0;
}
int pf_emotion2vec_set_max_samples(pf_emotion2vec* hh, int64_t max_samples) {
    E2v* h = reinterpret_cast<E2v*>(hh);
    PF_REQUIRE(h && max_samples > 0, "emotion2vec_set_max_samples: null handle or non-positive size");
    h->max_samples = max_samples;
    return 0;
}
int32_t pf_emotion2vec_num_frames(const pf_emotion2vec* hh, int64_t n_samples) {
    const E2v* h = reinterpret_cast<const E2v*>(hh);
    return h ? (int32_t)h->frames(n_samples, h->cfg.n_conv - 1) : -1;
}
int pf_emotion2vec_forward(pf_emotion2vec* hh, const float* wav, const int64_t* lens_host, int32_t B, float* feats, float* pooled,
                           float* probs, void* stream) {
    E2v* h = reinterpret_cast<E2v*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && wav && lens_host && B > 0, "emotion2vec_forward: null/empty argument");
    PF_REQUIRE(!probs || h->cfg.vocab_size > 0, "emotion2vec_forward: probabilities need vocab_size > 0 (proj)");
    for (int b = 0; b < B; ++b)
        if (h->frames(lens_host[b], h->cfg.n_conv - 1) < 1) {
            int64_t need = 1;
            while (h->frames(need, h->cfg.n_conv - 1) < 1) ++need;
            set_error("emotion2vec: utterance " + std::to_string(b) + " has " + std::to_string(lens_host[b]) + " samples; the conv encoder needs at least " +
                      std::to_string(need));
            return -1;
        }
    int rc;
    if ((rc = h->tt.require_all("emotion2vec"))) return rc;
    if (h->prepared != h->tt.version && (rc = h->prepare(s))) return rc;
    int64_t so = 0, fo = 0;
    for (int b0 = 0; b0 < B;) {
        int b1 = b0 + 1;
        int64_t tot = lens_host[b0];
        while (b1 < B && tot + lens_host[b1] <= h->max_samples) tot += lens_host[b1++];
        if ((rc = run(h, wav + so, lens_host + b0, b1 - b0, feats ? feats + fo * h->D() : nullptr, pooled ? pooled + (size_t)b0 * h->D() : nullptr,
                      probs ? probs + (size_t)b0 * h->C() : nullptr, s)))
            return rc;
        for (int b = b0; b < b1; ++b) fo += h->frames(lens_host[b], h->cfg.n_conv - 1);
        so += tot;
        b0 = b1;
    }
    return 0;
}

}  // extern "C"
