// C-ABI layer, chunk Conformer encoder of the Transducer family (funasr/models/conformer/encoder.py ConformerChunkEncoder, registered
// as ChunkConformerEncoder): pf_chunkconformer_* and the pf_k_cc_* hooks (kernels in chunk_conformer.hip; LayerNorm, Swish and every
// linear are the shared launchers; the un-masked, symmetric convolution module is conformer.hip's).
//
// Load time (prepare(), again whenever the table version moves): the second conv [O, I, kt, kf] is repacked tap-major / channel-minor
// (column (kt k + kf) I + i), embed.output's columns go from the reference's (c, f) order to the layout's (f, c), the BatchNorms are
// folded to scale / shift with conv_mod_norm_eps, and 0.5 (feed_forward_scale) is folded into both w_2 and their biases.
//
// One forward over the zero-padded batch [B, Tin, F], every row of it computed as the reference does:
//   front (StreamingConvInput, vgg_like = False): with a chunk size c the clips are cut into pieces of c * factor frames (the last
//   zero-filled) and EVERY piece of EVERY clip goes through the same launches: conv0 + ReLU -> the second conv as operand gather +
//   exact-fp32 GEMM (K in slices of 1024) + ReLU, in slabs of at most SLAB_FLOATS operand floats -> the output linear over rows of
//   F2 C floats -> the first T = ceil(ceil(Tin / 2) / s2) rows of each clip. No sqrt(D) scaling, no positional add.
//   per branch (utt: no chunk mask; chunk: the mask of (c, left_chunk)), per block:
//     x += w_2#half(swish(w_1(norm_macaron x))); x += linear_out(window attention(norm_self_att x)); x += pointwise_conv2(GLU /
//     depthwise / BatchNorm / Swish (pointwise_conv1(norm_conv x))); x += w_2#half(swish(w_1(norm_feed_forward x))); x = norm_final x
//   norm_blocks, then every time_reduction-th row.
// Both branches read the front's rows; the utt branch alone costs one pass (Transducer decoding needs nothing else).
// fp32 only: exact-fp32 MFMA GEMMs throughout.
#include <algorithm>

#include "engine_internal.h"
#include "chunk_conformer.h"
#include "conformer.h"

using namespace pf;

namespace {

constexpr int K_SLICE = 1024;                              // K extent of one launch of the long-K GEMMs (conv1, the output linear)
constexpr size_t SLAB_FLOATS = (size_t)64 << 20;           // operand floats of one conv1 slab (256 MB)
constexpr long long FRONT_MAX_FLOATS = 1ll << 31;         // floats of the first conv's output over a whole batch (8 GB)
constexpr int POS_HALF = 5000;                             // the positional table holds rows for positions 4999 .. -4999

struct Cc {
    pf_chunkconformer_config cfg;
    TensorTable tt;
    unsigned long long prepared_for = TensorTable::NOT_PREPARED;
    DevBuf y0, col, y1, t1, e2, t2, emb, xa, xb, xn, qkv, P, att, hid, planes, klens;
    int k2() const { return cfg.subsampling == 6 ? 5 : 3; }
    int s2() const { return cfg.subsampling / 2; }
    int F1() const { return (cfg.input_dim - 3) / 2 + 1; }
    int F2() const { return (F1() - k2()) / s2() + 1; }
    int out_len(int n) const { return ((n + 1) / 2 + s2() - 1) / s2(); }
    int prepare();
};

std::string blk(int i) { return "encoders.blocks." + std::to_string(i) + "."; }

#define CC_CHECK(cond)                                                                          \
    do {                                                                                        \
        if (!(cond)) { set_error("chunkconformer: weight preparation failed (HIP copy)"); return -2; } \
    } while (0)

int Cc::prepare() {
    const int D = cfg.d_model, k = k2(), f2 = F2();
    {   // [O, I, kt, kf] -> [O, (kt k + kf) I + i]
        std::vector<float> src = tt.host("embed.conv.2.weight"), dst(src.size());
        CC_CHECK(!src.empty());
        for (int o = 0; o < D; ++o)
            for (int i = 0; i < D; ++i)
                for (int kk = 0; kk < k * k; ++kk) dst[((size_t)o * k * k + kk) * D + i] = src[((size_t)o * D + i) * k * k + kk];
        CC_CHECK(!tt.put_derived("#conv1", dst));
    }
    {   // embed.output [D, D F2]: column c F2 + f -> f D + c
        std::vector<float> src = tt.host("embed.output.weight"), dst(src.size());
        CC_CHECK(!src.empty());
        const size_t K = (size_t)D * f2;
        for (int o = 0; o < D; ++o)
            for (int c = 0; c < D; ++c)
                for (int f = 0; f < f2; ++f) dst[o * K + (size_t)f * D + c] = src[o * K + (size_t)c * f2 + f];
        CC_CHECK(!tt.put_derived("#embed.output", dst));
    }
    std::vector<float> bnv((size_t)cfg.n_blocks * 2 * D);
    for (int i = 0; i < cfg.n_blocks; ++i) {
        const std::string p = blk(i);
        std::vector<double> sc, sh;
        CC_CHECK(tt.bn_fold(p + "conv_mod.norm.", true, (double)cfg.bn_eps, sc, sh));
        for (int c = 0; c < D; ++c) {
            bnv[((size_t)i * 2) * D + c] = (float)sc[c];
            bnv[((size_t)i * 2 + 1) * D + c] = (float)sh[c];
        }
        for (const char* ff : {"feed_forward.", "feed_forward_macaron."}) {
            std::vector<float> w = tt.host(p + ff + "w_2.weight"), bb = tt.host(p + ff + "w_2.bias");
            CC_CHECK(!w.empty() && !bb.empty());
            for (float& v : w) v *= 0.5f;
            for (float& v : bb) v *= 0.5f;
            CC_CHECK(!tt.put_derived(p + ff + "w_2.weight#half", w) && !tt.put_derived(p + ff + "w_2.bias#half", bb));
        }
    }
    CC_CHECK(!tt.put_derived("#bn", bnv));
    prepared_for = tt.version;
    return 0;
}

int ready(Cc* e) {
    if (e->tt.require_all("chunkconformer")) return -3;
    if (e->prepared_for != e->tt.version) return e->prepare();
    return 0;
}

// out_a / out_b so that the last K slice lands in dst
int sliced(const float* A, const float* W, const float* bias, int M, int N, int K, float* dst, float* tmp, hipStream_t s) {
    const int ns = ceil_div(K, K_SLICE);
    const float* last = nullptr;
    if (int rc = gemm_f32_ksliced(A, K, W, K, bias, M, N, K, K_SLICE, ns % 2 ? dst : tmp, ns % 2 ? tmp : dst, &last, "cc.front", s)) return rc;
    if (last != dst) { set_error("chunkconformer: internal error (a sliced GEMM ended in its scratch buffer)"); return -2; }
    return 0;
}

// feats [B, Tin, F] -> emb [B, T, D]; chunk == 0: the clips whole
int run_front(Cc* e, const float* feats, int B, int Tin, int chunk, int T, hipStream_t s) {
    const pf_chunkconformer_config& c = e->cfg;
    const int D = c.d_model, F = c.input_dim, k = e->k2(), st = e->s2(), f1 = e->F1(), f2 = e->F2();
    const int LC = chunk > 0 ? chunk * c.subsampling : Tin, NC = chunk > 0 ? ceil_div(Tin, LC) : 1;
    const int T1 = (LC - 1) / 2 + 1, T2 = (T1 - 1) / st + 1, NP = B * NC;
    const long long R = (long long)NP * T2 * f2;
    const int K1 = k * k * D;
    // the front's workspace grows with the batch: conv0's output for every piece (NP T1 F1 D floats: 1.9 GB for sixteen 30-s clips at
    // D 512 and 80 features), the second conv's output (a quarter of that) and one operand slab; a batch past FRONT_MAX_FLOATS is refused
    if ((long long)NP * T1 * f1 * D > FRONT_MAX_FLOATS) {
        set_error("chunkconformer_forward: batch too large for the front (its first conv's output would pass 8 GB; split the batch)");
        return -1;
    }
    const int slab = (int)std::min<long long>(R, std::max<long long>(1, (long long)(SLAB_FLOATS / (size_t)K1)));
    if (e->y0.ensure(sizeof(float) * (size_t)NP * T1 * f1 * D) || e->col.ensure(sizeof(float) * (size_t)slab * K1) ||
        e->y1.ensure(sizeof(float) * (size_t)R * D) || e->t1.ensure(sizeof(float) * (size_t)slab * D) ||
        e->e2.ensure(sizeof(float) * (size_t)NP * T2 * D) || e->t2.ensure(sizeof(float) * (size_t)NP * T2 * D) ||
        e->emb.ensure(sizeof(float) * (size_t)B * T * D))
        return -2;
    int rc;
    {
        ProfScope ps(PROF_GEMM, 18.0 * NP * (double)T1 * f1 * D, s, "cc.front");
        if ((rc = launch_cc_conv0(feats, B, Tin, F, NC, LC, e->tt.get("embed.conv.0.weight"), e->tt.get("embed.conv.0.bias"), D,
                                  e->y0.as<float>(), s)))
            return rc;
    }
    float* y1 = e->y1.as<float>();
    for (long long r0 = 0; r0 < R; r0 += slab) {
        const int n = (int)std::min<long long>(slab, R - r0);
        if ((rc = launch_cc_im2col(e->y0.as<float>(), NP, T1, f1, D, k, st, r0, n, e->col.as<float>(), s))) return rc;
        if ((rc = sliced(e->col.as<float>(), e->tt.get("#conv1"), e->tt.get("embed.conv.2.bias"), n, D, K1, y1 + (size_t)r0 * D,
                         e->t1.as<float>(), s)))
            return rc;
    }
    if ((rc = launch_cf_act(y1, (size_t)R * D, 0, s))) return rc;
    if ((rc = sliced(y1, e->tt.get("#embed.output"), e->tt.get("embed.output.bias"), NP * T2, D, f2 * D, e->e2.as<float>(),
                     e->t2.as<float>(), s)))
        return rc;
    return launch_cc_copy_rows(e->e2.as<float>(), NC * T2, 1, e->emb.as<float>(), B, T, D, s);
}

// the blocks over emb -> out [B, To, D]; mask_chunk == 0: no chunk mask. stages (nullable, entries nullable): [B, T, D] copies of the
// front's rows, every block's output and norm_blocks' output
int run_branch(Cc* e, int B, int T, int mask_chunk, float* out, float* const* stages, hipStream_t s) {
    const pf_chunkconformer_config& c = e->cfg;
    const int D = c.d_model, FF = c.ffn_dim, M = B * T, r = c.time_reduction, nP = 2 * T - 1;
    const size_t MD = (size_t)M * D;
    float *emb = e->emb.as<float>(), *xn = e->xn.as<float>(), *qkv = e->qkv.as<float>(), *Pm = e->P.as<float>(), *att = e->att.as<float>(),
          *hid = e->hid.as<float>();
    const float* x = emb;
    float *y = e->xa.as<float>(), *spare = e->xb.as<float>();
    auto adv = [&]() {                                   // y holds the new x; emb is never written
        float* was = x == emb ? spare : const_cast<float*>(x);
        x = y;
        y = was;
    };
    auto lin = [&](const float* A, int K, const std::string& w, const float* bias, int N, const float* R1, float* C) {
        ProfScope ps(PROF_GEMM, 2.0 * M * (double)N * K, s, "cc.linear");
        return gemm_two_mode(e->tt, e->planes, false, A, K, (size_t)M, K, M, K, w, N, bias, R1, C, N, 0, 0, s);
    };
    auto ln = [&](const std::string& p, const float* in, float* o) {
        return layernorm(in, D, e->tt.get(p + "weight"), e->tt.get(p + "bias"), o, D, M, D, D, c.ln_eps, s);
    };
    auto stage = [&](int which, const float* src) -> int {
        if (stages && stages[which]) PF_HIP_TRY(hipMemcpyAsync(stages[which], src, sizeof(float) * MD, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    // matrix work of one attention launch: per 32-key tile a workgroup takes, 128 queries x 64 dims x (32 keys + 64 band rows + 32 keys)
    double att_flops = 0.0;
    for (int q0 = 0; q0 < T; q0 += 128) {
        int lo, hi, t;
        cc_window(q0, T, mask_chunk, c.left_chunk, T, &lo, &t);
        cc_window(std::min(q0 + 127, T - 1), T, mask_chunk, c.left_chunk, T, &t, &hi);
        att_flops += 2.0 * 128 * 64 * 128 * ((hi - 1) / 32 - lo / 32 + 1);
    }
    att_flops *= (double)B * c.n_heads;
    int rc;
    if ((rc = stage(0, emb))) return rc;
    const float* pos = e->tt.get("pos_table") + (size_t)(POS_HALF - T) * D;
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        auto ffn = [&](const std::string& f, const std::string& norm) {
            int q;
            if ((q = ln(p + norm, x, xn))) return q;
            if ((q = lin(xn, D, p + f + "w_1.weight", e->tt.get(p + f + "w_1.bias"), FF, nullptr, hid))) return q;
            if ((q = launch_cf_act(hid, (size_t)M * FF, 1, s))) return q;
            if ((q = lin(hid, FF, p + f + "w_2.weight#half", e->tt.get(p + f + "w_2.bias#half"), D, x, y))) return q;
            adv();
            return 0;
        };
        if ((rc = ffn("feed_forward_macaron.", "norm_macaron."))) return rc;
        // chunk-window relative-position self-attention
        if ((rc = ln(p + "norm_self_att.", x, xn))) return rc;
        const char* names[3] = {"self_att.linear_q.", "self_att.linear_k.", "self_att.linear_v."};
        for (int j = 0; j < 3; ++j) {
            GemmArgs g{};
            g.A = xn; g.lda = D; g.W = e->tt.get(p + names[j] + "weight"); g.ldw = D; g.bias = e->tt.get(p + names[j] + "bias");
            g.C = qkv + (size_t)j * D; g.ldc = 3 * D; g.M = M; g.N = D; g.K = D;
            ProfScope ps(PROF_GEMM, 2.0 * M * (double)D * D, s, "cc.linear");
            if ((rc = launch_gemm_f32(g, s))) return rc;
        }
        {
            GemmArgs g{};
            g.A = pos; g.lda = D; g.W = e->tt.get(p + "self_att.linear_pos.weight"); g.ldw = D; g.C = Pm; g.ldc = D; g.M = nP; g.N = D; g.K = D;
            if ((rc = launch_gemm_f32(g, s))) return rc;
        }
        {
            ProfScope ps(PROF_ATTN, att_flops, s, "cc.attention");
            if ((rc = launch_cc_window_attention(qkv, Pm, e->tt.get(p + "self_att.pos_bias_u"), e->tt.get(p + "self_att.pos_bias_v"),
                                                 e->klens.as<int>(), B, T, c.n_heads, mask_chunk, c.left_chunk, att, s)))
                return rc;
        }
        if ((rc = lin(att, D, p + "self_att.linear_out.weight", e->tt.get(p + "self_att.linear_out.bias"), D, x, y))) return rc;
        adv();
        // convolution module
        if ((rc = ln(p + "norm_conv.", x, xn))) return rc;
        if ((rc = lin(xn, D, p + "conv_mod.pointwise_conv1.weight", e->tt.get(p + "conv_mod.pointwise_conv1.bias"), 2 * D, nullptr, hid)))
            return rc;
        const float* bnp = e->tt.get("#bn") + (size_t)i * 2 * D;
        if ((rc = launch_cc_glu_dw(hid, e->tt.get(p + "conv_mod.depthwise_conv.weight"), e->tt.get(p + "conv_mod.depthwise_conv.bias"), bnp,
                                   bnp + D, B, T, D, c.kernel_size, c.causal_conv, att, s)))
            return rc;
        if ((rc = lin(att, D, p + "conv_mod.pointwise_conv2.weight", e->tt.get(p + "conv_mod.pointwise_conv2.bias"), D, x, y))) return rc;
        adv();
        if ((rc = ffn("feed_forward.", "norm_feed_forward."))) return rc;
        if ((rc = ln(p + "norm_final.", x, y))) return rc;
        adv();
        if ((rc = stage(1 + i, x))) return rc;
    }
    if ((rc = ln("encoders.norm_blocks.", x, y))) return rc;
    if ((rc = stage(1 + c.n_blocks, y))) return rc;
    return launch_cc_copy_rows(y, T, r, out, B, (T - 1) / r + 1, D, s);
}

int run(Cc* e, const float* feats, const int32_t* lens, int B, int Tin, int chunk, int branches, float* out_utt, float* out_chunk,
        int32_t* olens, float* const* stages, hipStream_t s) {
    const pf_chunkconformer_config& c = e->cfg;
    const int D = c.d_model, FF = c.ffn_dim, r = c.time_reduction;
    PF_REQUIRE(chunk >= 0 && chunk <= 65535, "chunkconformer_forward: chunk size in 0 .. 65535 (0: no chunks)");
    PF_REQUIRE((branches & ~3) == 0 && branches != 0 && (!(branches & 1) || out_utt) && (!(branches & 2) || out_chunk),
               "chunkconformer_forward: branches = 1 (utt), 2 (chunk) or 3, each with its output");
    const int T = e->out_len(Tin);
    if (T > POS_HALF) { set_error("chunkconformer: " + std::to_string(T) + " encoder frames; the positional table holds 5000"); return -1; }
    PF_REQUIRE((long long)B * T <= 0x7fffffff / 4 / std::max(3 * D, FF), "chunkconformer_forward: batch too large");
    std::vector<int32_t> kl(B);
    for (int b = 0; b < B; ++b) {
        PF_REQUIRE(lens[b] >= 1 && lens[b] <= Tin, "chunkconformer_forward: every length must lie in 1 .. Tin");
        kl[b] = e->out_len(lens[b]);
        if (olens) olens[b] = (kl[b] - 1) / r + 1;
    }
    int rc;
    if ((rc = ready(e))) return rc;
    const size_t M = (size_t)B * T;
    if (e->xa.ensure(sizeof(float) * M * D) || e->xb.ensure(sizeof(float) * M * D) || e->xn.ensure(sizeof(float) * M * D) ||
        e->qkv.ensure(sizeof(float) * M * 3 * D) || e->att.ensure(sizeof(float) * M * D) || e->hid.ensure(sizeof(float) * M * std::max(FF, 2 * D)) ||
        e->P.ensure(sizeof(float) * (size_t)(2 * T - 1) * D) || e->klens.ensure(sizeof(int32_t) * B))
        return -2;
    if (upload_h2d(e->klens.p, kl.data(), sizeof(int32_t) * B, s)) return -2;
    if ((rc = run_front(e, feats, B, Tin, chunk, T, s))) return rc;
    // `stages` follow the chunk branch where it runs, else the utt branch
    if ((branches & 1) && (rc = run_branch(e, B, T, 0, out_utt, (branches & 2) ? nullptr : stages, s))) return rc;
    if ((branches & 2) && (rc = run_branch(e, B, T, chunk, out_chunk, stages, s))) return rc;
    return 0;
}

}  // namespace

extern "C" {

pf_chunkconformer* pf_chunkconformer_create(const pf_chunkconformer_config* cfg) {
    if (!cfg) { set_error("chunkconformer: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_chunkconformer_config& c = *cfg;
    const bool sub_ok = c.subsampling == 2 || c.subsampling == 4 || c.subsampling == 6;
    if (!sub_ok || c.input_dim < 16 || c.input_dim > 256 || c.n_heads < 1 || c.d_model != 64 * c.n_heads || c.d_model > 2048 || c.ffn_dim < 32 ||
        c.ffn_dim % 32 != 0 || c.n_blocks < 1 || c.kernel_size < 1 || c.kernel_size > 31 || c.kernel_size % 2 != 1 || c.time_reduction < 1 ||
        !(c.ln_eps > 0.f) || !(c.bn_eps > 0.f)) {
        set_error("chunkconformer: unsupported config (built: subsampling 2 / 4 / 6, 16 .. 256 input features, d_model = 64 n_heads up to "
                  "2048, ffn_dim a multiple of 32, odd kernel_size up to 31, n_blocks >= 1, time_reduction >= 1)");
        return nullptr;
    }
    std::unique_ptr<Cc> h(new Cc());
    h->cfg = c;
    const int D = c.d_model, FF = c.ffn_dim, k = h->k2();
    int rc = 0;
    rc |= h->tt.add_linear("embed.conv.0.", D, 9);
    rc |= h->tt.add_linear("embed.conv.2.", D, (int64_t)D * k * k);
    rc |= h->tt.add_linear("embed.output.", D, (int64_t)D * h->F2());
    rc |= h->tt.add("pos_table", (int64_t)(2 * POS_HALF - 1) * D);
    rc |= h->tt.add_linear("encoders.norm_blocks.", D, 1);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk(i);
        for (const char* n : {"self_att.linear_q.", "self_att.linear_k.", "self_att.linear_v.", "self_att.linear_out.", "conv_mod.pointwise_conv2."})
            rc |= h->tt.add_linear(p + n, D, D);
        rc |= h->tt.add_linear(p + "self_att.linear_pos.", D, D, false);
        rc |= h->tt.add(p + "self_att.pos_bias_u", D);
        rc |= h->tt.add(p + "self_att.pos_bias_v", D);
        for (const char* f : {"feed_forward.", "feed_forward_macaron."}) {
            rc |= h->tt.add_linear(p + f + "w_1.", FF, D);
            rc |= h->tt.add_linear(p + f + "w_2.", D, FF);
        }
        rc |= h->tt.add_linear(p + "conv_mod.pointwise_conv1.", 2 * D, D);
        rc |= h->tt.add_linear(p + "conv_mod.depthwise_conv.", D, c.kernel_size);
        rc |= h->tt.add_linear(p + "conv_mod.norm.", D, 1);
        rc |= h->tt.add(p + "conv_mod.norm.running_mean", D);
        rc |= h->tt.add(p + "conv_mod.norm.running_var", D);
        for (const char* n : {"norm_feed_forward.", "norm_self_att.", "norm_macaron.", "norm_conv.", "norm_final."}) rc |= h->tt.add_linear(p + n, D, 1);
    }
    if (rc) return nullptr;
    return reinterpret_cast<pf_chunkconformer*>(h.release());
}
void pf_chunkconformer_destroy(pf_chunkconformer* h) { delete reinterpret_cast<Cc*>(h); }
int pf_chunkconformer_set_tensor(pf_chunkconformer* hh, const char* name, const float* data, int64_t numel) {
    Cc* h = reinterpret_cast<Cc*>(hh);
    PF_REQUIRE(h && name && data, "chunkconformer_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_chunkconformer_missing(const pf_chunkconformer* hh) {
    const Cc* h = reinterpret_cast<const Cc*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_chunkconformer_set_precision(pf_chunkconformer* hh, int32_t precision) {
    PF_REQUIRE(hh && precision == 0, "chunkconformer_set_precision: 0 (fp32) is the one arithmetic built");
    return 0;
}
int32_t pf_chunkconformer_num_frames(const pf_chunkconformer* hh, int32_t n_frames) {
    const Cc* h = reinterpret_cast<const Cc*>(hh);
    if (!h || n_frames < 1) return -1;
    return (h->out_len(n_frames) - 1) / h->cfg.time_reduction + 1;
}
int pf_chunkconformer_debug_poison(pf_chunkconformer* hh) {
    Cc* h = reinterpret_cast<Cc*>(hh);
    PF_REQUIRE(h, "chunkconformer_debug_poison: null handle");
    PF_HIP_TRY(hipDeviceSynchronize());
    for (DevBuf* b : {&h->y0, &h->col, &h->y1, &h->t1, &h->e2, &h->t2, &h->emb, &h->xa, &h->xb, &h->xn, &h->qkv, &h->P, &h->att, &h->hid})
        if (b->p) PF_HIP_TRY(hipMemset(b->p, 0xff, b->cap));
    return 0;
}
int pf_chunkconformer_forward(pf_chunkconformer* hh, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, int32_t chunk,
                              int32_t branches, float* out_utt, float* out_chunk, int32_t* out_lens_host, float* const* stages_dev,
                              void* stream) {
    Cc* h = reinterpret_cast<Cc*>(hh);
    PF_REQUIRE(h && feats && lens_host && B > 0 && B <= 65535 && Tin > 0, "chunkconformer_forward: null/empty argument");
    return run(h, feats, lens_host, B, Tin, chunk, branches, out_utt, out_chunk, out_lens_host, stages_dev, reinterpret_cast<hipStream_t>(stream));
}
int pf_chunkconformer_front(pf_chunkconformer* hh, const float* feats, int32_t B, int32_t Tin, int32_t chunk, float* out, void* stream) {
    Cc* h = reinterpret_cast<Cc*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && feats && out && B > 0 && B <= 65535 && Tin > 0 && chunk >= 0 && chunk <= 65535, "chunkconformer_front: null/empty argument");
    if (int rc = ready(h)) return rc;
    const int T = h->out_len(Tin);
    if (int rc = run_front(h, feats, B, Tin, chunk, T, s)) return rc;
    PF_HIP_TRY(hipMemcpyAsync(out, h->emb.p, sizeof(float) * (size_t)B * T * h->cfg.d_model, hipMemcpyDeviceToDevice, s));
    return 0;
}

int pf_k_cc_window_attention(const float* qkv_dev, const float* P_dev, const float* u_dev, const float* v_dev, const int32_t* klens_dev,
                             int32_t B, int32_t T, int32_t H, int32_t chunk, int32_t left, float* out_dev, void* stream) {
    return launch_cc_window_attention(qkv_dev, P_dev, u_dev, v_dev, klens_dev, B, T, H, chunk, left, out_dev, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_cc_glu_dw(const float* g_dev, const float* dw_dev, const float* dw_bias_dev, const float* bn_scale_dev, const float* bn_shift_dev,
                   int32_t B, int32_t T, int32_t D, int32_t taps, int32_t causal, float* y_dev, void* stream) {
    return launch_cc_glu_dw(g_dev, dw_dev, dw_bias_dev, bn_scale_dev, bn_shift_dev, B, T, D, taps, causal, y_dev, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_cc_copy_rows(const float* x_dev, int32_t Ti, int32_t step, float* y_dev, int32_t B, int32_t To, int32_t D, void* stream) {
    return launch_cc_copy_rows(x_dev, Ti, step, y_dev, B, To, D, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
