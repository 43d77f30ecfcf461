// C-ABI layer, CAM++ speaker embedding: pf_campplus_* (kernels in campplus.hip).
//
// Load time: the reference's tensors are kept as set; at the first forward after a change every BatchNorm that FOLLOWS a conv is
// folded into that conv (float64 on the host), the 3x3 / k-tap weights are repacked tap-major for the gather of the implicit
// GEMM, the TDNN weight is permuted to the head's channels-last column order (f * 32 + c instead of c * 10 + f) and the final
// dense weight is transposed. The BatchNorm-ReLU in FRONT of a dense / transit conv stays a per-channel scale / shift that the
// GEMM applies to its A operand.
//
// One forward, per sub-batch of chunks (workspace bounded by max_batch):
//   head  [n T 80, 1] -> conv3x3 [n T 80, 32] -> 2 x 2 BasicResBlocks (the first of each with stride 2 in frequency; conv2 and
//         the projection shortcut are one GEMM over concatenated K) -> conv3x3 stride 2 -> [n T, 10 * 32]
//   tdnn  k 5 stride 2 -> columns 0..127 of block 1's concat buffer [n T', 512]
//   3 D-TDNN blocks: per layer, 1x1 GEMM with BN-ReLU on load -> bottleneck [n T', 128]; CAM context -> mask [n, nseg, 32];
//         dilated k-3 local conv times the mask -> the layer's 32 columns of the concat buffer; transit: BN-ReLU on load 1x1
//         GEMM into the first columns of the next buffer
//   pool  out BN-ReLU, mean / std over time, dense 1024 -> 192, affine-free BN
#include "engine_internal.h"
#include "campplus.h"

using namespace pf;

namespace {

const int kLayers[3] = {12, 24, 16};
const int kDil[3] = {1, 2, 2};

struct DenseW {
    const float *pre_sc, *pre_sh, *w1, *b1, *wl, *cw1, *cb1, *cw2, *cb2;
};

struct Campplus {
    pf_campplus_config cfg;
    TensorTable tt;
    pf_frontend* fe = nullptr;
    int max_batch = 256;
    unsigned long long folded_version = ~0ull;
    std::vector<DenseW> layers;
    DevBuf fa, fb, fc, h, mask, wav, feats, starts, valid;
    ~Campplus() { if (fe) pf_frontend_destroy(fe); }

    int fold();
};

#define CAM_CHECK(cond)                                                              \
    do {                                                                             \
        if (!(cond)) { set_error("campplus: weight folding failed (HIP copy)"); return -2; } \
    } while (0)

// conv2d [O, I, 3, 3] (+ BN) -> [O, 9 I (+ I2)] tap-major, the shortcut's 1x1 conv (+ its BN) appended; bias = both BN shifts
int Campplus::fold() {
    const int mc = cfg.m_channels;
    const double eps = (double)cfg.bn_eps;
    auto conv3 = [&](const std::string& key, const std::string& conv, const std::string& bnp, const std::string& sc_conv,
                     const std::string& sc_bn, int I) -> int {
        std::vector<float> w = tt.host(conv + "weight");
        std::vector<double> s, t, s2, t2;
        CAM_CHECK(!w.empty() && tt.bn_fold(bnp, true, eps, s, t));
        const int O = mc, I2 = sc_conv.empty() ? 0 : mc, K = 9 * I + I2;
        std::vector<float> wp((size_t)O * K), bias(O);
        std::vector<float> ws;
        if (I2) { ws = tt.host(sc_conv + "weight"); CAM_CHECK(!ws.empty() && tt.bn_fold(sc_bn, true, eps, s2, t2)); }
        for (int o = 0; o < O; ++o) {
            for (int i = 0; i < I; ++i)
                for (int tap = 0; tap < 9; ++tap) wp[(size_t)o * K + tap * I + i] = (float)(w[((size_t)o * I + i) * 9 + tap] * s[o]);
            for (int i = 0; i < I2; ++i) wp[(size_t)o * K + 9 * I + i] = (float)(ws[(size_t)o * I2 + i] * s2[o]);
            bias[o] = (float)(t[o] + (I2 ? t2[o] : 0.0));
        }
        CAM_CHECK(!tt.put_derived(key + ".w", wp) && !tt.put_derived(key + ".b", bias));
        return 0;
    };
    int rc;
    if ((rc = conv3("head.conv1", "head.conv1.", "head.bn1.", "", "", 1))) return rc;
    for (int l = 1; l <= 2; ++l)
        for (int b = 0; b < 2; ++b) {
            const std::string p = "head.layer" + std::to_string(l) + "." + std::to_string(b) + ".";
            if ((rc = conv3(p + "conv1", p + "conv1.", p + "bn1.", "", "", mc))) return rc;
            if ((rc = conv3(p + "conv2", p + "conv2.", p + "bn2.", b == 0 ? p + "shortcut.0." : "", p + "shortcut.1.", mc))) return rc;
        }
    if ((rc = conv3("head.conv2", "head.conv2.", "head.bn2.", "", "", mc))) return rc;
    // TDNN [C0, mc * F, 5]: input channel c * F + f of the reference is column f * mc + c of the head's output
    {
        const int F = cfg.feat_dim / 8, Cin = mc * F, O = cfg.init_channels;
        std::vector<float> w = tt.host("xvector.tdnn.linear.weight");
        std::vector<double> s, t;
        CAM_CHECK(!w.empty() && tt.bn_fold("xvector.tdnn.nonlinear.batchnorm.", true, eps, s, t));
        std::vector<float> wp((size_t)O * 5 * Cin), bias(O);
        for (int o = 0; o < O; ++o) {
            for (int c = 0; c < mc; ++c)
                for (int f = 0; f < F; ++f)
                    for (int k = 0; k < 5; ++k)
                        wp[(size_t)o * 5 * Cin + k * Cin + f * mc + c] = (float)(w[((size_t)o * Cin + c * F + f) * 5 + k] * s[o]);
            bias[o] = (float)t[o];
        }
        CAM_CHECK(!tt.put_derived("tdnn.w", wp) && !tt.put_derived("tdnn.b", bias));
    }
    auto pre = [&](const std::string& key, const std::string& bnp) -> int {
        std::vector<double> s, t;
        CAM_CHECK(tt.bn_fold(bnp, true, eps, s, t));
        CAM_CHECK(!tt.put_derived(key + ".sc", std::vector<float>(s.begin(), s.end())) && !tt.put_derived(key + ".sh", std::vector<float>(t.begin(), t.end())));
        return 0;
    };
    const int G = cfg.growth_rate, BNC = cfg.bn_size * cfg.growth_rate;
    int ch = cfg.init_channels;
    layers.clear();
    for (int blk = 0; blk < 3; ++blk) {
        for (int i = 0; i < kLayers[blk]; ++i) {
            const std::string p = "xvector.block" + std::to_string(blk + 1) + ".tdnnd" + std::to_string(i + 1) + ".";
            const int Cin = ch + i * G;
            if ((rc = pre(p + "pre", p + "nonlinear1.batchnorm."))) return rc;
            std::vector<float> w1 = tt.host(p + "linear1.weight"), wl = tt.host(p + "cam_layer.linear_local.weight");
            std::vector<double> s, t;
            CAM_CHECK(!w1.empty() && !wl.empty() && tt.bn_fold(p + "nonlinear2.batchnorm.", true, eps, s, t));
            std::vector<float> w1p((size_t)BNC * Cin), b1(BNC), wlp((size_t)G * 3 * BNC);
            for (int o = 0; o < BNC; ++o) {
                for (int c = 0; c < Cin; ++c) w1p[(size_t)o * Cin + c] = (float)(w1[(size_t)o * Cin + c] * s[o]);
                b1[o] = (float)t[o];
            }
            for (int o = 0; o < G; ++o)
                for (int c = 0; c < BNC; ++c)
                    for (int k = 0; k < 3; ++k) wlp[(size_t)o * 3 * BNC + k * BNC + c] = wl[((size_t)o * BNC + c) * 3 + k];
            CAM_CHECK(!tt.put_derived(p + "w1", w1p) && !tt.put_derived(p + "b1", b1) && !tt.put_derived(p + "wl", wlp));
            DenseW d;
            d.pre_sc = tt.get(p + "pre.sc"); d.pre_sh = tt.get(p + "pre.sh");
            d.w1 = tt.get(p + "w1"); d.b1 = tt.get(p + "b1"); d.wl = tt.get(p + "wl");
            d.cw1 = tt.get(p + "cam_layer.linear1.weight"); d.cb1 = tt.get(p + "cam_layer.linear1.bias");
            d.cw2 = tt.get(p + "cam_layer.linear2.weight"); d.cb2 = tt.get(p + "cam_layer.linear2.bias");
            layers.push_back(d);
        }
        ch += kLayers[blk] * G;
        const std::string p = "xvector.transit" + std::to_string(blk + 1) + ".";
        if ((rc = pre(p + "pre", p + "nonlinear.batchnorm."))) return rc;
        ch /= 2;
    }
    if ((rc = pre("out", "xvector.out_nonlinear.batchnorm."))) return rc;
    {
        const int E = cfg.embedding_size, K = 2 * ch;
        std::vector<float> w = tt.host("xvector.dense.linear.weight"), wt((size_t)K * E);
        std::vector<double> s, t;
        CAM_CHECK(!w.empty() && tt.bn_fold("xvector.dense.nonlinear.batchnorm.", false, eps, s, t));
        for (int o = 0; o < E; ++o)
            for (int k = 0; k < K; ++k) wt[(size_t)k * E + o] = w[(size_t)o * K + k];
        CAM_CHECK(!tt.put_derived("dense.wt", wt) && !tt.put_derived("dense.sc", std::vector<float>(s.begin(), s.end())) &&
                  !tt.put_derived("dense.sh", std::vector<float>(t.begin(), t.end())));
    }
    folded_version = tt.version;
    return 0;
}

// conv2d GEMM over [n T Fin, Cin] -> [n T Fo, mc]
int head_conv(Campplus* c, const std::string& key, const float* A, int Cin, int Fin, int Fo, int fstride, const float* A2, int Fin2,
              int fstride2, const float* R, float* out, int n, int T, hipStream_t s) {
    const int mc = c->cfg.m_channels;
    CamGemmArgs g{};
    g.conv2d = 1;
    g.M = n * T * Fo; g.N = mc; g.K = 9 * Cin + (A2 ? mc : 0);
    g.W = c->tt.get(key + ".w"); g.ldw = g.K; g.bias = c->tt.get(key + ".b");
    g.C = out; g.ldc = mc; g.R = R; g.ldr = mc; g.relu = 1;
    g.A = A; g.lda = Cin; g.Cin = Cin; g.T = T; g.Fin = Fin; g.Fo = Fo; g.fstride = fstride;
    g.A2 = A2; g.Cin2 = A2 ? mc : 0; g.Fin2 = Fin2; g.fstride2 = fstride2;
    return launch_cam_gemm(g, s);
}

// 1-D conv / 1x1 GEMM over rows of n chunks
int tdnn_gemm(const float* A, int lda, int Tin, int To, int Cin, int taps, int stride, int dil, int pad, const float* W, int N,
              const float* bias, int relu, const float* pre_sc, const float* pre_sh, const float* mask, float* C, int ldc, int n,
              hipStream_t s) {
    CamGemmArgs g{};
    g.M = n * To; g.N = N; g.K = taps * Cin;
    g.W = W; g.ldw = g.K; g.bias = bias; g.relu = relu;
    g.C = C; g.ldc = ldc;
    g.mask = mask; g.nseg = (To + 99) / 100;
    g.A = A; g.lda = lda; g.Tin = Tin; g.To = To; g.Cin = Cin; g.taps = taps; g.stride = stride; g.dil = dil; g.pad = pad;
    g.pre_scale = pre_sc; g.pre_shift = pre_sh;
    return launch_cam_gemm(g, s);
}

// the network on n chunks of T frames: feats [n, T, 80] -> emb [n, E]
int run_net(Campplus* c, const float* feats, int n, int T, float* emb, hipStream_t s) {
    const int mc = c->cfg.m_channels, F0 = c->cfg.feat_dim, F1 = F0 / 2, F2 = F0 / 4, F3 = F0 / 8;
    const int T2 = (T - 1) / 2 + 1;
    const int G = c->cfg.growth_rate, BNC = c->cfg.bn_size * G;
    const size_t head = (size_t)n * T * F0 * mc;
    const size_t tail = (size_t)n * T2 * 1024;
    const size_t big = head > tail ? head : tail;
    if (c->fa.ensure(sizeof(float) * big) || c->fb.ensure(sizeof(float) * big) || c->fc.ensure(sizeof(float) * big) ||
        c->h.ensure(sizeof(float) * (size_t)n * T2 * BNC) || c->mask.ensure(sizeof(float) * (size_t)n * ((T2 + 99) / 100) * G))
        return -2;
    float *A = c->fa.as<float>(), *B = c->fb.as<float>(), *Cc = c->fc.as<float>();
    int rc;
    // ---- head
    if ((rc = head_conv(c, "head.conv1", feats, 1, F0, F0, 1, nullptr, 0, 0, nullptr, A, n, T, s))) return rc;
    int F = F0;
    for (int l = 1; l <= 2; ++l) {
        const int Fo = l == 1 ? F1 : F2;
        const std::string p = "head.layer" + std::to_string(l) + ".";
        // block 0: A [F] -> B [Fo] -> C [Fo] (+ projection shortcut of A)
        if ((rc = head_conv(c, p + "0.conv1", A, mc, F, Fo, 2, nullptr, 0, 0, nullptr, B, n, T, s))) return rc;
        if ((rc = head_conv(c, p + "0.conv2", B, mc, Fo, Fo, 1, A, F, 2, nullptr, Cc, n, T, s))) return rc;
        // block 1: C -> B -> A (+ C)
        if ((rc = head_conv(c, p + "1.conv1", Cc, mc, Fo, Fo, 1, nullptr, 0, 0, nullptr, B, n, T, s))) return rc;
        if ((rc = head_conv(c, p + "1.conv2", B, mc, Fo, Fo, 1, nullptr, 0, 0, Cc, A, n, T, s))) return rc;
        F = Fo;
    }
    if ((rc = head_conv(c, "head.conv2", A, mc, F2, F3, 2, nullptr, 0, 0, nullptr, B, n, T, s))) return rc;
    // ---- tdnn: B [n T, F3 mc] -> A cols 0..C0
    const int C0 = c->cfg.init_channels;
    int ld = C0 + kLayers[0] * G;
    if ((rc = tdnn_gemm(B, F3 * mc, T, T2, F3 * mc, 5, 2, 1, 2, c->tt.get("tdnn.w"), C0, c->tt.get("tdnn.b"), 1, nullptr, nullptr,
                        nullptr, A, ld, n, s)))
        return rc;
    // ---- D-TDNN blocks; buffers: block 1 in A, block 2 in C, block 3 in A, transit 3 out in C
    float* cur = A;
    float* nxt = Cc;
    int ch = C0, li = 0;
    float* hb = c->h.as<float>();
    float* mk = c->mask.as<float>();
    for (int blk = 0; blk < 3; ++blk) {
        for (int i = 0; i < kLayers[blk]; ++i, ++li) {
            const DenseW& d = c->layers[li];
            const int Cin = ch + i * G, dil = kDil[blk];
            if ((rc = tdnn_gemm(cur, ld, T2, T2, Cin, 1, 1, 1, 0, d.w1, BNC, d.b1, 1, d.pre_sc, d.pre_sh, nullptr, hb, BNC, n, s)))
                return rc;
            if ((rc = launch_cam_context(hb, T2, n, d.cw1, d.cb1, d.cw2, d.cb2, mk, s))) return rc;
            if ((rc = tdnn_gemm(hb, BNC, T2, T2, BNC, 3, 1, dil, dil, d.wl, G, nullptr, 0, nullptr, nullptr, mk, cur + Cin, ld, n, s)))
                return rc;
        }
        ch += kLayers[blk] * G;
        const int out_ch = ch / 2;
        const int nld = blk < 2 ? out_ch + kLayers[blk + 1] * G : out_ch;
        const std::string p = "xvector.transit" + std::to_string(blk + 1) + ".";
        if ((rc = tdnn_gemm(cur, ld, T2, T2, ch, 1, 1, 1, 0, c->tt.get(p + "linear.weight"), out_ch, nullptr, 0, c->tt.get(p + "pre.sc"),
                            c->tt.get(p + "pre.sh"), nullptr, nxt, nld, n, s)))
            return rc;
        ch = out_ch;
        ld = nld;
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    return launch_cam_pool_dense(cur, T2, ch, n, c->tt.get("out.sc"), c->tt.get("out.sh"), c->tt.get("dense.wt"), c->cfg.embedding_size,
                                 c->tt.get("dense.sc"), c->tt.get("dense.sh"), emb, s);
}

int ready(Campplus* c) {
    if (c->tt.require_all("campplus")) return -3;
    if (c->folded_version != c->tt.version) return c->fold();
    return 0;
}

}  // namespace

extern "C" {

pf_campplus* pf_campplus_create(const pf_campplus_config* cfg) {
    if (!cfg) { set_error("campplus: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_campplus_config& c = *cfg;
    if (c.feat_dim != 80 || c.embedding_size <= 0 || c.embedding_size > 512 || c.growth_rate != 32 || c.bn_size != 4 ||
        c.init_channels != 128 || c.m_channels != 32 || !(c.bn_eps > 0.f)) {
        set_error("campplus: unsupported config (built: feat_dim 80, growth_rate 32, bn_size 4, init_channels 128, m_channels 32)");
        return nullptr;
    }
    std::unique_ptr<Campplus> h(new Campplus());
    h->cfg = c;
    const int mc = c.m_channels;
    int rc = 0;
    auto bn = [&](const std::string& p, int C, bool affine) {
        if (affine) rc |= h->tt.add_linear(p, C, 1);
        rc |= h->tt.add(p + "running_mean", C);
        rc |= h->tt.add(p + "running_var", C);
    };
    rc |= h->tt.add("head.conv1.weight", mc * 9);
    bn("head.bn1.", mc, true);
    for (int l = 1; l <= 2; ++l)
        for (int b = 0; b < 2; ++b) {
            const std::string p = "head.layer" + std::to_string(l) + "." + std::to_string(b) + ".";
            rc |= h->tt.add(p + "conv1.weight", mc * mc * 9);
            bn(p + "bn1.", mc, true);
            rc |= h->tt.add(p + "conv2.weight", mc * mc * 9);
            bn(p + "bn2.", mc, true);
            if (b == 0) {
                rc |= h->tt.add(p + "shortcut.0.weight", mc * mc);
                bn(p + "shortcut.1.", mc, true);
            }
        }
    rc |= h->tt.add("head.conv2.weight", mc * mc * 9);
    bn("head.bn2.", mc, true);
    rc |= h->tt.add("xvector.tdnn.linear.weight", (int64_t)c.init_channels * mc * (c.feat_dim / 8) * 5);
    bn("xvector.tdnn.nonlinear.batchnorm.", c.init_channels, true);
    const int G = c.growth_rate, BNC = c.bn_size * G;
    int ch = c.init_channels;
    for (int blk = 0; blk < 3; ++blk) {
        for (int i = 0; i < kLayers[blk]; ++i) {
            const std::string p = "xvector.block" + std::to_string(blk + 1) + ".tdnnd" + std::to_string(i + 1) + ".";
            const int Cin = ch + i * G;
            bn(p + "nonlinear1.batchnorm.", Cin, true);
            rc |= h->tt.add(p + "linear1.weight", (int64_t)BNC * Cin);
            bn(p + "nonlinear2.batchnorm.", BNC, true);
            rc |= h->tt.add(p + "cam_layer.linear_local.weight", G * BNC * 3);
            rc |= h->tt.add_linear(p + "cam_layer.linear1.", BNC / 2, BNC);
            rc |= h->tt.add_linear(p + "cam_layer.linear2.", G, BNC / 2);
        }
        ch += kLayers[blk] * G;
        const std::string p = "xvector.transit" + std::to_string(blk + 1) + ".";
        bn(p + "nonlinear.batchnorm.", ch, true);
        rc |= h->tt.add(p + "linear.weight", (int64_t)(ch / 2) * ch);
        ch /= 2;
    }
    bn("xvector.out_nonlinear.batchnorm.", ch, true);
    rc |= h->tt.add("xvector.dense.linear.weight", (int64_t)c.embedding_size * 2 * ch);
    bn("xvector.dense.nonlinear.batchnorm.", c.embedding_size, false);
    if (rc) return nullptr;
    // the kaldi fbank of extract_feature (campplus/utils.py:119-137): 25 / 10 ms, 80 bins, povey window, no 2^15 scaling, no LFR
    pf_frontend_config fc{16000, 400, 160, c.feat_dim, 1, 1, 20.f, 0.f, 0.97f, 1.f};
    h->fe = pf_frontend_create(&fc);
    if (!h->fe || pf_frontend_set_window(h->fe, "povey", 0.42f)) return nullptr;
    return reinterpret_cast<pf_campplus*>(h.release());
}
void pf_campplus_destroy(pf_campplus* h) { delete reinterpret_cast<Campplus*>(h); }
int pf_campplus_set_tensor(pf_campplus* hh, const char* name, const float* data, int64_t numel) {
    Campplus* h = reinterpret_cast<Campplus*>(hh);
    PF_REQUIRE(h && name && data, "campplus_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_campplus_missing(const pf_campplus* hh) {
    const Campplus* h = reinterpret_cast<const Campplus*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_campplus_set_max_batch(pf_campplus* hh, int32_t max_chunks) {
    Campplus* h = reinterpret_cast<Campplus*>(hh);
    PF_REQUIRE(h && max_chunks > 0, "campplus_set_max_batch: null handle or non-positive size");
    h->max_batch = max_chunks;
    return 0;
}
int pf_campplus_forward(pf_campplus* hh, const float* feats, int32_t B, int32_t T, float* emb, void* stream) {
    Campplus* h = reinterpret_cast<Campplus*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && feats && emb && B > 0, "campplus_forward: null/empty argument");
    PF_REQUIRE(T >= 3, "campplus_forward: fewer than 2 frames after the stride-2 TDNN (T >= 3 needed)");
    int rc;
    if ((rc = ready(h))) return rc;
    const int D = h->cfg.feat_dim, E = h->cfg.embedding_size;
    for (int b0 = 0; b0 < B; b0 += h->max_batch) {
        const int n = B - b0 < h->max_batch ? B - b0 : h->max_batch;
        if ((rc = run_net(h, feats + (size_t)b0 * T * D, n, T, emb + (size_t)b0 * E, s))) return rc;
    }
    return 0;
}
int pf_campplus_embed_chunks(pf_campplus* hh, const float* wav, int64_t n_samples, const int64_t* starts_host,
                             const int32_t* valid_host, int32_t N, int32_t chunk_len, float* emb, void* stream) {
    Campplus* h = reinterpret_cast<Campplus*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && wav && starts_host && emb && N > 0 && n_samples > 0, "campplus_embed_chunks: null/empty argument");
    const int T = pf_frontend_num_fbank_frames(h->fe, chunk_len);
    PF_REQUIRE(chunk_len > 0 && T >= 3, "campplus_embed_chunks: chunk shorter than 3 fbank frames");
    int rc;
    if ((rc = ready(h))) return rc;
    const int D = h->cfg.feat_dim, E = h->cfg.embedding_size;
    const int nb_max = h->max_batch < 65535 ? h->max_batch : 65535;
    std::vector<int32_t> ns((size_t)nb_max, chunk_len), fl((size_t)nb_max);
    for (int b0 = 0; b0 < N; b0 += nb_max) {
        const int n = N - b0 < nb_max ? N - b0 : nb_max;
        if (h->wav.ensure(sizeof(float) * (size_t)n * chunk_len) || h->feats.ensure(sizeof(float) * (size_t)n * T * D) ||
            h->starts.ensure(sizeof(int64_t) * n) || (valid_host && h->valid.ensure(sizeof(int32_t) * n)))
            return -2;
        if (upload_h2d(h->starts.p, starts_host + b0, sizeof(int64_t) * n, s)) return -2;
        if (valid_host && upload_h2d(h->valid.p, valid_host + b0, sizeof(int32_t) * n, s)) return -2;
        if ((rc = launch_cam_gather_chunks(wav, n_samples, h->starts.as<int64_t>(), valid_host ? h->valid.as<int>() : nullptr, n,
                                           chunk_len, h->wav.as<float>(), s)))
            return rc;
        if ((rc = pf_frontend_forward(h->fe, h->wav.as<float>(), chunk_len, ns.data(), n, h->feats.as<float>(), T, fl.data(), nullptr,
                                      stream)))
            return rc;
        if ((rc = launch_cam_sub_mean(h->feats.as<float>(), n, T, D, s))) return rc;
        if ((rc = run_net(h, h->feats.as<float>(), n, T, emb + (size_t)b0 * E, s))) return rc;
    }
    return 0;
}

}  // extern "C"
