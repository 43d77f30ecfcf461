// C-ABI layer, ERes2NetV2 speaker embedding: pf_eres2net_* and the pf_k_eres_conv hook (kernels in eres2net.hip).
//
// Load time: the reference's tensors are kept as set; at the first forward after a change every BatchNorm is folded into the conv
// in front of it (float64 on the host; a conv's own bias, as in AFF, goes through the BatchNorm into the folded bias), conv weights
// [O, I, kh, kw] are repacked tap-major / channel-minor with I padded to a multiple of 4 (zero columns), the projection shortcut's
// 1x1 conv is appended to conv3's K, and seg_1's columns are permuted from the reference's (c, f) order to the layout's (f, c).
// Where a conv writes a channel count that is no multiple of 4 into a buffer a later conv reads as ONE operand (the two halves
// `spx` of conv1, the concat buffer of convs[0] / convs[1]), its weight has zero ROWS for the pad channels, so the pads hold zeros.
//
// One forward, per sub-batch of n chunks (workspace bounded by max_batch), w = floor(26 planes / 64), wp = pad4(w):
//   stem  [n T F] -> 3x3, ReLU -> [n T F, mc]
//   block conv1 1x1 (stride s) -> H [.., 2 wp] = spx[0] | spx[1]; convs[0] 3x3 on spx[0] -> G[:, 0:wp];
//         plain: convs[1] 3x3 on (G[:, 0:wp] + spx[1], summed by the loader) -> G[:, wp:2wp]
//         AFF:   1x1 over cat(G[:, 0:wp], spx[1]) (K-concatenated), SiLU -> Q; 1x1 on Q with the AFF combine -> Z; convs[1] on Z
//         conv3 1x1 on G (+ the projection shortcut on K, or + the identity shortcut in the epilogue), clamp(0, 20)
//   layer3_ds 3x3 stride 2 on out3; fuse34 = AFF(out4, ds); TSTP pool -> stats [n, 2 S]; seg_1 in K slices of 1024 (each slice a
//   chain of its own, the running sum rides in as the addend of the next launch)
#include <algorithm>

#include "engine_internal.h"
#include "campplus.h"
#include "eres2net.h"

using namespace pf;

namespace {

struct EresBlk {
    int layer, in, w, wp, inter, interp, O, stride;
    bool aff, proj;
    const float *c1w, *c1b, *cv0w, *cv0b, *cv1w, *cv1b, *a0w, *a0b, *a1w, *a1b, *c3w, *c3b;
};

struct Eres2net {
    pf_eres2net_config cfg;
    TensorTable tt;
    pf_frontend* fe = nullptr;
    int max_batch = 256;
    unsigned long long folded_version = TensorTable::NOT_PREPARED;
    std::vector<EresBlk> blocks;
    DevBuf xa, xb, x3, h, g, z, q, ds, q34, fu, stats, seg, wav, feats, starts, valid;
    ~Eres2net() { if (fe) pf_frontend_destroy(fe); }

    int fold();
};

#define ERES_CHECK(cond)                                                              \
    do {                                                                              \
        if (!(cond)) { set_error("eres2net: weight folding failed (HIP copy)"); return -2; } \
    } while (0)

std::string blk_name(int layer, int b) { return "model.layer" + std::to_string(layer) + "." + std::to_string(b) + "."; }

// the blocks of the network in order, shapes only
std::vector<EresBlk> block_table(const pf_eres2net_config& c) {
    std::vector<EresBlk> v;
    int in = c.m_channels;
    for (int l = 1; l <= 4; ++l) {
        const int planes = c.m_channels << (l - 1);
        for (int b = 0; b < c.num_blocks[l - 1]; ++b) {
            EresBlk k{};
            k.layer = l; k.in = in; k.w = planes * 26 / 64; k.wp = eres_pad4(k.w); k.O = 2 * planes;
            k.stride = (b == 0 && l > 1) ? 2 : 1;
            k.aff = l >= 3; k.inter = k.w / 4; k.interp = eres_pad4(k.inter);
            k.proj = k.stride != 1 || k.in != k.O;
            v.push_back(k);
            in = k.O;
        }
    }
    return v;
}

// AFF(channels C stored with stride Cp per half, inner width I): local_att.0 (+ .1) -> [I, 2 Cp], local_att.3 (+ .4) -> [C, pad4(I)]
int fold_aff(Eres2net* e, const std::string& rp, const std::string& key, int C, int Cp, int I) {
    const double eps = (double)e->cfg.bn_eps;
    const int Ip = eres_pad4(I);
    std::vector<float> w0 = e->tt.host(rp + "0.weight"), b0 = e->tt.host(rp + "0.bias"), w1 = e->tt.host(rp + "3.weight"),
                       b1 = e->tt.host(rp + "3.bias");
    std::vector<double> s0, t0, s1, t1;
    ERES_CHECK(!w0.empty() && !b0.empty() && !w1.empty() && !b1.empty() && e->tt.bn_fold(rp + "1.", true, eps, s0, t0) &&
               e->tt.bn_fold(rp + "4.", true, eps, s1, t1));
    std::vector<float> p0((size_t)I * 2 * Cp, 0.f), q0(I), p1((size_t)C * Ip, 0.f), q1(C);
    for (int o = 0; o < I; ++o) {
        for (int hf = 0; hf < 2; ++hf)
            for (int c = 0; c < C; ++c) p0[(size_t)o * 2 * Cp + hf * Cp + c] = (float)(w0[(size_t)o * 2 * C + hf * C + c] * s0[o]);
        q0[o] = (float)(b0[o] * s0[o] + t0[o]);
    }
    for (int o = 0; o < C; ++o) {
        for (int c = 0; c < I; ++c) p1[(size_t)o * Ip + c] = (float)(w1[(size_t)o * I + c] * s1[o]);
        q1[o] = (float)(b1[o] * s1[o] + t1[o]);
    }
    ERES_CHECK(!e->tt.put_derived(key + "a0.w", p0) && !e->tt.put_derived(key + "a0.b", q0) && !e->tt.put_derived(key + "a1.w", p1) &&
               !e->tt.put_derived(key + "a1.b", q1));
    return 0;
}

int Eres2net::fold() {
    const int mc = cfg.m_channels;
    const double eps = (double)cfg.bn_eps;
    int rc;
    {   // stem [mc, 1, 3, 3] -> [mc, 9]
        std::vector<float> w = tt.host("model.conv1.weight"), b(mc);
        std::vector<double> s, t;
        ERES_CHECK(!w.empty() && tt.bn_fold("model.bn1.", true, eps, s, t));
        for (int o = 0; o < mc; ++o) {
            for (int k = 0; k < 9; ++k) w[(size_t)o * 9 + k] = (float)(w[(size_t)o * 9 + k] * s[o]);
            b[o] = (float)t[o];
        }
        ERES_CHECK(!tt.put_derived("d.stem.w", w) && !tt.put_derived("d.stem.b", b));
    }
    blocks = block_table(cfg);
    std::vector<int> seen(5, 0);
    for (EresBlk& k : blocks) {
        const std::string rp = blk_name(k.layer, seen[k.layer]), key = "d." + rp;
        ++seen[k.layer];
        const int w = k.w, wp = k.wp, in = k.in, O = k.O;
        {   // conv1 [2 w, in] -> [2 wp, in], the halves at rows 0 and wp
            std::vector<float> src = tt.host(rp + "conv1.weight"), dst((size_t)2 * wp * in, 0.f), b(2 * wp, 0.f);
            std::vector<double> s, t;
            ERES_CHECK(!src.empty() && tt.bn_fold(rp + "bn1.", true, eps, s, t));
            for (int hf = 0; hf < 2; ++hf)
                for (int j = 0; j < w; ++j) {
                    for (int i = 0; i < in; ++i) dst[(size_t)(hf * wp + j) * in + i] = (float)(src[(size_t)(hf * w + j) * in + i] * s[hf * w + j]);
                    b[hf * wp + j] = (float)t[hf * w + j];
                }
            ERES_CHECK(!tt.put_derived(key + "c1.w", dst) && !tt.put_derived(key + "c1.b", b));
        }
        for (int i = 0; i < 2; ++i) {   // convs[i] [w, w, 3, 3] -> [wp, 9 wp] tap-major
            const std::string ci = std::to_string(i);
            std::vector<float> src = tt.host(rp + "convs." + ci + ".weight"), dst((size_t)wp * 9 * wp, 0.f), b(wp, 0.f);
            std::vector<double> s, t;
            ERES_CHECK(!src.empty() && tt.bn_fold(rp + "bns." + ci + ".", true, eps, s, t));
            for (int o = 0; o < w; ++o) {
                for (int c = 0; c < w; ++c)
                    for (int tap = 0; tap < 9; ++tap) dst[(size_t)o * 9 * wp + tap * wp + c] = (float)(src[((size_t)o * w + c) * 9 + tap] * s[o]);
                b[o] = (float)t[o];
            }
            ERES_CHECK(!tt.put_derived(key + "cv" + ci + ".w", dst) && !tt.put_derived(key + "cv" + ci + ".b", b));
        }
        if (k.aff && (rc = fold_aff(this, rp + "fuse_models.0.local_att.", key, w, wp, k.inter))) return rc;
        {   // conv3 [O, 2 w] (+ shortcut [O, in]) -> [O, 2 wp (+ in)]
            const int K = 2 * wp + (k.proj ? in : 0);
            std::vector<float> src = tt.host(rp + "conv3.weight"), dst((size_t)O * K, 0.f), b(O), ws;
            std::vector<double> s, t, s2, t2;
            ERES_CHECK(!src.empty() && tt.bn_fold(rp + "bn3.", true, eps, s, t));
            if (k.proj) { ws = tt.host(rp + "shortcut.0.weight"); ERES_CHECK(!ws.empty() && tt.bn_fold(rp + "shortcut.1.", true, eps, s2, t2)); }
            for (int o = 0; o < O; ++o) {
                for (int hf = 0; hf < 2; ++hf)
                    for (int c = 0; c < w; ++c) dst[(size_t)o * K + hf * wp + c] = (float)(src[(size_t)o * 2 * w + hf * w + c] * s[o]);
                for (int i = 0; k.proj && i < in; ++i) dst[(size_t)o * K + 2 * wp + i] = (float)(ws[(size_t)o * in + i] * s2[o]);
                b[o] = (float)(t[o] + (k.proj ? t2[o] : 0.0));
            }
            ERES_CHECK(!tt.put_derived(key + "c3.w", dst) && !tt.put_derived(key + "c3.b", b));
        }
        k.c1w = tt.get(key + "c1.w"); k.c1b = tt.get(key + "c1.b");
        k.cv0w = tt.get(key + "cv0.w"); k.cv0b = tt.get(key + "cv0.b");
        k.cv1w = tt.get(key + "cv1.w"); k.cv1b = tt.get(key + "cv1.b");
        k.c3w = tt.get(key + "c3.w"); k.c3b = tt.get(key + "c3.b");
        if (k.aff) { k.a0w = tt.get(key + "a0.w"); k.a0b = tt.get(key + "a0.b"); k.a1w = tt.get(key + "a1.w"); k.a1b = tt.get(key + "a1.b"); }
    }
    {   // layer3_ds [16 mc, 8 mc, 3, 3] -> tap-major (no BatchNorm, no bias)
        const int O = 16 * mc, I = 8 * mc;
        std::vector<float> src = tt.host("model.layer3_ds.weight"), dst((size_t)O * 9 * I);
        ERES_CHECK(!src.empty());
        for (int o = 0; o < O; ++o)
            for (int c = 0; c < I; ++c)
                for (int tap = 0; tap < 9; ++tap) dst[(size_t)o * 9 * I + tap * I + c] = src[((size_t)o * I + c) * 9 + tap];
        ERES_CHECK(!tt.put_derived("d.ds.w", dst));
    }
    if ((rc = fold_aff(this, "model.fuse34.local_att.", "d.fuse34.", 16 * mc, 16 * mc, 4 * mc))) return rc;
    {   // seg_1 [E, 2 S]: column c * F4 + f of each half -> f * C + c
        const int C = 16 * mc, F4 = cfg.feat_dim / 8, S = C * F4, E = cfg.embedding_size;
        std::vector<float> src = tt.host("model.seg_1.weight"), dst((size_t)E * 2 * S);
        ERES_CHECK(!src.empty());
        for (int o = 0; o < E; ++o)
            for (int hf = 0; hf < 2; ++hf)
                for (int c = 0; c < C; ++c)
                    for (int f = 0; f < F4; ++f) dst[(size_t)o * 2 * S + hf * S + f * C + c] = src[(size_t)o * 2 * S + hf * S + c * F4 + f];
        ERES_CHECK(!tt.put_derived("d.seg.w", dst));
    }
    folded_version = tt.version;
    return 0;
}

// a conv over n chunks of [Tin, Fin] positions -> [To, Fo]; the caller fills operands and epilogue
EresConvArgs conv_args(int n, int Tin, int Fin, int stride, int taps) {
    EresConvArgs a{};
    a.taps = taps; a.st = a.sf = stride;
    a.Tin = Tin; a.Fin = Fin; a.To = (Tin - 1) / stride + 1; a.Fo = (Fin - 1) / stride + 1;
    a.M = n * a.To * a.Fo;
    return a;
}

constexpr int SEG_SLICE = 1024;

// floats of every workspace buffer of run_net for n chunks of T frames: the largest of each kind over the layers
struct EresSizes {
    size_t io, hg, zz, qq, x3, c4, q34, stats, seg;
    int T3, F3, T4, F4;
    size_t total() const { return 2 * io + 2 * hg + zz + qq + x3 + 2 * c4 + q34 + stats + seg; }
};
EresSizes eres_sizes(const pf_eres2net_config& c, int n, int T) {
    const int mc = c.m_channels;
    EresSizes z{};
    z.io = (size_t)n * T * c.feat_dim * mc; z.zz = z.qq = 4;
    int Tl = T, Fl = c.feat_dim;
    for (const EresBlk& k : block_table(c)) {
        if (k.stride == 2) { Tl = (Tl - 1) / 2 + 1; Fl = (Fl - 1) / 2 + 1; }
        const size_t pos = (size_t)n * Tl * Fl;
        z.io = std::max(z.io, pos * k.O);
        z.hg = std::max(z.hg, pos * 2 * k.wp);
        if (k.aff) { z.zz = std::max(z.zz, pos * k.wp); z.qq = std::max(z.qq, pos * k.interp); }
        if (k.layer == 3) { z.T3 = Tl; z.F3 = Fl; }
    }
    z.T4 = Tl; z.F4 = Fl;
    z.x3 = (size_t)n * z.T3 * z.F3 * 8 * mc;
    z.c4 = (size_t)n * z.T4 * z.F4 * 16 * mc;
    z.q34 = (size_t)n * z.T4 * z.F4 * 4 * mc;
    z.stats = (size_t)n * 2 * z.F4 * 16 * mc;
    z.seg = (size_t)n * c.embedding_size;
    return z;
}

// the network on n chunks of T frames: feats [n, T, F] -> emb [n, E]
// `taps` (tests; nullable, and each entry nullable): device buffers that receive a copy of the stem, layer1 .. layer4, layer3_ds,
// fuse34 (channels-last [n, t, f, c]) and the pooled stats [n, 2 S] as they are computed
enum { TAP_STEM = 0, TAP_LAYER1 = 1, TAP_DS = 5, TAP_FUSE = 6, TAP_STATS = 7, TAP_COUNT = 8 };
int run_net(Eres2net* e, const float* feats, int n, int T, float* emb, hipStream_t s, float* const* taps = nullptr) {
    auto tap = [&](int which, const float* src, size_t floats) -> int {
        if (taps && taps[which]) PF_HIP_TRY(hipMemcpyAsync(taps[which], src, sizeof(float) * floats, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    const pf_eres2net_config& c = e->cfg;
    const int mc = c.m_channels, F0 = c.feat_dim, E = c.embedding_size;
    const EresSizes z = eres_sizes(c, n, T);
    const int T3 = z.T3, F3 = z.F3, T4 = z.T4, F4 = z.F4;
    const int C3 = 8 * mc, C4 = 16 * mc, S = F4 * C4;
    if (e->xa.ensure(sizeof(float) * z.io) || e->xb.ensure(sizeof(float) * z.io) || e->h.ensure(sizeof(float) * z.hg) ||
        e->g.ensure(sizeof(float) * z.hg) || e->z.ensure(sizeof(float) * z.zz) || e->q.ensure(sizeof(float) * z.qq) ||
        e->x3.ensure(sizeof(float) * z.x3) || e->ds.ensure(sizeof(float) * z.c4) || e->q34.ensure(sizeof(float) * z.q34) ||
        e->fu.ensure(sizeof(float) * z.c4) || e->stats.ensure(sizeof(float) * z.stats) || e->seg.ensure(sizeof(float) * z.seg))
        return -2;
    float* const XA = e->xa.as<float>();
    float* const XB = e->xb.as<float>();
    float* cur = XA;
    float *H = e->h.as<float>(), *G = e->g.as<float>(), *Z = e->z.as<float>(), *Q = e->q.as<float>();
    int rc;
    if ((rc = launch_eres_stem(feats, n, T, F0, e->tt.get("d.stem.w"), e->tt.get("d.stem.b"), mc, cur, s))) return rc;
    if ((rc = tap(TAP_STEM, cur, (size_t)n * T * F0 * mc))) return rc;
    int Tl = T, Fl = F0;
    for (size_t bi = 0; bi < e->blocks.size(); ++bi) {
        const EresBlk& k = e->blocks[bi];
        const int Tin = Tl, Fin = Fl, wp = k.wp;
        if (k.stride == 2) { Tl = (Tl - 1) / 2 + 1; Fl = (Fl - 1) / 2 + 1; }
        // the last block of layer 3 writes out3, which layer3_ds reads after layer 4 has run
        const bool last3 = k.layer == 3 && (bi + 1 == e->blocks.size() || e->blocks[bi + 1].layer == 4);
        float* out = last3 ? e->x3.as<float>() : (cur == XA ? XB : XA);
        {   // conv1: cur [Tin, Fin, in] -> H [Tl, Fl, 2 wp]
            EresConvArgs a = conv_args(n, Tin, Fin, k.stride, 1);
            a.A = cur; a.lda = k.in; a.Cin = k.in;
            a.W = k.c1w; a.ldw = k.in; a.bias = k.c1b; a.act = ERES_ACT_CLAMP20;
            a.N = 2 * wp; a.C = H; a.ldc = 2 * wp;
            if ((rc = launch_eres_conv(a, s))) return rc;
        }
        {   // convs[0]: spx[0] = H[:, 0:wp] -> G[:, 0:wp]
            EresConvArgs a = conv_args(n, Tl, Fl, 1, 9);
            a.A = H; a.lda = 2 * wp; a.Cin = k.w;
            a.W = k.cv0w; a.ldw = 9 * wp; a.bias = k.cv0b; a.act = ERES_ACT_CLAMP20;
            a.N = wp; a.C = G; a.ldc = 2 * wp;
            if ((rc = launch_eres_conv(a, s))) return rc;
        }
        {   // convs[1] on sp + spx[1] (plain) or on AFF(sp, spx[1]) -> G[:, wp:2wp]
            EresConvArgs a = conv_args(n, Tl, Fl, 1, 9);
            if (!k.aff) {
                a.A = G; a.lda = 2 * wp; a.Cin = k.w;
                a.a2_mode = ERES_A2_SUM; a.A2 = H + wp; a.lda2 = 2 * wp;
            } else {
                EresConvArgs f = conv_args(n, Tl, Fl, 1, 1);
                f.A = G; f.lda = 2 * wp; f.Cin = k.w;
                f.a2_mode = ERES_A2_CONCAT; f.A2 = H + wp; f.lda2 = 2 * wp; f.Cin2 = k.w; f.Tin2 = Tl; f.Fin2 = Fl; f.st2 = f.sf2 = 1;
                f.W = k.a0w; f.ldw = 2 * wp; f.bias = k.a0b; f.act = ERES_ACT_SILU;
                f.N = k.inter; f.C = Q; f.ldc = k.interp;
                if ((rc = launch_eres_conv(f, s))) return rc;
                EresConvArgs h2 = conv_args(n, Tl, Fl, 1, 1);
                h2.A = Q; h2.lda = k.interp; h2.Cin = k.inter;
                h2.W = k.a1w; h2.ldw = k.interp; h2.bias = k.a1b;
                h2.X = G; h2.ldx = 2 * wp; h2.Y = H + wp; h2.ldy = 2 * wp;
                h2.N = k.w; h2.C = Z; h2.ldc = wp;
                if ((rc = launch_eres_conv(h2, s))) return rc;
                a.A = Z; a.lda = wp; a.Cin = k.w;
            }
            a.W = k.cv1w; a.ldw = 9 * wp; a.bias = k.cv1b; a.act = ERES_ACT_CLAMP20;
            a.N = wp; a.C = G + wp; a.ldc = 2 * wp;
            if ((rc = launch_eres_conv(a, s))) return rc;
        }
        {   // conv3 on G (the pad channels hold zeros and meet zero weights) + shortcut
            EresConvArgs a = conv_args(n, Tl, Fl, 1, 1);
            a.A = G; a.lda = 2 * wp; a.Cin = 2 * wp;
            a.W = k.c3w; a.bias = k.c3b; a.act = ERES_ACT_CLAMP20;
            if (k.proj) {
                a.a2_mode = ERES_A2_CONCAT; a.A2 = cur; a.lda2 = k.in; a.Cin2 = k.in; a.Tin2 = Tin; a.Fin2 = Fin; a.st2 = a.sf2 = k.stride;
            } else {
                a.R = cur; a.ldr = k.O;
            }
            a.ldw = eres_conv_k(a);
            a.N = k.O; a.C = out; a.ldc = k.O;
            if ((rc = launch_eres_conv(a, s))) return rc;
        }
        cur = out;
        if ((bi + 1 == e->blocks.size() || e->blocks[bi + 1].layer != k.layer) &&
            (rc = tap(TAP_LAYER1 + k.layer - 1, cur, (size_t)n * Tl * Fl * k.O)))
            return rc;
    }
    // cur = out4 [n T4 F4, C4]; out3 in x3
    float* out3 = e->x3.as<float>();
    float* out4 = cur;
    float *DS = e->ds.as<float>(), *Q34 = e->q34.as<float>(), *FU = e->fu.as<float>();
    {
        EresConvArgs a = conv_args(n, T3, F3, 2, 9);
        a.A = out3; a.lda = C3; a.Cin = C3; a.W = e->tt.get("d.ds.w"); a.ldw = 9 * C3;
        a.N = C4; a.C = DS; a.ldc = C4;
        if (a.To != T4 || a.Fo != F4) { set_error("eres2net: internal shape mismatch"); return -2; }
        if ((rc = launch_eres_conv(a, s))) return rc;
        if ((rc = tap(TAP_DS, DS, z.c4))) return rc;
    }
    {
        EresConvArgs f = conv_args(n, T4, F4, 1, 1);
        f.A = out4; f.lda = C4; f.Cin = C4;
        f.a2_mode = ERES_A2_CONCAT; f.A2 = DS; f.lda2 = C4; f.Cin2 = C4; f.Tin2 = T4; f.Fin2 = F4; f.st2 = f.sf2 = 1;
        f.W = e->tt.get("d.fuse34.a0.w"); f.ldw = 2 * C4; f.bias = e->tt.get("d.fuse34.a0.b"); f.act = ERES_ACT_SILU;
        f.N = 4 * mc; f.C = Q34; f.ldc = 4 * mc;
        if ((rc = launch_eres_conv(f, s))) return rc;
        EresConvArgs h2 = conv_args(n, T4, F4, 1, 1);
        h2.A = Q34; h2.lda = 4 * mc; h2.Cin = 4 * mc;
        h2.W = e->tt.get("d.fuse34.a1.w"); h2.ldw = 4 * mc; h2.bias = e->tt.get("d.fuse34.a1.b");
        h2.X = out4; h2.ldx = C4; h2.Y = DS; h2.ldy = C4;
        h2.N = C4; h2.C = FU; h2.ldc = C4;
        if ((rc = launch_eres_conv(h2, s))) return rc;
        if ((rc = tap(TAP_FUSE, FU, z.c4))) return rc;
    }
    float* ST = e->stats.as<float>();
    if ((rc = launch_eres_pool(FU, n, T4, S, ST, s))) return rc;
    if ((rc = tap(TAP_STATS, ST, z.stats))) return rc;
    // seg_1: slices of K, the last one writes emb
    const int K = 2 * S, ns = ceil_div(K, SEG_SLICE);
    for (int i = 0; i < ns; ++i) {
        const int k0 = i * SEG_SLICE;
        const bool to_emb = (ns - 1 - i) % 2 == 0;
        EresConvArgs a = conv_args(n, 1, 1, 1, 1);
        a.A = ST + k0; a.lda = K; a.Cin = std::min(SEG_SLICE, K - k0);
        a.W = e->tt.get("d.seg.w") + k0; a.ldw = K;
        a.bias = i == 0 ? e->tt.get("model.seg_1.bias") : nullptr;
        if (i > 0) { a.R = to_emb ? e->seg.as<float>() : emb; a.ldr = E; }
        a.N = E; a.C = to_emb ? emb : e->seg.as<float>(); a.ldc = E;
        if ((rc = launch_eres_conv(a, s))) return rc;
    }
    return 0;
}

int ready(Eres2net* e) {
    if (e->tt.require_all("eres2net")) return -3;
    if (e->folded_version != e->tt.version) return e->fold();
    return 0;
}

// frames left after the three stride-2 stages
int frames_out(int T) {
    for (int i = 0; i < 3; ++i) T = (T - 1) / 2 + 1;
    return T;
}

}  // namespace

extern "C" {

pf_eres2net* pf_eres2net_create(const pf_eres2net_config* cfg) {
    if (!cfg) { set_error("eres2net: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_eres2net_config& c = *cfg;
    if (c.feat_dim < 8 || c.feat_dim > 128 || c.feat_dim % 8 != 0 || c.m_channels < 8 || c.m_channels > 64 || c.m_channels % 8 != 0 ||
        c.embedding_size < 1 || c.num_blocks[0] < 1 || c.num_blocks[1] < 1 || c.num_blocks[2] < 1 || c.num_blocks[3] < 1 || !(c.bn_eps > 0.f)) {
        set_error("eres2net: unsupported config (built: feat_dim 8 .. 128 and m_channels 8 .. 64 in multiples of 8, positive num_blocks, "
                  "embedding_size >= 1)");
        return nullptr;
    }
    std::unique_ptr<Eres2net> h(new Eres2net());
    h->cfg = c;
    const int mc = c.m_channels;
    int rc = 0;
    auto bn = [&](const std::string& p, int C) {
        rc |= h->tt.add_linear(p, C, 1);
        rc |= h->tt.add(p + "running_mean", C);
        rc |= h->tt.add(p + "running_var", C);
    };
    auto aff = [&](const std::string& p, int C, int I) {
        rc |= h->tt.add_linear(p + "0.", I, 2 * C);
        bn(p + "1.", I);
        rc |= h->tt.add_linear(p + "3.", C, I);
        bn(p + "4.", C);
    };
    rc |= h->tt.add("model.conv1.weight", mc * 9);
    bn("model.bn1.", mc);
    std::vector<int> seen(5, 0);
    for (const EresBlk& k : block_table(c)) {
        const std::string p = blk_name(k.layer, seen[k.layer]++);
        rc |= h->tt.add(p + "conv1.weight", (int64_t)2 * k.w * k.in);
        bn(p + "bn1.", 2 * k.w);
        for (int i = 0; i < 2; ++i) {
            rc |= h->tt.add(p + "convs." + std::to_string(i) + ".weight", (int64_t)k.w * k.w * 9);
            bn(p + "bns." + std::to_string(i) + ".", k.w);
        }
        if (k.aff) aff(p + "fuse_models.0.local_att.", k.w, k.inter);
        rc |= h->tt.add(p + "conv3.weight", (int64_t)k.O * 2 * k.w);
        bn(p + "bn3.", k.O);
        if (k.proj) {
            rc |= h->tt.add(p + "shortcut.0.weight", (int64_t)k.O * k.in);
            bn(p + "shortcut.1.", k.O);
        }
    }
    rc |= h->tt.add("model.layer3_ds.weight", (int64_t)16 * mc * 8 * mc * 9);
    aff("model.fuse34.local_att.", 16 * mc, 4 * mc);
    rc |= h->tt.add_linear("model.seg_1.", c.embedding_size, (int64_t)2 * (c.feat_dim / 8) * 16 * mc);
    if (rc) return nullptr;
    // the kaldi fbank of extract_feature (campplus/utils.py:119-137): 25 / 10 ms, povey window, no 2^15 scaling, no LFR
    pf_frontend_config fc{16000, 400, 160, c.feat_dim, 1, 1, 20.f, 0.f, 0.97f, 1.f};
    h->fe = pf_frontend_create(&fc);
    if (!h->fe || pf_frontend_set_window(h->fe, "povey", 0.42f)) return nullptr;
    return reinterpret_cast<pf_eres2net*>(h.release());
}
void pf_eres2net_destroy(pf_eres2net* h) { delete reinterpret_cast<Eres2net*>(h); }
int pf_eres2net_set_tensor(pf_eres2net* hh, const char* name, const float* data, int64_t numel) {
    Eres2net* h = reinterpret_cast<Eres2net*>(hh);
    PF_REQUIRE(h && name && data, "eres2net_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_eres2net_missing(const pf_eres2net* hh) {
    const Eres2net* h = reinterpret_cast<const Eres2net*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_eres2net_set_max_batch(pf_eres2net* hh, int32_t max_chunks) {
    Eres2net* h = reinterpret_cast<Eres2net*>(hh);
    PF_REQUIRE(h && max_chunks > 0, "eres2net_set_max_batch: null handle or non-positive size");
    h->max_batch = max_chunks;
    return 0;
}
int64_t pf_eres2net_workspace_bytes(const pf_eres2net* hh, int32_t T) {
    const Eres2net* h = reinterpret_cast<const Eres2net*>(hh);
    if (!h || T < 1) return -1;
    return (int64_t)(sizeof(float) * eres_sizes(h->cfg, 1, T).total());
}
int pf_eres2net_debug_poison(pf_eres2net* hh) {
    Eres2net* h = reinterpret_cast<Eres2net*>(hh);
    PF_REQUIRE(h, "eres2net_debug_poison: null handle");
    PF_HIP_TRY(hipDeviceSynchronize());
    for (DevBuf* b : {&h->xa, &h->xb, &h->x3, &h->h, &h->g, &h->z, &h->q, &h->ds, &h->q34, &h->fu, &h->stats, &h->seg, &h->wav, &h->feats})
        if (b->p) PF_HIP_TRY(hipMemset(b->p, 0xff, b->cap));
    return 0;
}
int pf_eres2net_forward(pf_eres2net* hh, const float* feats, int32_t B, int32_t T, float* emb, void* stream) {
    Eres2net* h = reinterpret_cast<Eres2net*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && feats && emb && B > 0, "eres2net_forward: null/empty argument");
    PF_REQUIRE(T >= 9 && frames_out(T) >= 2, "eres2net_forward: fewer than 2 frames after the three stride-2 stages (T >= 9 needed)");
    int rc;
    if ((rc = ready(h))) return rc;
    const int D = h->cfg.feat_dim, E = h->cfg.embedding_size;
    const int nb_max = h->max_batch < 65535 ? h->max_batch : 65535;
    for (int b0 = 0; b0 < B; b0 += nb_max) {
        const int n = B - b0 < nb_max ? B - b0 : nb_max;
        if ((rc = run_net(h, feats + (size_t)b0 * T * D, n, T, emb + (size_t)b0 * E, s))) return rc;
    }
    return 0;
}
int pf_eres2net_forward_stages(pf_eres2net* hh, const float* feats, int32_t B, int32_t T, float* emb, float* const* stages_dev,
                               void* stream) {
    Eres2net* h = reinterpret_cast<Eres2net*>(hh);
    PF_REQUIRE(h && feats && emb && stages_dev && B > 0 && B <= h->max_batch && B <= 65535,
               "eres2net_forward_stages: null/empty argument, or more chunks than one sub-batch");
    PF_REQUIRE(T >= 9 && frames_out(T) >= 2, "eres2net_forward_stages: fewer than 2 frames after the three stride-2 stages (T >= 9 needed)");
    int rc;
    if ((rc = ready(h))) return rc;
    return run_net(h, feats, B, T, emb, reinterpret_cast<hipStream_t>(stream), stages_dev);
}
int pf_eres2net_embed_chunks(pf_eres2net* hh, const float* wav, int64_t n_samples, const int64_t* starts_host,
                             const int32_t* valid_host, int32_t N, int32_t chunk_len, float* emb, void* stream) {
    Eres2net* h = reinterpret_cast<Eres2net*>(hh);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && wav && starts_host && emb && N > 0 && n_samples > 0, "eres2net_embed_chunks: null/empty argument");
    const int T = chunk_len > 0 ? pf_frontend_num_fbank_frames(h->fe, chunk_len) : 0;
    PF_REQUIRE(T >= 9 && frames_out(T) >= 2, "eres2net_embed_chunks: chunk shorter than 9 fbank frames");
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

int pf_k_eres_conv(const float* a_dev, int32_t lda, int32_t a_col, int32_t cin, const float* a2_dev, int32_t lda2, int32_t a2_col,
                   int32_t cin2, int32_t a2_mode, int32_t tin2, int32_t fin2, int32_t st2, int32_t sf2, const float* w_dev, int32_t ldw,
                   const float* bias_dev, const float* r_dev, int32_t ldr, const float* x_dev, int32_t ldx, const float* y_dev,
                   int32_t ldy, float* c_dev, int32_t ldc, int32_t c_col, int32_t n_chunks, int32_t tin, int32_t fin, int32_t taps,
                   int32_t st, int32_t sf, int32_t N, int32_t act, void* stream) {
    PF_REQUIRE(a_dev && w_dev && c_dev && n_chunks > 0 && tin > 0 && fin > 0 && N > 0 && cin > 0, "k_eres_conv: null/empty argument");
    PF_REQUIRE((st == 1 || st == 2) && (sf == 1 || sf == 2), "k_eres_conv: strides 1 / 2");
    PF_REQUIRE(a_col >= 0 && a_col % 4 == 0 && a_col + eres_pad4(cin) <= lda, "k_eres_conv: the A slice must start at a multiple of 4 and fit its stride");
    PF_REQUIRE(c_col >= 0 && c_col + N <= ldc, "k_eres_conv: the C slice must fit its stride");
    if (a2_mode != ERES_A2_NONE)
        PF_REQUIRE(a2_dev && a2_col >= 0 && a2_col % 4 == 0 && a2_col + eres_pad4(a2_mode == ERES_A2_SUM ? cin : cin2) <= lda2,
                   "k_eres_conv: the A2 slice must start at a multiple of 4 and fit its stride");
    EresConvArgs a{};
    a.taps = taps; a.st = st; a.sf = sf; a.Tin = tin; a.Fin = fin;
    a.To = (tin - 1) / st + 1; a.Fo = (fin - 1) / sf + 1;
    a.M = n_chunks * a.To * a.Fo; a.N = N;
    a.A = a_dev + a_col; a.lda = lda; a.Cin = cin;
    a.a2_mode = a2_mode; a.A2 = a2_dev ? a2_dev + a2_col : nullptr; a.lda2 = lda2; a.Cin2 = cin2;
    a.Tin2 = tin2; a.Fin2 = fin2; a.st2 = st2; a.sf2 = sf2;
    a.W = w_dev; a.ldw = ldw; a.bias = bias_dev; a.R = r_dev; a.ldr = ldr; a.act = act;
    a.X = x_dev; a.ldx = ldx; a.Y = y_dev; a.ldy = ldy;
    a.C = c_dev + c_col; a.ldc = ldc;
    return launch_eres_conv(a, reinterpret_cast<hipStream_t>(stream));
}

// measurement hook (tools/bench_eres2net.py): a 3x3 stride-1 conv over [n_chunks, T, F, C] -> N channels (C % 4 == 0; both kernels take
// the same tap-major weight [N, 9 C] and the same row order) timed on eres_conv_kernel (ms_out[0]) and on CAM++'s cam_gemm_kernel
// (ms_out[1]), `iters` launches each after a warm-up
int pf_k_eres_conv_vs_cam_time(const float* a_dev, const float* w_dev, float* c_dev, int32_t n_chunks, int32_t T, int32_t F, int32_t C,
                               int32_t N, int32_t iters, float* ms_out, void* stream) {
    PF_REQUIRE(a_dev && w_dev && c_dev && ms_out && n_chunks > 0 && T > 0 && F > 0 && C > 0 && C % 4 == 0 && N > 0 && iters > 0,
               "k_eres_conv_vs_cam_time: null/empty argument, or C no multiple of 4");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    EresConvArgs a = conv_args(n_chunks, T, F, 1, 9);
    a.A = a_dev; a.lda = C; a.Cin = C; a.W = w_dev; a.ldw = 9 * C; a.N = N; a.C = c_dev; a.ldc = N; a.act = ERES_ACT_RELU;
    CamGemmArgs g{};
    g.conv2d = 1; g.M = a.M; g.N = N; g.K = 9 * C; g.W = w_dev; g.ldw = 9 * C; g.C = c_dev; g.ldc = N; g.ldr = N; g.relu = 1;
    g.A = a_dev; g.lda = C; g.Cin = C; g.T = T; g.Fin = F; g.Fo = F; g.fstride = 1;
    int rc;
    if ((rc = time_launches([&] { return launch_eres_conv(a, s); }, iters, &ms_out[0], s))) return rc;
    return time_launches([&] { return launch_cam_gemm(g, s); }, iters, &ms_out[1], s);
}

}  // extern "C"
