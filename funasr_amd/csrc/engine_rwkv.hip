// C-ABI layer, RWKV encoder of the Transducer family (funasr/models/rwkv_bat/rwkv_encoder.py): pf_rwkvencoder_* and the
// pf_k_rwkv_* hooks (kernels in rwkv.hip; the convs of the front are eres2net.hip's, every linear is gemm_f32.hip's).
//
// Load time (prepare(), again whenever the table version moves): the six conv weights [O, I, kt, kf] are repacked tap-major /
// channel-minor with tap = kf * 3 + kt, embed.output's columns are permuted from the reference's (c, f) order to the layout's (f, c),
// and w = -exp(time_decay) is computed once per block.
//
// One forward over B clips of lens[b] <= Tin frames, T2 = ceil(ceil(Tin / 2) / 2), M = B T2 rows:
//   front, CLIP BY CLIP at the clip's own length (the convs see the zero padding a lone clip sees; two ping-pong buffers sized by the
//   longest clip): stem 3x3 + ReLU -> five 3x3 convs + ReLU, strides (2,2) (1,1) (2,2) (1,1) (1,1) -> the output linear over
//   [T2_b, F2 D] rows in K slices of 1024 -> E[b]
//   embed_norm E -> X (rows past a clip's T2_b zero)
//   per block, 13 launches:
//     mix(LN_att(X); key, value, receptance) -> MIX [M, 3 D]; three GEMMs -> KVR [M, 3 D]; WKV (two launches) -> ATT = sigmoid(r) wkv;
//     proj_output GEMM + X -> X'
//     mix(LN_ffn(X'); key, receptance) -> MIX; proj_key GEMM -> HID [M, linear_size]; relu^2 in place; proj_receptance GEMM -> KVR[:, 0:D];
//     proj_value GEMM -> KVR[:, D:2D]; gate X = X' + sigmoid(r) val
//   final_norm over the rows that survive x[:, ::time_reduction] -> out [B, ceil(T2 / r), D]
// The blocks run over the whole padded batch; every kernel's result for a row depends on earlier rows of the same clip only, and the
// WKV chunk boundaries are fixed, so a clip's rows are bitwise what the clip gets alone.
#include <algorithm>

#include "engine_internal.h"
#include "eres2net.h"
#include "rwkv.h"

using namespace pf;

namespace {

struct RwkvBlk {
    const float *ln1g, *ln1b, *ln2g, *ln2b, *w, *u, *amk, *amv, *amr, *kw, *kb, *vw, *vb, *rw, *rb, *ow, *ob;
    const float *fmk, *fmr, *fkw, *fkb, *fvw, *fvb, *frw, *frb;
};

struct Rwkv {
    pf_rwkvencoder_config cfg;
    TensorTable tt;
    unsigned long long prepared_for = TensorTable::NOT_PREPARED;
    std::vector<RwkvBlk> blk;
    const float *conv_w[6], *conv_b[6];
    DevBuf ca, cb, etmp, emb, xa, xb, mix, kvr, att, hid, sum, lens2;

    int prepare();
};

constexpr int OUT_SLICE = 1024;
const int CONV_ST[6] = {1, 2, 1, 2, 1, 1};

int conv_channels(const pf_rwkvencoder_config& c, int i) { return i < 2 ? c.d_model / 4 : (i < 4 ? c.d_model / 2 : c.d_model); }
std::string conv_name(int i) { return "embed.conv." + std::to_string(2 * i) + "."; }
std::string blk_name(int i) { return "rwkv_blocks." + std::to_string(i) + "."; }
int sub2(int n) { return (n + 1) / 2; }

#define RWKV_CHECK(cond)                                                                   \
    do {                                                                                   \
        if (!(cond)) { set_error("rwkvencoder: weight preparation failed (HIP copy)"); return -2; } \
    } while (0)

int Rwkv::prepare() {
    const int D = cfg.d_model, F2 = cfg.input_dim / 4;
    {   // stem [C, 1, kt, kf] -> [C, 9], tap = kf * 3 + kt
        const int C = conv_channels(cfg, 0);
        std::vector<float> src = tt.host(conv_name(0) + "weight"), dst((size_t)C * 9);
        RWKV_CHECK(!src.empty());
        for (int o = 0; o < C; ++o)
            for (int kt = 0; kt < 3; ++kt)
                for (int kf = 0; kf < 3; ++kf) dst[(size_t)o * 9 + kf * 3 + kt] = src[(size_t)o * 9 + kt * 3 + kf];
        RWKV_CHECK(!tt.put_derived("d.conv0.w", dst));
        conv_w[0] = tt.get("d.conv0.w"); conv_b[0] = tt.get(conv_name(0) + "bias");
    }
    for (int i = 1; i < 6; ++i) {   // [O, I, kt, kf] -> [O, 9 I] tap-major
        const int O = conv_channels(cfg, i), I = conv_channels(cfg, i - 1);
        std::vector<float> src = tt.host(conv_name(i) + "weight"), dst((size_t)O * 9 * I);
        RWKV_CHECK(!src.empty());
        for (int o = 0; o < O; ++o)
            for (int c = 0; c < I; ++c)
                for (int kt = 0; kt < 3; ++kt)
                    for (int kf = 0; kf < 3; ++kf)
                        dst[((size_t)o * 9 + kf * 3 + kt) * I + c] = src[(((size_t)o * I + c) * 3 + kt) * 3 + kf];
        const std::string key = "d.conv" + std::to_string(i) + ".w";
        RWKV_CHECK(!tt.put_derived(key, dst));
        conv_w[i] = tt.get(key); conv_b[i] = tt.get(conv_name(i) + "bias");
    }
    {   // embed.output [D, D F2]: column c * F2 + f -> f * D + c
        std::vector<float> src = tt.host("embed.output.weight"), dst(src.size());
        RWKV_CHECK(!src.empty());
        const size_t K = (size_t)D * F2;
        for (int o = 0; o < D; ++o)
            for (int c = 0; c < D; ++c)
                for (int f = 0; f < F2; ++f) dst[o * K + (size_t)f * D + c] = src[o * K + (size_t)c * F2 + f];
        RWKV_CHECK(!tt.put_derived("d.out.w", dst));
    }
    blk.assign(cfg.n_blocks, RwkvBlk{});
    for (int i = 0; i < cfg.n_blocks; ++i) {
        const std::string p = blk_name(i), key = "d.blk" + std::to_string(i) + ".w";
        std::vector<float> td = tt.host(p + "att.time_decay");
        RWKV_CHECK(!td.empty());
        for (float& v : td) v = (float)-std::exp((double)v);
        RWKV_CHECK(!tt.put_derived(key, td));
        RwkvBlk& k = blk[i];
        k.ln1g = tt.get(p + "layer_norm_att.weight"); k.ln1b = tt.get(p + "layer_norm_att.bias");
        k.ln2g = tt.get(p + "layer_norm_ffn.weight"); k.ln2b = tt.get(p + "layer_norm_ffn.bias");
        k.w = tt.get(key); k.u = tt.get(p + "att.time_first");
        k.amk = tt.get(p + "att.time_mix_key"); k.amv = tt.get(p + "att.time_mix_value"); k.amr = tt.get(p + "att.time_mix_receptance");
        k.kw = tt.get(p + "att.proj_key.weight"); k.kb = tt.get(p + "att.proj_key.bias");
        k.vw = tt.get(p + "att.proj_value.weight"); k.vb = tt.get(p + "att.proj_value.bias");
        k.rw = tt.get(p + "att.proj_receptance.weight"); k.rb = tt.get(p + "att.proj_receptance.bias");
        k.ow = tt.get(p + "att.proj_output.weight"); k.ob = tt.get(p + "att.proj_output.bias");
        k.fmk = tt.get(p + "ffn.time_mix_key"); k.fmr = tt.get(p + "ffn.time_mix_receptance");
        k.fkw = tt.get(p + "ffn.proj_key.weight"); k.fkb = tt.get(p + "ffn.proj_key.bias");
        k.fvw = tt.get(p + "ffn.proj_value.weight"); k.fvb = tt.get(p + "ffn.proj_value.bias");
        k.frw = tt.get(p + "ffn.proj_receptance.weight"); k.frb = tt.get(p + "ffn.proj_receptance.bias");
    }
    prepared_for = tt.version;
    return 0;
}

int ready(Rwkv* e) {
    if (e->tt.require_all("rwkvencoder")) return -3;
    if (e->prepared_for != e->tt.version) return e->prepare();
    return 0;
}

int linear(const float* A, int lda, const float* W, const float* bias, const float* R1, int ldr1, float* C, int ldc, int M, int N, int K,
           hipStream_t s) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.bias = bias; g.R1 = R1; g.ldr1 = ldr1; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    ProfScope ps(PROF_GEMM, 2.0 * M * (double)N * K, s, "rwkv.linear");
    return launch_gemm_f32(g, s);
}

// the front of ONE clip of n frames: feats [n, F] -> dst [T2, D]
int run_front(Rwkv* e, const float* feats, int n, float* dst, hipStream_t s) {
    const pf_rwkvencoder_config& c = e->cfg;
    const int D = c.d_model;
    float* bufs[2] = {e->ca.as<float>(), e->cb.as<float>()};
    int T = n, F = c.input_dim, rc;
    {
        ProfScope ps(PROF_GEMM, 2.0 * 9 * (double)T * F * conv_channels(c, 0), s, "rwkv.conv");
        if ((rc = launch_eres_stem(feats, 1, T, F, e->conv_w[0], e->conv_b[0], conv_channels(c, 0), bufs[0], s))) return rc;
    }
    for (int i = 1; i < 6; ++i) {
        EresConvArgs a{};
        a.taps = 9; a.st = a.sf = CONV_ST[i];
        a.Tin = T; a.Fin = F; a.To = (T - 1) / a.st + 1; a.Fo = (F - 1) / a.sf + 1;
        a.Cin = conv_channels(c, i - 1); a.N = conv_channels(c, i);
        a.M = a.To * a.Fo;
        a.A = bufs[(i - 1) & 1]; a.lda = a.Cin;
        a.W = e->conv_w[i]; a.ldw = 9 * a.Cin; a.bias = e->conv_b[i]; a.act = ERES_ACT_RELU;
        a.C = bufs[i & 1]; a.ldc = a.N;
        ProfScope ps(PROF_GEMM, 2.0 * a.M * (double)a.N * 9 * a.Cin, s, "rwkv.conv");
        if ((rc = launch_eres_conv(a, s))) return rc;
        T = a.To; F = a.Fo;
    }
    // conv 5 wrote bufs[1] = [T2, F2, D]: rows of F2 D columns in the (f, c) order of d.out.w. Long K: slices whose chains start at
    // zero, the running sum riding in as the next launch's addend; the last slice writes dst
    const int K = F * D, ns = ceil_div(K, OUT_SLICE);
    float* tmp = e->etmp.as<float>();
    const float* last = nullptr;
    if ((rc = gemm_f32_ksliced(bufs[1], K, e->tt.get("d.out.w"), K, e->tt.get("embed.output.bias"), T, D, K, OUT_SLICE, ns % 2 ? dst : tmp,
                               ns % 2 ? tmp : dst, &last, "rwkv.linear", s)))
        return rc;
    if (last != dst) { set_error("rwkvencoder: internal error (the output linear ended in its scratch buffer)"); return -2; }
    return 0;
}

// `stages` (tests; nullable, and each entry nullable): device buffers [B, T2, D] that receive the front output, the embed_norm
// output and every block's output as they are computed (rows past a clip's length: unspecified in the first, zeros in the others)
int run(Rwkv* e, const float* feats, const int32_t* lens_host, int B, int Tin, float* out, int32_t* out_lens_host, float* const* stages,
        hipStream_t s) {
    const pf_rwkvencoder_config& c = e->cfg;
    const int D = c.d_model, H = c.linear_size, F = c.input_dim, r = c.time_reduction;
    int nmax = 0;
    for (int b = 0; b < B; ++b) {
        PF_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= Tin, "rwkvencoder_forward: every length must lie in 1 .. Tin");
        nmax = std::max(nmax, lens_host[b]);
    }
    const int T2 = sub2(sub2(Tin)), To = (T2 - 1) / r + 1;
    PF_REQUIRE((long long)B * T2 <= 0x7fffffff / 4 / std::max(3 * D, H), "rwkvencoder_forward: batch too large");
    const int M = B * T2;
    int rc;
    if ((rc = ready(e))) return rc;
    {   // the largest conv outputs of the longest clip: even convs write ca, odd ones cb
        size_t za = 0, zb = 0;
        int T = nmax, Fl = F;
        for (int i = 0; i < 6; ++i) {
            T = (T - 1) / CONV_ST[i] + 1; Fl = (Fl - 1) / CONV_ST[i] + 1;
            size_t& z = i & 1 ? zb : za;
            z = std::max(z, (size_t)T * Fl * conv_channels(c, i));
        }
        if (e->ca.ensure(sizeof(float) * za) || e->cb.ensure(sizeof(float) * zb)) return -2;
    }
    const size_t MD = (size_t)M * D;
    if (e->etmp.ensure(sizeof(float) * (size_t)T2 * D) || e->emb.ensure(sizeof(float) * MD) || e->xa.ensure(sizeof(float) * MD) ||
        e->xb.ensure(sizeof(float) * MD) || e->mix.ensure(sizeof(float) * 3 * MD) || e->kvr.ensure(sizeof(float) * 3 * MD) ||
        e->att.ensure(sizeof(float) * MD) || e->hid.ensure(sizeof(float) * (size_t)M * H) ||
        e->sum.ensure(sizeof(float) * rwkv_wkv_scratch_floats(B, T2, D)))
        return -2;
    float *E = e->emb.as<float>(), *X = e->xa.as<float>(), *X2 = e->xb.as<float>(), *MIX = e->mix.as<float>(), *KVR = e->kvr.as<float>(),
          *ATT = e->att.as<float>(), *HID = e->hid.as<float>();
    std::vector<int32_t> l2(B);
    for (int b = 0; b < B; ++b) {
        l2[b] = sub2(sub2(lens_host[b]));
        if (out_lens_host) out_lens_host[b] = (l2[b] - 1) / r + 1;
        if ((rc = run_front(e, feats + (size_t)b * Tin * F, lens_host[b], E + (size_t)b * T2 * D, s))) return rc;
    }
    if (upload_lens(e->lens2, l2.data(), B, s)) return -2;
    const int* L2 = e->lens2.as<int>();
    auto stage = [&](int which, const float* src) -> int {
        if (stages && stages[which]) PF_HIP_TRY(hipMemcpyAsync(stages[which], src, sizeof(float) * MD, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    if ((rc = stage(0, E))) return rc;
    {
        ProfScope ps(PROF_LN, 8.0 * MD, s, "rwkv.row");
        if ((rc = launch_rwkv_norm(E, D, e->tt.get("embed_norm.weight"), e->tt.get("embed_norm.bias"), c.ln_eps, X, D, L2, B, T2, 1, T2, D, s)))
            return rc;
    }
    if ((rc = stage(1, X))) return rc;
    for (int i = 0; i < c.n_blocks; ++i) {
        const RwkvBlk& k = e->blk[i];
        RwkvMixArgs m{};
        m.X = X; m.ldx = D; m.gamma = k.ln1g; m.beta = k.ln1b; m.eps = c.ln_eps;
        m.mix[0] = k.amk; m.mix[1] = k.amv; m.mix[2] = k.amr; m.n_out = 3;
        m.Y = MIX; m.ldy = 3 * D; m.lens = L2; m.B = B; m.T = T2; m.D = D;
        {
            ProfScope ps(PROF_LN, 20.0 * MD, s, "rwkv.row");
            if ((rc = launch_rwkv_mix(m, s))) return rc;
        }
        if ((rc = linear(MIX, 3 * D, k.kw, k.kb, nullptr, 0, KVR, 3 * D, M, D, D, s))) return rc;
        if ((rc = linear(MIX + D, 3 * D, k.vw, k.vb, nullptr, 0, KVR + D, 3 * D, M, D, D, s))) return rc;
        if ((rc = linear(MIX + 2 * D, 3 * D, k.rw, k.rb, nullptr, 0, KVR + 2 * D, 3 * D, M, D, D, s))) return rc;
        RwkvWkvArgs w{};
        w.k = KVR; w.v = KVR + D; w.r = KVR + 2 * D; w.ld = 3 * D; w.w = k.w; w.u = k.u; w.lens = L2; w.B = B; w.T = T2; w.D = D;
        w.out = ATT; w.ldo = D; w.sum = e->sum.as<float>();
        {
            ProfScope ps(PROF_LN, 16.0 * MD, s, "rwkv.wkv");
            if ((rc = launch_rwkv_wkv(w, s))) return rc;
        }
        if ((rc = linear(ATT, D, k.ow, k.ob, X, D, X2, D, M, D, D, s))) return rc;
        m.X = X2; m.gamma = k.ln2g; m.beta = k.ln2b; m.mix[0] = k.fmk; m.mix[1] = k.fmr; m.mix[2] = nullptr; m.n_out = 2;
        {
            ProfScope ps(PROF_LN, 16.0 * MD, s, "rwkv.row");
            if ((rc = launch_rwkv_mix(m, s))) return rc;
        }
        if ((rc = linear(MIX, 3 * D, k.fkw, k.fkb, nullptr, 0, HID, H, M, H, D, s))) return rc;
        {
            ProfScope ps(PROF_LN, 8.0 * M * (double)H, s, "rwkv.row");
            if ((rc = launch_rwkv_sqrelu(HID, H, L2, B, T2, H, s))) return rc;
        }
        if ((rc = linear(MIX + D, 3 * D, k.frw, k.frb, nullptr, 0, KVR, 3 * D, M, D, D, s))) return rc;
        if ((rc = linear(HID, H, k.fvw, k.fvb, nullptr, 0, KVR + D, 3 * D, M, D, H, s))) return rc;
        {
            ProfScope ps(PROF_LN, 16.0 * MD, s, "rwkv.row");
            if ((rc = launch_rwkv_gate(X2, D, KVR, 3 * D, KVR + D, 3 * D, X, D, L2, B, T2, D, s))) return rc;
        }
        if ((rc = stage(2 + i, X))) return rc;
    }
    ProfScope ps(PROF_LN, 8.0 * B * (double)To * D, s, "rwkv.row");
    return launch_rwkv_norm(X, D, e->tt.get("final_norm.weight"), e->tt.get("final_norm.bias"), c.ln_eps, out, D, L2, B, T2, r, To, D, s);
}

}  // namespace

extern "C" {

pf_rwkvencoder* pf_rwkvencoder_create(const pf_rwkvencoder_config* cfg) {
    if (!cfg) { set_error("rwkvencoder: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_rwkvencoder_config& c = *cfg;
    if (c.input_dim < 8 || c.input_dim > 256 || c.input_dim % 4 != 0 || c.d_model < 32 || c.d_model > RWKV_MAX_D || c.d_model % 32 != 0 ||
        c.linear_size < 32 || c.linear_size > 4096 || c.linear_size % 32 != 0 || c.n_blocks < 1 || c.time_reduction < 1 || !(c.ln_eps > 0.f)) {
        set_error("rwkvencoder: unsupported config (built: 8 .. 256 input features in multiples of 4, d_model up to 1024 and linear_size up "
                  "to 4096 in multiples of 32, n_blocks >= 1, time_reduction >= 1)");
        return nullptr;
    }
    std::unique_ptr<Rwkv> h(new Rwkv());
    h->cfg = c;
    const int D = c.d_model, H = c.linear_size;
    int rc = 0;
    for (int i = 0; i < 6; ++i)
        rc |= h->tt.add_linear(conv_name(i), conv_channels(c, i), (int64_t)9 * (i ? conv_channels(c, i - 1) : 1));
    rc |= h->tt.add_linear("embed.output.", D, (int64_t)D * (c.input_dim / 4));
    rc |= h->tt.add_linear("embed_norm.", D, 1);
    rc |= h->tt.add_linear("final_norm.", D, 1);
    for (int i = 0; i < c.n_blocks; ++i) {
        const std::string p = blk_name(i);
        rc |= h->tt.add_linear(p + "layer_norm_att.", D, 1);
        rc |= h->tt.add_linear(p + "layer_norm_ffn.", D, 1);
        for (const char* n : {"att.time_decay", "att.time_first", "att.time_mix_key", "att.time_mix_value", "att.time_mix_receptance",
                              "ffn.time_mix_key", "ffn.time_mix_receptance"})
            rc |= h->tt.add(p + n, D);
        for (const char* n : {"att.proj_key.", "att.proj_value.", "att.proj_receptance.", "att.proj_output.", "ffn.proj_receptance."})
            rc |= h->tt.add_linear(p + n, D, D);
        rc |= h->tt.add_linear(p + "ffn.proj_key.", H, D);
        rc |= h->tt.add_linear(p + "ffn.proj_value.", D, H);
    }
    if (rc) return nullptr;
    return reinterpret_cast<pf_rwkvencoder*>(h.release());
}
void pf_rwkvencoder_destroy(pf_rwkvencoder* h) { delete reinterpret_cast<Rwkv*>(h); }
int pf_rwkvencoder_set_tensor(pf_rwkvencoder* hh, const char* name, const float* data, int64_t numel) {
    Rwkv* h = reinterpret_cast<Rwkv*>(hh);
    PF_REQUIRE(h && name && data, "rwkvencoder_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_rwkvencoder_missing(const pf_rwkvencoder* hh) {
    const Rwkv* h = reinterpret_cast<const Rwkv*>(hh);
    return h ? h->tt.missing() : -1;
}
int32_t pf_rwkvencoder_num_frames(const pf_rwkvencoder* hh, int32_t n_frames) {
    const Rwkv* h = reinterpret_cast<const Rwkv*>(hh);
    if (!h || n_frames < 1) return -1;
    return (sub2(sub2(n_frames)) - 1) / h->cfg.time_reduction + 1;
}
int pf_rwkvencoder_debug_poison(pf_rwkvencoder* hh) {
    Rwkv* h = reinterpret_cast<Rwkv*>(hh);
    PF_REQUIRE(h, "rwkvencoder_debug_poison: null handle");
    PF_HIP_TRY(hipDeviceSynchronize());
    for (DevBuf* b : {&h->ca, &h->cb, &h->etmp, &h->emb, &h->xa, &h->xb, &h->mix, &h->kvr, &h->att, &h->hid, &h->sum})
        if (b->p) PF_HIP_TRY(hipMemset(b->p, 0xff, b->cap));
    return 0;
}
int pf_rwkvencoder_forward(pf_rwkvencoder* hh, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, float* out,
                           int32_t* out_lens_host, void* stream) {
    Rwkv* h = reinterpret_cast<Rwkv*>(hh);
    PF_REQUIRE(h && feats && lens_host && out && B > 0 && B <= 65535 && Tin > 0, "rwkvencoder_forward: null/empty argument");
    return run(h, feats, lens_host, B, Tin, out, out_lens_host, nullptr, reinterpret_cast<hipStream_t>(stream));
}
int pf_rwkvencoder_forward_stages(pf_rwkvencoder* hh, const float* feats, const int32_t* lens_host, int32_t B, int32_t Tin, float* out,
                                  int32_t* out_lens_host, float* const* stages_dev, void* stream) {
    Rwkv* h = reinterpret_cast<Rwkv*>(hh);
    PF_REQUIRE(h && feats && lens_host && out && stages_dev && B > 0 && B <= 65535 && Tin > 0, "rwkvencoder_forward_stages: null/empty argument");
    return run(h, feats, lens_host, B, Tin, out, out_lens_host, stages_dev, reinterpret_cast<hipStream_t>(stream));
}

int pf_k_rwkv_chunk(void) { return RWKV_CHUNK; }
int pf_k_rwkv_mix(const float* x_dev, int32_t ldx, const float* gamma_dev, const float* beta_dev, float eps, const float* mix0_dev,
                  const float* mix1_dev, const float* mix2_dev, float* y_dev, int32_t ldy, const int32_t* lens_dev, int32_t B, int32_t T,
                  int32_t D, void* stream) {
    RwkvMixArgs m{};
    m.X = x_dev; m.ldx = ldx; m.gamma = gamma_dev; m.beta = beta_dev; m.eps = eps;
    m.mix[0] = mix0_dev; m.mix[1] = mix1_dev; m.mix[2] = mix2_dev; m.n_out = mix2_dev ? 3 : 2;
    m.Y = y_dev; m.ldy = ldy; m.lens = lens_dev; m.B = B; m.T = T; m.D = D;
    return launch_rwkv_mix(m, reinterpret_cast<hipStream_t>(stream));
}
int pf_k_rwkv_wkv(const float* k_dev, const float* v_dev, const float* r_dev, int32_t ld, const float* w_dev, const float* u_dev,
                  const int32_t* lens_dev, int32_t B, int32_t T, int32_t D, float* out_dev, int32_t ldo, float* scratch_dev,
                  int64_t scratch_floats, void* stream) {
    PF_REQUIRE(B > 0 && T > 0 && D > 0 && scratch_floats >= (int64_t)rwkv_wkv_scratch_floats(B, T, D),
               "k_rwkv_wkv: the scratch holds fewer than B * ceil(T / chunk) * 3 * D floats");
    RwkvWkvArgs w{};
    w.k = k_dev; w.v = v_dev; w.r = r_dev; w.ld = ld; w.w = w_dev; w.u = u_dev; w.lens = lens_dev; w.B = B; w.T = T; w.D = D;
    w.out = out_dev; w.ldo = ldo; w.sum = scratch_dev;
    return launch_rwkv_wkv(w, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
