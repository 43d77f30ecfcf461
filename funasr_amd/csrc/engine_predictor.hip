// C-ABI layer, predictor family: pf_predictor_* (CIF predictor, the V3 timestamp head) and the LSTM direction-pair it shares with pf_k_lstm.
#include "engine_internal.h"

namespace pf {

// relu(Conv1d(D, D, l + r + 1)(pad(hidden))) (cif_predictor.py:275-278) as ONE exact-fp32 GEMM whose A operand is gathered from the
// row-shifted views of `hidden` by the DMA sources (gemm_f32.hip, GemmArgs.conv_*): the k order per output element is that of the
// im2col GEMM of rounds 1-5, so alphas are bitwise unchanged, and the [M, taps D] column matrix (197 MB written + 196 MB read per
// headline step) is gone
static int predictor_conv(Predictor* p, const float* hidden, int B, int T, hipStream_t s) {
    const pf_predictor_config& c = p->cfg;
    const int D = c.d_model, taps = c.l_order + c.r_order + 1;
    const size_t M = (size_t)B * T;
    if (p->conv.ensure(sizeof(float) * M * D)) return -2;
    if (!p->zero_row.p) {
        if (p->zero_row.ensure(256)) return -2;
        PF_HIP_TRY(hipMemsetAsync(p->zero_row.p, 0, 256, s));
    }
    GemmArgs g{};
    g.A = hidden; g.lda = D; g.W = p->tt.get("cif_conv1d.weight"); g.ldw = taps * D; g.bias = p->tt.get("cif_conv1d.bias");
    g.C = p->conv.as<float>(); g.ldc = D; g.M = (int)M; g.N = D; g.K = taps * D; g.relu = 1;
    g.conv_taps = taps; g.conv_D = D; g.conv_T = T; g.conv_left = c.l_order; g.conv_zero = p->zero_row.as<float>();
    ProfScope ps(PROF_GEMM, 2.0 * (double)M * D * (double)(taps * D), s);
    return launch_gemm_f32(g, s);
}

// everything of pf_predictor_alphas up to the scan, ENQUEUED into scan-state slot `slot`; the token counts stay on the device
// (predictor_counts_dev)
int predictor_alphas_enqueue(Predictor* p, int slot, const float* hidden, const int32_t* lens_host, int B, int T, hipStream_t s) {
    PF_REQUIRE(p && hidden && lens_host && B > 0 && T > 0 && (slot == 0 || slot == 1), "predictor_alphas: null/empty argument");
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= T, "predictor_alphas: lens out of range");
    if (p->tt.require_all("predictor")) return -3;
    const pf_predictor_config& c = p->cfg;
    const int D = c.d_model, Te = T + 1;
    Predictor::CifState& S = p->st[slot];
    if (S.alphas.ensure(sizeof(float) * (size_t)B * Te) || S.peaks.ensure(sizeof(float) * (size_t)B * Te) ||
        S.rems.ensure(sizeof(float) * (size_t)B * Te) || S.flags.ensure(sizeof(int) * (size_t)B * Te) ||
        S.nfires.ensure(sizeof(int) * (size_t)B))
        return -2;
    int rc;
    if ((rc = upload_lens(S.lens, lens_host, B, s))) return rc;
    if ((rc = predictor_conv(p, hidden, B, T, s))) return rc;
    AlphaArgs aa{};
    aa.conv = p->conv.as<float>(); aa.w = p->tt.get("cif_output.weight"); aa.bias = p->tt.get("cif_output.bias");
    aa.lens = S.lens.as<int>(); aa.alphas = S.alphas.as<float>(); aa.B = B; aa.T = T; aa.D = D; aa.T_ext = Te;
    aa.smooth = c.smooth_factor; aa.noise = c.noise_threshold;
    if ((rc = launch_alpha(aa, s))) return rc;
    CifScanArgs sa{};
    sa.alphas = S.alphas.as<float>(); sa.peaks = S.peaks.as<float>(); sa.rems = S.rems.as<float>();
    sa.fire_flag = S.flags.as<int>(); sa.n_fires = S.nfires.as<int>(); sa.lens = S.lens.as<int>(); sa.B = B;
    sa.T = T; sa.tail_threshold = c.tail_threshold; sa.tail_mask = c.tail_mask;
    if (p->v3) {
        if (S.curs.ensure(sizeof(float) * (size_t)B * Te) || S.ntok.ensure(sizeof(int) * (size_t)B)) return -2;
        if ((rc = launch_cif_scan_loop(sa, S.curs.as<float>(), S.ntok.as<int>(), s))) return rc;
    } else if ((rc = launch_cif_scan(sa, s))) {
        return rc;
    }
    S.B = B; S.T = T;
    return 0;
}
// V3 reports floor(sum alphas) (cif_predictor.py:383), V2's count of fires is the same number by construction
const int32_t* predictor_counts_dev(Predictor* p, int slot) {
    return reinterpret_cast<const int32_t*>(p->v3 ? p->st[slot].ntok.p : p->st[slot].nfires.p);
}
const float* predictor_alphas_dev(Predictor* p, int slot) { return p->st[slot].alphas.as<float>(); }
const float* predictor_peaks_dev(Predictor* p, int slot) { return p->st[slot].peaks.as<float>(); }
int predictor_embeds_slot(Predictor* p, int slot, const float* hidden, int B, int T, int N, float* embeds, hipStream_t s) {
    PF_REQUIRE(p && hidden && embeds && N >= 0 && (slot == 0 || slot == 1), "predictor_embeds: null argument");
    Predictor::CifState& S = p->st[slot];
    PF_REQUIRE(B == S.B && T == S.T, "predictor_embeds: call pf_predictor_alphas with the same batch first");
    CifEmitArgs ea{};
    ea.hidden = hidden; ea.alphas = S.alphas.as<float>(); ea.rems = S.rems.as<float>();
    ea.fire_flag = S.flags.as<int>(); ea.embeds = embeds; ea.B = B; ea.T = T; ea.D = p->cfg.d_model; ea.N = N;
    if (p->v3) {
        if (N <= 0) return 0;
        ea.alphas = S.curs.as<float>();
        return launch_cif_emit_loop(ea, s);
    }
    return launch_cif_emit(ea, s);
}

// one direction-pair of torch.nn.LSTM on a time-major input: gates-major input projections by the fp32 MFMA GEMM
// (W_ih . X_tm^T, one GEMM per direction), then the per-step recurrence (lstm.hip)
int lstm_forward(const LstmW& w, const float* x_tm, int T, int B, int D, int H, int ndir, float* out, int out_layout,
                        DevBuf& pre, DevBuf& h_a, DevBuf& h_b, DevBuf& cell, hipStream_t s) {
    const size_t cols = (size_t)T * B, ldp = (cols + 3) / 4 * 4;
    const int Bs = (B + 63) / 64 * 64;
    const size_t state = sizeof(float) * (size_t)ndir * H * Bs;
    if (pre.ensure(sizeof(float) * (size_t)ndir * 4 * H * ldp) || h_a.ensure(state) || h_b.ensure(state) || cell.ensure(state))
        return -2;
    int rc;
    for (int d = 0; d < ndir; ++d)
        if ((rc = gemm_simple(w.w_ih[d], D, x_tm, D, nullptr, pre.as<float>() + (size_t)d * 4 * H * ldp, (int)ldp, 4 * H,
                              (int)cols, D, 0, nullptr, 0, nullptr, 0, s))) return rc;
    LstmStepArgs a{};
    a.pre = pre.as<float>(); a.whh = w.w_hh; a.b_ih = w.b_ih; a.b_hh = w.b_hh; a.h_a = h_a.as<float>();
    a.h_b = h_b.as<float>(); a.c = cell.as<float>(); a.out = out; a.ld_pre = ldp; a.T = T; a.B = B; a.Bs = Bs; a.H = H;
    a.ndir = ndir; a.out_layout = out_layout;
    return launch_lstm_steps(a, s);
}

}  // namespace pf

using namespace pf;

extern "C" {

pf_predictor* pf_predictor_create(const pf_predictor_config* cfg) {
    if (!cfg) { set_error("predictor: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_predictor_config& c = *cfg;
    if (c.d_model <= 0 || c.d_model % 32 || c.l_order < 0 || c.r_order < 0 || c.threshold != 1.0f) {
        set_error("predictor: unsupported config (d_model % 32 == 0; threshold must be 1.0: cif_wo_hidden_v1 "
                  "detects fires with floor(), cif_predictor.py:838-846)");
        return nullptr;
    }
    std::unique_ptr<Predictor> p(new Predictor());
    p->cfg = c;
    const int D = c.d_model, taps = c.l_order + c.r_order + 1;
    int rc = 0;
    rc |= p->tt.add_conv("cif_conv1d.weight", D, D, taps);
    rc |= p->tt.add("cif_conv1d.bias", D);
    rc |= p->tt.add("cif_output.weight", D);
    rc |= p->tt.add("cif_output.bias", 1);
    if (rc) return nullptr;
    return reinterpret_cast<pf_predictor*>(p.release());
}
pf_predictor* pf_predictor_create_v3(const pf_predictor_config* cfg, const pf_predictor_v3_config* cfg3) {
    if (!cfg3) { set_error("predictor_v3: null config"); return nullptr; }
    const pf_predictor_v3_config& c3 = *cfg3;
    if (c3.upsample_times < 1 || c3.upsample_times > 8 || (c3.upsample_type != 0 && c3.upsample_type != 1)) {
        set_error("predictor_v3: unsupported config (upsample_times 1..8; upsample_type 0 = cnn, 1 = cnn_blstm)");
        return nullptr;
    }
    if (cfg && !cfg->tail_mask && cfg->tail_threshold > 0.f) {
        set_error("predictor_v3: the reference always applies the tail threshold through the mask (tail_mask = 1)");
        return nullptr;
    }
    pf_predictor* ph = pf_predictor_create(cfg);
    if (!ph) return nullptr;
    Predictor* p = reinterpret_cast<Predictor*>(ph);
    p->v3 = true;
    p->c3 = c3;
    const int D = p->cfg.d_model, U = c3.upsample_times;
    int rc = 0;
    rc |= p->tt.add_upsample("upsample_cnn.weight", D, D, U);
    rc |= p->tt.add_tiled("upsample_cnn.bias", D, U);
    if (c3.upsample_type == 1) {
        for (const char* sfx : {"", "_reverse"}) {
            const std::string s(sfx);
            rc |= p->tt.add("blstm.weight_ih_l0" + s, (int64_t)4 * D * D);
            rc |= p->tt.add_lstm_hh("blstm.weight_hh_l0" + s, D);
            rc |= p->tt.add("blstm.bias_ih_l0" + s, (int64_t)4 * D);
            rc |= p->tt.add("blstm.bias_hh_l0" + s, (int64_t)4 * D);
        }
        rc |= p->tt.add("cif_output2.weight", 2 * D);
    } else {
        rc |= p->tt.add("cif_output2.weight", D);
    }
    rc |= p->tt.add("cif_output2.bias", 1);
    if (rc) { pf_predictor_destroy(ph); return nullptr; }
    return ph;
}
void pf_predictor_destroy(pf_predictor* p) { delete reinterpret_cast<Predictor*>(p); }
int pf_predictor_set_tensor(pf_predictor* ph, const char* name, const float* data, int64_t numel) {
    Predictor* p = reinterpret_cast<Predictor*>(ph);
    PF_REQUIRE(p && name && data, "predictor_set_tensor: null");
    return p->tt.set(name, data, numel);
}
int pf_predictor_missing(const pf_predictor* ph) {
    const Predictor* p = reinterpret_cast<const Predictor*>(ph);
    return p ? p->tt.missing() : -1;
}

int pf_predictor_alphas(pf_predictor* ph, const float* hidden, const int32_t* lens_host, int32_t B, int32_t T,
                        float* alphas, float* peaks, int32_t* token_num, void* stream) {
    Predictor* p = reinterpret_cast<Predictor*>(ph);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(p && token_num, "predictor_alphas: null/empty argument");
    int rc;
    if ((rc = predictor_alphas_enqueue(p, 0, hidden, lens_host, B, T, s))) return rc;
    const size_t Te = (size_t)T + 1;
    if (alphas) PF_HIP_TRY(hipMemcpyAsync(alphas, p->st[0].alphas.p, sizeof(float) * (size_t)B * Te, hipMemcpyDeviceToDevice, s));
    if (peaks) PF_HIP_TRY(hipMemcpyAsync(peaks, p->st[0].peaks.p, sizeof(float) * (size_t)B * Te, hipMemcpyDeviceToDevice, s));
    PF_HIP_TRY(hipMemcpyAsync(token_num, predictor_counts_dev(p, 0), sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int pf_predictor_embeds(pf_predictor* ph, const float* hidden, int32_t B, int32_t T, int32_t N, float* embeds,
                        void* stream) {
    return predictor_embeds_slot(reinterpret_cast<Predictor*>(ph), 0, hidden, B, T, N, embeds, reinterpret_cast<hipStream_t>(stream));
}

// The two steps without the synchronisation between them, for callers that keep two batches in flight (include/paraformer_hip.h)
int pf_predictor_alphas_begin(pf_predictor* ph, int32_t slot, const float* hidden, const int32_t* lens_host, int32_t B, int32_t T,
                              float* alphas, float* peaks, int32_t* counts_pinned_host, void* stream) {
    Predictor* p = reinterpret_cast<Predictor*>(ph);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(p && counts_pinned_host && (slot == 0 || slot == 1), "predictor_alphas_begin: null argument or slot not 0 / 1");
    int rc;
    if ((rc = predictor_alphas_enqueue(p, slot, hidden, lens_host, B, T, s))) return rc;
    const size_t Te = (size_t)T + 1;
    if (alphas) PF_HIP_TRY(hipMemcpyAsync(alphas, p->st[slot].alphas.p, sizeof(float) * (size_t)B * Te, hipMemcpyDeviceToDevice, s));
    if (peaks) PF_HIP_TRY(hipMemcpyAsync(peaks, p->st[slot].peaks.p, sizeof(float) * (size_t)B * Te, hipMemcpyDeviceToDevice, s));
    PF_HIP_TRY(hipMemcpyAsync(counts_pinned_host, predictor_counts_dev(p, slot), sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
    return 0;
}

int pf_predictor_embeds_slot(pf_predictor* ph, int32_t slot, const float* hidden, int32_t B, int32_t T, int32_t N, float* embeds,
                             void* stream) {
    return predictor_embeds_slot(reinterpret_cast<Predictor*>(ph), slot, hidden, B, T, N, embeds, reinterpret_cast<hipStream_t>(stream));
}

int pf_predictor_timestamp(pf_predictor* ph, const float* hidden, const int32_t* lens_host, const int32_t* token_num_host,
                           int32_t B, int32_t T, float* us_alphas, float* us_peaks, void* stream) {
    Predictor* p = reinterpret_cast<Predictor*>(ph);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(p && hidden && lens_host && token_num_host && us_alphas && us_peaks && B > 0 && T > 0,
               "predictor_timestamp: null/empty argument");
    PF_REQUIRE(p->v3, "predictor_timestamp: the handle was not made by pf_predictor_create_v3");
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= T, "predictor_timestamp: lens out of range");
    if (p->tt.require_all("predictor")) return -3;
    const pf_predictor_config& c = p->cfg;
    const int D = c.d_model, U = p->c3.upsample_times, taps = c.l_order + c.r_order + 1, Tu = T * U;
    const size_t M = (size_t)B * T;
    int rc;
    if ((rc = upload_lens(p->ts_lens, lens_host, B, s))) return rc;        // (its own buffer: both scan-state slots may be in flight)
    if (p->tok_dev.ensure(sizeof(int) * (size_t)B)) return -2;
    if (upload_h2d(p->tok_dev.p, token_num_host, sizeof(int32_t) * (size_t)B, s)) return -2;
    const float* src = hidden;
    if (p->c3.use_cif1_cnn) {                                   // the head sees relu(cif_conv1d(hidden)) instead (:317-320)
        if ((rc = predictor_conv(p, hidden, B, T, s))) return rc;
        src = p->conv.as<float>();
    }
    // ConvTranspose1d(k = stride = U) == one GEMM: row (b, t) of the output holds frames U t .. U t + U - 1
    if (p->up.ensure(sizeof(float) * M * U * D)) return -2;
    if ((rc = gemm_simple(src, D, p->tt.get("upsample_cnn.weight"), D, p->tt.get("upsample_cnn.bias"), p->up.as<float>(),
                          U * D, (int)M, U * D, D, 0, nullptr, 0, nullptr, 0, s))) return rc;
    if (p->c3.upsample_type == 1) {
        const int Bs = (B + 63) / 64 * 64;
        if (p->x_tm.ensure(sizeof(float) * (size_t)Tu * B * D) || p->lstm_out.ensure(sizeof(float) * (size_t)Tu * 2 * D * Bs))
            return -2;
        if ((rc = launch_rows_bt_to_tb(p->up.as<float>(), p->x_tm.as<float>(), B, Tu, D, s))) return rc;
        // the two directions' recurrent weights / biases live back to back so that one launch serves both
        LstmW w{};
        w.w_ih[0] = p->tt.get("blstm.weight_ih_l0"); w.w_ih[1] = p->tt.get("blstm.weight_ih_l0_reverse");
        const size_t hh = (size_t)4 * D * D, bb = (size_t)4 * D;
        if (p->pack.ensure(sizeof(float) * (2 * hh + 4 * bb))) return -2;
        float* pack = p->pack.as<float>();
        float* bi = pack + 2 * hh;
        float* bh = bi + 2 * bb;
        if (p->packed_for != p->tt.version) {
            PF_HIP_TRY(hipMemcpyAsync(pack, p->tt.get("blstm.weight_hh_l0"), sizeof(float) * hh, hipMemcpyDeviceToDevice, s));
            PF_HIP_TRY(hipMemcpyAsync(pack + hh, p->tt.get("blstm.weight_hh_l0_reverse"), sizeof(float) * hh, hipMemcpyDeviceToDevice, s));
            PF_HIP_TRY(hipMemcpyAsync(bi, p->tt.get("blstm.bias_ih_l0"), sizeof(float) * bb, hipMemcpyDeviceToDevice, s));
            PF_HIP_TRY(hipMemcpyAsync(bi + bb, p->tt.get("blstm.bias_ih_l0_reverse"), sizeof(float) * bb, hipMemcpyDeviceToDevice, s));
            PF_HIP_TRY(hipMemcpyAsync(bh, p->tt.get("blstm.bias_hh_l0"), sizeof(float) * bb, hipMemcpyDeviceToDevice, s));
            PF_HIP_TRY(hipMemcpyAsync(bh + bb, p->tt.get("blstm.bias_hh_l0_reverse"), sizeof(float) * bb, hipMemcpyDeviceToDevice, s));
            p->packed_for = p->tt.version;
        }
        w.w_hh = pack; w.b_ih = bi; w.b_hh = bh;
        if ((rc = lstm_forward(w, p->x_tm.as<float>(), Tu, B, D, D, 2, p->lstm_out.as<float>(), 1, p->pre, p->h_a, p->h_b,
                               p->cell, s))) return rc;
        UsAlphaArgs ua{};
        ua.out_t = p->lstm_out.as<float>(); ua.w = p->tt.get("cif_output2.weight"); ua.bias = p->tt.get("cif_output2.bias");
        ua.lens = p->ts_lens.as<int>(); ua.alphas = us_alphas; ua.B = B; ua.Bs = Bs; ua.T = Tu; ua.C = 2 * D; ua.U = U;
        ua.smooth = p->c3.smooth_factor2; ua.noise = p->c3.noise_threshold2;
        if ((rc = launch_us_alpha_t(ua, s))) return rc;
    } else {
        // plain `cnn` head: the row-major upsampled frames go straight through the one-wave-per-row dot kernel
        p->ul_host.resize(B);
        for (int b = 0; b < B; ++b) p->ul_host[b] = lens_host[b] * U;
        DevBuf& ulens = p->ulens;
        if ((rc = upload_lens(ulens, p->ul_host.data(), B, s))) return rc;
        AlphaArgs aa{};
        aa.conv = p->up.as<float>(); aa.w = p->tt.get("cif_output2.weight"); aa.bias = p->tt.get("cif_output2.bias");
        aa.lens = ulens.as<int>(); aa.alphas = us_alphas; aa.B = B; aa.T = Tu; aa.D = D; aa.T_ext = Tu;
        aa.smooth = p->c3.smooth_factor2; aa.noise = p->c3.noise_threshold2;
        if ((rc = launch_alpha(aa, s))) return rc;
    }
    return launch_us_scale_scan(us_alphas, us_peaks, p->tok_dev.as<int>(), B, Tu, (float)((double)c.threshold - 1e-4), s);
}

}  // extern "C"
