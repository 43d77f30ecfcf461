// C-ABI layer, Paraformer-v2 posterior embedder: pf_posterior_embed_* and the pf_k_ctc_runs hook.
//
// The decoder input of Paraformer-v2 is made from the CTC head (funasr/models/paraformer_v2_community/model.py:451-482,545-574 and
// decoder.py:318-325): frame-wise softmax, greedy path, runs of one non-blank label, the mean posterior of each run, then
// Linear(V -> D), LayerNorm(1e-5), ReLU, x * sqrt(D) + pe. The first layer is linear and a run's weights sum to one, so
// Linear(mean_t p_t) = mean_t(p_t W^T) + b: the stage works in the FRAME domain -- E = probs W^T for every frame, in row chunks, then
// one small row kernel per token -- and needs neither a [B, N, V] buffer nor a run that straddles a row chunk.
#include <algorithm>

#include "ctc_merge.h"
#include "engine_internal.h"

namespace pf {

constexpr size_t PE_WORKSPACE_CAP = (size_t)256 << 20;   // logits / probabilities (and their planes) of one row chunk: a choice, not a tuned number
constexpr int PE_K_SLICE = 1024;                         // K = V goes in slices like the Conformer's output linear (engine_conformer.hip)
constexpr int PE_POS_ROWS = 5000;                        // PositionalEncoding(max_len = 5000)

struct PosteriorEmbed {
    int V = 0, Vp = 0, D = 0, blank = 0;
    TensorTable tt;
    int precision = 3;          // 0: both GEMMs on the exact-fp32 MFMA; 3: two-plane fp16 operands on the fp16 MFMA (fp32-class)
    int chunk_rows = 0;         // rows per chunk; 0 = from PE_WORKSPACE_CAP
    DevBuf probs, planes, h2, dsc, Ea, Eb, ids, lens, counts, ranges;
    int32_t* counts_pinned = nullptr; int pinned_cap = 0;
    const float* E = nullptr;   // what the last pf_posterior_embed_runs left: E [B * T, D] (in Ea or Eb), its counts and ranges
    int B = 0, T = 0;
    ~PosteriorEmbed() { if (counts_pinned) (void)hipHostFree(counts_pinned); }
};

// logits of rows [r0, r0 + m) -> probs (row stride Vp). x2: the f16x2 GEMM's epilogue writes columns in fours, so it computes columns
// [0, V4), V4 = V rounded down to a multiple of 4, and the last V - V4 <= 3 columns come from the exact-fp32 MFMA on the same borrowed
// weights (V = 261, 25055: one column). A rule of the vocabulary size, never of the batch.
static int pe_logits(PosteriorEmbed* h, Ctc* c, bool x2, const float* hidden, size_t M, size_t r0, int m, int ew, const unsigned short* w2,
                     hipStream_t s) {
    const int D = h->D, V = h->V;
    const int V4 = x2 ? V / 4 * 4 : 0;
    int rc;
    if (V4 > 0) {
        const float* dsc = h->dsc.as<float>();
        Gemm2Args g{};
        g.A = h->h2.as<unsigned short>() + r0 * D; g.lda = D; g.a_plane = M * D; g.W = w2; g.ldw = D; g.w_plane = (size_t)V * D;
        g.oscale = pow2f(-ew); g.oscale_dev = dsc + 2; g.bias = c->tt.get("ctc_lo.bias");
        g.C = h->probs.as<float>(); g.ldc = h->Vp; g.M = m; g.N = V4; g.K = D;
        ProfScope ps(PROF_GEMM3, 2.0 * m * (double)V4 * D, s, "pe.logits");
        if ((rc = launch_gemm_f16x2(g, s))) return rc;
    }
    if (V4 == V) return 0;
    GemmArgs g{};
    g.A = hidden + r0 * D; g.lda = D; g.W = c->tt.get("ctc_lo.weight") + (size_t)V4 * D; g.ldw = D; g.bias = c->tt.get("ctc_lo.bias") + V4;
    g.C = h->probs.as<float>() + V4; g.ldc = h->Vp; g.M = m; g.N = V - V4; g.K = D;
    ProfScope ps(PROF_GEMM, 2.0 * m * (double)(V - V4) * D, s, "pe.logits");
    return launch_gemm_f32(g, s);
}

// E[r0 .. r0 + m) = probs W0^T in K slices of PE_K_SLICE: a slice's chain starts at zero and the running sum rides in as the addend
// of the next launch (ping-pong between Ea and Eb: no in-place addend; fp32: gemm_f32_ksliced). Returns the buffer the last slice wrote.
static int pe_project(PosteriorEmbed* h, bool x2, size_t r0, int m, const float** out, hipStream_t s) {
    const int D = h->D, Vp = h->Vp;
    float* cur = h->Ea.as<float>() + r0 * D;
    float* prev = h->Eb.as<float>() + r0 * D;
    int ew = 0, rc;
    if (!x2) {
        if ((rc = gemm_f32_ksliced(h->probs.as<float>(), Vp, h->tt.get("embed.0.weight"), Vp, nullptr, m, D, Vp, PE_K_SLICE, cur, prev, out,
                                   "pe.project", s)))
            return rc;
        *out -= r0 * D;
        return 0;
    }
    const int e_a = exp_for_bound(1.f);                   // probabilities: |p| <= 1
    const size_t plane = (size_t)m * Vp;
    unsigned short* P = h->planes.as<unsigned short>();
    if ((rc = launch_split2(h->probs.as<float>(), Vp, P, Vp, plane, m, Vp, pow2f(e_a), s))) return rc;
    const unsigned short* W2 = h->tt.get_split2("embed.0.weight", D, Vp, &ew, s);
    if (!W2) return -2;
    for (int k0 = 0; k0 < Vp; k0 += PE_K_SLICE) {
        const int K = std::min(PE_K_SLICE, Vp - k0);
        ProfScope ps(PROF_GEMM3, 2.0 * m * (double)D * K, s, "pe.project");
        Gemm2Args g{};
        g.A = P + k0; g.lda = Vp; g.a_plane = plane; g.W = W2 + k0; g.ldw = Vp; g.w_plane = (size_t)D * Vp;
        g.oscale = pow2f(-(e_a + ew)); g.R1 = k0 == 0 ? nullptr : prev; g.ldr1 = D;
        g.C = cur; g.ldc = D; g.M = m; g.N = D; g.K = K;
        if ((rc = launch_gemm_f16x2(g, s))) return rc;
        std::swap(cur, prev);
    }
    *out = prev - r0 * D;                                  // (after the last swap `prev` is what was written last)
    return 0;
}

}  // namespace pf

using namespace pf;

extern "C" {

pf_posterior_embed* pf_posterior_embed_create(int32_t vocab, int32_t d_model, int32_t blank_id) {
    if (check_device()) return nullptr;
    if (vocab <= 0 || d_model <= 0 || d_model % 32 || d_model > 2048 || blank_id < 0 || blank_id >= vocab) {
        set_error("posterior_embed: vocab > 0, d_model % 32 == 0, d_model <= 2048 and 0 <= blank_id < vocab required");
        return nullptr;
    }
    std::unique_ptr<PosteriorEmbed> h(new PosteriorEmbed());
    h->V = vocab; h->Vp = round_up(vocab, 32); h->D = d_model; h->blank = blank_id;
    // embed.0.weight [D, V] is the [N, K] operand of E = probs W^T: its rows are zero-padded to K = Vp (a multiple of 32)
    if (h->tt.add_padded("embed.0.weight", d_model, vocab, h->Vp) || h->tt.add("embed.0.bias", d_model) ||
        h->tt.add("embed.1.weight", d_model) || h->tt.add("embed.1.bias", d_model) ||
        h->tt.add("pos_table", (int64_t)PE_POS_ROWS * d_model))
        return nullptr;
    return reinterpret_cast<pf_posterior_embed*>(h.release());
}
void pf_posterior_embed_destroy(pf_posterior_embed* h) { delete reinterpret_cast<PosteriorEmbed*>(h); }
int pf_posterior_embed_set_tensor(pf_posterior_embed* hh, const char* name, const float* data, int64_t numel) {
    PosteriorEmbed* h = reinterpret_cast<PosteriorEmbed*>(hh);
    PF_REQUIRE(h && name && data, "posterior_embed_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_posterior_embed_missing(const pf_posterior_embed* hh) {
    const PosteriorEmbed* h = reinterpret_cast<const PosteriorEmbed*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_posterior_embed_set_precision(pf_posterior_embed* hh, int32_t mode) {
    PosteriorEmbed* h = reinterpret_cast<PosteriorEmbed*>(hh);
    PF_REQUIRE(h && (mode == 0 || mode == 3), "posterior_embed_set_precision: mode must be 0 (fp32 MFMA) or 3 (fp32 via f16x2)");
    h->precision = mode;
    return 0;
}
int pf_posterior_embed_set_chunk_rows(pf_posterior_embed* hh, int32_t rows) {
    PosteriorEmbed* h = reinterpret_cast<PosteriorEmbed*>(hh);
    PF_REQUIRE(h && rows >= 0, "posterior_embed_set_chunk_rows: rows >= 0 (0: from the 256 MB workspace cap)");
    h->chunk_rows = rows;
    return 0;
}

/* test hook: fill every activation workspace of the handle with `byte` (a forward must not depend on what earlier batches left) */
int pf_posterior_embed_debug_poison(pf_posterior_embed* hh, int32_t byte) {
    PosteriorEmbed* h = reinterpret_cast<PosteriorEmbed*>(hh);
    PF_REQUIRE(h, "posterior_embed_debug_poison: null");
    for (DevBuf* b : {&h->probs, &h->planes, &h->h2, &h->Ea, &h->Eb, &h->ids, &h->counts, &h->ranges})
        if (b->p) PF_HIP_TRY(hipMemset(b->p, byte, b->cap));
    PF_HIP_TRY(hipDeviceSynchronize());
    h->E = nullptr;                                         // what pf_posterior_embed_runs left is gone
    return 0;
}

int pf_posterior_embed_runs(pf_posterior_embed* hh, pf_ctc* ch, const float* hidden, const int32_t* lens_host, int32_t B, int32_t T,
                            int32_t* counts_host, int32_t* path_dev, void* stream) {
    PosteriorEmbed* h = reinterpret_cast<PosteriorEmbed*>(hh);
    Ctc* c = reinterpret_cast<Ctc*>(ch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(h && c && hidden && lens_host && counts_host && B > 0 && T > 0, "posterior_embed_runs: null/empty");
    PF_REQUIRE(c->d_model == h->D && c->vocab == h->V, "posterior_embed_runs: the CTC head's d_model / vocab differ from the embedder's");
    PF_REQUIRE((long)B * T <= 0x7fffffffL / std::max(h->D, 2), "posterior_embed_runs: B * T * d_model must stay below 2^31");
    PF_REQUIRE(((uintptr_t)hidden & 15) == 0, "posterior_embed_runs: hidden must be 16-B aligned");
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= T, "posterior_embed_runs: lens out of range");
    if (c->tt.require_all("ctc") || h->tt.require_all("posterior_embed")) return -3;
    h->E = nullptr;
    const int D = h->D, V = h->V, Vp = h->Vp;
    const size_t M = (size_t)B * T;
    const bool x2 = h->precision == 3, x2_logits = x2 && V >= 4;
    size_t R = h->chunk_rows > 0 ? (size_t)h->chunk_rows : std::max<size_t>(1, PE_WORKSPACE_CAP / ((size_t)Vp * sizeof(float) * (x2 ? 2 : 1)));
    if (R > M) R = M;
    if (B > h->pinned_cap) {
        if (h->counts_pinned) { (void)hipHostFree(h->counts_pinned); h->counts_pinned = nullptr; h->pinned_cap = 0; }
        PF_HIP_TRY(hipHostMalloc((void**)&h->counts_pinned, sizeof(int32_t) * (size_t)round_up(B, 64)));
        h->pinned_cap = round_up(B, 64);
    }
    if (h->probs.ensure(sizeof(float) * R * Vp) || (x2 && h->planes.ensure(sizeof(unsigned short) * 2 * R * Vp)) ||
        h->Ea.ensure(sizeof(float) * M * D) || h->Eb.ensure(sizeof(float) * M * D) || h->ids.ensure(sizeof(int32_t) * M) ||
        h->counts.ensure(sizeof(int32_t) * (size_t)B) || h->ranges.ensure(sizeof(int32_t) * 2 * M))
        return -2;
    int rc, ew = 0;
    const unsigned short* w2 = nullptr;
    if (x2_logits) {
        // the route of pf_ctc_greedy: planes of the hidden states at a scale chosen on the device from max |hidden| over ALL rows (so
        // that a row's result does not depend on the chunking), the CTC handle's cached weight planes
        if (!(w2 = c->tt.get_split2("ctc_lo.weight", V, D, &ew, s))) return -2;
        if (h->h2.ensure(sizeof(unsigned short) * 2 * M * D) || h->dsc.ensure(sizeof(float) * 4)) return -2;
        float* dsc = h->dsc.as<float>();
        if ((rc = launch_absmax(hidden, M * D, dsc, s))) return rc;
        if ((rc = launch_pow2_scale(dsc, dsc + 1, s))) return rc;
        if ((rc = launch_split2(hidden, D, h->h2.as<unsigned short>(), D, M * D, (int)M, D, 1.f, s, dsc + 1))) return rc;
    }
    const float* E = nullptr;
    for (size_t r0 = 0; r0 < M; r0 += R) {
        const int m = (int)std::min(R, M - r0);
        if ((rc = pe_logits(h, c, x2_logits, hidden, M, r0, m, ew, w2, s))) return rc;
        if ((rc = launch_softmax_argmax_rows(h->probs.as<float>(), Vp, m, V, Vp, h->ids.as<int>() + r0, s))) return rc;
        if ((rc = pe_project(h, x2, r0, m, &E, s))) return rc;
    }
    if ((rc = upload_lens(h->lens, lens_host, B, s))) return rc;
    if ((rc = launch_ctc_runs(h->ids.as<int>(), h->lens.as<int>(), B, T, h->blank, h->counts.as<int>(), h->ranges.as<int>(), T, s))) return rc;
    if (path_dev) PF_HIP_TRY(hipMemcpyAsync(path_dev, h->ids.p, sizeof(int32_t) * M, hipMemcpyDeviceToDevice, s));
    // the stage's one host synchronisation: the run counts size the decoder (the counterpart of the CIF count in pf_predictor_alphas)
    PF_HIP_TRY(hipMemcpyAsync(h->counts_pinned, h->counts.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
    PF_HIP_TRY(hipStreamSynchronize(s));
    int N = 0;
    for (int b = 0; b < B; ++b) { counts_host[b] = h->counts_pinned[b]; N = std::max(N, (int)counts_host[b]); }
    h->E = E; h->B = B; h->T = T;
    return N;
}

int pf_posterior_embed_embeds(pf_posterior_embed* hh, int32_t B, int32_t T, int32_t N, float* embeds, int32_t* run_ranges, void* stream) {
    PosteriorEmbed* h = reinterpret_cast<PosteriorEmbed*>(hh);
    PF_REQUIRE(h && B > 0 && T > 0 && N >= 0, "posterior_embed_embeds: null/empty");
    PF_REQUIRE(h->E && B == h->B && T == h->T, "posterior_embed_embeds: B / T are not those of the last pf_posterior_embed_runs");
    if (N == 0) return 0;                                   // every clip blank: nothing to write
    PF_REQUIRE(embeds && N <= T && N <= PE_POS_ROWS, "posterior_embed_embeds: null output, or N above T / the 5000 positions of the table");
    PosteriorEmbedArgs a{};
    a.E = h->E; a.counts = h->counts.as<int>(); a.ranges = h->ranges.as<int>(); a.ld = T;
    a.bias = h->tt.get("embed.0.bias"); a.gamma = h->tt.get("embed.1.weight"); a.beta = h->tt.get("embed.1.bias"); a.pe = h->tt.get("pos_table");
    a.xscale = (float)std::sqrt((double)h->D); a.eps = 1e-5f;
    a.embeds = embeds; a.ranges_out = run_ranges; a.B = B; a.T = T; a.D = h->D; a.N = N;
    return launch_posterior_embed(a, reinterpret_cast<hipStream_t>(stream));
}

/* the run scan alone on caller-provided paths (tests): ids_dev int32 [B, T], lens_host [B] (0 .. T) -> counts_dev int32 [B],
 * ranges_dev int32 [B, ld, 2] (runs j >= min(count, ld) are left as they were). Synchronises (the upload reads the host array). */
int pf_k_ctc_runs(const int32_t* ids_dev, const int32_t* lens_host, int32_t B, int32_t T, int32_t blank, int32_t* counts_dev,
                  int32_t* ranges_dev, int32_t ld, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(ids_dev && lens_host && counts_dev && ranges_dev && B > 0 && T > 0 && ld > 0, "k_ctc_runs: null/empty");
    for (int b = 0; b < B; ++b) PF_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= T, "k_ctc_runs: lens out of range");
    static DevBuf ln;
    int rc;
    if ((rc = upload_lens(ln, lens_host, B, s))) return rc;
    if ((rc = launch_ctc_runs(ids_dev, ln.as<int>(), B, T, blank, counts_dev, ranges_dev, ld, s))) return rc;
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
