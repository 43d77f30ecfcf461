// C-ABI layer of the Transducer (RNN-T): the pf_transducer handle and the search loop. The loop is a behavioural restatement of
// funasr/models/transducer/beam_search_transducer.py:272-366 (default_beam_search) as the reference's Transducer drives it
// (transducer/model.py:481-486,550: one utterance, is_final, no LM, sort_nbest without length normalisation), on the host side of the
// library: per expansion a prediction step only for a label prefix not seen in this utterance (RNNTDecoder.score's cache becomes a
// map from prefix to state slot), two launches of the joint step and one read-back of its 1 + 2 k words.
//
// State slots: [slot][layer][h | c][H] and [slot][J] (dec_proj = lin_dec . h' of the last layer), slot 0 the zero initial state. The
// pool grows by chunks of SLOT_CHUNK slots, each its own allocation, so a long utterance cannot overrun a size guessed up front and
// growing moves nothing that queued kernels read.
//
// The reference's `while True` has no guard; here a non-finite joint record and a per-frame expansion cap end the search with a code.
#include <algorithm>

#include "engine_internal.h"
#include "transducer.h"

namespace pf {

namespace {

constexpr int SLOT_CHUNK = 256;

struct Transducer {
    pf_transducer_config cfg;
    TensorTable tt;
    std::vector<float*> state_chunks, proj_chunks;      // [SLOT_CHUNK][L][2][H] and [SLOT_CHUNK][J] each
    DevBuf enc_proj, partials, record;
    float* host_record = nullptr;                       // pinned [1 + 2 RNNT_MAX_K]
    std::string error;                                  // of the last search
    ~Transducer() {
        for (float* p : state_chunks) (void)hipFree(p);
        for (float* p : proj_chunks) (void)hipFree(p);
        if (host_record) (void)hipHostFree(host_record);
    }
    size_t slot_floats() const { return (size_t)cfg.n_layers * 2 * cfg.hidden; }
    float* state(int slot) { return state_chunks[slot / SLOT_CHUNK] + (size_t)(slot % SLOT_CHUNK) * slot_floats(); }
    float* proj(int slot) { return proj_chunks[slot / SLOT_CHUNK] + (size_t)(slot % SLOT_CHUNK) * cfg.joint_dim; }
    int ensure_slots(int n) {
        while ((int)state_chunks.size() * SLOT_CHUNK < n) {
            float *s = nullptr, *p = nullptr;
            PF_HIP_TRY(hipMalloc((void**)&s, sizeof(float) * SLOT_CHUNK * slot_floats()));
            state_chunks.push_back(s);
            PF_HIP_TRY(hipMalloc((void**)&p, sizeof(float) * SLOT_CHUNK * (size_t)cfg.joint_dim));
            proj_chunks.push_back(p);
        }
        return 0;
    }
};

std::string layer_name(int l, const char* what) { return "decoder.rnn." + std::to_string(l) + "." + what; }

// one prediction step: slot src + label -> slot dst (n_layers cell launches, then dec_proj)
int pred_step(Transducer* h, int label, int src, int dst, hipStream_t s) {
    const pf_transducer_config& c = h->cfg;
    const int H = c.hidden;
    const float* x = h->tt.get("decoder.embed.weight") + (size_t)label * c.embed_dim;
    int in_dim = c.embed_dim, rc;
    float* out = h->state(dst);
    const float* in = h->state(src);
    for (int l = 0; l < c.n_layers; ++l) {
        RnntCellArgs a{};
        a.x = x; a.in_dim = in_dim; a.H = H;
        a.w_ih = h->tt.get(layer_name(l, "weight_ih_l0")); a.w_hh = h->tt.get(layer_name(l, "weight_hh_l0"));
        a.b_ih = h->tt.get(layer_name(l, "bias_ih_l0")); a.b_hh = h->tt.get(layer_name(l, "bias_hh_l0"));
        a.h_prev = in + (size_t)l * 2 * H; a.c_prev = a.h_prev + H;
        a.h_out = out + (size_t)l * 2 * H; a.c_out = a.h_out + H;
        if ((rc = launch_rnnt_cell(a, s))) return rc;
        x = a.h_out; in_dim = H;
    }
    return launch_rnnt_matvec(h->tt.get("joint_network.lin_dec.weight"), x, h->proj(dst), c.joint_dim, H, s);
}

struct Hyp {
    double score;
    std::vector<int32_t> ids;
    int parent;              // the slot holding the state BEFORE ids.back() was consumed (the reference's hyp.dec_state)
};

// the first of the largest scores, in list order (Python's max)
size_t argmax_first(const std::vector<Hyp>& v) {
    size_t best = 0;
    for (size_t i = 1; i < v.size(); ++i) if (v[i].score > v[best].score) best = i;
    return best;
}

int search(Transducer* h, const float* enc_out, int T, int beam, int nbest, int cap, int32_t* ids_out, int32_t* lens_out, double* scores_out,
           int max_len, int32_t* n_out, int64_t* stats, hipStream_t s) {
    const pf_transducer_config& c = h->cfg;
    const int J = c.joint_dim, V = c.vocab, k = std::min(beam, V - 1);
    int rc;
    if ((rc = h->tt.require_all("transducer"))) return rc;
    if (h->enc_proj.ensure(sizeof(float) * (size_t)T * J) || h->partials.ensure(sizeof(float) * rnnt_joint_partial_floats(V, k)) ||
        h->record.ensure(sizeof(float) * (1 + 2 * RNNT_MAX_K)) || h->ensure_slots(2))
        return -2;
    // enc_proj = lin_enc(enc_out) for all T frames: one exact-fp32 GEMM before the search starts
    GemmArgs g{};
    g.A = enc_out; g.lda = c.enc_dim; g.W = h->tt.get("joint_network.lin_enc.weight"); g.ldw = c.enc_dim;
    g.bias = h->tt.get("joint_network.lin_enc.bias"); g.C = h->enc_proj.as<float>(); g.ldc = J; g.M = T; g.N = J; g.K = c.enc_dim;
    if ((rc = launch_gemm_f32(g, s))) return rc;
    PF_HIP_TRY(hipMemsetAsync(h->state(0), 0, sizeof(float) * h->slot_floats(), s));       // slot 0: init_state

    std::map<std::vector<int32_t>, int> cache;          // label prefix -> slot; dropped at the end (reset_inference_cache)
    int n_slots = 1;
    std::vector<Hyp> kept{Hyp{0.0, {0}, 0}}, hyps;
    const int words = 1 + 2 * k;
    const float* rec = h->host_record;
    const int32_t* rec_i = reinterpret_cast<const int32_t*>(h->host_record);
    for (int t = 0; t < T; ++t) {
        hyps.swap(kept);
        kept.clear();
        int64_t frame_evals = 0;
        while (true) {
            const size_t at = argmax_first(hyps);
            Hyp mx = std::move(hyps[at]);
            hyps.erase(hyps.begin() + at);
            if (frame_evals >= cap) {
                h->error = "transducer search: frame " + std::to_string(t) + " of " + std::to_string(T) + " needs more than " +
                           "max_expansions_per_frame = " + std::to_string(cap) + " joint evaluations (the search does not settle: " +
                           "the output layer rarely prefers blank)";
                set_error(h->error);
                return PF_TRANSDUCER_CAP;
            }
            int slot;
            auto it = cache.find(mx.ids);
            if (it != cache.end()) {
                slot = it->second;
            } else {
                slot = n_slots++;
                if (h->ensure_slots(n_slots)) return -2;
                if ((rc = pred_step(h, mx.ids.back(), mx.parent, slot, s))) return rc;
                cache.emplace(mx.ids, slot);
                ++stats[1];
            }
            RnntJointArgs ja{};
            ja.enc_proj = h->enc_proj.as<float>() + (size_t)t * J; ja.dec_proj = h->proj(slot);
            ja.w_out = h->tt.get("joint_network.lin_out.weight"); ja.b_out = h->tt.get("joint_network.lin_out.bias");
            ja.partials = h->partials.as<float>(); ja.record = h->record.as<float>(); ja.V = V; ja.J = J; ja.k = k;
            if ((rc = launch_rnnt_joint_topk(ja, s))) return rc;
            PF_HIP_TRY(hipMemcpyAsync(h->host_record, h->record.p, sizeof(float) * words, hipMemcpyDeviceToHost, s));
            PF_HIP_TRY(hipStreamSynchronize(s));
            ++stats[0];
            ++frame_evals;
            if (frame_evals > stats[2]) stats[2] = frame_evals;
            bool ok = true;
            for (int i = 0; i <= k; ++i) ok = ok && std::isfinite(rec[i]);
            for (int i = 0; i < k; ++i) ok = ok && rec_i[1 + k + i] >= 1 && rec_i[1 + k + i] < V;
            if (!ok) {
                h->error = "transducer search: non-finite joint output at frame " + std::to_string(t) +
                           " (NaN or inf in the encoder output or the weights)";
                set_error(h->error);
                return PF_TRANSDUCER_NONFINITE;
            }
            kept.push_back(Hyp{mx.score + (double)rec[0], mx.ids, mx.parent});
            for (int i = 0; i < k; ++i) {
                Hyp n{mx.score + (double)rec[1 + i], mx.ids, slot};
                n.ids.push_back(rec_i[1 + k + i]);
                hyps.push_back(std::move(n));
            }
            const double hyps_max = hyps[argmax_first(hyps)].score;
            std::vector<Hyp> most;
            for (const Hyp& x : kept) if (x.score > hyps_max) most.push_back(x);
            if ((int)most.size() >= beam) {
                std::stable_sort(most.begin(), most.end(), [](const Hyp& a, const Hyp& b) { return a.score < b.score; });
                kept.swap(most);
                break;
            }
        }
    }
    std::stable_sort(kept.begin(), kept.end(), [](const Hyp& a, const Hyp& b) { return a.score > b.score; });   // sort_nbest
    const int n = std::min<int>(nbest, (int)kept.size());
    for (int i = 0; i < n; ++i) {
        const int len = (int)kept[i].ids.size();
        lens_out[i] = len;
        scores_out[i] = kept[i].score;
        if (len > max_len) {
            h->error = "transducer search: a hypothesis of " + std::to_string(len) + " labels does not fit max_len = " + std::to_string(max_len);
            set_error(h->error);
            return -1;
        }
        std::copy(kept[i].ids.begin(), kept[i].ids.end(), ids_out + (size_t)i * max_len);
    }
    *n_out = n;
    return 0;
}

}  // namespace

}  // namespace pf

using namespace pf;

extern "C" {

pf_transducer* pf_transducer_create(const pf_transducer_config* cfg) {
    if (!cfg) { set_error("transducer: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_transducer_config& c = *cfg;
    auto dim = [](int d) { return d >= 4 && d % 4 == 0 && d <= RNNT_MAX_DIM; };
    const char* bad = nullptr;
    if (c.vocab < 2 || c.vocab > 65536) bad = "vocab (2 .. 65536)";
    else if (!dim(c.enc_dim) || c.enc_dim % 32 != 0) bad = "enc_dim (a multiple of 32, at most 1024)";
    else if (!dim(c.embed_dim)) bad = "embed_dim (a multiple of 4, at most 1024)";
    else if (!dim(c.hidden)) bad = "hidden (a multiple of 4, at most 1024)";
    else if (!dim(c.joint_dim)) bad = "joint_dim (a multiple of 4, at most 1024)";
    else if (c.n_layers < 1 || c.n_layers > 4) bad = "n_layers (1 .. 4)";
    else if (c.blank_id != 0) bad = "blank_id (only 0: the search takes row 0 as the blank)";
    if (bad) { set_error(std::string("transducer: unsupported config: ") + bad); return nullptr; }
    std::unique_ptr<Transducer> h(new Transducer());
    h->cfg = c;
    int rc = 0;
    rc |= h->tt.add("decoder.embed.weight", (int64_t)c.vocab * c.embed_dim);
    for (int l = 0; l < c.n_layers; ++l) {
        rc |= h->tt.add(layer_name(l, "weight_ih_l0"), (int64_t)4 * c.hidden * (l == 0 ? c.embed_dim : c.hidden));
        rc |= h->tt.add(layer_name(l, "weight_hh_l0"), (int64_t)4 * c.hidden * c.hidden);
        rc |= h->tt.add(layer_name(l, "bias_ih_l0"), (int64_t)4 * c.hidden);
        rc |= h->tt.add(layer_name(l, "bias_hh_l0"), (int64_t)4 * c.hidden);
    }
    rc |= h->tt.add("joint_network.lin_enc.weight", (int64_t)c.joint_dim * c.enc_dim);
    rc |= h->tt.add("joint_network.lin_enc.bias", c.joint_dim);
    rc |= h->tt.add("joint_network.lin_dec.weight", (int64_t)c.joint_dim * c.hidden);
    rc |= h->tt.add("joint_network.lin_out.weight", (int64_t)c.vocab * c.joint_dim);
    rc |= h->tt.add("joint_network.lin_out.bias", c.vocab);
    if (rc) return nullptr;
    if (hipHostMalloc((void**)&h->host_record, sizeof(float) * (1 + 2 * RNNT_MAX_K), hipHostMallocDefault) != hipSuccess) {
        set_error("transducer: pinned read-back buffer");
        return nullptr;
    }
    return reinterpret_cast<pf_transducer*>(h.release());
}
void pf_transducer_destroy(pf_transducer* h) { delete reinterpret_cast<Transducer*>(h); }
int pf_transducer_set_weights(pf_transducer* hh, const char* name, const float* data, int64_t numel) {
    Transducer* h = reinterpret_cast<Transducer*>(hh);
    PF_REQUIRE(h && name && data, "transducer_set_weights: null");
    return h->tt.set(name, data, numel);
}
int pf_transducer_missing(const pf_transducer* hh) {
    const Transducer* h = reinterpret_cast<const Transducer*>(hh);
    return h ? h->tt.missing() : -1;
}
const char* pf_transducer_last_error(const pf_transducer* hh) {
    const Transducer* h = reinterpret_cast<const Transducer*>(hh);
    return h ? h->error.c_str() : "";
}
int pf_transducer_search(pf_transducer* hh, const float* enc_out, int32_t T, int32_t beam, int32_t nbest, int32_t max_expansions_per_frame,
                         int32_t* ids_out, int32_t* lens_out, double* scores_out, int32_t max_len, int32_t* n_out, int64_t* stats_out,
                         void* stream) {
    Transducer* h = reinterpret_cast<Transducer*>(hh);
    PF_REQUIRE(h && enc_out && ids_out && lens_out && scores_out && n_out, "transducer_search: null");
    PF_REQUIRE(T >= 1 && nbest >= 1 && max_len >= 1, "transducer_search: T, nbest and max_len must be positive");
    PF_REQUIRE(beam >= 1 && beam <= RNNT_MAX_K, "transducer_search: beam_size must be 1 .. 16");
    PF_REQUIRE(beam <= h->cfg.vocab, "transducer_search: beam_size above the vocabulary size");
    int64_t stats[3] = {0, 0, 0};
    *n_out = 0;
    h->error.clear();
    const int cap = max_expansions_per_frame > 0 ? max_expansions_per_frame : 64 * beam;
    const int rc = search(h, enc_out, T, beam, nbest, cap, ids_out, lens_out, scores_out, max_len, n_out, stats,
                          reinterpret_cast<hipStream_t>(stream));
    if (rc && h->error.empty()) h->error = get_error();
    if (stats_out) std::copy(stats, stats + 3, stats_out);
    return rc;
}

int pf_k_rnnt_pred_step(const float* embed, const float* weights, const float* lin_dec, float* state, float* dec_proj, int32_t n_slots,
                        int32_t V, int32_t E, int32_t H, int32_t L, int32_t J, int32_t label, int32_t src, int32_t dst, void* stream) {
    PF_REQUIRE(embed && weights && lin_dec && state && dec_proj, "rnnt_pred_step: null");
    PF_REQUIRE(L >= 1 && L <= 4 && V >= 1 && E >= 4 && H >= 4 && J >= 4, "rnnt_pred_step: 1 .. 4 layers, positive sizes");
    PF_REQUIRE(E % 4 == 0 && H % 4 == 0 && J % 4 == 0, "rnnt_pred_step: sizes must be multiples of 4");
    PF_REQUIRE(label >= 0 && label < V, "rnnt_pred_step: label outside the embedding table");
    PF_REQUIRE(n_slots >= 2 && src >= 0 && src < n_slots && dst >= 0 && dst < n_slots, "rnnt_pred_step: slot outside the pool");
    PF_REQUIRE(src != dst, "rnnt_pred_step: src == dst (a step writes another slot than it reads)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t slot = (size_t)L * 2 * H;
    const float* x = embed + (size_t)label * E;
    const float* w = weights;
    int in_dim = E, rc;
    for (int l = 0; l < L; ++l) {
        RnntCellArgs a{};
        a.x = x; a.in_dim = in_dim; a.H = H;
        a.w_ih = w; w += (size_t)4 * H * in_dim;
        a.w_hh = w; w += (size_t)4 * H * H;
        a.b_ih = w; w += (size_t)4 * H;
        a.b_hh = w; w += (size_t)4 * H;
        a.h_prev = state + src * slot + (size_t)l * 2 * H; a.c_prev = a.h_prev + H;
        a.h_out = state + dst * slot + (size_t)l * 2 * H; a.c_out = a.h_out + H;
        if ((rc = launch_rnnt_cell(a, s))) return rc;
        x = a.h_out; in_dim = H;
    }
    return launch_rnnt_matvec(lin_dec, x, dec_proj + (size_t)dst * J, J, H, s);
}
int64_t pf_k_rnnt_joint_partial_floats(int32_t V, int32_t k) {
    return V >= 1 && k >= 1 ? (int64_t)rnnt_joint_partial_floats(V, k) : -1;
}
int pf_k_rnnt_joint_topk(const float* enc_proj, const float* dec_proj, const float* w_out, const float* b_out, int32_t V, int32_t J, int32_t k,
                         float* partials, float* record, void* stream) {
    RnntJointArgs a{};
    a.enc_proj = enc_proj; a.dec_proj = dec_proj; a.w_out = w_out; a.b_out = b_out; a.partials = partials; a.record = record;
    a.V = V; a.J = J; a.k = k;
    return launch_rnnt_joint_topk(a, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
