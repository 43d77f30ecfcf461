// C-ABI layer, keyword spotting: pf_kws_candidates (the per-frame candidate step on the device, kws.hip), pf_kws_search (the CTC
// prefix search over keyword tokens and the hit test: host code, no device work, usable without a GPU) and the single-kernel hooks
// of the memory block. The FSMN network itself is pf_vad (engine_vad.hip: pf_vad_logits).
//
// pf_kws_search restates KwsCtcPrefixDecoder.beam_search / is_sublist / _decode_inside (funasr/utils/kws_utils.py:125-292) with
// score_beam_size 3 (the candidate step) and path_beam_size 20. The reference's hypotheses carry LISTS OF DICTS whose copies are
// shallow: a node is one object that every hypothesis descended from it points at, and `nodes[-1]['prob'] = ps` changes it for
// all of them. Here a node is a record in a pool and a hypothesis holds indices; copying a list copies indices, a mutation writes
// the pool. Probabilities arrive as fp32 and everything after that is double, as `.item()` and Python floats make it there.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <map>

using namespace pf;

namespace {

constexpr int KWS_PATH_BEAM = 20;

struct KwsNode { int token, frame; double prob; };
struct KwsHyp {
    std::vector<int> prefix;
    double pb = 0.0, pnb = 0.0;
    std::vector<int> nodes;                 // indices into the clip's pool
};
struct KwsClip {
    std::vector<KwsNode> pool;
    std::vector<KwsHyp> hyps;               // final order
};
struct KwsSearch {
    int vocab;
    std::vector<std::vector<int>> keywords;
    bool keywords_set = false;
    std::vector<KwsClip> clips;             // of the last decode
};

#pragma clang fp contract(off)

// `not math.isclose(p, 0.0, abs_tol=1e-6)`
inline bool not_close_to_zero(double p) { return !(std::fabs(p) <= 1e-6); }

// rec: [T, 7] words of one clip (n, ids[3], fp32 bits of probs[3])
void kws_beam_search(const int32_t* rec, int T, KwsClip& clip) {
    clip.pool.clear();
    std::vector<KwsHyp> cur(1);
    cur[0].pb = 1.0;
    std::vector<KwsHyp> next;
    std::map<std::vector<int>, int> index;
    auto entry = [&](const std::vector<int>& prefix) -> int {          // next_hyps[prefix] of a defaultdict: insertion order kept
        auto it = index.find(prefix);
        if (it != index.end()) return it->second;
        next.emplace_back();
        next.back().prefix = prefix;
        index.emplace(prefix, (int)next.size() - 1);
        return (int)next.size() - 1;
    };
    for (int t = 0; t < T; ++t) {
        const int32_t* r = rec + (size_t)t * 7;
        const int n = r[0];
        if (n <= 0) continue;                                          // no kept candidate: neither re-sorted nor pruned
        next.clear();
        index.clear();
        for (int k = 0; k < n && k < 3; ++k) {
            const int s = r[1 + k];
            float pf32;
            memcpy(&pf32, &r[4 + k], sizeof(float));
            const double ps = (double)pf32;
            for (size_t h = 0; h < cur.size(); ++h) {
                const KwsHyp& c = cur[h];
                const int last = c.prefix.empty() ? -1 : c.prefix.back();
                if (s == 0) {
                    KwsHyp& e = next[entry(c.prefix)];
                    e.pb = e.pb + c.pb * ps + c.pnb * ps;
                    e.nodes = c.nodes;
                } else if (s == last) {
                    if (not_close_to_zero(c.pnb)) {                    // *ss -> *s
                        KwsHyp& e = next[entry(c.prefix)];
                        e.pnb = e.pnb + c.pnb * ps;
                        e.nodes = c.nodes;
                        KwsNode& nd = clip.pool[e.nodes.back()];
                        if (ps > nd.prob) { nd.prob = ps; nd.frame = t; }
                    }
                    if (not_close_to_zero(c.pb)) {                     // *s-s -> *ss
                        std::vector<int> np = c.prefix;
                        np.push_back(s);
                        KwsHyp& e = next[entry(np)];
                        e.pnb = e.pnb + c.pb * ps;
                        e.nodes = c.nodes;
                        clip.pool.push_back({s, t, ps});
                        e.nodes.push_back((int)clip.pool.size() - 1);
                    }
                } else {
                    std::vector<int> np = c.prefix;
                    np.push_back(s);
                    KwsHyp& e = next[entry(np)];
                    if (!e.nodes.empty()) {                            // already there: ITS last node is updated in place
                        KwsNode& nd = clip.pool[e.nodes.back()];
                        if (ps > nd.prob) { nd.prob = ps; nd.frame = t; }
                    } else {
                        e.nodes = c.nodes;
                        clip.pool.push_back({s, t, ps});
                        e.nodes.push_back((int)clip.pool.size() - 1);
                    }
                    e.pnb = e.pnb + c.pb * ps + c.pnb * ps;
                }
            }
        }
        std::stable_sort(next.begin(), next.end(), [](const KwsHyp& a, const KwsHyp& b) { return a.pb + a.pnb > b.pb + b.pnb; });
        if ((int)next.size() > KWS_PATH_BEAM) next.resize(KWS_PATH_BEAM);
        cur.swap(next);
    }
    clip.hyps.swap(cur);
}

// is_sublist: equal lengths -> whole-list equality; otherwise the first offset with a full match
int kws_is_sublist(const std::vector<int>& main_list, const std::vector<int>& check) {
    if (main_list.size() < check.size()) return -1;
    if (main_list.size() == check.size()) return main_list == check ? 0 : -1;
    for (size_t i = 0; i + check.size() <= main_list.size(); ++i)
        if (std::equal(check.begin(), check.end(), main_list.begin() + i)) return (int)i;
    return -1;
}

}  // namespace

extern "C" {

/* logits_dev [M, V] at row stride ld -> out_dev [M, 7] words per row: n <= 3, ids[3], fp32 bits of probs[3] */
int pf_kws_candidates(const float* logits, int64_t ld, int32_t M, int32_t V, const uint32_t* mask, int32_t* out, void* stream) {
    PF_REQUIRE(ld >= 0 && ld <= INT32_MAX, "kws_candidates: row stride");
    return launch_kws_candidates(logits, (long)ld, M, V, mask, out, reinterpret_cast<hipStream_t>(stream));
}

pf_kws_search* pf_kws_search_create(int32_t vocab_size) {
    if (vocab_size < 3) {
        set_error("kws_search: V < 3 (the candidate step takes the top 3 of a row; torch.topk(3) raises there)");
        return nullptr;
    }
    KwsSearch* k = new KwsSearch();
    k->vocab = vocab_size;
    return reinterpret_cast<pf_kws_search*>(k);
}
void pf_kws_search_destroy(pf_kws_search* h) { delete reinterpret_cast<KwsSearch*>(h); }
int pf_kws_search_set_keywords(pf_kws_search* h, const int32_t* ids, const int32_t* offsets, int32_t n_keywords) {
    KwsSearch* k = reinterpret_cast<KwsSearch*>(h);
    PF_REQUIRE(k && ids && offsets && n_keywords >= 1, "kws_search_set_keywords: null/empty argument");
    std::vector<std::vector<int>> kw(n_keywords);
    for (int i = 0; i < n_keywords; ++i) {
        PF_REQUIRE(offsets[i + 1] > offsets[i], "kws_search_set_keywords: a keyword without tokens");
        for (int j = offsets[i]; j < offsets[i + 1]; ++j) {
            PF_REQUIRE(ids[j] >= 0 && ids[j] < k->vocab, "kws_search_set_keywords: token id outside the vocabulary");
            kw[i].push_back(ids[j]);
        }
    }
    k->keywords.swap(kw);
    k->keywords_set = true;
    return 0;
}
int pf_kws_search_missing(const pf_kws_search* h) {
    const KwsSearch* k = reinterpret_cast<const KwsSearch*>(h);
    return k ? (k->keywords_set ? 0 : 1) : -1;
}
int pf_kws_search_token_mask(const pf_kws_search* h, uint32_t* mask, int32_t n_words) {
    const KwsSearch* k = reinterpret_cast<const KwsSearch*>(h);
    PF_REQUIRE(k && mask && k->keywords_set, "kws_search_token_mask: null argument, or no keywords set");
    PF_REQUIRE(n_words == (k->vocab + 31) / 32, "kws_search_token_mask: ceil(V / 32) words");
    for (int i = 0; i < n_words; ++i) mask[i] = 0;
    mask[0] |= 1u;                                                     // blank
    for (const auto& kw : k->keywords)
        for (int id : kw) mask[id >> 5] |= 1u << (id & 31);
    return 0;
}
int pf_kws_search_decode(pf_kws_search* h, const int32_t* cand, const int32_t* lens, int32_t B, int32_t T, int32_t* hit,
                         int32_t* offset, double* score) {
    KwsSearch* k = reinterpret_cast<KwsSearch*>(h);
    PF_REQUIRE(k && cand && lens && hit && score && B > 0 && T > 0, "kws_search_decode: null/empty argument");
    PF_REQUIRE(k->keywords_set, "kws_search_decode: no keywords set");
    for (int b = 0; b < B; ++b) {
        PF_REQUIRE(lens[b] >= 0 && lens[b] <= T, "kws_search_decode: a length outside 0 .. T");
        for (int t = 0; t < lens[b]; ++t) {
            const int32_t* r = cand + ((size_t)b * T + t) * 7;
            PF_REQUIRE(r[0] >= 0 && r[0] <= 3, "kws_search_decode: a candidate count outside 0 .. 3");
            for (int j = 0; j < r[0]; ++j)
                PF_REQUIRE(r[1 + j] >= 0 && r[1 + j] < k->vocab, "kws_search_decode: a candidate id outside the vocabulary");
        }
    }
    k->clips.assign(B, KwsClip());
    for (int b = 0; b < B; ++b) {
        KwsClip& clip = k->clips[b];
        kws_beam_search(cand + (size_t)b * T * 7, lens[b], clip);
        hit[b] = -1;
        if (offset) offset[b] = -1;
        score[b] = 0.0;
        for (const KwsHyp& hyp : clip.hyps) {                          // hypotheses in final order, keywords in the order given
            double sc = 1.0;
            for (size_t w = 0; w < k->keywords.size() && hit[b] < 0; ++w) {
                const int off = kws_is_sublist(hyp.prefix, k->keywords[w]);
                if (off < 0) continue;
                hit[b] = (int)w;
                if (offset) offset[b] = off;
                for (size_t i = off; i < off + k->keywords[w].size(); ++i) sc *= clip.pool[hyp.nodes[i]].prob;
            }
            if (hit[b] >= 0) { score[b] = std::sqrt(sc); break; }
        }
    }
    return 0;
}
int pf_kws_search_nbest_count(const pf_kws_search* h, int32_t clip) {
    const KwsSearch* k = reinterpret_cast<const KwsSearch*>(h);
    if (!k || clip < 0 || clip >= (int)k->clips.size()) return -1;
    return (int)k->clips[clip].hyps.size();
}
int pf_kws_search_nbest(const pf_kws_search* h, int32_t clip, int32_t i, int32_t capacity, int32_t* prefix, double* score,
                        int32_t* node_token, int32_t* node_frame, double* node_prob) {
    const KwsSearch* k = reinterpret_cast<const KwsSearch*>(h);
    if (!k || clip < 0 || clip >= (int)k->clips.size() || i < 0 || i >= (int)k->clips[clip].hyps.size()) {
        set_error("kws_search_nbest: no such clip / hypothesis");
        return -1;
    }
    const KwsClip& c = k->clips[clip];
    const KwsHyp& hyp = c.hyps[i];
    const int n = (int)hyp.prefix.size();
    if (hyp.nodes.size() != hyp.prefix.size()) { set_error("kws_search_nbest: prefix and nodes differ in length"); return -1; }
    if (score) *score = hyp.pb + hyp.pnb;
    if (n > capacity) return n;                                        // the caller sizes its arrays and calls again
    for (int j = 0; j < n; ++j) {
        if (prefix) prefix[j] = hyp.prefix[j];
        const KwsNode& nd = c.pool[hyp.nodes[j]];
        if (node_token) node_token[j] = nd.token;
        if (node_frame) node_frame[j] = nd.frame;
        if (node_prob) node_prob[j] = nd.prob;
    }
    return n;
}

/* the memory block alone (dense [B, T, C] rows at strides ldx / ldy): rorder 0 is the left-only block */
int pf_k_kws_fsmn(const float* x, int32_t ldx, const float* w_left, const float* w_right, float* y, int32_t ldy, int32_t B, int32_t T,
                  int32_t C, int32_t lorder, int32_t lstride, int32_t rorder, int32_t rstride, void* stream) {
    return launch_kws_fsmn(x, ldx, w_left, w_right, y, ldy, B, T, C, lorder, lstride, rorder, rstride > 0 ? rstride : 1,
                           reinterpret_cast<hipStream_t>(stream));
}
/* the VAD network's left-only block without a cache: what pf_k_kws_fsmn with rorder 0 must equal bit for bit */
int pf_k_vad_fsmn(const float* x, int32_t ldx, const float* w_left, float* y, int32_t ldy, int32_t B, int32_t T, int32_t C,
                  int32_t lorder, int32_t lstride, void* stream) {
    PF_REQUIRE(x && w_left && y && ldx >= C && ldy >= C, "k_vad_fsmn: null argument / stride < C");
    return launch_vad_fsmn(x, ldx, w_left, nullptr, nullptr, y, ldy, B, T, C, lorder, lstride, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
