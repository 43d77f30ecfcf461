// C-ABI layer, Qwen3 causal LM decoder with a KV cache (the LM of funasr/models/fun_asr_nano/model.py): pf_qwen3_* and the
// pf_k_qwen3_* hooks (kernels in qwen3.hip; every projection is the exact-fp32 GEMM of gemm_f32.hip / gemm_skinny.hip, the vocabulary
// projection the fused GEMM + arg-max of engine_decoder.hip).
//
// Load time (prepare(), again whenever the table version moves): q_proj | k_proj | v_proj and gate_proj | up_proj are concatenated row-wise
// into one weight each, so the three / two projections are one launch.
//
// Rows: a batch is B <= 16 sequences, each at its own length, with no padding rows: the activations are [M, width] with per-row
// (cache slot, position) beside them. Prefill: M = sum of the prompts' rows, tile GEMMs. Decode step: M = sequences still running, small-M
// weight-streaming GEMMs (StreamModeScope). Per layer:
//   RMSNorm X -> XN; XN Wqkv^T -> QKV; q/k norm + RoPE: QKV -> Q, cache; attention (prefill: 1 launch, step: 2) -> ATT;
//   ATT Wo^T + X -> X2; RMSNorm X2 -> XN; XN Wgu^T -> GU; SwiGLU GU -> ACT; ACT Wdown^T + X2 -> X
// then the last rows (prefill) or all rows (step): RMSNorm, vocabulary GEMM with the arg-max in its epilogue, partials -> ids, ids -> host.
#include <algorithm>

#include "engine_internal.h"
#include "qwen3.h"

using namespace pf;

namespace {

constexpr int Q3_MAX_B = 16;

struct Q3Layer { const float *ln1, *qkv, *qn, *kn, *o, *ln2, *gu, *down; };

struct Q3 {
    pf_qwen3_config cfg;
    TensorTable tt;
    unsigned long long prepared_for = TensorTable::NOT_PREPARED;
    std::vector<Q3Layer> layers;
    const float *embed = nullptr, *norm = nullptr, *head = nullptr;
    DevBuf kc, vc, cos_t, sin_t;
    int rope_rows = 0;
    DevBuf x, x2, xn, qkv, q, att, gu, act, part, meta, last, ids, pval, pidx;
    // the batch of the last prefill: sequences, positions the cache holds per sequence, their lengths and last ids
    int B = 0, cap = 0;
    int len[Q3_MAX_B];
    int32_t cur[Q3_MAX_B];

    int nqkv() const { return (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim; }
    size_t layer_floats() const { return (size_t)B * cfg.n_kv_heads * cap * cfg.head_dim; }
    int prepare();
};

std::string lname(int i) { return "model.layers." + std::to_string(i) + "."; }

int Q3::prepare() {
    const pf_qwen3_config& c = cfg;
    layers.assign(c.n_layers, Q3Layer{});
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string p = lname(i), kq = "d.L" + std::to_string(i) + ".qkv", kg = "d.L" + std::to_string(i) + ".gate_up";
        std::vector<float> cat;
        for (const char* n : {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"}) {
            const std::vector<float> w = tt.host(p + n);
            if (w.empty()) { set_error("qwen3: weight preparation failed (HIP copy)"); return -2; }
            cat.insert(cat.end(), w.begin(), w.end());
        }
        if (tt.put_derived(kq, cat)) return -2;
        cat.clear();
        for (const char* n : {"mlp.gate_proj.weight", "mlp.up_proj.weight"}) {
            const std::vector<float> w = tt.host(p + n);
            if (w.empty()) { set_error("qwen3: weight preparation failed (HIP copy)"); return -2; }
            cat.insert(cat.end(), w.begin(), w.end());
        }
        if (tt.put_derived(kg, cat)) return -2;
        Q3Layer& l = layers[i];
        l.ln1 = tt.get(p + "input_layernorm.weight"); l.ln2 = tt.get(p + "post_attention_layernorm.weight");
        l.qkv = tt.get(kq); l.gu = tt.get(kg);
        l.qn = tt.get(p + "self_attn.q_norm.weight"); l.kn = tt.get(p + "self_attn.k_norm.weight");
        l.o = tt.get(p + "self_attn.o_proj.weight"); l.down = tt.get(p + "mlp.down_proj.weight");
    }
    embed = tt.get("model.embed_tokens.weight");
    norm = tt.get("model.norm.weight");
    head = c.tie_word_embeddings ? embed : tt.get("lm_head.weight");
    prepared_for = tt.version;
    return 0;
}

int ready(Q3* e) {
    if (e->tt.require_all("qwen3")) return -3;
    if (e->prepared_for != e->tt.version) return e->prepare();
    return 0;
}

// what the attention of one pass needs beside the rows: prefill (seq != nullptr) or decode step
struct Q3Pass {
    int M;
    const int *row_seq, *row_pos;                      // device [M]
    const int *seq, *row0, *nrows, *p0; int nseq, max_rows;
    const int* row_len; int max_len;
};

int ensure_rows(Q3* e, int M) {
    const pf_qwen3_config& c = e->cfg;
    const size_t m = (size_t)M, f = sizeof(float);
    if (e->x.ensure(f * m * c.hidden_size) || e->x2.ensure(f * m * c.hidden_size) || e->xn.ensure(f * m * c.hidden_size) ||
        e->qkv.ensure(f * m * e->nqkv()) || e->q.ensure(f * m * c.n_heads * c.head_dim) || e->att.ensure(f * m * c.n_heads * c.head_dim) ||
        e->gu.ensure(f * m * 2 * c.intermediate_size) || e->act.ensure(f * m * c.intermediate_size))
        return -2;
    return 0;
}

// every layer over the rows in e->x (left there)
int run_layers(Q3* e, const Q3Pass& ps, hipStream_t s) {
    const pf_qwen3_config& c = e->cfg;
    const int M = ps.M, H = c.hidden_size, I = c.intermediate_size, NQ = c.n_heads * c.head_dim, NQKV = e->nqkv();
    float *X = e->x.as<float>(), *X2 = e->x2.as<float>(), *XN = e->xn.as<float>(), *QKV = e->qkv.as<float>(), *Q = e->q.as<float>(),
          *ATT = e->att.as<float>(), *GU = e->gu.as<float>(), *ACT = e->act.as<float>();
    const float scale = 1.0f / sqrtf((float)c.head_dim);
    int rc;
    for (int i = 0; i < c.n_layers; ++i) {
        const Q3Layer& l = e->layers[i];
        float* kc = e->kc.as<float>() + (size_t)i * e->layer_floats();
        float* vc = e->vc.as<float>() + (size_t)i * e->layer_floats();
        {
            ProfScope p(PROF_LN, 8.0 * M * (double)H, s, "qwen3.row");
            if ((rc = launch_q3_rmsnorm(X, H, l.ln1, c.rms_eps, XN, H, M, H, s))) return rc;
        }
        if ((rc = gemm_simple(XN, H, l.qkv, H, nullptr, QKV, NQKV, M, NQKV, H, 0, nullptr, 0, nullptr, 0, s))) return rc;
        Q3RopeArgs r{};
        r.qkv = QKV; r.ld = NQKV; r.qw = l.qn; r.kw = l.kn; r.eps = c.rms_eps;
        r.cos_t = e->cos_t.as<float>(); r.sin_t = e->sin_t.as<float>(); r.row_seq = ps.row_seq; r.row_pos = ps.row_pos;
        r.q_out = Q; r.ldq = NQ; r.kc = kc; r.vc = vc; r.cap = e->cap; r.M = M; r.Hq = c.n_heads; r.Hkv = c.n_kv_heads; r.hd = c.head_dim;
        {
            ProfScope p(PROF_LN, 8.0 * M * (double)NQKV, s, "qwen3.row");
            if ((rc = launch_q3_qk_rope(r, s))) return rc;
        }
        if (ps.seq) {
            Q3PrefillArgs a{};
            a.q = Q; a.ldq = NQ; a.kc = kc; a.vc = vc; a.cap = e->cap; a.out = ATT; a.ldo = NQ;
            a.seq = ps.seq; a.row0 = ps.row0; a.nrows = ps.nrows; a.p0 = ps.p0; a.nseq = ps.nseq; a.max_rows = ps.max_rows;
            a.Hq = c.n_heads; a.Hkv = c.n_kv_heads; a.hd = c.head_dim; a.scale = scale;
            ProfScope p(PROF_ATTN, 2.0 * M * (double)ps.max_rows * NQ, s, "qwen3.attn");
            if ((rc = launch_q3_prefill_attention(a, s))) return rc;
        } else {
            Q3DecodeArgs a{};
            a.q = Q; a.ldq = NQ; a.kc = kc; a.vc = vc; a.cap = e->cap; a.out = ATT; a.ldo = NQ;
            a.row_seq = ps.row_seq; a.row_len = ps.row_len; a.M = M; a.max_len = ps.max_len;
            a.Hq = c.n_heads; a.Hkv = c.n_kv_heads; a.hd = c.head_dim; a.scale = scale; a.part = e->part.as<float>();
            ProfScope p(PROF_ATTN, 4.0 * M * (double)ps.max_len * NQ, s, "qwen3.attn");
            if ((rc = launch_q3_decode_attention(a, s))) return rc;
        }
        if ((rc = gemm_simple(ATT, NQ, l.o, NQ, nullptr, X2, H, M, H, NQ, 0, X, H, nullptr, 0, s))) return rc;
        {
            ProfScope p(PROF_LN, 8.0 * M * (double)H, s, "qwen3.row");
            if ((rc = launch_q3_rmsnorm(X2, H, l.ln2, c.rms_eps, XN, H, M, H, s))) return rc;
        }
        if ((rc = gemm_simple(XN, H, l.gu, H, nullptr, GU, 2 * I, M, 2 * I, H, 0, nullptr, 0, nullptr, 0, s))) return rc;
        {
            ProfScope p(PROF_LN, 12.0 * M * (double)I, s, "qwen3.row");
            if ((rc = launch_q3_swiglu(GU, 2 * I, ACT, I, M, I, s))) return rc;
        }
        if ((rc = gemm_simple(ACT, I, l.down, I, nullptr, X, H, M, H, I, 0, X2, H, nullptr, 0, s))) return rc;
    }
    return 0;
}

// final norm of n rows (in place), their arg-max ids -> ids_host; logits (nullable, [n, V]) of the same normed rows. Synchronises.
int project(Q3* e, float* rows, int n, int32_t* ids_host, float* logits, hipStream_t s) {
    const pf_qwen3_config& c = e->cfg;
    const int H = c.hidden_size, V = c.vocab_size;
    int rc;
    if ((rc = launch_q3_rmsnorm(rows, H, e->norm, c.rms_eps, rows, H, n, H, s))) return rc;
    if (logits && (rc = gemm_simple(rows, H, e->head, H, nullptr, logits, V, n, V, H, 0, nullptr, 0, nullptr, 0, s))) return rc;
    if (e->ids.ensure(sizeof(int32_t) * Q3_MAX_B) || argmax_scratch(e->pval, e->pidx, n, argmax_f32_parts(V))) return -2;
    if ((rc = argmax_f32(rows, H, e->head, H, nullptr, n, V, H, 0, e->pval.as<float>(), e->pidx.as<int>(), e->ids.as<int32_t>(), s))) return rc;
    PF_HIP_TRY(hipMemcpyAsync(ids_host, e->ids.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int prefill(Q3* e, const float* embeds, const int32_t* rows_host, int B, int max_new, int32_t* first_ids, float* logits, hipStream_t s) {
    const pf_qwen3_config& c = e->cfg;
    const int H = c.hidden_size;
    PF_REQUIRE(B >= 1 && B <= Q3_MAX_B, "qwen3_prefill: a batch is 1 .. 16 sequences");
    PF_REQUIRE(max_new >= 0 && max_new <= (1 << 20), "qwen3_prefill: max_new_tokens out of range");
    long long total = 0;
    int longest = 0;
    for (int b = 0; b < B; ++b) {
        PF_REQUIRE(rows_host[b] >= 1 && rows_host[b] <= (1 << 20), "qwen3_prefill: every sequence needs 1 .. 2^20 rows");
        total += rows_host[b];
        longest = std::max(longest, (int)rows_host[b]);
    }
    const int cap = longest + max_new, M = (int)total;
    PF_REQUIRE(total * std::max(std::max(e->nqkv(), 2 * c.intermediate_size), c.vocab_size) <= 0x7fffffffLL, "qwen3_prefill: batch too large");
    if (e->rope_rows < cap) {
        set_error("qwen3_prefill: the rotary table holds " + std::to_string(e->rope_rows) + " positions, this batch needs " + std::to_string(cap) +
                  " (pf_qwen3_set_rope_table)");
        return -1;
    }
    int rc;
    if ((rc = ready(e))) return rc;
    e->B = 0;                                            // (no batch while this one is being set up)
    const size_t cache = (size_t)c.n_layers * B * c.n_kv_heads * cap * c.head_dim;
    if (e->kc.ensure(sizeof(float) * cache) || e->vc.ensure(sizeof(float) * cache) || ensure_rows(e, M) ||
        e->last.ensure(sizeof(float) * (size_t)B * H) || e->meta.ensure(sizeof(int32_t) * ((size_t)2 * M + 5 * B)))
        return -2;
    // row_seq [M] | row_pos [M] | seq [B] | row0 [B] | nrows [B] | p0 [B] | last row [B]
    std::vector<int32_t> meta((size_t)2 * M + 5 * B);
    int r = 0;
    for (int b = 0; b < B; ++b) {
        meta[2 * M + b] = b; meta[2 * M + B + b] = r; meta[2 * M + 2 * B + b] = rows_host[b]; meta[2 * M + 3 * B + b] = 0;
        for (int j = 0; j < rows_host[b]; ++j, ++r) { meta[r] = b; meta[M + r] = j; }
        meta[2 * M + 4 * B + b] = r - 1;
    }
    if (upload_h2d(e->meta.p, meta.data(), sizeof(int32_t) * meta.size(), s)) return -2;
    const int* d = e->meta.as<int>();
    PF_HIP_TRY(hipMemcpyAsync(e->x.p, embeds, sizeof(float) * (size_t)M * H, hipMemcpyDeviceToDevice, s));
    e->B = B; e->cap = cap;                              // (layer_floats() of this batch; B goes back to 0 on every failure below)
    Q3Pass ps{};
    ps.M = M; ps.row_seq = d; ps.row_pos = d + M; ps.seq = d + 2 * M; ps.row0 = ps.seq + B; ps.nrows = ps.seq + 2 * B; ps.p0 = ps.seq + 3 * B;
    ps.nseq = B; ps.max_rows = longest;
    if ((rc = run_layers(e, ps, s))) { e->B = 0; return rc; }
    float* X = e->x.as<float>();
    if (logits) {      // tests: every row's logits (the final norm out of place: X keeps the hidden rows for the last-row path)
        if ((rc = launch_q3_rmsnorm(X, H, e->norm, c.rms_eps, e->xn.as<float>(), H, M, H, s)) ||
            (rc = gemm_simple(e->xn.as<float>(), H, e->head, H, nullptr, logits, c.vocab_size, M, c.vocab_size, H, 0, nullptr, 0, nullptr, 0, s))) {
            e->B = 0;
            return rc;
        }
    }
    if ((rc = launch_gather_rows(X, H, M, d + 2 * M + 4 * B, e->last.as<float>(), B, H, s)) ||
        (rc = project(e, e->last.as<float>(), B, first_ids, nullptr, s))) {
        e->B = 0;
        return rc;
    }
    for (int b = 0; b < B; ++b) { e->len[b] = rows_host[b]; e->cur[b] = first_ids[b]; }
    return 0;
}

// one decode step of the n sequences slots[0 .. n): ids[i] is appended to sequence slots[i]; next[i] = arg-max of its logits
int step_rows(Q3* e, const int* slots, const int32_t* ids, int n, int32_t* next, float* logits, hipStream_t s) {
    const pf_qwen3_config& c = e->cfg;
    int max_len = 0, rc;
    for (int i = 0; i < n; ++i) {
        if (e->len[slots[i]] + 1 > e->cap) { set_error("qwen3_step: the KV cache of a sequence is full (max_new_tokens of the prefill)"); return -1; }
        max_len = std::max(max_len, e->len[slots[i]] + 1);
    }
    if ((rc = ready(e))) return rc;
    if (ensure_rows(e, n) || e->meta.ensure(sizeof(int32_t) * 4 * Q3_MAX_B) ||
        e->part.ensure(sizeof(float) * q3_decode_part_floats(Q3_MAX_B, c.n_heads, c.head_dim, e->cap)))
        return -2;
    int32_t meta[4 * Q3_MAX_B];      // row_seq | row_pos | row_len | ids, n each
    for (int i = 0; i < n; ++i) {
        meta[i] = slots[i]; meta[n + i] = e->len[slots[i]]; meta[2 * n + i] = e->len[slots[i]] + 1; meta[3 * n + i] = ids[i];
    }
    if (upload_h2d(e->meta.p, meta, sizeof(int32_t) * 4 * n, s)) return -2;
    const int* d = e->meta.as<int>();
    StreamModeScope small_m;
    if ((rc = launch_gather_rows(e->embed, c.hidden_size, c.vocab_size, d + 3 * n, e->x.as<float>(), n, c.hidden_size, s))) return rc;
    Q3Pass ps{};
    ps.M = n; ps.row_seq = d; ps.row_pos = d + n; ps.row_len = d + 2 * n; ps.max_len = max_len;
    if ((rc = run_layers(e, ps, s))) return rc;
    if ((rc = project(e, e->x.as<float>(), n, next, logits, s))) return rc;
    for (int i = 0; i < n; ++i) { e->len[slots[i]] += 1; e->cur[slots[i]] = next[i]; }
    return 0;
}

// host int32 metadata of a hook on the device (synchronous; freed with the object)
struct HookInts {
    int* p = nullptr;
    ~HookInts() { if (p) (void)hipFree(p); }
    int put(const std::vector<int32_t>& v) {
        PF_HIP_TRY(hipMalloc((void**)&p, sizeof(int32_t) * v.size()));
        PF_HIP_TRY(hipMemcpy(p, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice));
        return 0;
    }
};

}  // namespace

extern "C" {

pf_qwen3* pf_qwen3_create(const pf_qwen3_config* cfg) {
    if (!cfg) { set_error("qwen3: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_qwen3_config& c = *cfg;
    if (!q3_head_dim_ok(c.head_dim)) { set_error("qwen3: head_dim " + std::to_string(c.head_dim) + " is not built (64 or 128)"); return nullptr; }
    if (c.hidden_size < 32 || c.hidden_size % 32 != 0) { set_error("qwen3: hidden_size must be a multiple of 32"); return nullptr; }
    if (c.intermediate_size < 32 || c.intermediate_size % 32 != 0) { set_error("qwen3: intermediate_size must be a multiple of 32"); return nullptr; }
    if (c.n_heads < 1 || c.n_kv_heads < 1 || c.n_heads % c.n_kv_heads != 0 || c.n_heads > 1024) {
        set_error("qwen3: num_key_value_heads must divide num_attention_heads");
        return nullptr;
    }
    if (c.vocab_size < 2 || c.n_layers < 1 || !(c.rms_eps > 0.f)) { set_error("qwen3: vocab_size >= 2, n_layers >= 1, rms_eps > 0"); return nullptr; }
    std::unique_ptr<Q3> h(new Q3());
    h->cfg = c;
    const int64_t H = c.hidden_size, I = c.intermediate_size, NQ = (int64_t)c.n_heads * c.head_dim, NK = (int64_t)c.n_kv_heads * c.head_dim;
    int rc = h->tt.add("model.embed_tokens.weight", (int64_t)c.vocab_size * H) | h->tt.add("model.norm.weight", H);
    if (!c.tie_word_embeddings) rc |= h->tt.add("lm_head.weight", (int64_t)c.vocab_size * H);
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string p = lname(i);
        rc |= h->tt.add(p + "input_layernorm.weight", H) | h->tt.add(p + "post_attention_layernorm.weight", H);
        rc |= h->tt.add(p + "self_attn.q_proj.weight", NQ * H) | h->tt.add(p + "self_attn.k_proj.weight", NK * H);
        rc |= h->tt.add(p + "self_attn.v_proj.weight", NK * H) | h->tt.add(p + "self_attn.o_proj.weight", H * NQ);
        rc |= h->tt.add(p + "self_attn.q_norm.weight", c.head_dim) | h->tt.add(p + "self_attn.k_norm.weight", c.head_dim);
        rc |= h->tt.add(p + "mlp.gate_proj.weight", I * H) | h->tt.add(p + "mlp.up_proj.weight", I * H) | h->tt.add(p + "mlp.down_proj.weight", H * I);
    }
    if (rc) return nullptr;
    return reinterpret_cast<pf_qwen3*>(h.release());
}
void pf_qwen3_destroy(pf_qwen3* h) { delete reinterpret_cast<Q3*>(h); }
int pf_qwen3_set_tensor(pf_qwen3* hh, const char* name, const float* data, int64_t numel) {
    Q3* h = reinterpret_cast<Q3*>(hh);
    PF_REQUIRE(h && name && data, "qwen3_set_tensor: null");
    return h->tt.set(name, data, numel);
}
int pf_qwen3_missing(const pf_qwen3* hh) {
    const Q3* h = reinterpret_cast<const Q3*>(hh);
    return h ? h->tt.missing() : -1;
}
int pf_qwen3_set_rope_table(pf_qwen3* hh, const float* cos_t, const float* sin_t, int32_t positions) {
    Q3* h = reinterpret_cast<Q3*>(hh);
    PF_REQUIRE(h && cos_t && sin_t && positions >= 1 && positions <= (1 << 22), "qwen3_set_rope_table: null argument or no positions");
    const size_t bytes = sizeof(float) * (size_t)positions * (h->cfg.head_dim / 2);
    h->rope_rows = 0;
    if (h->cos_t.ensure(bytes) || h->sin_t.ensure(bytes)) return -2;
    PF_HIP_TRY(hipDeviceSynchronize());                 // (a step in flight may still read the old rows)
    PF_HIP_TRY(hipMemcpy(h->cos_t.p, cos_t, bytes, hipMemcpyDefault));
    PF_HIP_TRY(hipMemcpy(h->sin_t.p, sin_t, bytes, hipMemcpyDefault));
    h->rope_rows = positions;
    return 0;
}
int32_t pf_qwen3_rope_positions(const pf_qwen3* hh) {
    const Q3* h = reinterpret_cast<const Q3*>(hh);
    return h ? h->rope_rows : -1;
}
int pf_qwen3_embed(pf_qwen3* hh, const int32_t* ids_dev, int32_t n, float* out_dev, void* stream) {
    Q3* h = reinterpret_cast<Q3*>(hh);
    PF_REQUIRE(h && ids_dev && out_dev && n > 0, "qwen3_embed: null/empty argument");
    int rc;
    if ((rc = ready(h))) return rc;
    return launch_gather_rows(h->embed, h->cfg.hidden_size, h->cfg.vocab_size, ids_dev, out_dev, n, h->cfg.hidden_size,
                              reinterpret_cast<hipStream_t>(stream));
}
int pf_qwen3_prefill(pf_qwen3* hh, const float* inputs_embeds_dev, const int32_t* rows_host, int32_t B, int32_t max_new_tokens,
                     int32_t* first_ids_host, float* logits_dev, void* stream) {
    Q3* h = reinterpret_cast<Q3*>(hh);
    PF_REQUIRE(h && inputs_embeds_dev && rows_host && first_ids_host, "qwen3_prefill: null argument");
    return prefill(h, inputs_embeds_dev, rows_host, B, max_new_tokens, first_ids_host, logits_dev, reinterpret_cast<hipStream_t>(stream));
}
int pf_qwen3_step(pf_qwen3* hh, const int32_t* ids_host, int32_t* next_ids_host, float* logits_dev, void* stream) {
    Q3* h = reinterpret_cast<Q3*>(hh);
    PF_REQUIRE(h && ids_host && next_ids_host, "qwen3_step: null argument");
    PF_REQUIRE(h->B >= 1, "qwen3_step: no batch (pf_qwen3_prefill first)");
    int slots[Q3_MAX_B];
    for (int b = 0; b < h->B; ++b) slots[b] = b;
    return step_rows(h, slots, ids_host, h->B, next_ids_host, logits_dev, reinterpret_cast<hipStream_t>(stream));
}
int pf_qwen3_generate(pf_qwen3* hh, int32_t max_new_tokens, const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id,
                      int32_t* out_ids_host, int32_t* n_out, void* stream) {
    Q3* h = reinterpret_cast<Q3*>(hh);
    PF_REQUIRE(h && out_ids_host && n_out && max_new_tokens >= 1 && n_eos >= 0 && (n_eos == 0 || eos_ids_host), "qwen3_generate: null/empty argument");
    PF_REQUIRE(h->B >= 1, "qwen3_generate: no batch (pf_qwen3_prefill first)");
    const int B = h->B;
    for (int b = 0; b < B; ++b)
        PF_REQUIRE(h->len[b] + max_new_tokens - 1 <= h->cap, "qwen3_generate: more tokens than the prefill reserved (max_new_tokens)");
    for (size_t i = 0; i < (size_t)B * max_new_tokens; ++i) out_ids_host[i] = pad_id;
    bool fin[Q3_MAX_B] = {false};
    int n = 0;
    for (;;) {
        int live = 0;
        for (int b = 0; b < B; ++b) {
            if (fin[b]) continue;
            out_ids_host[(size_t)b * max_new_tokens + n] = h->cur[b];
            for (int k = 0; k < n_eos; ++k) fin[b] = fin[b] || h->cur[b] == eos_ids_host[k];
            live += fin[b] ? 0 : 1;
        }
        ++n;
        if (!live || n == max_new_tokens) break;
        int slots[Q3_MAX_B];
        int32_t ids[Q3_MAX_B], next[Q3_MAX_B];
        int m = 0;
        for (int b = 0; b < B; ++b)
            if (!fin[b]) { slots[m] = b; ids[m] = h->cur[b]; ++m; }
        const int rc = step_rows(h, slots, ids, m, next, nullptr, reinterpret_cast<hipStream_t>(stream));
        if (rc) return rc;
    }
    *n_out = n;
    return 0;
}
int pf_qwen3_debug_poison(pf_qwen3* hh) {
    Q3* h = reinterpret_cast<Q3*>(hh);
    PF_REQUIRE(h, "qwen3_debug_poison: null handle");
    PF_HIP_TRY(hipDeviceSynchronize());
    for (DevBuf* b : {&h->kc, &h->vc, &h->x, &h->x2, &h->xn, &h->qkv, &h->q, &h->att, &h->gu, &h->act, &h->part, &h->last})
        if (b->p) PF_HIP_TRY(hipMemset(b->p, 0xff, b->cap));
    h->B = 0;                                            // the cache of the last prefill is gone
    return 0;
}

int pf_k_qwen3_tiles(int32_t G, int32_t hd, int32_t* q_tile, int32_t* k_tile, int32_t* k_split) {
    PF_REQUIRE(G >= 1 && q3_head_dim_ok(hd) && q_tile && k_tile && k_split, "k_qwen3_tiles: head_dim 64 or 128, G >= 1");
    *q_tile = q3_qtile(G); *k_tile = q3_ktile(hd); *k_split = Q3_KSPLIT;
    return 0;
}
int pf_k_qwen3_rmsnorm(const float* x_dev, int32_t ldx, const float* w_dev, float eps, float* y_dev, int32_t ldy, int32_t M, int32_t D,
                       void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = launch_q3_rmsnorm(x_dev, ldx, w_dev, eps, y_dev, ldy, M, D, s);
    if (rc) return rc;
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
int pf_k_qwen3_qk_rope(const float* qkv_dev, int32_t ld, const float* qw_dev, const float* kw_dev, float eps, const float* cos_dev,
                       const float* sin_dev, int32_t table_rows, const int32_t* row_seq_host, const int32_t* row_pos_host, float* q_out_dev,
                       int32_t ldq, float* kcache_dev, float* vcache_dev, int32_t slots, int32_t cap, int32_t M, int32_t Hq, int32_t Hkv,
                       int32_t hd, void* stream) {
    PF_REQUIRE(row_seq_host && row_pos_host && M > 0 && slots > 0 && cap > 0 && table_rows > 0, "k_qwen3_qk_rope: null/empty argument");
    std::vector<int32_t> meta((size_t)2 * M);
    for (int r = 0; r < M; ++r) {
        PF_REQUIRE(row_seq_host[r] >= 0 && row_seq_host[r] < slots && row_pos_host[r] >= 0 && row_pos_host[r] < cap && row_pos_host[r] < table_rows,
                   "k_qwen3_qk_rope: a row's slot or position lies outside the cache or the table");
        meta[r] = row_seq_host[r]; meta[M + r] = row_pos_host[r];
    }
    HookInts d;
    if (d.put(meta)) return -2;
    Q3RopeArgs a{};
    a.qkv = qkv_dev; a.ld = ld; a.qw = qw_dev; a.kw = kw_dev; a.eps = eps; a.cos_t = cos_dev; a.sin_t = sin_dev;
    a.row_seq = d.p; a.row_pos = d.p + M; a.q_out = q_out_dev; a.ldq = ldq; a.kc = kcache_dev; a.vc = vcache_dev; a.cap = cap;
    a.M = M; a.Hq = Hq; a.Hkv = Hkv; a.hd = hd;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = launch_q3_qk_rope(a, s);
    if (rc) return rc;
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
int pf_k_qwen3_prefill_attention(const float* q_dev, int32_t ldq, const float* kcache_dev, const float* vcache_dev, int32_t slots,
                                 int32_t cap, float* out_dev, int32_t ldo, int32_t M, const int32_t* seq_host, const int32_t* row0_host,
                                 const int32_t* nrows_host, const int32_t* p0_host, int32_t nseq, int32_t Hq, int32_t Hkv, int32_t hd,
                                 float scale, void* stream) {
    PF_REQUIRE(seq_host && row0_host && nrows_host && p0_host && nseq > 0 && M > 0 && slots > 0 && cap > 0, "k_qwen3_prefill_attention: null/empty argument");
    std::vector<int32_t> meta((size_t)4 * nseq);
    int max_rows = 0;
    for (int i = 0; i < nseq; ++i) {
        PF_REQUIRE(seq_host[i] >= 0 && seq_host[i] < slots && nrows_host[i] >= 1 && row0_host[i] >= 0 &&
                   (long long)row0_host[i] + nrows_host[i] <= M && p0_host[i] >= 0 && (long long)p0_host[i] + nrows_host[i] <= cap,
                   "k_qwen3_prefill_attention: a sequence's rows or positions lie outside q or the cache");
        meta[i] = seq_host[i]; meta[nseq + i] = row0_host[i]; meta[2 * nseq + i] = nrows_host[i]; meta[3 * nseq + i] = p0_host[i];
        max_rows = std::max(max_rows, (int)nrows_host[i]);
    }
    HookInts d;
    if (d.put(meta)) return -2;
    Q3PrefillArgs a{};
    a.q = q_dev; a.ldq = ldq; a.kc = kcache_dev; a.vc = vcache_dev; a.cap = cap; a.out = out_dev; a.ldo = ldo;
    a.seq = d.p; a.row0 = d.p + nseq; a.nrows = d.p + 2 * nseq; a.p0 = d.p + 3 * nseq; a.nseq = nseq; a.max_rows = max_rows;
    a.Hq = Hq; a.Hkv = Hkv; a.hd = hd; a.scale = scale;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = launch_q3_prefill_attention(a, s);
    if (rc) return rc;
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
int pf_k_qwen3_decode_attention(const float* q_dev, int32_t ldq, const float* kcache_dev, const float* vcache_dev, int32_t slots,
                                int32_t cap, float* out_dev, int32_t ldo, const int32_t* row_seq_host, const int32_t* row_len_host, int32_t M,
                                int32_t Hq, int32_t Hkv, int32_t hd, float scale, void* stream) {
    PF_REQUIRE(row_seq_host && row_len_host && M > 0 && slots > 0 && cap > 0 && Hq > 0 && q3_head_dim_ok(hd), "k_qwen3_decode_attention: null/empty argument");
    std::vector<int32_t> meta((size_t)2 * M);
    int max_len = 0;
    for (int r = 0; r < M; ++r) {
        PF_REQUIRE(row_seq_host[r] >= 0 && row_seq_host[r] < slots && row_len_host[r] >= 1 && row_len_host[r] <= cap,
                   "k_qwen3_decode_attention: a row's slot or length lies outside the cache");
        meta[r] = row_seq_host[r]; meta[M + r] = row_len_host[r];
        max_len = std::max(max_len, (int)row_len_host[r]);
    }
    HookInts d;
    if (d.put(meta)) return -2;
    DevBuf part;
    if (part.ensure(sizeof(float) * q3_decode_part_floats(M, Hq, hd, max_len))) return -2;
    Q3DecodeArgs a{};
    a.q = q_dev; a.ldq = ldq; a.kc = kcache_dev; a.vc = vcache_dev; a.cap = cap; a.out = out_dev; a.ldo = ldo;
    a.row_seq = d.p; a.row_len = d.p + M; a.M = M; a.max_len = max_len; a.Hq = Hq; a.Hkv = Hkv; a.hd = hd; a.scale = scale;
    a.part = part.as<float>();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = launch_q3_decode_attention(a, s);
    if (rc) return rc;
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
int pf_k_qwen3_swiglu(const float* gu_dev, int32_t ld, float* out_dev, int32_t ldo, int32_t M, int32_t I, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = launch_q3_swiglu(gu_dev, ld, out_dev, ldo, M, I, s);
    if (rc) return rc;
    PF_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
