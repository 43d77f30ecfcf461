// C-ABI layer, decoder / CTC family: pf_decoder_*, pf_ctc_*.
#include "engine_internal.h"

namespace pf {

// ContextualParaformerDecoder keeps its last attention block under "last_decoder." (contextual_paraformer/decoder.py:241)
static std::string dec_layer_prefix(bool contextual, int n_blocks, int i) {
    return (contextual && i == n_blocks - 1) ? std::string("last_decoder.") : "decoders." + std::to_string(i) + ".";
}
static std::string dec2_layer_prefix(int i) { return "decoders2." + std::to_string(i) + "."; }

// ---- THE description of a decoder layer (DecoderLayerSANM, paraformer/decoder.py:78-121): the tensors under its prefix, by kind
// (DecLayerW.kind). These two functions are the only place that spells the names: a tensor added to a layer is added here, and a new
// decoder variant adds a kind, not a copy of the list.
static int dec_layer_add(TensorTable& tt, const pf_decoder_config& c, const std::string& p, int kind) {
    const int D = c.d_model, F = c.ffn_dim;
    int rc = 0;
    rc |= tt.add(p + "norm1.weight", D);
    rc |= tt.add(p + "norm1.bias", D);
    rc |= tt.add(p + "feed_forward.w_1.weight", (int64_t)F * D);
    rc |= tt.add(p + "feed_forward.w_1.bias", F);
    rc |= tt.add(p + "feed_forward.norm.weight", F);
    rc |= tt.add(p + "feed_forward.norm.bias", F);
    rc |= tt.add(p + "feed_forward.w_2.weight", (int64_t)D * F);
    if (kind >= DEC_FFN_FSMN) {
        rc |= tt.add(p + "norm2.weight", D);
        rc |= tt.add(p + "norm2.bias", D);
        rc |= tt.add(p + "self_attn.fsmn_block.weight", (int64_t)D * c.kernel_size);
    }
    if (kind >= DEC_FFN_FSMN_ATTN) {
        rc |= tt.add(p + "norm3.weight", D);
        rc |= tt.add(p + "norm3.bias", D);
        rc |= tt.add(p + "src_attn.linear_q.weight", (int64_t)D * D);
        rc |= tt.add(p + "src_attn.linear_q.bias", D);
        rc |= tt.add(p + "src_attn.linear_k_v.weight", (int64_t)2 * D * D);
        rc |= tt.add(p + "src_attn.linear_k_v.bias", 2 * D);
        rc |= tt.add(p + "src_attn.linear_out.weight", (int64_t)D * D);
        rc |= tt.add(p + "src_attn.linear_out.bias", D);
    }
    return rc;
}
static DecLayerW dec_layer_resolve(const TensorTable& tt, const std::string& p, int kind) {
    DecLayerW w;
    w.prefix = p; w.kind = kind;
    w.n1g = tt.get(p + "norm1.weight"); w.n1b = tt.get(p + "norm1.bias");
    w.w1 = tt.get(p + "feed_forward.w_1.weight"); w.b1 = tt.get(p + "feed_forward.w_1.bias");
    w.fng = tt.get(p + "feed_forward.norm.weight"); w.fnb = tt.get(p + "feed_forward.norm.bias");
    w.w2 = tt.get(p + "feed_forward.w_2.weight");
    if (kind >= DEC_FFN_FSMN) {
        w.n2g = tt.get(p + "norm2.weight"); w.n2b = tt.get(p + "norm2.bias");
        w.fsmn_w = tt.get(p + "self_attn.fsmn_block.weight");
    }
    if (kind >= DEC_FFN_FSMN_ATTN) {
        w.n3g = tt.get(p + "norm3.weight"); w.n3b = tt.get(p + "norm3.bias");
        w.q_w = tt.get(p + "src_attn.linear_q.weight"); w.q_b = tt.get(p + "src_attn.linear_q.bias");
        w.kv_w = tt.get(p + "src_attn.linear_k_v.weight"); w.kv_b = tt.get(p + "src_attn.linear_k_v.bias");
        w.o_w = tt.get(p + "src_attn.linear_out.weight"); w.o_b = tt.get(p + "src_attn.linear_out.bias");
    }
    return w;
}

static int decoder_resolve(Decoder* d) {
    if (d->tt.require_all("decoder")) return -3;
    d->layers.clear();
    for (int i = 0; i < d->cfg.n_blocks; ++i)
        d->layers.push_back(dec_layer_resolve(d->tt, dec_layer_prefix(d->contextual, d->cfg.n_blocks, i), DEC_FFN_FSMN_ATTN));
    d->layers2.clear();
    for (int i = 0; i < d->n_blocks2; ++i) d->layers2.push_back(dec_layer_resolve(d->tt, dec2_layer_prefix(i), DEC_FFN_FSMN));
    d->last = dec_layer_resolve(d->tt, "decoders3.0.", DEC_FFN);
    d->resolved_for = d->tt.version;
    d->x2_for = TensorTable::NOT_PREPARED;
    return 0;
}

// ---- the fused arg-max tails of the vocabulary / CTC projections, one per arithmetic: ids[row] = argmax_n (A W^T + bias)[row, n],
// lowest index on ties, from the GEMM epilogue's partials sval / sidx [M, parts] (argmax_scratch) and one reduction; no [M, N] logits
int argmax_scratch(DevBuf& pval, DevBuf& pidx, int M, int parts) {
    return (pval.ensure(sizeof(float) * (size_t)M * parts) || pidx.ensure(sizeof(int) * (size_t)M * parts)) ? -2 : 0;
}
// fp32 MFMA tile from fp32 or (ab_bf16) bf16 operands; parts = argmax_f32_parts(N)
int argmax_f32(const float* A, int lda, const float* W, int ldw, const float* bias, int M, int N, int K, int ab_bf16, float* sval,
               int* sidx, int32_t* ids, hipStream_t s) {
    const int parts = argmax_f32_parts(N);
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.M = M; g.N = N; g.K = K; g.ab_bf16 = ab_bf16;
    g.amax_val = sval; g.amax_idx = sidx; g.amax_ld = parts;
    int rc;
    if ((rc = gemm(g, s))) return rc;
    return launch_argmax_reduce(sval, sidx, parts, parts, ids, nullptr, M, s);
}
// fp16 matrix cores from two-plane operands (gemm_f16x2.hip); the result scale is oscale (times *oscale_dev when the planes' scale
// was chosen on the device); parts = gemm_f16x2_argmax_parts(M, N)
int argmax_f16x2(const unsigned short* A2, int lda, size_t a_plane, const unsigned short* W2, int ldw, size_t w_plane, float oscale,
                 const float* oscale_dev, const float* bias, int M, int N, int K, float* sval, int* sidx, int32_t* ids, hipStream_t s) {
    const int parts = gemm_f16x2_argmax_parts(M, N);
    Gemm2Args g{};
    g.A = A2; g.lda = lda; g.a_plane = a_plane; g.W = W2; g.ldw = ldw; g.w_plane = w_plane;
    g.oscale = oscale; g.oscale_dev = oscale_dev; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.amax_val = sval; g.amax_idx = sidx; g.amax_ld = parts;
    int rc;
    {
        ProfScope ps(PROF_GEMM3, 2.0 * M * (double)N * K, s);
        if ((rc = launch_gemm_f16x2(g, s))) return rc;
    }
    return launch_argmax_reduce(sval, sidx, parts, parts, ids, nullptr, M, s);
}

// shared tail: logits / fused argmax of a [M, D] hidden against a [V, D] vocabulary projection
int vocab_project(const float* hidden, int M, int D, const float* W, const float* bias, int V, float* logits,
                         int32_t* ids, DevBuf& pval, DevBuf& pidx, hipStream_t s) {
    int rc;
    if (logits) {
        if ((rc = gemm_simple(hidden, D, W, D, bias, logits, V, M, V, D, 0, nullptr, 0, nullptr, 0, s))) return rc;
        if (ids) return launch_argmax_rows(logits, V, M, V, ids, s);
        return 0;
    }
    if (!ids) return 0;
    if (g_stream_mode && D % 16 == 0) {
        // small M (streaming): weight-streaming GEMM into a scratch logits block, then a row arg-max
        if (pval.ensure(sizeof(float) * (size_t)M * V)) return -2;
        if ((rc = gemm_simple(hidden, D, W, D, bias, pval.as<float>(), V, M, V, D, 0, nullptr, 0, nullptr, 0, s))) return rc;
        return launch_argmax_rows(pval.as<float>(), V, M, V, ids, s);
    }
    if (argmax_scratch(pval, pidx, M, argmax_f32_parts(V))) return -2;
    return argmax_f32(hidden, D, W, D, bias, M, V, D, 0, pval.as<float>(), pidx.as<int>(), ids, s);
}

// PositionwiseFeedForwardDecoderSANM (sanm/positionwise_feed_forward.py:12-33): w_2(LN(relu(w_1 x))), w_2 bias-free
int gemm3_simple(const unsigned short* A3, int lda, int M, const unsigned short* W3, const float* bias, float* C,
                        int ldc, int N, int K, int relu, hipStream_t s) {
    if (!W3) return -2;
    Gemm3Args g{};
    g.A = A3; g.lda = lda; g.a_plane = (size_t)M * lda; g.W = W3; g.ldw = K; g.w_plane = (size_t)N * K;
    g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.relu = relu;
    ProfScope ps(PROF_GEMM3, 2.0 * M * (double)N * K, s);
    return launch_gemm_split3(g, s);
}

int gemm2_simple(const unsigned short* A2, int lda, int M, int ea, const unsigned short* W2, int ew, const float* bias,
                        float* C, int ldc, int N, int K, int relu, const float* R2, int ldr2, hipStream_t s,
                        const float* oscale_dev, float* splitk_part) {
    if (!W2) return -2;
    Gemm2Args g{};
    g.A = A2; g.lda = lda; g.a_plane = (size_t)M * lda; g.W = W2; g.ldw = K; g.w_plane = (size_t)N * K;
    g.oscale = pow2f(-(ea + ew)); g.oscale_dev = oscale_dev; g.bias = bias; g.R2 = R2; g.ldr2 = ldr2;
    g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.relu = relu;
    if (splitk_part && K % 128 == 0) { g.ksplit = 4; g.part = splitk_part; }     // streaming step: w_2 in its split-K form
    ProfScope ps(PROF_GEMM3, 2.0 * M * (double)N * K, s);
    return launch_gemm_f16x2(g, s);
}

// f16x2 mode: exponents and weight planes of one decoder layer (the per-layer worker of decoder_prepare)
static int dec_layer_x2(Decoder* d, DecLayerW& w, hipStream_t s) {
    const int D = d->cfg.d_model, F = d->cfg.ffn_dim;
    const std::string& p = w.prefix;
    float b;
    if (TensorTable::dev_ln_bound(w.n1g, w.n1b, D, &b, s)) return -2;
    w.e_n1 = exp_for_bound(b);
    if (TensorTable::dev_ln_bound(w.fng, w.fnb, F, &b, s)) return -2;
    w.e_fn = exp_for_bound(b);
    w.w1_2 = d->tt.get_split2(p + "feed_forward.w_1.weight", F, D, &w.ew_1, s);
    w.w2_2 = d->tt.get_split2(p + "feed_forward.w_2.weight", D, F, &w.ew_2, s);
    if (!w.w1_2 || !w.w2_2) return -2;
    if (w.kind == DEC_FFN_FSMN_ATTN) {
        if (TensorTable::dev_ln_bound(w.n3g, w.n3b, D, &b, s)) return -2;
        w.e_n3 = exp_for_bound(b);
        w.q_2 = d->tt.get_split2(p + "src_attn.linear_q.weight", D, D, &w.ew_q, s);
        w.kv_2 = d->tt.get_split2(p + "src_attn.linear_k_v.weight", 2 * D, D, &w.ew_kv, s);
        w.o_2 = d->tt.get_split2(p + "src_attn.linear_out.weight", D, D, &w.ew_o, s);
        if (!w.q_2 || !w.kv_2 || !w.o_2) return -2;
        float bq;
        if (TensorTable::dev_linear_bound(w.q_w, D, D, D, w.q_b, b, &bq, s)) return -2;
        w.e_q = exp_for_bound(bq * powf((float)(D / d->cfg.n_heads), -0.5f));
        if (TensorTable::dev_linear_bound(w.kv_w, D, D, D, nullptr, 1.f, &w.kv_l1b[0], s) ||
            TensorTable::dev_absmax(w.kv_b, D, &w.kv_l1b[1], s) ||
            TensorTable::dev_linear_bound(w.kv_w + (size_t)D * D, D, D, D, nullptr, 1.f, &w.kv_l1b[2], s) ||
            TensorTable::dev_absmax(w.kv_b + D, D, &w.kv_l1b[3], s)) return -2;
    }
    return 0;
}

// The f16x2 state in one piece: every layer's planes and exponents, the linear_k_v bounds on the device (dlb), after_norm's exponent
// and the vocabulary planes (load-time reductions with host round trips -- never inside a graph capture)
int decoder_prepare(Decoder* d, bool x2, hipStream_t s) {
    int rc;
    if (d->resolved_for != d->tt.version && (rc = decoder_resolve(d))) return rc;
    if (!x2 || d->x2_for == d->tt.version) return 0;
    const pf_decoder_config& c = d->cfg;
    for (DecLayerW& w : d->layers) if ((rc = dec_layer_x2(d, w, s))) return rc;
    for (DecLayerW& w : d->layers2) if ((rc = dec_layer_x2(d, w, s))) return rc;
    if ((rc = dec_layer_x2(d, d->last, s))) return rc;
    std::vector<float> lb((size_t)4 * c.n_blocks);
    for (int l = 0; l < c.n_blocks; ++l) for (int j = 0; j < 4; ++j) lb[4 * l + j] = d->layers[l].kv_l1b[j];
    if (d->dlb.ensure(sizeof(float) * lb.size())) return -2;
    PF_HIP_TRY(hipMemcpyAsync(d->dlb.p, lb.data(), sizeof(float) * lb.size(), hipMemcpyHostToDevice, s));
    PF_HIP_TRY(hipStreamSynchronize(s));                     // `lb` is a stack object
    float b;
    if (TensorTable::dev_ln_bound(d->tt.get("after_norm.weight"), d->tt.get("after_norm.bias"), c.d_model, &b, s)) return -2;
    d->e_an = exp_for_bound(b);
    int ew_v = 0;
    if (c.vocab_size > 0 && !d->tt.get_split2("output_layer.weight", c.vocab_size, c.d_model, &ew_v, s)) return -2;
    d->x2_for = d->tt.version;
    return 0;
}

// f16x2 form of dec_ffn: both LayerNorms write two-plane fp16 operands, w_1 and w_2 run on the fp16 matrix cores
// ln (streaming step, split-K w_2): the LayerNorm that follows the block rides in w_2's second launch (Gemm2Args.ln_*)
int dec_ffn_x2(Decoder* d, const DecLayerW& w, const float* x, float* out, int M, hipStream_t s, float* splitk_part, const FoldedLn* ln) {
    const int D = d->cfg.d_model, F = d->cfg.ffn_dim;
    float* ffn = d->ffn.as<float>();
    unsigned short* t2p = d->t16.as<unsigned short>();
    unsigned short* f2p = d->ffn16.as<unsigned short>();
    int rc;
    {
        ProfScope ps(PROF_LN, 8.0 * M * (double)D, s);
        if ((rc = launch_layernorm(x, D, w.n1g, w.n1b, reinterpret_cast<float*>(t2p), D, M, D, D, d->cfg.ln_eps, s, 3, 0,
                                   (size_t)M * D, pow2f(w.e_n1)))) return rc;
    }
    if ((rc = gemm2_simple(t2p, D, M, w.e_n1, w.w1_2, w.ew_1, w.b1, ffn, F, F, D, 1, nullptr, 0, s))) return rc;
    {
        ProfScope ps(PROF_LN, 8.0 * M * (double)F, s);
        if ((rc = launch_layernorm(ffn, F, w.fng, w.fnb, reinterpret_cast<float*>(f2p), F, M, F, F, d->cfg.ln_eps, s, 3, 0,
                                   (size_t)M * F, pow2f(w.e_fn)))) return rc;
    }
    if (ln && splitk_part && F % 128 == 0) {
        Gemm2Args g{};
        g.A = f2p; g.lda = F; g.a_plane = (size_t)M * F; g.W = w.w2_2; g.ldw = F; g.w_plane = (size_t)D * F;
        g.oscale = pow2f(-(w.e_fn + w.ew_2)); g.C = out; g.ldc = D; g.M = M; g.N = D; g.K = F; g.ksplit = 4; g.part = splitk_part;
        g.ln_g = ln->g; g.ln_b = ln->b; g.ln_eps = d->cfg.ln_eps; g.ln_y = ln->y; g.ln_ldy = D; g.ln_out = ln->out; g.ln_plane = (size_t)M * D;
        g.ln_oscale = ln->oscale;
        if (!w.w2_2) return -2;
        ProfScope ps(PROF_GEMM3, 2.0 * M * (double)D * F, s);
        return launch_gemm_f16x2(g, s);
    }
    if (ln) { set_error("decoder: LayerNorm folding needs the split-K form of w_2"); return -1; }
    return gemm2_simple(f2p, F, M, w.e_fn, w.w2_2, w.ew_2, nullptr, out, D, D, F, 0, nullptr, 0, s, nullptr, splitk_part);
}

// w1_3 != nullptr (bf16x3 mode): norm1 writes the three planes and w_1 runs on the bf16 matrix cores
int dec_ffn(Decoder* d, const DecLayerW& w, const float* x, float* out, int M, hipStream_t s,
                   const unsigned short* w1_3) {
    const int D = d->cfg.d_model, F = d->cfg.ffn_dim;
    float* t1 = d->t1.as<float>();
    float* ffn = d->ffn.as<float>();
    float* ffn2 = d->ffn2.as<float>();
    int rc;
    if (w1_3) {
        unsigned short* t3 = d->t16.as<unsigned short>();
        {
            ProfScope ps(PROF_LN, 10.0 * M * (double)D, s);
            if ((rc = launch_layernorm(x, D, w.n1g, w.n1b, reinterpret_cast<float*>(t3), D, M, D, D, d->cfg.ln_eps, s, 2, 0,
                                       (size_t)M * D))) return rc;
        }
        if ((rc = gemm3_simple(t3, D, M, w1_3, w.b1, ffn, F, F, D, 1, s))) return rc;
        if ((rc = layernorm(ffn, F, w.fng, w.fnb, ffn2, F, M, F, F, d->cfg.ln_eps, s))) return rc;
        return gemm_simple(ffn2, F, w.w2, F, nullptr, out, D, M, D, F, 0, nullptr, 0, nullptr, 0, s);
    }
    if ((rc = layernorm(x, D, w.n1g, w.n1b, t1, D, M, D, D, d->cfg.ln_eps, s))) return rc;
    if ((rc = gemm_simple(t1, D, w.w1, D, w.b1, ffn, F, M, F, D, 1, nullptr, 0, nullptr, 0, s))) return rc;
    if ((rc = layernorm(ffn, F, w.fng, w.fnb, ffn2, F, M, F, F, d->cfg.ln_eps, s))) return rc;
    return gemm_simple(ffn2, F, w.w2, F, nullptr, out, D, M, D, F, 0, nullptr, 0, nullptr, 0, s);
}

// bf16-operand GEMM (throughput mode): A and W bf16, fp32 accumulation, C fp32 or (c16) bf16
static int gemm_bf16(const unsigned short* A, int lda, const unsigned short* W, int ldw, const float* bias, void* C, int ldc, int M,
                     int N, int K, int relu, const float* R2, int ldr2, int c16, hipStream_t s) {
    if (!W) return -2;
    GemmArgs g{};
    g.A = reinterpret_cast<const float*>(A); g.lda = lda; g.W = reinterpret_cast<const float*>(W); g.ldw = ldw;
    g.bias = bias; g.R2 = R2; g.ldr2 = ldr2; g.C = reinterpret_cast<float*>(C); g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.relu = relu; g.ab_bf16 = 1; g.c_bf16 = c16;
    ProfScope ps(PROF_GEMM, 2.0 * M * (double)N * K, s);
    return launch_gemm_f32(g, s);
}

// bf16 form of dec_ffn: both LayerNorms write bf16 rows, w_1 and w_2 take bf16 operands (the copies are cached by the table)
static int dec_ffn_bf16(Decoder* d, const DecLayerW& w, const float* x, float* out, int M, hipStream_t s) {
    const int D = d->cfg.d_model, F = d->cfg.ffn_dim;
    unsigned short* t16 = d->t16.as<unsigned short>();
    unsigned short* ffn16 = d->ffn16.as<unsigned short>();
    unsigned short* ffn2_16 = d->ffn2_16.as<unsigned short>();
    int rc;
    if ((rc = launch_layernorm(x, D, w.n1g, w.n1b, reinterpret_cast<float*>(t16), D, M, D, D, d->cfg.ln_eps, s, 1, 0))) return rc;
    if ((rc = gemm_bf16(t16, D, d->tt.get_bf16(w.prefix + "feed_forward.w_1.weight", s), D, w.b1, ffn16, F, M, F, D, 1, nullptr, 0, 1, s)))
        return rc;
    if ((rc = launch_layernorm(reinterpret_cast<const float*>(ffn16), F, w.fng, w.fnb, reinterpret_cast<float*>(ffn2_16), F, M, F, F,
                               d->cfg.ln_eps, s, 1, 1))) return rc;
    return gemm_bf16(ffn2_16, F, d->tt.get_bf16(w.prefix + "feed_forward.w_2.weight", s), F, nullptr, out, D, M, D, F, 0, nullptr, 0, 0, s);
}

// ---- THE block step of the offline forwards. What a forward tells it about the token rows in flight:
struct DecRows {
    int mode;           // arithmetic of the FFN: 0 fp32, 1 bf16 operands, 2 bf16x3 (w_1 on three planes), 3 f16x2
    int M;              // rows per token-side op: B * N, or the valid rows when they are packed
    int B, N;           // sequences and padded tokens per sequence (the FSMN runs per sequence, along tokens)
    const int* offs;    // packed rows: device offsets per sequence (FsmnArgs.offs); nullptr: the padded layout
    int left_pad;       // FSMN taps left of the centre: (K - 1) / 2 + sanm_shfit in the attention blocks, (K - 1) / 2 in decoders2
    hipStream_t s;
};
// out = FFN(norm1(x)) in the forward's arithmetic (decoders3 is this alone)
static int dec_ffn_rows(Decoder* d, const DecLayerW& w, const float* x, float* out, const DecRows& r) {
    if (r.mode == 3) return dec_ffn_x2(d, w, x, out, r.M, r.s);
    if (r.mode == 1) return dec_ffn_bf16(d, w, x, out, r.M, r.s);
    const unsigned short* w1_3 = nullptr;
    if (r.mode == 2 && !(w1_3 = d->tt.get_split3(w.prefix + "feed_forward.w_1.weight", d->cfg.ffn_dim, d->cfg.d_model, r.s))) return -2;
    return dec_ffn(d, w, x, out, r.M, r.s, w1_3);
}
// DecoderLayerSANM.forward up to its cross-attention (paraformer/decoder.py:78-107), all of it for a decoders2 block:
// tgt = FFN(norm1(x)) -> norm2 -> x = x + fsmn(tgt), in place on x (d->t2 and d->t1 hold the two intermediates)
static int dec_block_step(Decoder* d, const DecLayerW& w, float* x, const DecRows& r) {
    const int D = d->cfg.d_model;
    float* t1 = d->t1.as<float>();
    float* t2 = d->t2.as<float>();
    int rc;
    if ((rc = dec_ffn_rows(d, w, x, t2, r))) return rc;
    if ((rc = layernorm(t2, D, w.n2g, w.n2b, t1, D, r.M, D, D, d->cfg.ln_eps, r.s))) return rc;
    FsmnArgs fa{};
    fa.in = t1; fa.ldin = D; fa.w = w.fsmn_w; fa.R = x; fa.ldr = D; fa.out = x; fa.ldo = D;
    fa.lens = d->tok_lens.as<int>(); fa.B = r.B; fa.T = r.N; fa.C = D; fa.K = d->cfg.kernel_size; fa.left_pad = r.left_pad;
    fa.offs = r.offs;
    return fsmn(fa, r.s);
}

// bf16-operand decoder (throughput mode): every GEMM and the cross-attention take bf16 operands with fp32
// accumulation; the token stream x, the FSMN and the LayerNorm statistics stay fp32. Expects x = embeds and the
// length arrays already staged by pf_decoder_forward.
static int decoder_forward_bf16(Decoder* d, const float* memory, int B, int T, int N, int32_t* ids, float* hidden_out, hipStream_t s) {
    const pf_decoder_config& c = d->cfg;
    const int D = c.d_model, F = c.ffn_dim, V = c.vocab_size, Mq = B * N, Mk = B * T;
    typedef unsigned short u16;
    if (d->t16.ensure(sizeof(u16) * (size_t)Mq * D) || d->ffn16.ensure(sizeof(u16) * (size_t)Mq * F) ||
        d->ffn2_16.ensure(sizeof(u16) * (size_t)Mq * F) || d->q16.ensure(sizeof(u16) * (size_t)Mq * D) ||
        d->kv16.ensure(sizeof(u16) * (size_t)Mk * 2 * D) || d->ctx16.ensure(sizeof(u16) * (size_t)Mq * D) ||
        d->mem16.ensure(sizeof(u16) * (size_t)Mk * D) || d->hid16.ensure(sizeof(u16) * (size_t)Mq * D))
        return -2;
    u16* t16 = d->t16.as<u16>(); u16* q16 = d->q16.as<u16>(); u16* kv16 = d->kv16.as<u16>(); u16* ctx16 = d->ctx16.as<u16>();
    u16* mem16 = d->mem16.as<u16>();
    float* x = d->x.as<float>(); float* t2 = d->t2.as<float>();
    int rc;
    if ((rc = launch_cast_bf16(memory, mem16, (size_t)Mk * D, s))) return rc;
    auto w16 = [&](const std::string& name) { return d->tt.get_bf16(name, s); };
    DecRows rows{1, Mq, B, N, nullptr, (c.kernel_size - 1) / 2 + (c.sanm_shift > 0 ? c.sanm_shift : 0), s};
    for (const DecLayerW& w : d->layers) {
        const std::string& p = w.prefix;
        if ((rc = dec_block_step(d, w, x, rows))) return rc;
        if ((rc = launch_layernorm(x, D, w.n3g, w.n3b, reinterpret_cast<float*>(t16), D, Mq, D, D, c.ln_eps, s, 1, 0))) return rc;
        if ((rc = gemm_bf16(t16, D, w16(p + "src_attn.linear_q.weight"), D, w.q_b, q16, D, Mq, D, D, 0, nullptr, 0, 1, s))) return rc;
        if ((rc = gemm_bf16(mem16, D, w16(p + "src_attn.linear_k_v.weight"), D, w.kv_b, kv16, 2 * D, Mk, 2 * D, D, 0, nullptr, 0, 1, s)))
            return rc;
        AttnArgs aa{};
        aa.Q = reinterpret_cast<const float*>(q16); aa.ldq = D; aa.K = reinterpret_cast<const float*>(kv16); aa.ldk = 2 * D;
        aa.V = reinterpret_cast<const float*>(kv16 + D); aa.ldv = 2 * D; aa.O = reinterpret_cast<float*>(ctx16); aa.ldo = D;
        aa.klens = d->mem_lens.as<int>(); aa.B = B; aa.H = c.n_heads; aa.Tq = N; aa.Tk = T;
        aa.scale = powf((float)(D / c.n_heads), -0.5f);
        {
            ProfScope ps(PROF_ATTN, 4.0 * B * (double)N * T * D, s);
            if ((rc = launch_attention_bf16(aa, s))) return rc;
        }
        if ((rc = gemm_bf16(ctx16, D, w16(p + "src_attn.linear_out.weight"), D, w.o_b, x, D, Mq, D, D, 0, x, D, 0, s))) return rc;
    }
    rows.left_pad = (c.kernel_size - 1) / 2;                       // decoders2 (decoder.py:363-380): no cross-attention, taps centred
    for (const DecLayerW& w : d->layers2) if ((rc = dec_block_step(d, w, x, rows))) return rc;
    if ((rc = dec_ffn_rows(d, d->last, x, t2, rows))) return rc;
    u16* hid16 = d->hid16.as<u16>();
    if (hidden_out) {
        if ((rc = layernorm(t2, D, d->tt.get("after_norm.weight"), d->tt.get("after_norm.bias"), hidden_out, D, Mq, D, D,
                            c.ln_eps, s))) return rc;
    }
    if (!ids) return 0;
    if ((rc = launch_layernorm(t2, D, d->tt.get("after_norm.weight"), d->tt.get("after_norm.bias"),
                               reinterpret_cast<float*>(hid16), D, Mq, D, D, c.ln_eps, s, 1, 0))) return rc;
    const u16* ow = w16("output_layer.weight");
    if (!ow) return -2;
    if (argmax_scratch(d->pval, d->pidx, Mq, argmax_f32_parts(V))) return -2;
    return argmax_f32(reinterpret_cast<const float*>(hid16), D, reinterpret_cast<const float*>(ow), D, d->tt.get("output_layer.bias"),
                      Mq, V, D, 1, d->pval.as<float>(), d->pidx.as<int>(), ids, s);
}

static pf_decoder* decoder_create_impl(const pf_decoder_config* cfg, bool contextual) {
    if (!cfg) { set_error("decoder: null config"); return nullptr; }
    if (check_device()) return nullptr;
    const pf_decoder_config& c = *cfg;
    const int dk = (c.n_heads > 0 && c.d_model > 0) ? c.d_model / c.n_heads : 0;
    if (c.d_model <= 0 || c.n_heads <= 0 || c.d_model % c.n_heads || !(dk == 128 || (dk <= 64 && dk % 4 == 0 && !contextual)) ||
        c.ffn_dim % 32 || c.d_model % 32 || c.n_blocks < 1 || (c.kernel_size != 11 && c.kernel_size != 21) ||
        (c.kernel_size == 21 && c.sanm_shift > 0) || c.vocab_size < 0) {
        set_error("decoder: unsupported config (need d_model/n_heads == 128, or <= 64 for the small-head kernel in the fp32 mode of the plain decoder; kernel_size 11 or 21 (21: sanm_shfit 0), "
                  "dims % 32 == 0; vocab_size 0 = no output layer)");
        return nullptr;
    }
    std::unique_ptr<Decoder> d(new Decoder());
    d->cfg = c;
    d->precision = (c.n_heads > 0 && c.d_model / c.n_heads == 128 && c.d_model % 256 == 0 && c.ffn_dim % 256 == 0) ? 3 : 0;
    d->contextual = contextual;
    const int D = c.d_model;
    int rc = 0;
    for (int i = 0; i < c.n_blocks; ++i) rc |= dec_layer_add(d->tt, c, dec_layer_prefix(contextual, c.n_blocks, i), DEC_FFN_FSMN_ATTN);
    if (contextual) {
        rc |= d->tt.add("bias_decoder.norm3.weight", D);
        rc |= d->tt.add("bias_decoder.norm3.bias", D);
        rc |= d->tt.add("bias_decoder.src_attn.linear_q.weight", (int64_t)D * D);
        rc |= d->tt.add("bias_decoder.src_attn.linear_q.bias", D);
        rc |= d->tt.add("bias_decoder.src_attn.linear_k_v.weight", (int64_t)2 * D * D);
        rc |= d->tt.add("bias_decoder.src_attn.linear_k_v.bias", 2 * D);
        rc |= d->tt.add("bias_decoder.src_attn.linear_out.weight", (int64_t)D * D);
        rc |= d->tt.add("bias_decoder.src_attn.linear_out.bias", D);
        rc |= d->tt.add("bias_output.weight", (int64_t)D * 2 * D);
    }
    rc |= dec_layer_add(d->tt, c, "decoders3.0.", DEC_FFN);
    rc |= d->tt.add("after_norm.weight", D);
    rc |= d->tt.add("after_norm.bias", D);
    if (c.vocab_size > 0) {          // SeACo's bias decoder has no output layer (use_output_layer: false)
        rc |= d->tt.add("output_layer.weight", (int64_t)c.vocab_size * D);
        rc |= d->tt.add("output_layer.bias", c.vocab_size);
    }
    if (rc) return nullptr;
    return reinterpret_cast<pf_decoder*>(d.release());
}

// asf_layer >= 0: run blocks 0 .. asf_layer - 1, then block asf_layer up to its cross-attention SCORES and return the
// attention-score filter of sequence 0 in asf_scores [T] (decoder.py:485-513 forward_asf6 / :696-714 get_attn_mat)
static int decoder_forward_impl(Decoder* d, const float* memory, const int32_t* mem_lens, const float* embeds,
                                const int32_t* tok_lens, int32_t B, int32_t T, int32_t N, float* logits, int32_t* ids,
                                float* hidden_out, hipStream_t s, int asf_layer, float* asf_scores, const DecCtxArgs* cx = nullptr) {
    PF_REQUIRE(d && memory && mem_lens && embeds && tok_lens && B > 0 && T > 0 && N > 0, "decoder_forward: null/empty");
    for (int b = 0; b < B; ++b) {
        PF_REQUIRE(mem_lens[b] >= 1 && mem_lens[b] <= T, "decoder_forward: memory lens out of range");
        PF_REQUIRE(tok_lens[b] >= 0 && tok_lens[b] <= N, "decoder_forward: token lens out of range");
    }
    PF_REQUIRE(d->precision == 0 || d->cfg.d_model / d->cfg.n_heads == 128, "decoder_forward: heads of d_k <= 64 exist in the fp32 mode only");
    int rc;
    if ((rc = decoder_prepare(d, d->precision == 3 && asf_layer < 0 && !cx, s))) return rc;
    const pf_decoder_config& c = d->cfg;
    const int D = c.d_model, F = c.ffn_dim, V = c.vocab_size;
    int Mq = B * N;                                          // rows processed per token-side op (shrinks when packed, below)
    const int Mq_pad = B * N, Mk = B * T;
    if (d->x.ensure(sizeof(float) * (size_t)Mq * D) || d->t1.ensure(sizeof(float) * (size_t)Mq * D) ||
        d->t2.ensure(sizeof(float) * (size_t)Mq * D) || d->ffn.ensure(sizeof(float) * (size_t)Mq * F) ||
        d->ffn2.ensure(sizeof(float) * (size_t)Mq * F) || d->q.ensure(sizeof(float) * (size_t)Mq * D) ||
        d->kv.ensure(sizeof(float) * (size_t)Mk * 2 * D) || d->ctx.ensure(sizeof(float) * (size_t)Mq * D) ||
        d->hid.ensure(sizeof(float) * (size_t)Mq * D))
        return -2;
    if ((rc = upload_lens(d->mem_lens, mem_lens, B, s))) return rc;
    if ((rc = upload_lens(d->tok_lens, tok_lens, B, s))) return rc;
    float* x = d->x.as<float>();
    float* t1 = d->t1.as<float>();
    float* t2 = d->t2.as<float>();
    // the f16x2 greedy route may pack the token rows instead (below); every other route starts from the padded embeddings
    const bool may_pack = d->precision == 3 && asf_layer < 0 && !cx && ids && !logits && !hidden_out && V > 0;
    if (!may_pack) PF_HIP_TRY(hipMemcpyAsync(x, embeds, sizeof(float) * (size_t)Mq * D, hipMemcpyDeviceToDevice, s));
    if (V == 0 && asf_layer < 0) PF_REQUIRE(!logits && !ids && hidden_out && d->precision != 1,
                           "decoder_forward: a decoder without output layer returns hidden states only (fp32 / bf16x3)");
    PF_REQUIRE(d->contextual == (cx != nullptr) || asf_layer >= 0, "decoder_forward: a contextual decoder runs through pf_decoder_forward_contextual");
    if (d->precision == 1 && !logits && asf_layer < 0 && !cx) return decoder_forward_bf16(d, memory, B, T, N, ids, hidden_out, s);
    // bf16x3 mode: the two GEMMs that are large at every batch size (w_1: N = ffn_dim; linear_k_v: M = B * T) take
    // three-plane operands on the bf16 matrix cores; the D x D projections and w_2 keep the fp32 MFMA tiles
    const bool x3 = d->precision == 2 && asf_layer < 0 && !cx;
    const bool x2 = d->precision == 3 && asf_layer < 0 && !cx;      // the score filter / hotword branch run on the fp32 kernels
    const int Tp = round_up(T, 16), Mkp = B * Tp;           // f16x2: padded key rows per sequence
    // profiling scopes count algorithmic work: valid memory rows, valid (token, frame) pairs
    double mem_rows = 0, tok_mem = 0;
    for (int b = 0; b < B; ++b) { mem_rows += mem_lens[b]; tok_mem += (double)mem_lens[b] * tok_lens[b]; }
    const unsigned short* mem3 = nullptr;
    const unsigned short* mem2 = nullptr;
    float* dsc = nullptr;
    if (x2) {
        // f16x2 mode: w_1, w_2, linear_q, linear_k_v on the fp16 matrix cores (gemm_f16x2.hip). The memory planes' scale
        // is chosen on the device from max |memory| (no host round trip); linear_out keeps the fp32 MFMA tile (its operand,
        // the attention output, has no a-priori bound here)
        const size_t cap_k = d->k2.cap, cap_v = d->vt2.cap;
        if (d->t16.ensure(sizeof(unsigned short) * 2 * (size_t)Mq * D) || d->ffn16.ensure(sizeof(unsigned short) * 2 * (size_t)Mq * F) ||
            d->q16.ensure(sizeof(unsigned short) * 2 * (size_t)Mq * D) || d->ctx16.ensure(sizeof(unsigned short) * 2 * (size_t)Mq * D) ||
            d->mem16.ensure(sizeof(unsigned short) * 2 * (size_t)Mkp * D) || d->dsc.ensure(sizeof(float) * 4) ||
            d->k2.ensure(sizeof(unsigned short) * 2 * ((size_t)Mkp + 32) * D) || d->vt2.ensure(sizeof(unsigned short) * 2 * D * ((size_t)Mkp + 64)) ||
            d->dscl.ensure(sizeof(float) * 4 * c.n_blocks))
            return -2;
        // rows / columns past the last sequence are read by the last key tile (and masked): keep them finite
        if (d->k2.cap != cap_k) PF_HIP_TRY(hipMemsetAsync(d->k2.p, 0, d->k2.cap, s));
        if (d->vt2.cap != cap_v) PF_HIP_TRY(hipMemsetAsync(d->vt2.p, 0, d->vt2.cap, s));
        dsc = d->dsc.as<float>();
        if ((rc = launch_absmax(memory, (size_t)Mk * D, dsc, s))) return rc;
        if ((rc = launch_pow2_scale(dsc, dsc + 1, s))) return rc;
        if ((rc = launch_kv_scales(dsc, d->dlb.as<float>(), c.n_blocks, d->dscl.as<float>(), s))) return rc;
        // memory planes in the padded row layout of attention_f16x2.hip (Tp rows per sequence, padding rows zero)
        if ((rc = launch_split2(memory, D, d->mem16.as<unsigned short>(), D, (size_t)Mkp * D, Mkp, D, 1.f, s, dsc + 1, Tp, T))) return rc;
        mem2 = d->mem16.as<unsigned short>();
    }
    // Token packing (f16x2 greedy route): a batch is padded to its longest hypothesis (N = max token count), but every
    // token-side op is row-wise except the FSMN (per sequence, along tokens) and the attention (per query). So only the
    // VALID token rows are processed, packed back to back: sequence b owns rows [offs[b], offs[b] + tok_lens[b]). The FSMN
    // and the attention kernel take the offsets; ids are scattered back to the caller's [B, N] layout at the end.
    bool pack = false;
    const int* offs_dev = nullptr;
    if (may_pack) {
        int total = 0;
        d->h_offs.assign((size_t)B + 1, 0);
        for (int b = 0; b < B; ++b) { d->h_offs[b] = total; total += tok_lens[b]; }
        d->h_offs[B] = total;
        if (total > 0 && total < Mq_pad) {
            d->h_map.resize((size_t)total);
            for (int b = 0; b < B; ++b) for (int t = 0; t < tok_lens[b]; ++t) d->h_map[(size_t)d->h_offs[b] + t] = b * N + t;
            if (d->offs_dev.ensure(sizeof(int32_t) * ((size_t)B + 1)) || d->map_dev.ensure(sizeof(int32_t) * (size_t)Mq_pad) ||
                d->ids_packed.ensure(sizeof(int32_t) * (size_t)Mq_pad)) return -2;
            if (upload_h2d(d->offs_dev.p, d->h_offs.data(), sizeof(int32_t) * ((size_t)B + 1), s) ||
                upload_h2d(d->map_dev.p, d->h_map.data(), sizeof(int32_t) * (size_t)total, s)) return -2;
            if ((rc = launch_gather_rows(embeds, D, Mq_pad, d->map_dev.as<int>(), x, total, D, s))) return rc;
            pack = true; offs_dev = d->offs_dev.as<int>(); Mq = total;
        }
    }
    if (may_pack && !pack) PF_HIP_TRY(hipMemcpyAsync(x, embeds, sizeof(float) * (size_t)Mq * D, hipMemcpyDeviceToDevice, s));
    if (x3) {
        if (d->t16.ensure(sizeof(unsigned short) * 3 * (size_t)Mq * D) || d->mem16.ensure(sizeof(unsigned short) * 3 * (size_t)Mk * D))
            return -2;
        if ((rc = launch_split3(memory, D, d->mem16.as<unsigned short>(), D, (size_t)Mk * D, Mk, D, s))) return rc;
        mem3 = d->mem16.as<unsigned short>();
    }
    DecRows rows{x2 ? 3 : x3 ? 2 : 0, Mq, B, N, offs_dev, (c.kernel_size - 1) / 2 + (c.sanm_shift > 0 ? c.sanm_shift : 0), s};
    for (int l = 0; l < c.n_blocks; ++l) {
        const DecLayerW& w = d->layers[l];
        // DecoderLayerSANM.forward (paraformer/decoder.py:78-121)
        if ((rc = dec_block_step(d, w, x, rows))) return rc;                                  // FFN, norm2, x = residual + fsmn
        if (x2) {                                                                             // norm3 -> linear_q
            unsigned short* t2p = d->t16.as<unsigned short>();
            {
                ProfScope ps(PROF_LN, 8.0 * Mq * (double)D, s);
                if ((rc = launch_layernorm(x, D, w.n3g, w.n3b, reinterpret_cast<float*>(t2p), D, Mq, D, D, c.ln_eps, s, 3, 0,
                                           (size_t)Mq * D, pow2f(w.e_n3)))) return rc;
            }
            Gemm2Args g{};                                                                    // q planes, pre-multiplied by d_k^-0.5
            g.A = t2p; g.lda = D; g.a_plane = (size_t)Mq * D; g.W = w.q_2; g.ldw = D; g.w_plane = (size_t)D * D;
            g.oscale = pow2f(-(w.e_n3 + w.ew_q)); g.bias = w.q_b; g.C2 = d->q16.as<unsigned short>(); g.ldc2 = D;
            g.c_plane = (size_t)Mq * D; g.cscale = powf((float)(D / c.n_heads), -0.5f) * pow2f(w.e_q);
            g.M = Mq; g.N = D; g.K = D;
            ProfScope ps(PROF_GEMM3, 2.0 * Mq * (double)D * D, s);
            if ((rc = launch_gemm_f16x2(g, s))) return rc;
        } else {
            if ((rc = layernorm(x, D, w.n3g, w.n3b, t1, D, Mq, D, D, c.ln_eps, s))) return rc;    // norm3
            if ((rc = gemm_simple(t1, D, w.q_w, D, w.q_b, d->q.as<float>(), D, Mq, D, D, 0, nullptr, 0, nullptr, 0, s)))
                return rc;
        }
        if (x2) {
            // linear_k_v in its KV form: K planes and V^T planes straight into the attention kernel's operand layout
            const float* lsc = d->dscl.as<float>() + 4 * l;
            unsigned short* k2 = d->k2.as<unsigned short>();
            unsigned short* vt2 = d->vt2.as<unsigned short>();
            {
                Gemm2Args g{};
                g.A = mem2; g.lda = D; g.a_plane = (size_t)Mkp * D; g.W = w.kv_2; g.ldw = D; g.w_plane = (size_t)2 * D * D;
                g.oscale = pow2f(-w.ew_kv); g.oscale_dev = dsc + 2; g.bias = w.kv_b; g.M = Mkp; g.N = 2 * D; g.K = D;
                g.qkv_D = D; g.kv_form = 1; g.Kp = k2; g.qk_plane = ((size_t)Mkp + 32) * D; g.VT = vt2; g.ldvt = Mkp + 64;
                g.vt_plane = (size_t)D * (Mkp + 64); g.k_mul = 1.f; g.v_mul = 1.f; g.kv_mul_dev = lsc;
                ProfScope ps(PROF_GEMM3, 2.0 * mem_rows * 2.0 * D * D, s);
                if ((rc = launch_gemm_f16x2(g, s))) return rc;
            }
            {
                Attn2Args aa{};
                aa.Q = d->q16.as<unsigned short>(); aa.ldq = D; aa.q_plane = (size_t)Mq * D;
                aa.K = k2; aa.ldk = D; aa.k_plane = ((size_t)Mkp + 32) * D; aa.VT = vt2; aa.ldvt = Mkp + 64;
                aa.vt_plane = (size_t)D * (Mkp + 64); aa.O = d->ctx16.as<unsigned short>(); aa.ldo = D; aa.o_plane = (size_t)Mq * D;
                aa.klens = d->mem_lens.as<int>(); aa.B = B; aa.H = c.n_heads; aa.Tp = Tp; aa.Tq = N; aa.qoffs = offs_dev;
                aa.sscale = pow2f(-w.e_q); aa.sscale_dev = lsc + 2; aa.oscale = pow2f(-10);        // ctx planes carry v's scale
                aa.variant = 3;                                                                   // lazy rescale (attention_f16x2.hip)
                ProfScope ps(PROF_ATTN, 4.0 * tok_mem * D, s);
                if ((rc = launch_attention_f16x2(aa, s))) return rc;
            }
            if ((rc = gemm2_simple(d->ctx16.as<unsigned short>(), D, Mq, 0, w.o_2, w.ew_o, w.o_b, x, D, D, D, 0, x, D, s, lsc + 3)))
                return rc;                                                                        // x = residual + att
            continue;
        } else if (x3) {
            if ((rc = gemm3_simple(mem3, D, Mk, d->tt.get_split3(w.prefix + "src_attn.linear_k_v.weight", 2 * D, D, s), w.kv_b,
                                   d->kv.as<float>(), 2 * D, 2 * D, D, 0, s))) return rc;
        } else if ((rc = gemm_simple(memory, D, w.kv_w, D, w.kv_b, d->kv.as<float>(), 2 * D, Mk, 2 * D, D, 0, nullptr, 0,
                                     nullptr, 0, s))) return rc;
        const bool ctx_block = cx && l == c.n_blocks - 1;
        if (ctx_block) {
            // x (after the FSMN residual) is x_self_attn: keep it, it is the hotword branch's query and the final residual
            if (d->xself.ensure(sizeof(float) * (size_t)Mq * D) || d->xcat.ensure(sizeof(float) * (size_t)Mq * 2 * D)) return -2;
            PF_HIP_TRY(hipMemcpyAsync(d->xself.p, x, sizeof(float) * (size_t)Mq * D, hipMemcpyDeviceToDevice, s));
        }
        if (l == asf_layer) {
            if (d->asf_p.ensure(sizeof(float) * (size_t)c.n_heads * N * T)) return -2;
            return launch_asf_scores(d->q.as<float>(), D, d->kv.as<float>(), 2 * D, d->asf_p.as<float>(), asf_scores, c.n_heads,
                                     D / c.n_heads, N, T, mem_lens[0], powf((float)(D / c.n_heads), -0.5f), s);
        }
        AttnArgs aa{};
        aa.Q = d->q.as<float>(); aa.ldq = D; aa.K = d->kv.as<float>(); aa.ldk = 2 * D;
        aa.V = d->kv.as<float>() + D; aa.ldv = 2 * D; aa.O = d->ctx.as<float>(); aa.ldo = D;
        aa.klens = d->mem_lens.as<int>(); aa.B = B; aa.H = c.n_heads; aa.Tq = N; aa.Tk = T;
        aa.scale = powf((float)(D / c.n_heads), -0.5f);
        // cross-attention keeps the fp32 MFMA kernel in every fp32-accurate mode: with Tq = tokens (~120) one 128-query
        // block per (utterance, head) is the better shape (102 us vs 111 us for the 256-query split kernel)
        // (heads of d_k <= 64: the small-head kernel, fp32 mode only)
        if ((rc = attention(aa, 4.0 * B * (double)N * T * D, s, false, D / c.n_heads))) return rc;
        if (ctx_block) {
            float* xcat = d->xcat.as<float>();                   // [Mq, 2D]: x_src_attn | cx * clas_scale
            const float* xs = d->xself.as<float>();
            if ((rc = gemm_simple(d->ctx.as<float>(), D, w.o_w, D, w.o_b, xcat, 2 * D, Mq, D, D, 0, nullptr, 0, nullptr, 0, s)))
                return rc;                                                                    // x_src_attn (no residual)
            // bias_decoder: norm3 -> cross-attention over the hotword embeddings (decoder.py:114-130)
            const int Mh = B * cx->n_hot;
            if (d->kv.ensure(sizeof(float) * (size_t)(Mh > Mk ? Mh : Mk) * 2 * D)) return -2;
            std::vector<int32_t> hl((size_t)B, cx->n_hot);
            if ((rc = upload_lens(d->ctx_lens, hl.data(), B, s))) return rc;
            PF_HIP_TRY(hipStreamSynchronize(s));                  // `hl` is a stack object
            if ((rc = layernorm(xs, D, d->tt.get("bias_decoder.norm3.weight"), d->tt.get("bias_decoder.norm3.bias"), t1, D, Mq, D, D,
                                c.ln_eps, s))) return rc;
            if ((rc = gemm_simple(t1, D, d->tt.get("bias_decoder.src_attn.linear_q.weight"), D,
                                  d->tt.get("bias_decoder.src_attn.linear_q.bias"), d->q.as<float>(), D, Mq, D, D, 0, nullptr, 0, nullptr, 0, s))) return rc;
            if ((rc = gemm_simple(cx->info, D, d->tt.get("bias_decoder.src_attn.linear_k_v.weight"), D,
                                  d->tt.get("bias_decoder.src_attn.linear_k_v.bias"), d->kv.as<float>(), 2 * D, Mh, 2 * D, D, 0, nullptr, 0,
                                  nullptr, 0, s))) return rc;
            AttnArgs ab{};
            ab.Q = d->q.as<float>(); ab.ldq = D; ab.K = d->kv.as<float>(); ab.ldk = 2 * D; ab.V = d->kv.as<float>() + D; ab.ldv = 2 * D;
            ab.O = d->ctx.as<float>(); ab.ldo = D; ab.klens = d->ctx_lens.as<int>(); ab.B = B; ab.H = c.n_heads; ab.Tq = N; ab.Tk = cx->n_hot;
            ab.scale = aa.scale;
            if ((rc = attention(ab, 4.0 * B * (double)N * cx->n_hot * D, s))) return rc;
            if ((rc = gemm_simple(d->ctx.as<float>(), D, d->tt.get("bias_decoder.src_attn.linear_out.weight"), D,
                                  d->tt.get("bias_decoder.src_attn.linear_out.bias"), xcat + D, 2 * D, Mq, D, D, 0, nullptr, 0, nullptr, 0, s)))
                return rc;                                                                    // cx
            if (cx->clas_scale != 1.0f && (rc = launch_scale_cols(xcat + D, 2 * D, Mq, D, cx->clas_scale, s))) return rc;
            // bias_output (Conv1d(2D -> D, k = 1, no bias)) and the residual: x = x_self_attn + W [x_src_attn | cx * scale]
            if ((rc = gemm_simple(xcat, 2 * D, d->tt.get("bias_output.weight"), 2 * D, nullptr, x, D, Mq, D, 2 * D, 0, nullptr, 0, xs, D, s)))
                return rc;
            continue;
        }
        if ((rc = gemm_simple(d->ctx.as<float>(), D, w.o_w, D, w.o_b, x, D, Mq, D, D, 0, nullptr, 0, x, D, s)))
            return rc;                                                                        // x = residual + att
    }
    // decoders2: FFN -> norm2 -> FSMN memory + residual, no cross-attention; the blocks are built with sanm_shfit 0 whatever the
    // attention blocks use (decoder.py:363-380, DecoderLayerSANM.forward :97-107 with src_attn None)
    rows.left_pad = (c.kernel_size - 1) / 2;
    for (const DecLayerW& w : d->layers2) if ((rc = dec_block_step(d, w, x, rows))) return rc;
    // decoders3: FFN only, no residual (decoder.py:438, DecoderLayerSANM with self_attn = src_attn = None)
    if ((rc = dec_ffn_rows(d, d->last, x, t2, rows))) return rc;
    float* hid = hidden_out ? hidden_out : d->hid.as<float>();
    if (x2 && V > 0 && ids && !logits && !hidden_out) {
        // greedy route in the f16x2 mode: after_norm writes two-plane operands, the vocabulary projection runs on the fp16
        // matrix cores with the row arg-max fused into its epilogue (no [Mq, V] logits, no fp32 copy of the hidden states)
        int ew_v = 0;
        const unsigned short* wv2 = d->tt.get_split2("output_layer.weight", V, D, &ew_v, s);
        if (!wv2) return -2;
        unsigned short* h2 = d->t16.as<unsigned short>();
        {
            ProfScope ps(PROF_LN, 8.0 * Mq * (double)D, s);
            if ((rc = launch_layernorm(t2, D, d->tt.get("after_norm.weight"), d->tt.get("after_norm.bias"), reinterpret_cast<float*>(h2), D,
                                       Mq, D, D, c.ln_eps, s, 3, 0, (size_t)Mq * D, pow2f(d->e_an)))) return rc;
        }
        if (argmax_scratch(d->pval, d->pidx, Mq, gemm_f16x2_argmax_parts(Mq, V))) return -2;
        rc = argmax_f16x2(h2, D, (size_t)Mq * D, wv2, D, (size_t)V * D, pow2f(-(d->e_an + ew_v)), nullptr, d->tt.get("output_layer.bias"),
                          Mq, V, D, d->pval.as<float>(), d->pidx.as<int>(), pack ? d->ids_packed.as<int>() : ids, s);
        if (rc || !pack) return rc;
        PF_HIP_TRY(hipMemsetAsync(ids, 0, sizeof(int32_t) * (size_t)Mq_pad, s));       // padding positions: id 0, like an untouched row
        return launch_scatter_i32(d->ids_packed.as<int>(), d->map_dev.as<int>(), ids, Mq, s);
    }
    if ((rc = layernorm(t2, D, d->tt.get("after_norm.weight"), d->tt.get("after_norm.bias"), hid, D, Mq, D, D,
                        c.ln_eps, s))) return rc;
    if (V == 0) return 0;
    return vocab_project(hid, Mq, D, d->tt.get("output_layer.weight"), d->tt.get("output_layer.bias"), V, logits, ids,
                         d->pval, d->pidx, s);
}

}  // namespace pf

using namespace pf;

extern "C" {

// --------------------------------------------------------------------------------------------------- decoder
pf_decoder* pf_decoder_create(const pf_decoder_config* cfg) { return decoder_create_impl(cfg, false); }
/* ContextualParaformerDecoder (funasr/models/contextual_paraformer/decoder.py:133-352): n_blocks - 1 standard blocks
 * ("decoders.{i}."), the last block under "last_decoder.", plus the hotword branch "bias_decoder.norm3.*",
 * "bias_decoder.src_attn.linear_{q,k_v,out}.*" and the 1x1 fusion "bias_output.weight" [D, 2D, 1] */
pf_decoder* pf_decoder_create_contextual(const pf_decoder_config* cfg) { return decoder_create_impl(cfg, true); }
void pf_decoder_destroy(pf_decoder* d) { delete reinterpret_cast<Decoder*>(d); }
/* decoders2 (paraformer/decoder.py:363-380, :436-437): n_layers = num_blocks - att_layer_num blocks of FFN + FSMN memory (built with
 * sanm_shfit 0: the taps centred) and NO cross-attention, run between `decoders` and `decoders3`. Tensors "decoders2.<i>.norm1|norm2.*",
 * "decoders2.<i>.feed_forward.*", "decoders2.<i>.self_attn.fsmn_block.weight". Call once, before the first set_tensor. */
int pf_decoder_set_decoders2(pf_decoder* dh, int32_t n_layers) {
    Decoder* d = reinterpret_cast<Decoder*>(dh);
    PF_REQUIRE(d && n_layers >= 0 && n_layers <= 64, "decoder_set_decoders2: null handle or layer count out of range");
    PF_REQUIRE(d->n_blocks2 == 0 || d->n_blocks2 == n_layers, "decoder_set_decoders2: already set");
    if (d->n_blocks2 == n_layers) return 0;
    int rc = 0;
    for (int i = 0; i < n_layers; ++i) rc |= dec_layer_add(d->tt, d->cfg, dec2_layer_prefix(i), DEC_FFN_FSMN);
    if (rc) return -2;
    d->n_blocks2 = n_layers;
    ++d->tt.version;         // the table's structure changed: what was resolved and prepared before is stale
    return 0;
}
int pf_decoder_set_tensor(pf_decoder* dh, const char* name, const float* data, int64_t numel) {
    Decoder* d = reinterpret_cast<Decoder*>(dh);
    PF_REQUIRE(d && name && data, "decoder_set_tensor: null");
    return d->tt.set(name, data, numel);
}
/* same modes as pf_encoder_set_precision; the bf16 mode serves the fused arg-max route (logits_dev == NULL) */
int pf_decoder_set_precision(pf_decoder* dh, int32_t mode) {
    Decoder* d = reinterpret_cast<Decoder*>(dh);
    PF_REQUIRE(d && mode >= 0 && mode <= 3, "decoder_set_precision: mode must be 0 (fp32 MFMA), 1 (bf16 operands), 2 (fp32 via bf16x3) or 3 (fp32 via f16x2)");
    PF_REQUIRE(mode == 0 || d->cfg.d_model / d->cfg.n_heads == 128, "decoder_set_precision: heads of d_k <= 64 exist in the fp32 mode only (attention_small.hip)");
    d->precision = mode;
    return 0;
}
int pf_decoder_missing(const pf_decoder* dh) {
    const Decoder* d = reinterpret_cast<const Decoder*>(dh);
    return d ? d->tt.missing() : -1;
}

int pf_decoder_forward(pf_decoder* dh, const float* memory, const int32_t* mem_lens, const float* embeds,
                       const int32_t* tok_lens, int32_t B, int32_t T, int32_t N, float* logits, int32_t* ids,
                       float* hidden_out, void* stream) {
    return decoder_forward_impl(reinterpret_cast<Decoder*>(dh), memory, mem_lens, embeds, tok_lens, B, T, N, logits, ids,
                                hidden_out, reinterpret_cast<hipStream_t>(stream), -1, nullptr);
}
/* SeACo attention-score filter (seaco_paraformer/model.py:323-335): the bias decoder's blocks 0 .. n_blocks_before - 1 in
 * full, then block n_blocks_before up to its cross-attention probabilities over the T memory rows (= hotword embeddings);
 * scores_dev [T] receives their sum over heads and token positions for sequence 0 (attn[0].sum(0).sum(0)). fp32 kernels. */
int pf_decoder_asf_scores(pf_decoder* dh, const float* memory, const int32_t* mem_lens, const float* embeds,
                          const int32_t* tok_lens, int32_t B, int32_t T, int32_t N, int32_t n_blocks_before,
                          float* scores_dev, void* stream) {
    Decoder* d = reinterpret_cast<Decoder*>(dh);
    PF_REQUIRE(d && scores_dev && n_blocks_before >= 0 && n_blocks_before < d->cfg.n_blocks, "decoder_asf_scores: bad block index");
    return decoder_forward_impl(d, memory, mem_lens, embeds, tok_lens, B, T, N, nullptr, nullptr, nullptr,
                                reinterpret_cast<hipStream_t>(stream), n_blocks_before, scores_dev);
}

/* ContextualParaformerDecoder.forward (contextual_paraformer/decoder.py:293-352): the last attention block's FSMN-side state
 * x_self_attn also queries the hotword embeddings `contextual_dev` [B, n_hot, D] through bias_decoder; its output (times
 * clas_scale) and the block's own cross-attention output are fused by the 1x1 bias_output: x = x_self_attn + W [x_src | cx]. */
int pf_decoder_forward_contextual(pf_decoder* dh, const float* memory, const int32_t* mem_lens, const float* embeds,
                                  const int32_t* tok_lens, const float* contextual_dev, int32_t n_hot, float clas_scale,
                                  int32_t B, int32_t T, int32_t N, float* logits, int32_t* ids, float* hidden_out, void* stream) {
    Decoder* d = reinterpret_cast<Decoder*>(dh);
    PF_REQUIRE(d && d->contextual && contextual_dev && n_hot >= 1, "decoder_forward_contextual: needs a contextual decoder and >= 1 hotword row");
    DecCtxArgs cx{contextual_dev, n_hot, clas_scale};
    return decoder_forward_impl(d, memory, mem_lens, embeds, tok_lens, B, T, N, logits, ids, hidden_out,
                                reinterpret_cast<hipStream_t>(stream), -1, nullptr, &cx);
}

// ------------------------------------------------------------------------------------------------------- ctc
pf_ctc* pf_ctc_create(int32_t d_model, int32_t vocab) {
    if (check_device()) return nullptr;
    if (d_model <= 0 || d_model % 32 || vocab <= 0) { set_error("ctc: d_model % 32 == 0 required"); return nullptr; }
    std::unique_ptr<Ctc> c(new Ctc());
    c->d_model = d_model; c->vocab = vocab;
    c->precision = 3;                        // the fused arg-max route on the fp16 matrix cores (pf_ctc_set_precision(c, 0): fp32 MFMA)
    if (c->tt.add("ctc_lo.weight", (int64_t)vocab * d_model) || c->tt.add("ctc_lo.bias", vocab)) return nullptr;
    return reinterpret_cast<pf_ctc*>(c.release());
}
void pf_ctc_destroy(pf_ctc* c) { delete reinterpret_cast<Ctc*>(c); }
int pf_ctc_set_tensor(pf_ctc* ch, const char* name, const float* data, int64_t numel) {
    Ctc* c = reinterpret_cast<Ctc*>(ch);
    PF_REQUIRE(c && name && data, "ctc_set_tensor: null");
    return c->tt.set(name, data, numel);          // (the f16x2 arg-max route's cached weight planes follow the fp32 master there)
}
int pf_ctc_missing(const pf_ctc* ch) {
    const Ctc* c = reinterpret_cast<const Ctc*>(ch);
    return c ? c->tt.missing() : -1;
}
/* 0 = fp32 MFMA (default); 3 = the arg-max route (logits_dev == NULL) on the fp16 matrix cores from two-plane operands
 * (gemm_f16x2.hip): the hidden states' plane scale is chosen on the device from max |hidden|, fp32-class logits */
int pf_ctc_set_precision(pf_ctc* ch, int32_t mode) {
    Ctc* c = reinterpret_cast<Ctc*>(ch);
    PF_REQUIRE(c && (mode == 0 || mode == 3), "ctc_set_precision: mode must be 0 (fp32 MFMA) or 3 (fp32 via f16x2)");
    c->precision = mode;
    return 0;
}
int pf_ctc_greedy(pf_ctc* ch, const float* hidden, int32_t M, int32_t* ids, float* logits, void* stream) {
    Ctc* c = reinterpret_cast<Ctc*>(ch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PF_REQUIRE(c && hidden && M > 0, "ctc_greedy: null/empty");
    if (c->tt.require_all("ctc")) return -3;
    if (c->precision == 3 && ids && !logits && !g_stream_mode && c->d_model % 32 == 0) {
        const int D = c->d_model, V = c->vocab;
        int ew = 0, rc;
        const unsigned short* w2 = c->tt.get_split2("ctc_lo.weight", V, D, &ew, s);
        if (!w2) return -2;
        if (c->h2.ensure(sizeof(unsigned short) * 2 * (size_t)M * D) || c->dsc.ensure(sizeof(float) * 4) ||
            argmax_scratch(c->pval, c->pidx, M, gemm_f16x2_argmax_parts(M, V))) return -2;
        float* dsc = c->dsc.as<float>();
        if ((rc = launch_absmax(hidden, (size_t)M * D, dsc, s))) return rc;
        if ((rc = launch_pow2_scale(dsc, dsc + 1, s))) return rc;
        if ((rc = launch_split2(hidden, D, c->h2.as<unsigned short>(), D, (size_t)M * D, M, D, 1.f, s, dsc + 1))) return rc;
        return argmax_f16x2(c->h2.as<unsigned short>(), D, (size_t)M * D, w2, D, (size_t)V * D, pow2f(-ew), dsc + 2, c->tt.get("ctc_lo.bias"),
                            M, V, D, c->pval.as<float>(), c->pidx.as<int>(), ids, s);
    }
    return vocab_project(hidden, M, c->d_model, c->tt.get("ctc_lo.weight"), c->tt.get("ctc_lo.bias"), c->vocab, logits,
                         ids, c->pval, c->pidx, s);
}

}  // extern "C"
