/*
 * paraformer_hip.h -- C ABI of the MI355X-native (gfx950) Paraformer / SenseVoice inference hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / C++ types. Every module of the
 * reference's operator registry (funasr/register.py `tables`) that sits on the hot path has one opaque
 * handle here, with `create / set_tensor / forward / destroy` entry points whose tensor contract mirrors the
 * reference module's forward():
 *
 *   pf_frontend   <-> WavFrontend.forward                    funasr/frontends/wav_frontend.py:149-196
 *   pf_encoder    <-> SANMEncoder.forward                    funasr/models/sanm/encoder.py:392-461
 *                     SenseVoiceEncoderSmall.forward         funasr/models/sense_voice/model.py:623-655
 *   pf_predictor  <-> CifPredictorV2.forward                 funasr/models/paraformer/cif_predictor.py:253-314
 *                     CifPredictorV3.forward / get_upsample_timestamp (pf_predictor_create_v3, pf_predictor_timestamp)
 *                                                            funasr/models/bicif_paraformer/cif_predictor.py:215-352
 *   pf_decoder    <-> ParaformerSANMDecoder.forward          funasr/models/paraformer/decoder.py:397-449
 *                     (+ log_softmax/argmax of Paraformer.inference, funasr/models/paraformer/model.py:345,642;
 *                      kernel_size 21 / vocab_size 0 = SeACo's bias decoder, funasr/models/seaco_paraformer/model.py:98-108)
 *                     pf_decoder_asf_scores <-> ParaformerSANMDecoder.forward_asf6 as SeACo's hotword filter uses it
 *                                                            funasr/models/paraformer/decoder.py:485-513, seaco_paraformer/model.py:323-335
 *                     pf_decoder_create_contextual / pf_decoder_forward_contextual <-> ContextualParaformerDecoder.forward
 *                                                            funasr/models/contextual_paraformer/decoder.py:133-352
 *   pf_ctc        <-> CTC.log_softmax / argmax               funasr/models/ctc/ctc.py:192-216
 *   pf_k_log_softmax <-> the log_softmax feeding BeamSearchPara / CTCPrefixScorer
 *                                                            funasr/models/paraformer/model.py:345,629-637, transformer/scorers/ctc.py:46
 *   pf_stream     <-> ParaformerStreaming chunk step         funasr/models/paraformer_streaming/model.py
 *   pf_vad, pf_vad_decision <-> FsmnVADStreaming (network / state machine)   funasr/models/fsmn_vad_streaming/{encoder,model}.py
 *   pf_vad_logits, pf_kws_candidates, pf_kws_search <-> FsmnKWS / SanmKWS (FSMN without softmax; KwsCtcPrefixDecoder)
 *                                                            funasr/models/fsmn_kws/model.py, sanm_kws/model.py, utils/kws_utils.py
 *   pf_k_lstm     <-> torch.nn.LSTM layer (hotword encoder of SeACo, seaco_paraformer/model.py:388-424)
 *   pf_campplus   <-> CAMPPlus.forward (speaker embedding)  funasr/models/campplus/model.py, components.py
 *   pf_eres2net   <-> ERes2NetV2SV.forward (speaker embedding)  funasr/models/eres2net/model.py, eres2netv2.py, fusion.py
 *
 * The handle style (opaque pointer, int return codes, library-owned scratch) follows the reference's own C
 * API for the same path, runtime/onnxruntime/include/funasrruntime.h:21-24,58-73. Tensor names accepted by
 * `*_set_tensor` are the reference's state_dict keys relative to the module, e.g.
 * "encoders0.0.self_attn.linear_q_k_v.weight", so a real model.pt loads without a conversion step.
 *
 * Conventions
 *   - `*_dev` pointers are device (HBM) pointers, 16-byte aligned, row-major contiguous float32 unless stated.
 *   - `*_host` pointers are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream). All work is enqueued on it; a
 *     call only synchronises where it has to return a host value (documented per function).
 *   - return value: 0 = ok, -1 = invalid argument, -2 = HIP runtime error, -3 = missing tensor / not ready.
 *     pf_last_error() returns a thread-local message for the last failure.
 *   - the library never falls back to a CPU path: without a gfx950 device every create() fails with -2.
 */
#ifndef PARAFORMER_HIP_H_
#define PARAFORMER_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): everything added since the first release is covered by one number a dlsym-binding host can test -- pf_dp_*
 * (incl. pf_dp_broadcast_raw), pf_stream_step_begin / _end, pf_frontend_set_dither / _verify, pf_paraformer_forward, the
 * pf_k_* measurement entries. A library reporting 1 has none of them.
 * 3 (round 6): + pf_paraformer_begin / pf_paraformer_finish (the split-phase offline forward).
 * 4: + pf_predictor_alphas_begin / pf_predictor_embeds_slot.
 * 5: + pf_frontend_set_window / pf_frontend_set_snip_edges, pf_decoder_set_decoders2,
 *    pf_utterance_mvn / pf_global_mvn. */
#define PF_ABI_VERSION 5

const char* pf_last_error(void);
int pf_abi_version(void);
/* number of visible HIP devices (0 when there is no GPU); never fails */
int pf_device_count(void);

/* Process-wide fence: once on, every frontend handle runs fbank_kernel's cross-check (each frame evaluated twice until two runs
 * agree, pf_frontend_set_verify) whatever its own setting. The library switches it on itself at the first asynchronous streaming
 * step (pf_stream_step_begin); hosts that put several ranks or streams on one GPU call pf_set_concurrency_guard(1). */
int pf_set_concurrency_guard(int32_t on);
int pf_concurrency_guard(void);

/* ------------------------------------------------------------------------------------------------ frontend */
typedef struct pf_frontend pf_frontend;

typedef struct pf_frontend_config {
    int32_t sample_rate;      /* 16000 */
    int32_t frame_length;     /* samples per window: 400 (25 ms)      wav_frontend.py:100,174 */
    int32_t frame_shift;      /* samples per hop:    160 (10 ms)      wav_frontend.py:101 */
    int32_t n_mels;           /* 80                                   wav_frontend.py:99 */
    int32_t lfr_m;            /* 7 frames stacked                     wav_frontend.py:104 */
    int32_t lfr_n;            /* 6 frames hop                         wav_frontend.py:105 */
    float low_freq;           /* 20 Hz (Kaldi default) */
    float high_freq;          /* 0 -> Nyquist */
    float preemph;            /* 0.97 */
    float upscale;            /* 32768: waveform * (1 << 15)          wav_frontend.py:168-169 */
} pf_frontend_config;

pf_frontend* pf_frontend_create(const pf_frontend_config* cfg);
void pf_frontend_destroy(pf_frontend* f);
/* CMVN rows of am.mvn (<AddShift>, <Rescale>; wav_frontend.py:15-60): y = (x + shift) * scale. n = n_mels*lfr_m */
int pf_frontend_set_cmvn(pf_frontend* f, const float* shift_host, const float* scale_host, int32_t n);
/* kaldi.fbank's `dither` (wav_frontend.py:106,171-181; the reference default is 1.0): Gaussian noise of that standard deviation
 * on every sample of every frame, after the 2^15 scaling. 0 (default) = deterministic features. Noise comes from a counter-based
 * generator keyed by `seed` and the number of forwards since this call: the same seed gives the same feature sequence. Parity
 * with the reference is statistical by nature (its noise is torch.randn). */
int pf_frontend_set_dither(pf_frontend* f, float dither, uint64_t seed);
/* Cross-check of the fbank kernel (off by default): every frame is evaluated twice from its samples in registers and re-evaluated
 * until two consecutive results agree in every lane. It is how round 4 located the 'two-process frontend fault' (packed-fp32
 * VALU instructions next to waves of the 128 x 128 f16x2 GEMM; fixed at build level) and stays as a diagnostic. pf_frontend_faults:
 * disagreements seen since the handle was made. */
int pf_frontend_set_verify(pf_frontend* f, int32_t on);
int pf_frontend_faults(pf_frontend* f, uint32_t* count_host);
/* diagnostics: for the first 16 disagreements, 4 x uint32 each: shader-clock cycles of the two evaluations that disagreed, the
 * frame index, the retry number (an evaluation suspended in the middle -- another process's turn on the CU -- shows as a long one) */
int pf_frontend_fault_log(pf_frontend* f, uint32_t* log_host_64);
/* Optional: override the built-in Kaldi tables (float64 cos window, float32 mel triangles as in
 * kaldi-native-fbank feature-window.cc:25-47, mel-computations.cc:118-210) with caller-computed ones, e.g. the
 * float32 tables torchaudio.compliance.kaldi builds. window: [frame_length]; mel: dense [n_mels, 257]. */
int pf_frontend_set_tables(pf_frontend* f, const float* window_host, const float* mel_host);
/* The analysis window by name: hamming (default) | hanning | povey | rectangular | blackman | sine, evaluated as kaldi-native-fbank
 * does (float64 cosines, feature-window.cc:25-55; blackman_coeff 0.42 is Kaldi's default). The reference passes WavFrontend's
 * `window` to kaldi.fbank(window_type=...) (funasr/frontends/wav_frontend.py:178). */
int pf_frontend_set_window(pf_frontend* f, const char* window_type, float blackman_coeff);
/* snip_edges = 0: (n + shift / 2) / shift frames, frame i centred on sample i * shift + shift / 2, the waveform mirrored at both
 * ends (kaldi FrameExtractionOptions.snip_edges, feature-window.cc:66-90,152-171; funasr/frontends/wav_frontend.py:180). Default 1. */
int pf_frontend_set_snip_edges(pf_frontend* f, int32_t on);
/* frames after fbank and after LFR for an utterance of n_samples (by the handle's snip_edges setting) */
int32_t pf_frontend_num_fbank_frames(const pf_frontend* f, int64_t n_samples);
int32_t pf_frontend_num_frames(const pf_frontend* f, int64_t n_samples);
/* wav_dev: [B, wav_stride] float32 in [-1, 1]; n_samples_host: [B]; feats_dev: [B, T_out, n_mels*lfr_m] with
 * T_out >= max_b frames(b), rows past an utterance's length are zero-filled (pad_sequence, :195);
 * feat_lens_host: [B] output. Also accepts fbank_dev != NULL to export the raw [B, T_fb_max, n_mels] log-mel
 * (T_fb_max = max_b fbank frames). Does not synchronise. */
int pf_frontend_forward(pf_frontend* f, const float* wav_dev, int64_t wav_stride, const int32_t* n_samples_host,
                        int32_t B, float* feats_dev, int32_t T_out, int32_t* feat_lens_host, float* fbank_dev,
                        void* stream);

/* ---------------------------------------------------------------------------------- feature normalisation (normalize_classes)
 * The reference's `normalize` modules, applied between the frontend and the encoder (funasr/models/paraformer/model.py:305-306,
 * sense_voice/model.py:836-837). In place on x_dev [B, T, D]; lens_dev: device int32 [B]. No sync.
 * pf_utterance_mvn = UtteranceMVN (funasr/models/normalize/utterance_mvn.py:51-96), its arithmetic step by step -- including that
 * with norm_means the padded rows come out as -mean and, with norm_vars as well, take part in the variance and the divisor is
 * sqrt(std). pf_global_mvn = GlobalMVN.forward (global_mvn.py:66-92) with the mean / std vectors [D] the class derives from its
 * stats file: (x - mean), padded rows zero, / std -- bit-exact. */
int pf_utterance_mvn(float* x_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t D, int32_t norm_means, int32_t norm_vars,
                     float eps, void* stream);
int pf_global_mvn(float* x_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t D, const float* mean_dev, const float* std_dev,
                  int32_t norm_means, int32_t norm_vars, void* stream);

/* ------------------------------------------------------------------------------------------------- encoder */
typedef struct pf_encoder pf_encoder;

typedef struct pf_encoder_config {
    int32_t input_dim;        /* 560 = n_mels * lfr_m                         sanm/encoder.py:197 */
    int32_t d_model;          /* 512  output_size */
    int32_t n_heads;          /* 4    attention_heads (d_k must be 128) */
    int32_t ffn_dim;          /* 2048 linear_units */
    int32_t n_blocks;         /* 50   num_blocks: encoders0 (1) + encoders (n_blocks-1) */
    int32_t tp_blocks;        /* 0 (Paraformer) or 20 (SenseVoiceSmall tp_encoders, sense_voice/model.py:601-612) */
    int32_t kernel_size;      /* 11   FSMN taps */
    int32_t sanm_shift;       /* 0    sanm_shfit */
    float ln_eps;             /* 1e-12 (layer_norm.py:16) / 1e-5 (sense_voice/model.py:300-323) */
} pf_encoder_config;

pf_encoder* pf_encoder_create(const pf_encoder_config* cfg);
void pf_encoder_destroy(pf_encoder* e);
/* data may be a host or a device pointer; the tensor is copied (and repacked) into library-owned HBM */
int pf_encoder_set_tensor(pf_encoder* e, const char* name, const float* data, int64_t numel);
/* number of tensors still missing (0 = ready) */
int pf_encoder_missing(const pf_encoder* e);
/* Arithmetic mode. 3 = "f16x2", THE DEFAULT wherever its kernels exist (d_model / n_heads == 128, d_model % 256 == 0,
 * ffn_dim % 256 == 0; mode 0 otherwise): fp32-class results on the fp16 matrix cores -- every GEMM / attention operand is two
 * fp16 planes of the tensor times a power of two (x 2^e = hi + lo), three MFMA products per operand pair (the GEMMs on
 * v_mfma_f32_16x16x32_f16 over 32-deep K stages, the attention on v_mfma_f32_32x32x16_f16), fp32 accumulate,
 * fp32 residual stream / LayerNorm statistics / softmax / FSMN (gemm_f16x2.hip, gemm_f16x2_row.hip, attention_f16x2.hip).
 * Meets every parity bar of mode 0 (activations <= 1e-3, CIF indices equal to the CPU reference; tests/test_parity_gpu.py,
 * fixture f32_mode) and is the measured mode of bench.py. 0 = every product on the exact fp32 MFMA (the opt-out, 2.4x
 * slower). 1 = bf16 OPERANDS for the GEMMs and the attention with fp32 accumulation (bf16-class error; the reference's own
 * bf16=True casts the whole module, auto_model.py:665-668). 2 = fp32-class results from three bf16 planes per operand, six
 * bf16 MFMA products (gemm_split3.hip). */
int pf_encoder_set_precision(pf_encoder* e, int32_t mode);
/* Row packing (mode 3 only; other modes ignore it). The reference runs the encoder over every row of the padded batch
 * [B, T] (sanm/encoder.py:428-470: masks, not skipping); its consumers read only a prefix of each sequence: the CTC head
 * rows < len (sense_voice/model.py:1014), the CIF predictor rows <= len (the conv at the last valid frame and the tail
 * frame, cif_predictor.py:196-205,275-277), the decoder's cross-attention rows < len. extra_rows >= 0: sequence b gets
 * min(len_b + extra_rows, T) rows, laid out back to back (no alignment padding), identical in value to the same rows of
 * the padded computation up to the summation order of the attention's key tiles; the remaining rows of out_dev are
 * zero. extra_rows >= T keeps every row. extra_rows < 0 (default): padded layout, every row computed. */
int pf_encoder_set_row_packing(pf_encoder* e, int32_t extra_rows);
/* Options of mode 3 that do not change a result bit or only the kernel schedule: key "fuse_row" (1, default: linear_out / w_2
 * in their full-row form, residual adds + the following LayerNorm in the GEMM epilogue; 0: separate launches -- bitwise equal),
 * key "attn_variant" (attention_f16x2.hip: 3 lazy rescale, default; 1 pipelined; 0 plain), key "gemm_tile" (block shape of
 * the block's gemm_f16x2 launches: 0 by shape, default; 1 / 2 the 256 x 128 / 256 x 256 shapes; 5 the 128 x 256 shape with two
 * workgroups per CU -- all bitwise equal). Unknown keys return -1. */
int pf_encoder_set_option(pf_encoder* e, const char* key, int32_t value);
/* SANMVadEncoder (funasr/models/ct_transformer_streaming/encoder.py:175-430, the encoder of CTTransformerStreaming): the
 * SAN-M encoder whose self-attention is causal in every block and, in the last one, masked by the VAD corner of
 * transformer/utils/mask.py:38-52 (queries before vad_pos - 1 do not see keys from vad_pos on). vad_pos_host: one value
 * per sequence of the following forwards (copied), NULL switches the masks off again. fp32 mode, heads of d_k <= 64. */
int pf_encoder_set_vad_mask(pf_encoder* e, const int32_t* vad_pos_host, int32_t B);
/* xs_dev: [B, T, input_dim] (un-scaled features, exactly what SANMEncoder.forward receives), lens_host: [B],
 * pe_dev: [T, input_dim] sinusoidal table (embedding.py:396-420; NULL = library computes it with libm),
 * out_dev: [B, T, d_model]. run_blocks < 0 runs everything incl. the final norm(s); run_blocks = k >= 0 stops
 * after k encoder blocks and returns the raw residual stream (for per-layer parity checks). No sync. */
int pf_encoder_forward(pf_encoder* e, const float* xs_dev, const int32_t* lens_host, int32_t B, int32_t T,
                       const float* pe_dev, float* out_dev, int32_t run_blocks, void* stream);

/* ----------------------------------------------------------------------------------------------- predictor */
typedef struct pf_predictor pf_predictor;

typedef struct pf_predictor_config {
    int32_t d_model;          /* idim 512 */
    int32_t l_order;          /* 1 */
    int32_t r_order;          /* 1 */
    float threshold;          /* 1.0 (the prefix-sum/floor formulation of cif_v1 is only defined for 1.0) */
    float smooth_factor;      /* 1.0 */
    float noise_threshold;    /* 0.0 */
    float tail_threshold;     /* 0.45 */
    int32_t tail_mask;        /* 1 */
} pf_predictor_config;

pf_predictor* pf_predictor_create(const pf_predictor_config* cfg);
void pf_predictor_destroy(pf_predictor* p);
int pf_predictor_set_tensor(pf_predictor* p, const char* name, const float* data, int64_t numel);
int pf_predictor_missing(const pf_predictor* p);
/* Step 1: alphas + fire scan. hidden_dev: [B, T, d_model]; lens_host: [B];
 * alphas_dev / peaks_dev: [B, T+1] outputs (tail-extended alphas, cif_peak); token_num_host: [B] output =
 * number of fired tokens (= floor(sum alphas), cif_predictor.py:443-446). SYNCHRONISES the stream (the token
 * count decides the decoder's shape, like the .item() at cif_predictor.py:311). */
int pf_predictor_alphas(pf_predictor* p, const float* hidden_dev, const int32_t* lens_host, int32_t B, int32_t T,
                        float* alphas_dev, float* peaks_dev, int32_t* token_num_host, void* stream);
/* Step 2: acoustic embeddings for the scan of the last pf_predictor_alphas call: embeds_dev [B, N, d_model],
 * rows >= token_num[b] are zero. No sync. */
int pf_predictor_embeds(pf_predictor* p, const float* hidden_dev, int32_t B, int32_t T, int32_t N,
                        float* embeds_dev, void* stream);
/* The same two steps WITHOUT the synchronisation between them, for callers that keep two batches in flight (round 6; the
 * module-level counterpart of pf_paraformer_begin / _finish, used by the classes whose chain is not the plain offline one --
 * BiCifParaformer: funasr/models/bicif_paraformer/model.py:327-345 reads the counts between predictor and decoder).
 * pf_predictor_alphas_begin: everything of step 1 ENQUEUED into scan state `slot` (0 or 1); the token counts are copied by the
 * stream into counts_pinned_host (B int32 of PINNED host memory that stays alive until the caller has synchronised, e.g. on an
 * event recorded behind this call). pf_predictor_embeds_slot: step 2 for that slot -- before the slot's next _begin.
 * pf_predictor_alphas / _embeds are slot 0 of the same state. */
int pf_predictor_alphas_begin(pf_predictor* p, int32_t slot, const float* hidden_dev, const int32_t* lens_host, int32_t B, int32_t T,
                              float* alphas_dev, float* peaks_dev, int32_t* counts_pinned_host, void* stream);
int pf_predictor_embeds_slot(pf_predictor* p, int32_t slot, const float* hidden_dev, int32_t B, int32_t T, int32_t N,
                             float* embeds_dev, void* stream);

/* CifPredictorV3 (funasr/models/bicif_paraformer/cif_predictor.py:121-384), the predictor of BiCifParaformer and
 * SeACo-Paraformer ("paraformer-zh"): the same first head as V2 but integrated by the sequential fp32 loop `cif`
 * (:39-86), plus a second head on a `upsample_times` x finer time axis that gives the token timestamps
 * (`get_upsample_timestamp`, :301-352). A handle made by pf_predictor_create_v3 answers pf_predictor_alphas /
 * pf_predictor_embeds with V3's arithmetic (token_num = floor(sum alphas), :383) and accepts pf_predictor_timestamp.
 * Extra tensors: upsample_cnn.weight [d, d, U] / .bias [d]; cif_output2.weight [d or 2d] / .bias [1]; for
 * upsample_type 1 blstm.weight_ih_l0[_reverse] [4d, d], blstm.weight_hh_l0[_reverse] [4d, d], blstm.bias_ih_l0[_reverse],
 * blstm.bias_hh_l0[_reverse] [4d] (torch.nn.LSTM's state_dict, gates i, f, g, o). */
typedef struct pf_predictor_v3_config {
    int32_t upsample_times;   /* 3 */
    int32_t upsample_type;    /* 0 "cnn", 1 "cnn_blstm" ("cnn_attn" is not built) */
    int32_t use_cif1_cnn;     /* 0: the second head reads the encoder output, 1: relu(cif_conv1d(.)) */
    float smooth_factor2;     /* 0.25 */
    float noise_threshold2;   /* 0.01 */
} pf_predictor_v3_config;
pf_predictor* pf_predictor_create_v3(const pf_predictor_config* cfg, const pf_predictor_v3_config* cfg3);
/* hidden_dev [B, T, d_model], lens_host [B], token_num_host [B] (the rounded token counts of pf_predictor_alphas) ->
 * us_alphas_dev, us_peaks_dev [B, U * T]: the upsampled weights rescaled to sum to token_num per utterance and their
 * running integral at threshold 1 - 1e-4 (`cif_wo_hidden`, :89-118), the two inputs of ts_prediction_lfr6_standard
 * (funasr/utils/timestamp_tools.py:37). No sync. */
int pf_predictor_timestamp(pf_predictor* p, const float* hidden_dev, const int32_t* lens_host,
                           const int32_t* token_num_host, int32_t B, int32_t T, float* us_alphas_dev, float* us_peaks_dev,
                           void* stream);

/* ------------------------------------------------------------------------------------------------- decoder */
typedef struct pf_decoder pf_decoder;

typedef struct pf_decoder_config {
    int32_t vocab_size;       /* 8404; 0 = no output layer (SeACo's bias decoder): forward returns hidden states only */
    int32_t d_model;          /* 512 */
    int32_t n_heads;          /* 4: d_model / n_heads == 128; heads of d_k <= 64 (a multiple of 4) run in the fp32 mode only, <= 1024 memory rows */
    int32_t ffn_dim;          /* 2048 */
    int32_t n_blocks;         /* 16 = att_layer_num (blocks with cross-attention; decoders2: pf_decoder_set_decoders2) */
    int32_t kernel_size;      /* 11; 21 (with sanm_shift 0) for SeACo's bias decoder */
    int32_t sanm_shift;       /* 0 offline / 5 streaming model */
    float ln_eps;             /* 1e-12 */
} pf_decoder_config;

pf_decoder* pf_decoder_create(const pf_decoder_config* cfg);
void pf_decoder_destroy(pf_decoder* d);
/* decoders2 (funasr/models/paraformer/decoder.py:363-380,436-437): n_layers = num_blocks - att_layer_num further blocks of
 * FFN + FSMN memory (sanm_shfit 0) WITHOUT cross-attention between `decoders` and `decoders3`. Registers the tensors
 * "decoders2.<i>.{norm1,norm2}.{weight,bias}", "decoders2.<i>.feed_forward.*", "decoders2.<i>.self_attn.fsmn_block.weight";
 * call once, right after create. The published recipes have none (att_layer_num == num_blocks). */
int pf_decoder_set_decoders2(pf_decoder* d, int32_t n_layers);
int pf_decoder_set_tensor(pf_decoder* d, const char* name, const float* data, int64_t numel);
int pf_decoder_missing(const pf_decoder* d);
/* 0 = fp32 (default), 1 = bf16 operands for the GEMMs and the cross-attention (see pf_encoder_set_precision; applies
 * to the fused arg-max route, logits_dev == NULL), 2 = w_1 and linear_k_v on the three-plane split GEMM (fp32 results) */
int pf_decoder_set_precision(pf_decoder* d, int32_t mode);
/* memory_dev: [B, T, d_model] encoder output, mem_lens_host: [B]; embeds_dev: [B, N, d_model] CIF output,
 * tok_lens_host: [B]. Outputs (each may be NULL): logits_dev [B, N, vocab] (pre-softmax, decoder.py:444),
 * ids_dev int32 [B, N] = argmax over the vocabulary (fused into the output GEMM when logits_dev is NULL),
 * hidden_dev [B, N, d_model] (after_norm output). No sync. */
int pf_decoder_forward(pf_decoder* d, const float* memory_dev, const int32_t* mem_lens_host,
                       const float* embeds_dev, const int32_t* tok_lens_host, int32_t B, int32_t T, int32_t N,
                       float* logits_dev, int32_t* ids_dev, float* hidden_dev, void* stream);
/* ------------------------------------------------------------------------------------------------ offline pipeline
 * The whole offline forward in one call: what Paraformer.inference runs between the frontend and the tokenizer
 * (funasr/models/paraformer/model.py:286-346, 614-616, 642), at the tensor boundary the reference exports for this path
 * (funasr/models/paraformer/export_meta.py:44-68: speech f32 [B, T, 560], speech_lengths i32 [B] -> logits, token_num; the
 * arg-max is fused here, so token ids come back). The object borrows the three module handles (they must outlive it; a
 * CifPredictorV2 / V3 predictor and a plain ParaformerSANMDecoder) and owns the intermediate buffers; precision, row packing
 * and schedule options are whatever the module handles are set to. Bitwise the chain pf_encoder_forward -> pf_predictor_alphas
 * -> pf_predictor_embeds -> pf_decoder_forward. */
typedef struct pf_paraformer pf_paraformer;
pf_paraformer* pf_paraformer_create(pf_encoder* e, pf_predictor* p, pf_decoder* d);
void pf_paraformer_destroy(pf_paraformer* m);
/* feats_dev [B, T, input_dim], lens_host [B], pe_dev as pf_encoder_forward. Outputs: token_num_host [B] (rounded CIF counts,
 * written after the call's ONE host synchronisation); ids_dev int32 [B, ids_ld] (may be NULL), row b valid in
 * [0, token_num[b]); alphas_dev / peaks_dev [B, T + 1] (may be NULL: kept internally). Returns N = the batch's largest token
 * count (0: nothing fired, ids untouched -- model.py:615-616), or < 0. Everything behind the token count is only ENQUEUED. */
int pf_paraformer_forward(pf_paraformer* m, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t T,
                          const float* pe_dev, int32_t* ids_dev, int32_t ids_ld, int32_t* token_num_host,
                          float* alphas_dev, float* peaks_dev, void* stream);
/* The same forward in its two phases, for serving loops (round 6). pf_paraformer_begin ENQUEUES encoder + predictor (alphas, scan)
 * and the token counts' copy to a pinned host buffer, and returns a ticket (0 / 1) without any host synchronisation;
 * pf_paraformer_finish(ticket) waits for THAT copy (an event of this batch, not the stream), fills token_num_host, enqueues
 * embeds + decoder + arg-max and returns N like pf_paraformer_forward. Two batches may be in flight: issue begin(i + 1) BEFORE
 * finish(i) and the stream holds batch i + 1's encoder while the host reads batch i's counts -- the decoder is still sized by the
 * exact CIF count (cif_predictor.py:311), but the GPU never waits for the host. Tickets are finished in the order they were begun;
 * lens_host is copied by begin. (A V3 predictor keeps one scan state: one batch in flight.) pf_paraformer_forward == begin + finish.
 * `finish` may be given another stream than `begin` (the host has already waited for the batch's scan; the library orders the reuse of
 * the slot with an event): batch i's decoder then runs beside batch i + 1's encoder. ids_dev is valid once finish's stream has reached
 * the end of the call's work. */
int pf_paraformer_begin(pf_paraformer* m, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t T,
                        const float* pe_dev, void* stream);
int pf_paraformer_finish(pf_paraformer* m, int32_t ticket, int32_t* ids_dev, int32_t ids_ld, int32_t* token_num_host,
                         float* alphas_dev, float* peaks_dev, void* stream);
/* the last finished forward's encoder output [B, T, d_model] / acoustic embeddings [B, N, d_model] (library-owned; valid until
 * the next begin into the same slot / the next finish of this object) */
const float* pf_paraformer_encoder_out(const pf_paraformer* m);
const float* pf_paraformer_embeds(const pf_paraformer* m);

/* SeACo attention-score filter (funasr/models/seaco_paraformer/model.py:323-335 over paraformer/decoder.py:485-513
 * `forward_asf6`): blocks 0 .. n_blocks_before - 1 of the (bias) decoder in full, then block n_blocks_before up to its
 * cross-attention probabilities over the T memory rows (the hotword embeddings); scores_dev [T] receives their sum over
 * heads and token positions for sequence 0 (attn_mat[0].sum(0).sum(0)). */
int pf_decoder_asf_scores(pf_decoder* d, const float* memory_dev, const int32_t* mem_lens_host, const float* embeds_dev,
                          const int32_t* tok_lens_host, int32_t B, int32_t T, int32_t N, int32_t n_blocks_before,
                          float* scores_dev, void* stream);
/* ContextualParaformerDecoder (funasr/models/contextual_paraformer/decoder.py:133-352): created like pf_decoder_create with
 * n_blocks = att_layer_num; tensor names "decoders.{0..n_blocks-2}.*", "last_decoder.*", "bias_decoder.norm3.*",
 * "bias_decoder.src_attn.linear_{q,k_v,out}.*", "bias_output.weight", "decoders3.0.*", "after_norm.*", "output_layer.*".
 * forward_contextual additionally takes the hotword embeddings contextual_dev [B, n_hot, d_model] and clas_scale. */
pf_decoder* pf_decoder_create_contextual(const pf_decoder_config* cfg);
int pf_decoder_forward_contextual(pf_decoder* d, const float* memory_dev, const int32_t* mem_lens_host, const float* embeds_dev,
                                  const int32_t* tok_lens_host, const float* contextual_dev, int32_t n_hot, float clas_scale,
                                  int32_t B, int32_t T, int32_t N, float* logits_dev, int32_t* ids_dev, float* hidden_dev,
                                  void* stream);

/* ---------------------------------------------------------------------------------------------------- ctc */
/* ---- FSMN-VAD network (funasr/models/fsmn_vad_streaming/encoder.py:288-378 FSMN.forward), reduced to what the decision
 * logic reads: the summed posterior of the silence pdfs per frame (model.py:783-795), and the frame energies
 * (ComputeDecibel, model.py:513-530). Tensor names as in the reference state_dict below `encoder.`:
 * in_linear1|in_linear2|out_linear1|out_linear2 ".linear.weight|bias", "fsmn.<i>.linear.linear.weight",
 * "fsmn.<i>.fsmn_block.conv_left.weight" ([proj, 1, lorder, 1]), "fsmn.<i>.affine.linear.weight|bias". */
typedef struct pf_vad pf_vad;
typedef struct pf_vad_config {
    int32_t input_dim, input_affine_dim, fsmn_layers, linear_dim, proj_dim, lorder, rorder, lstride, rstride,
        output_affine_dim, output_dim;
} pf_vad_config;
pf_vad* pf_vad_create(const pf_vad_config* cfg);
void pf_vad_destroy(pf_vad* v);
int pf_vad_set_tensor(pf_vad* v, const char* name, const float* data, int64_t numel);
int pf_vad_missing(const pf_vad* v);
/* feats_dev [B, T, input_dim]; cache_dev [B, fsmn_layers, (lorder-1)*lstride, proj_dim]: left context of the memory
 * blocks, read and updated in place (NULL = zero left context); p_sil_dev [B, T]; probs_dev [B, T, output_dim] or NULL;
 * small_m != 0: weight-streaming GEMMs (chunks of a few frames). No sync. */
int pf_vad_forward(pf_vad* v, const float* feats_dev, int32_t B, int32_t T, float* cache_dev, const int32_t* sil_ids_host,
                   int32_t n_sil, float* p_sil_dev, float* probs_dev, int32_t small_m, void* stream);
int pf_vad_frame_decibel(const float* wav_dev, int64_t n_samples, int32_t n_frames, int32_t frame_len, int32_t frame_shift,
                         float* out_dev, void* stream);
/* The same network without its softmax (the FSMN of FsmnKWS: use_softmax false): logits_dev [B * T, ld] receives out_linear2's
 * output (ld % 4 == 0, ld >= output_dim; columns from output_dim on are not written). pf_vad_create takes rorder > 0 (a further
 * tensor "fsmn.<i>.fsmn_block.conv_right.weight" [proj, 1, rorder, 1]; the memory blocks then read future frames of the PADDED
 * batch, as the reference does, and a cache pointer is refused) and output_dim up to 65536; pf_vad_forward refuses
 * output_dim > 512, which its softmax kernel cannot do. No sync. */
int pf_vad_logits(pf_vad* v, const float* feats_dev, int32_t B, int32_t T, float* cache_dev, float* logits_dev, int32_t ld,
                  int32_t small_m, void* stream);

/* ---- keyword spotting (FsmnKWS / SanmKWS; funasr/utils/kws_utils.py KwsCtcPrefixDecoder)
 * pf_kws_candidates: the per-frame candidate step of beam_search (:156-171) for M rows of logits (row stride ld >= V, 3 <= V <=
 * 65536): the three largest of the row in descending order (equal values: the lower index first), p = exp(x - max) / sum exp(x - max),
 * an entry kept if p > 0.05 and bit id of mask_dev (ceil(V / 32) words; bit 0 = blank is always set by pf_kws_search_token_mask) is
 * set. out_dev [M, 7] words per row: n, ids[3] (-1 from n on), the fp32 bits of probs[3] (0 from n on). No sync.
 * pf_kws_search: host code without device work (creating it needs no GPU). Keywords are token-id lists (keyword k =
 * ids[offsets[k] .. offsets[k + 1])). pf_kws_search_decode runs the CTC prefix search (path beam 20) of B clips over the read-back
 * candidates cand_host [B, T, 7] (frames < lens_host[b]) and the hit test of _decode_inside: hit_host[b] = index of the keyword or -1,
 * offset_host[b] (nullable) where it starts in the hypothesis, score_host[b] = sqrt(product of the matched nodes' probabilities).
 * The n-best of the last decode stay readable: pf_kws_search_nbest returns the prefix length of hypothesis i of a clip (final order)
 * and, if it fits `capacity`, its prefix ids and per node token / frame / prob; *score = pb + pnb. */
typedef struct pf_kws_search pf_kws_search;
int pf_kws_candidates(const float* logits_dev, int64_t ld, int32_t M, int32_t V, const uint32_t* mask_dev, int32_t* out_dev,
                      void* stream);
pf_kws_search* pf_kws_search_create(int32_t vocab_size);
void pf_kws_search_destroy(pf_kws_search* k);
int pf_kws_search_set_keywords(pf_kws_search* k, const int32_t* ids, const int32_t* offsets, int32_t n_keywords);
int pf_kws_search_missing(const pf_kws_search* k);   /* 1 until keywords are set */
int pf_kws_search_token_mask(const pf_kws_search* k, uint32_t* mask_host, int32_t n_words);
int pf_kws_search_decode(pf_kws_search* k, const int32_t* cand_host, const int32_t* lens_host, int32_t B, int32_t T,
                         int32_t* hit_host, int32_t* offset_host, double* score_host);
int pf_kws_search_nbest_count(const pf_kws_search* k, int32_t clip);
int pf_kws_search_nbest(const pf_kws_search* k, int32_t clip, int32_t i, int32_t capacity, int32_t* prefix, double* score,
                        int32_t* node_token, int32_t* node_frame, double* node_prob);
/* the FSMN memory block with a right context alone, and the VAD network's left-only block it equals bit for bit at rorder 0 */
int pf_k_kws_fsmn(const float* x, int32_t ldx, const float* w_left, const float* w_right, float* y, int32_t ldy, int32_t B, int32_t T,
                  int32_t C, int32_t lorder, int32_t lstride, int32_t rorder, int32_t rstride, void* stream);
int pf_k_vad_fsmn(const float* x, int32_t ldx, const float* w_left, float* y, int32_t ldy, int32_t B, int32_t T, int32_t C,
                  int32_t lorder, int32_t lstride, void* stream);

/* ---- FSMN-VAD decision logic in native host code (no device work): silence posteriors + frame energies -> speech
 * segments; restates what FsmnVADStreaming.forward does after the network (model.py:552-905,1117-1302). Options = the
 * post-processing section of the model's config.yaml (VADXOptions, model.py:71-173). */
typedef struct pf_vad_decision pf_vad_decision;
typedef struct pf_vad_options {
    int32_t sample_rate, detect_mode, max_end_silence_time, max_start_silence_time, window_size_ms,
        sil_to_speech_time_thres, speech_to_sil_time_thres, do_extend, lookback_time_start_point,
        lookahead_time_end_point, max_single_segment_time, noise_frame_num_used_for_snr, frame_in_ms, frame_length_ms;
    double speech_2_noise_ratio, snr_thres, decibel_thres, speech_noise_thres, fe_prior_thres;
} pf_vad_options;
pf_vad_decision* pf_vad_decision_create(const pf_vad_options* opts);
void pf_vad_decision_destroy(pf_vad_decision* d);
/* the per-block dynamic end-silence schedule of FsmnVADStreaming.inference (model.py:1005-1019) */
void pf_vad_decision_set_thresholds(pf_vad_decision* d, double max_end_sil_ms, double speech_noise_thres);
int pf_vad_decision_state(const pf_vad_decision* d);   /* 1 start point not detected, 2 in speech, 3 end point detected */
/* next block of frames (host arrays). Returns the number of reportable segments (written as [beg_ms, end_ms] pairs up to
 * `capacity`; with streaming_events a started segment is [beg, -1] and closed later by [-1, end]); -1 on error. */
int pf_vad_decision_push(pf_vad_decision* d, const float* sil_scores, const float* decibels, int32_t n_frames,
                         int32_t is_final, int32_t streaming_events, int32_t* segments_out, int32_t capacity);

/* ---- CAM++ speaker embedding (funasr/models/campplus/model.py CAMPPlus.forward, output_level "segment",
 * config_str "batchnorm-relu"). Tensor names are the reference's state_dict keys: "head.conv1.weight", "head.bn1.running_mean",
 * "head.layer1.0.shortcut.0.weight", "xvector.tdnn.linear.weight", "xvector.block1.tdnnd1.cam_layer.linear1.bias",
 * "xvector.transit1.nonlinear.batchnorm.weight", "xvector.dense.nonlinear.batchnorm.running_var", ... (every parameter and
 * BatchNorm running statistic; num_batches_tracked is not taken). BatchNorms that follow a conv are folded into it at the
 * first forward after a set_tensor. Only the published shape is built: feat_dim 80, embedding 192, growth 32, bn_size 4,
 * init_channels 128, m_channels 32. Activations live in a handle-owned workspace (see pf_campplus_set_max_batch). */
typedef struct pf_campplus pf_campplus;
typedef struct pf_campplus_config {
    int32_t feat_dim, embedding_size, growth_rate, bn_size, init_channels, m_channels;
    float bn_eps;             /* 1e-5 (torch BatchNorm default) */
} pf_campplus_config;
pf_campplus* pf_campplus_create(const pf_campplus_config* cfg);
void pf_campplus_destroy(pf_campplus* h);
int pf_campplus_set_tensor(pf_campplus* h, const char* name, const float* data, int64_t numel);
int pf_campplus_missing(const pf_campplus* h);
/* chunks per launch sequence (default 256); never changes a result bit. The workspace grows with chunks x frames (about 31 KB per
 * input frame: the head's three 80 x 32 planes): this bounds it for the fixed 1.5-s chunks of embed_chunks, while ONE long
 * utterance through pf_campplus_forward needs workspace for its whole length (about 11 GB per hour of audio). */
int pf_campplus_set_max_batch(pf_campplus* h, int32_t max_chunks);
/* feats_dev [B, T, feat_dim] (already mean-normalised, as extract_feature gives them) -> emb_dev [B, embedding_size].
 * T must give at least 2 frames after the stride-2 TDNN (T >= 3). No sync. */
int pf_campplus_forward(pf_campplus* h, const float* feats_dev, int32_t B, int32_t T, float* emb_dev, void* stream);
/* N chunks of chunk_len samples cut from one device waveform wav_dev [n_samples]: chunk i = samples
 * [starts_host[i], starts_host[i] + valid_host[i]) followed by zeros up to chunk_len (valid_host NULL: chunk_len samples; samples
 * past the waveform read as zero) -> kaldi fbank (80 bins, povey window, no 2^15 scaling, dither 0, snip_edges) -> minus the
 * chunk's time mean -> the network -> emb_dev [N, embedding_size]. Every chunk's embedding is bitwise independent of N. No sync. */
int pf_campplus_embed_chunks(pf_campplus* h, const float* wav_dev, int64_t n_samples, const int64_t* starts_host,
                             const int32_t* valid_host, int32_t N, int32_t chunk_len, float* emb_dev, void* stream);

/* ---- ERes2NetV2 speaker embedding (funasr/models/eres2net/model.py ERes2NetV2SV.forward, eres2netv2.py, fusion.py; baseWidth 26,
 * scale 2, expansion 2, TSTP pooling, one embedding layer). Tensor names are the reference's state_dict keys: "model.conv1.weight",
 * "model.bn1.running_mean", "model.layer1.0.convs.1.weight", "model.layer2.0.shortcut.1.running_var",
 * "model.layer3.0.fuse_models.0.local_att.0.bias", "model.layer3_ds.weight", "model.fuse34.local_att.4.weight", "model.seg_1.bias", ...
 * (every parameter and BatchNorm running statistic; num_batches_tracked is not taken). Every BatchNorm is folded into the conv in
 * front of it at the first forward after a set_tensor. Built: feat_dim 8 .. 128 and m_channels 8 .. 64 in multiples of 8, any four
 * positive num_blocks, embedding_size >= 1. fp32-class arithmetic on the exact-f32 MFMA, the only mode. */
typedef struct pf_eres2net pf_eres2net;
typedef struct pf_eres2net_config {
    int32_t feat_dim, embedding_size, m_channels;
    int32_t num_blocks[4];
    float bn_eps;             /* 1e-5 (torch BatchNorm default) */
} pf_eres2net_config;
pf_eres2net* pf_eres2net_create(const pf_eres2net_config* cfg);
void pf_eres2net_destroy(pf_eres2net* h);
int pf_eres2net_set_tensor(pf_eres2net* h, const char* name, const float* data, int64_t numel);
int pf_eres2net_missing(const pf_eres2net* h);
/* chunks per launch sequence (default 256); never changes a result bit. The workspace of a sub-batch is
 * pf_eres2net_workspace_bytes(h, T) per chunk of T frames: twice the largest block input / output ([T, F, 2 m_channels] floats at
 * layer 1), twice the largest split / concat buffer ([T, F, 2 pad4(width)]), and the smaller AFF, layer3_ds, pool and embedding
 * buffers -- about 20 MB per 1.5-s chunk (150 frames) at the default configuration, 5.2 GB for 256 chunks. One long utterance through
 * pf_eres2net_forward needs that for its whole length. */
int pf_eres2net_set_max_batch(pf_eres2net* h, int32_t max_chunks);
int64_t pf_eres2net_workspace_bytes(const pf_eres2net* h, int32_t T);
/* test hook: fills every workspace buffer the handle owns with NaN bytes (after a device synchronise) */
int pf_eres2net_debug_poison(pf_eres2net* h);
/* feats_dev [B, T, feat_dim] (already mean-normalised, as extract_feature gives them) -> emb_dev [B, embedding_size].
 * T >= 9: fewer frames leave one after the three stride-2 stages and the pool's standard deviation is undefined. No sync. */
int pf_eres2net_forward(pf_eres2net* h, const float* feats_dev, int32_t B, int32_t T, float* emb_dev, void* stream);
/* test hook: pf_eres2net_forward of one sub-batch (B <= max_batch) that also copies out what the network computes on the way.
 * stages_dev: host array of 8 device pointers, each nullable: the stem, layer1 .. layer4, layer3_ds and fuse34 outputs
 * (channels-last [B, t, f, c]) and the pooled statistics [B, 2 S]. */
int pf_eres2net_forward_stages(pf_eres2net* h, const float* feats_dev, int32_t B, int32_t T, float* emb_dev, float* const* stages_dev,
                               void* stream);
/* as pf_campplus_embed_chunks (same gather, fbank with feat_dim bins, mean removal and zero-padding rule for short segments), then
 * this network. Chunks of fewer than 9 frames are refused. Every chunk's embedding is bitwise independent of N. No sync. */
int pf_eres2net_embed_chunks(pf_eres2net* h, const float* wav_dev, int64_t n_samples, const int64_t* starts_host,
                             const int32_t* valid_host, int32_t N, int32_t chunk_len, float* emb_dev, void* stream);
/* single-kernel hook (tests): ONE launch of the network's implicit-GEMM conv kernel on caller-supplied device buffers.
 * Activations are channels-last [n_chunks, t, f, c] with row strides (lda, lda2, ldc, ...) in floats; a_col / a2_col / c_col select a
 * column slice of a wider buffer (a_col, a2_col and the strides of A, A2 and W are multiples of 4, their bases 16-byte aligned).
 * C[m, n] = epilogue(sum_k A[m, k] W[n, k]) over rows m = ((chunk * To + to) * Fo + fo), To = (tin - 1) / st + 1, Fo likewise:
 *   taps 1 or 9 (3x3, padding 1, tap = kf * 3 + kt), strides st (time) and sf (frequency) in {1, 2}; k = tap * pad4(cin) + c;
 *   zero outside the row's own chunk; channels c >= cin of A are never used (W's columns there must be zero).
 *   a2_mode 0: none; 1: A2 (same geometry) is added to A by the loader; 2: K continues with pad4(cin2) columns, a 1x1 conv of
 *   A2 [n_chunks, tin2, fin2, lda2] sampled at (to * st2, fo * sf2).
 *   epilogue: + bias_dev[n] (nullable), + r_dev[m, n] (nullable), act 0 none / 1 max(., 0) / 2 min(max(., 0), 20) / 3 SiLU, then with
 *   x_dev and y_dev (both or neither): C = x[m, n] (1 + tanh v) + y[m, n] (1 - tanh v). */
int pf_k_eres_conv(const float* a_dev, int32_t lda, int32_t a_col, int32_t cin, const float* a2_dev, int32_t lda2, int32_t a2_col,
                   int32_t cin2, int32_t a2_mode, int32_t tin2, int32_t fin2, int32_t st2, int32_t sf2, const float* w_dev, int32_t ldw,
                   const float* bias_dev, const float* r_dev, int32_t ldr, const float* x_dev, int32_t ldx, const float* y_dev,
                   int32_t ldy, float* c_dev, int32_t ldc, int32_t c_col, int32_t n_chunks, int32_t tin, int32_t fin, int32_t taps,
                   int32_t st, int32_t sf, int32_t N, int32_t act, void* stream);
/* measurement hook (tools/bench_eres2net.py): one 3x3 stride-1 conv of [n_chunks, T, F, C] (C % 4 == 0) to N channels with ReLU, weight
 * [N, 9 C] tap-major, timed over `iters` launches on this network's conv kernel (ms_out[0]) and on CAM++'s (ms_out[1]). Synchronises. */
int pf_k_eres_conv_vs_cam_time(const float* a_dev, const float* w_dev, float* c_dev, int32_t n_chunks, int32_t T, int32_t F, int32_t C,
                               int32_t N, int32_t iters, float* ms_out, void* stream);

/* ---- emotion2vec (funasr/models/emotion2vec/model.py Emotion2vec.extract_features + the inference head): waveform norm, the
 * 512-channel conv encoder (extractor_mode "layer_norm"), project_features, the grouped positional conv, extra tokens, context
 * LayerNorm, prenet_depth + depth post-LN ALiBi blocks (head dim 64), then the mean over frames, proj and softmax. Tensor names
 * are the reference's state_dict keys: "modality_encoders.AUDIO.local_encoder.conv_layers.0.0.weight",
 * "modality_encoders.AUDIO.relative_positional_encoder.1.0.weight", "modality_encoders.AUDIO.context_encoder.blocks.0.attn.qkv.weight",
 * "blocks.0.mlp.fc2.bias", "proj.weight" (vocab_size > 0), ... (the training-only decoder.* keys are not taken).
 * precision 0: every GEMM on the exact-f32 MFMA; 3: on the fp16 MFMA with two-plane operands (fp32-class results; plane
 * exponents from a-priori bounds of the weights only). Attention, convs and LayerNorms are fp32 in both. Every utterance's
 * results are bitwise the same alone or in any batch. */
typedef struct pf_emotion2vec pf_emotion2vec;
typedef struct pf_emotion2vec_config {
    int32_t embed_dim, num_heads, ffn_dim, prenet_depth, depth;
    int32_t num_extra_tokens, num_alibi_heads;
    int32_t alibi_scale_layers;   /* rows of alibi_scale: 1, or prenet_depth + depth (learned_alibi_scale_per_layer) */
    int32_t alibi_scale_heads;    /* 1, or num_alibi_heads (learned_alibi_scale_per_head) */
    int32_t n_conv, conv_kernel[8], conv_stride[8];    /* the conv encoder: 512 channels per layer */
    int32_t conv_pos_depth, conv_pos_kernel, conv_pos_groups;
    int32_t vocab_size;           /* 0: no proj (features only) */
    int32_t normalize;            /* F.layer_norm over the whole waveform first */
    int32_t precision;            /* 0 fp32, 3 f16x2 */
    float norm_eps;
} pf_emotion2vec_config;
pf_emotion2vec* pf_emotion2vec_create(const pf_emotion2vec_config* cfg);
void pf_emotion2vec_destroy(pf_emotion2vec* h);
int pf_emotion2vec_set_tensor(pf_emotion2vec* h, const char* name, const float* data, int64_t numel);
int pf_emotion2vec_missing(const pf_emotion2vec* h);
/* classes whose label starts with "unuse" (mask_host[c] != 0) get -inf before the softmax; default none masked */
int pf_emotion2vec_set_label_mask(pf_emotion2vec* h, const int32_t* mask_host, int32_t n);
/* samples per launch sequence (default 8 M, about 7 GB of workspace): larger batches run as sub-batches of whole utterances;
 * never changes a result bit */
int pf_emotion2vec_set_max_samples(pf_emotion2vec* h, int64_t max_samples);
/* frames of an utterance of n samples (0 if it is too short for one frame) */
int32_t pf_emotion2vec_num_frames(const pf_emotion2vec* h, int64_t n_samples);
/* wav_dev: B utterances back to back (lens_host[b] samples each) -> optional outputs: feats_dev [sum of frames, D] (each
 * utterance's frames after the extra tokens, back to back), pooled_dev [B, D] (their mean), probs_dev [B, vocab_size].
 * Returns nonzero (pf_last_error) when an utterance is too short for one frame (400 samples for the published encoder). No sync. */
int pf_emotion2vec_forward(pf_emotion2vec* h, const float* wav_dev, const int64_t* lens_host, int32_t B, float* feats_dev,
                           float* pooled_dev, float* probs_dev, void* stream);

/* ---- Conformer encoder (funasr/models/conformer/encoder.py ConformerEncoder: Conv2dSubsampling, relative-position self-attention
 * in its "legacy" and "latest" forms, macaron feed-forwards, the GLU / depthwise / BatchNorm / Swish convolution module; head dim 64,
 * pre-LayerNorm). Tensor names are the reference's state_dict keys below `encoder.`: "embed.conv.0.weight", "embed.out.0.weight",
 * "encoders.0.self_attn.linear_pos.weight", "encoders.0.self_attn.pos_bias_u", "encoders.0.conv_module.norm.running_mean",
 * "encoders.0.norm_final.weight", "after_norm.bias", ... plus "pos_table": the positional table built on the host exactly as the
 * reference builds it ([5000, D] for legacy: row m = position 4999 - m; [9999, D] for latest: row k = position 4999 - k).
 * The forward takes the ZERO-PADDED feature batch and computes every row of it, as the reference does: a clip's frames and its
 * output length depend on the batch's padded length (the mask rule x_mask[:, :, :-2:2][:, :, :-2:2]).
 * precision 0: every GEMM on the exact-f32 MFMA; 3: the block GEMMs on the fp16 MFMA with two-plane operands (exponents from
 * a-priori bounds of the weights only); the subsampling GEMMs, linear_pos, attention, convs and LayerNorms are fp32 in both. */
typedef struct pf_conformer pf_conformer;
typedef struct pf_conformer_config {
    int32_t input_dim, d_model, n_heads, ffn_dim, n_blocks, kernel_size;
    int32_t macaron;              /* 1: macaron pair of feed-forwards (ff_scale 0.5) */
    int32_t legacy;               /* 1: LegacyRelPositionalEncoding / LegacyRelPositionMultiHeadedAttention (rel_pos_type "legacy") */
    int32_t precision;            /* 0 fp32, 3 f16x2 */
    float ln_eps;
} pf_conformer_config;
pf_conformer* pf_conformer_create(const pf_conformer_config* cfg);
void pf_conformer_destroy(pf_conformer* h);
int pf_conformer_set_tensor(pf_conformer* h, const char* name, const float* data, int64_t numel);
int pf_conformer_missing(const pf_conformer* h);
int pf_conformer_set_precision(pf_conformer* h, int32_t precision);
/* encoder frames of a clip of n_frames features inside a batch padded to padded_frames (-1: padded_frames < 7 or n_frames > padded_frames) */
int32_t pf_conformer_num_frames(const pf_conformer* h, int32_t n_frames, int32_t padded_frames);
/* feats_dev [B, Tin, input_dim] zero-padded, lens_host[b] valid frames -> out_dev [B, T, d_model] with T = num_frames(Tin, Tin),
 * out_lens_host[b] (optional) = num_frames(lens_host[b], Tin). Fails when Tin < 7 or T > 5000. No sync. */
int pf_conformer_forward(pf_conformer* h, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t Tin, float* out_dev,
                         int32_t* out_lens_host, void* stream);

/* ---- Transformer encoder (funasr/models/transformer/encoder.py TransformerEncoder: Conv2dSubsampling, x sqrt(D) + the absolute
 * sinusoid, pre-LayerNorm blocks of plain masked self-attention (MultiHeadedAttention, head dim 64) and a ReLU feed-forward).
 * Tensor names are the reference's keys below `encoder.`: "embed.conv.0.weight", "embed.out.0.weight",
 * "encoders.0.self_attn.linear_q.weight", "encoders.0.feed_forward.w_1.bias", "encoders.0.norm1.weight", "after_norm.bias", ...
 * plus "pos_table" [5000, D] (row p = the sinusoid of position p, built on the host as the reference does).
 * Shapes, lengths and precisions are pf_conformer's: the ZERO-PADDED batch in, every row computed, lengths by the mask rule;
 * precision 3 runs the block GEMMs on the fp16 MFMA with two-plane operands, the subsampling GEMMs and the attention stay fp32. */
typedef struct pf_tfencoder pf_tfencoder;
typedef struct pf_tfencoder_config {
    int32_t input_dim, d_model, n_heads, ffn_dim, n_blocks;
    int32_t precision;            /* 0 fp32, 3 f16x2 */
    float ln_eps;
} pf_tfencoder_config;
pf_tfencoder* pf_tfencoder_create(const pf_tfencoder_config* cfg);
void pf_tfencoder_destroy(pf_tfencoder* h);
int pf_tfencoder_set_tensor(pf_tfencoder* h, const char* name, const float* data, int64_t numel);
int pf_tfencoder_missing(const pf_tfencoder* h);
int pf_tfencoder_set_precision(pf_tfencoder* h, int32_t precision);
int32_t pf_tfencoder_num_frames(const pf_tfencoder* h, int32_t n_frames, int32_t padded_frames);
/* as pf_conformer_forward. Fails when Tin < 7 or T > 5000. No sync. */
int pf_tfencoder_forward(pf_tfencoder* h, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t Tin, float* out_dev,
                         int32_t* out_lens_host, void* stream);

/* ---- RWKV encoder (funasr/models/rwkv_bat/rwkv_encoder.py RWKVEncoder, the encoder of the reference's Transducer template: the VGG
 * front RWKVConvInput at subsampling_factor 4 -- six 3x3 convs + ReLU, an output linear --, embed_norm, blocks of time mix (token
 * shift, WKV recurrence, receptance gate) and channel mix (token shift, relu^2 feed-forward, receptance gate), final_norm, then every
 * time_reduction-th frame). fp32 throughout. Tensor names are the reference's keys below `encoder.`: "embed.conv.0.weight" ..
 * "embed.conv.10.bias", "embed.output.weight", "embed_norm.weight", "rwkv_blocks.0.layer_norm_att.weight", "rwkv_blocks.0.att.time_decay",
 * "rwkv_blocks.0.att.time_mix_key" ([1, 1, D]), "rwkv_blocks.0.att.proj_key.weight", "rwkv_blocks.0.ffn.proj_value.bias", "final_norm.bias".
 * Unlike the encoders above, the front runs CLIP BY CLIP at the clip's own length: clip b of a batch gets bit for bit what it gets
 * alone (the reference itself handles one clip per call). Behind the front every block looks back only: row n of a block's output
 * depends on the front's rows 0 .. n of the same clip (the front's six 3x3 convs each look one frame ahead, so an OUTPUT frame does
 * depend on a few feature frames after it). */
typedef struct pf_rwkvencoder pf_rwkvencoder;
typedef struct pf_rwkvencoder_config {
    int32_t input_dim;            /* 8 .. 256, a multiple of 4 */
    int32_t d_model;              /* output_size = attention_size: a multiple of 32 up to 1024 */
    int32_t linear_size;          /* a multiple of 32 up to 4096 */
    int32_t n_blocks, time_reduction;
    float ln_eps;
} pf_rwkvencoder_config;
pf_rwkvencoder* pf_rwkvencoder_create(const pf_rwkvencoder_config* cfg);
void pf_rwkvencoder_destroy(pf_rwkvencoder* h);
int pf_rwkvencoder_set_tensor(pf_rwkvencoder* h, const char* name, const float* data, int64_t numel);
int pf_rwkvencoder_missing(const pf_rwkvencoder* h);
/* output frames of a clip of n_frames: floor((ceil(ceil(n / 2) / 2) - 1) / time_reduction) + 1; -1 on a null handle or n < 1 */
int32_t pf_rwkvencoder_num_frames(const pf_rwkvencoder* h, int32_t n_frames);
/* feats_dev [B, Tin, input_dim], lens_host[b] in 1 .. Tin -> out_dev [B, num_frames(Tin), d_model], rows at or past
 * out_lens_host[b] (optional) = num_frames(lens_host[b]) are zeros. No sync. */
int pf_rwkvencoder_forward(pf_rwkvencoder* h, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t Tin, float* out_dev,
                           int32_t* out_lens_host, void* stream);
/* tests: the same, and stages_dev[0 .. n_blocks + 2) (a host array of device pointers, each nullable) receive [B, T2, d_model] copies,
 * T2 = ceil(ceil(Tin / 2) / 2), of the front's output (rows past a clip's own T2 unspecified), embed_norm's, and every block's */
int pf_rwkvencoder_forward_stages(pf_rwkvencoder* h, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t Tin,
                                  float* out_dev, int32_t* out_lens_host, float* const* stages_dev, void* stream);
/* tests: fill every workspace buffer with 0xff bytes (a forward must not read what it did not write) */
int pf_rwkvencoder_debug_poison(pf_rwkvencoder* h);
/* single-kernel hooks (csrc/rwkv.h). pf_k_rwkv_chunk: frames per WKV chunk. pf_k_rwkv_mix: y[row, j D + c] = LN(x[row]) mu_j + LN(x[row
 * - 1]) (1 - mu_j), two operands when mix2_dev is null. pf_k_rwkv_wkv: out = sigmoid(r) wkv(k, v; w = -exp(time_decay), u = time_first);
 * scratch_dev holds B * ceil(T / chunk) * 3 * D floats. lens_dev: device int32 [B]; rows at or past a length are written as zeros. */
int pf_k_rwkv_chunk(void);
int pf_k_rwkv_mix(const float* x_dev, int32_t ldx, const float* gamma_dev, const float* beta_dev, float eps, const float* mix0_dev,
                  const float* mix1_dev, const float* mix2_dev, float* y_dev, int32_t ldy, const int32_t* lens_dev, int32_t B, int32_t T,
                  int32_t D, void* stream);
int pf_k_rwkv_wkv(const float* k_dev, const float* v_dev, const float* r_dev, int32_t ld, const float* w_dev, const float* u_dev,
                  const int32_t* lens_dev, int32_t B, int32_t T, int32_t D, float* out_dev, int32_t ldo, float* scratch_dev,
                  int64_t scratch_floats, void* stream);

/* ---- Qwen3 causal LM decoder with a KV cache (the LM of funasr/models/fun_asr_nano/model.py FunASRNano; transformers'
 * Qwen3ForCausalLM): per layer input_layernorm (RMSNorm) -> one fused q | k | v projection -> per-head q_norm / k_norm + rotary
 * embedding, rotated K and plain V written into the cache -> causal grouped-query attention -> o_proj + residual ->
 * post_attention_layernorm -> one fused gate | up projection -> SwiGLU -> down_proj + residual; then the final norm and the vocabulary
 * projection with its arg-max. fp32 throughout, greedy search only, no biases (attention_bias = false). Tensor names are the
 * upstream state-dict keys: "model.embed_tokens.weight", "model.layers.0.input_layernorm.weight",
 * "model.layers.0.self_attn.q_proj.weight" (k_proj, v_proj, o_proj), "model.layers.0.self_attn.q_norm.weight" (k_norm),
 * "model.layers.0.post_attention_layernorm.weight", "model.layers.0.mlp.gate_proj.weight" (up_proj, down_proj), "model.norm.weight"
 * and, unless tie_word_embeddings, "lm_head.weight".
 * KV cache: K and V each [layer][sequence][kv_head][position][head_dim], sized by pf_qwen3_prefill for the longest prompt plus
 * max_new_tokens; a sequence's rows at or past its own length are never read. A batch is 1 .. 16 sequences, each at its own length (no
 * padding rows anywhere): every kernel takes per-row (sequence, position), so a sequence computes what it computes alone up to the
 * summation order of the GEMM tile its rows fall into.
 * Prefill runs the tile GEMM, a decode step the small-M weight-streaming GEMM; one decode step is 10 launches per layer plus 5 around
 * them, one of which is the read-back of the step's ids. */
typedef struct pf_qwen3 pf_qwen3;
typedef struct pf_qwen3_config {
    int32_t vocab_size;
    int32_t hidden_size;          /* a multiple of 32 */
    int32_t intermediate_size;    /* a multiple of 32 */
    int32_t n_layers;
    int32_t n_heads;              /* num_attention_heads */
    int32_t n_kv_heads;           /* divides n_heads */
    int32_t head_dim;             /* 64 or 128 */
    int32_t tie_word_embeddings;  /* != 0: the vocabulary projection reads model.embed_tokens.weight, lm_head.weight is no tensor */
    float rms_eps;
} pf_qwen3_config;
pf_qwen3* pf_qwen3_create(const pf_qwen3_config* cfg);
void pf_qwen3_destroy(pf_qwen3* h);
int pf_qwen3_set_tensor(pf_qwen3* h, const char* name, const float* data, int64_t numel);
int pf_qwen3_missing(const pf_qwen3* h);
/* cos / sin of the rotary embedding, [positions, head_dim / 2] each (host or device memory; copied before the call returns). The
 * caller computes them in float32 as upstream does; the library never evaluates a sine. A prefill or step that needs a position the
 * table does not hold is refused. pf_qwen3_rope_positions: rows the table holds now. */
int pf_qwen3_set_rope_table(pf_qwen3* h, const float* cos_t, const float* sin_t, int32_t positions);
int32_t pf_qwen3_rope_positions(const pf_qwen3* h);
/* out_dev [n, hidden_size] = model.embed_tokens.weight[ids_dev[i]] (ids clamped into the vocabulary). No sync. */
int pf_qwen3_embed(pf_qwen3* h, const int32_t* ids_dev, int32_t n, float* out_dev, void* stream);
/* Start B sequences: inputs_embeds_dev holds their rows back to back ([sum of rows_host, hidden_size], rows_host[b] >= 1), the cache is
 * sized for max(rows_host) + max_new_tokens positions per sequence and every sequence's length becomes rows_host[b]. first_ids_host[b]
 * = arg-max of the logits of sequence b's last row. logits_dev (tests; nullable): [sum of rows_host, vocab_size] logits of EVERY row.
 * Synchronises. */
int pf_qwen3_prefill(pf_qwen3* h, const float* inputs_embeds_dev, const int32_t* rows_host, int32_t B, int32_t max_new_tokens,
                     int32_t* first_ids_host, float* logits_dev, void* stream);
/* one decode step of every sequence of the last prefill: ids_host[b] is embedded, appended at position length[b], and next_ids_host[b]
 * = arg-max of its logits. logits_dev (tests; nullable): [B, vocab_size]. Refused when a cache is full. Synchronises. */
int pf_qwen3_step(pf_qwen3* h, const int32_t* ids_host, int32_t* next_ids_host, float* logits_dev, void* stream);
/* greedy generation after pf_qwen3_prefill, the loop inside the library: column 0 of out_ids_host [B, max_new_tokens] is the prefill's
 * first id; a sequence that has emitted one of eos_ids_host[0 .. n_eos) is finished, takes no further step and emits pad_id; the loop
 * ends when every sequence is finished or after max_new_tokens columns (at most the max_new_tokens the prefill reserved). *n_out =
 * columns written; the columns behind hold pad_id. One read-back of the step's ids per step; no HIP graph. */
int pf_qwen3_generate(pf_qwen3* h, int32_t max_new_tokens, const int32_t* eos_ids_host, int32_t n_eos, int32_t pad_id,
                      int32_t* out_ids_host, int32_t* n_out, void* stream);
/* tests: fill the KV cache and every workspace buffer with 0xff bytes (NaN) */
int pf_qwen3_debug_poison(pf_qwen3* h);
/* single-kernel hooks (csrc/qwen3.h). Caches: K and V of ONE layer, each [slots, Hkv, cap, hd]. Every *_host array is checked against
 * slots / cap / the table before the launch and copied to the device; each hook synchronises.
 * pf_k_qwen3_tiles: query rows per workgroup of the prefill attention for G = Hq / Hkv, keys per LDS tile for hd, keys per workgroup of
 * the decode attention. */
int pf_k_qwen3_tiles(int32_t G, int32_t hd, int32_t* q_tile, int32_t* k_tile, int32_t* k_split);
int pf_k_qwen3_rmsnorm(const float* x_dev, int32_t ldx, const float* w_dev, float eps, float* y_dev, int32_t ldy, int32_t M, int32_t D,
                       void* stream);
/* qkv_dev [M, (Hq + 2 Hkv) hd]; cos_dev / sin_dev [table_rows, hd / 2]; row r = position row_pos_host[r] of slot row_seq_host[r] */
int pf_k_qwen3_qk_rope(const float* qkv_dev, int32_t ld, const float* qw_dev, const float* kw_dev, float eps, const float* cos_dev,
                       const float* sin_dev, int32_t table_rows, const int32_t* row_seq_host, const int32_t* row_pos_host, float* q_out_dev,
                       int32_t ldq, float* kcache_dev, float* vcache_dev, int32_t slots, int32_t cap, int32_t M, int32_t Hq, int32_t Hkv,
                       int32_t hd, void* stream);
/* sequence i: rows [row0_host[i], row0_host[i] + nrows_host[i]) of q_dev / out_dev [M, Hq hd] at positions p0_host[i] .. of slot
 * seq_host[i]; row j attends to cache rows 0 .. p0 + j */
int pf_k_qwen3_prefill_attention(const float* q_dev, int32_t ldq, const float* kcache_dev, const float* vcache_dev, int32_t slots,
                                 int32_t cap, float* out_dev, int32_t ldo, int32_t M, const int32_t* seq_host, const int32_t* row0_host,
                                 const int32_t* nrows_host, const int32_t* p0_host, int32_t nseq, int32_t Hq, int32_t Hkv, int32_t hd,
                                 float scale, void* stream);
/* row r of q_dev / out_dev [M, Hq hd] attends to rows 0 .. row_len_host[r] - 1 of slot row_seq_host[r] */
int pf_k_qwen3_decode_attention(const float* q_dev, int32_t ldq, const float* kcache_dev, const float* vcache_dev, int32_t slots,
                                int32_t cap, float* out_dev, int32_t ldo, const int32_t* row_seq_host, const int32_t* row_len_host, int32_t M,
                                int32_t Hq, int32_t Hkv, int32_t hd, float scale, void* stream);
/* out_dev [M, I] = silu(gu_dev[:, 0 .. I)) * gu_dev[:, I .. 2 I) */
int pf_k_qwen3_swiglu(const float* gu_dev, int32_t ld, float* out_dev, int32_t ldo, int32_t M, int32_t I, void* stream);

/* ---- Chunk Conformer encoder (funasr/models/conformer/encoder.py ConformerChunkEncoder, registered as ChunkConformerEncoder: the
 * StreamingConvInput front at 1/2, 1/4 or 1/6 subsampling (vgg_like = False), blocks of macaron feed-forward, chunk-masked
 * relative-position self-attention (head dim 64), the convolution module (causal or symmetric), feed-forward and norm_final, then
 * norm_blocks and every time_reduction-th frame). fp32 throughout. Tensor names are the reference's keys below `encoder.`:
 * "embed.conv.0.weight", "embed.conv.2.bias", "embed.output.weight", "encoders.blocks.0.self_att.linear_pos.weight",
 * "encoders.blocks.0.self_att.pos_bias_u", "encoders.blocks.0.feed_forward_macaron.w_1.weight",
 * "encoders.blocks.0.conv_mod.norm.running_mean", "encoders.blocks.0.norm_self_att.weight", "encoders.norm_blocks.bias", ... plus
 * "pos_table" as for pf_conformer's "latest" form (9999 rows). The ZERO-PADDED batch goes in and every row of it is computed. The
 * front's workspace grows with the batch (its first conv's output, B pieces x frames / 2 x features / 2 x d_model floats, is the
 * largest part: 1.9 GB for sixteen 30-s clips at d_model 512); a batch whose first-conv output would pass 8 GB is refused. */
typedef struct pf_chunkconformer pf_chunkconformer;
typedef struct pf_chunkconformer_config {
    int32_t input_dim;            /* 16 .. 256 */
    int32_t d_model, n_heads;     /* d_model = 64 n_heads, up to 2048 */
    int32_t ffn_dim;              /* a multiple of 32 */
    int32_t n_blocks;
    int32_t kernel_size;          /* odd, up to 31 */
    int32_t subsampling;          /* 2, 4 or 6 */
    int32_t causal_conv;          /* dynamic_chunk_training or unified_model_training: the depthwise conv pads kernel_size - 1 on the left only */
    int32_t left_chunk;           /* left_chunk_size: chunks of the past a query sees beside its own (< 0: all of the past) */
    int32_t time_reduction;
    float ln_eps, bn_eps;
} pf_chunkconformer_config;
pf_chunkconformer* pf_chunkconformer_create(const pf_chunkconformer_config* cfg);
void pf_chunkconformer_destroy(pf_chunkconformer* h);
int pf_chunkconformer_set_tensor(pf_chunkconformer* h, const char* name, const float* data, int64_t numel);
int pf_chunkconformer_missing(const pf_chunkconformer* h);
/* 0 (fp32) is the one arithmetic built; anything else is refused */
int pf_chunkconformer_set_precision(pf_chunkconformer* h, int32_t precision);
/* output frames of a clip of n_frames: floor((ceil(ceil(n / 2) / s2) - 1) / time_reduction) + 1, s2 = subsampling / 2; -1 on error */
int32_t pf_chunkconformer_num_frames(const pf_chunkconformer* h, int32_t n_frames);
/* feats_dev [B, Tin, input_dim], lens_host[b] in 1 .. Tin. chunk > 0: the front convolves pieces of chunk * subsampling frames on their
 * own; chunk == 0: whole clips. branches: bit 0 = the blocks WITHOUT a chunk mask -> out_utt_dev, bit 1 = the blocks under the chunk
 * mask of (chunk, left_chunk) -> out_chunk_dev (chunk == 0: no mask either); both read one run of the front. Outputs
 * [B, num_frames(Tin), d_model]; out_lens_host (optional) = num_frames(lens_host[b]). stages_dev (tests; nullable, entries nullable):
 * a host array of n_blocks + 2 device pointers that receive [B, T, d_model] copies (T = frames before the time reduction) of the
 * front's rows, every block's output and norm_blocks' output, of the chunk branch where it runs, else of the utt branch. No sync. */
int pf_chunkconformer_forward(pf_chunkconformer* h, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t Tin, int32_t chunk,
                              int32_t branches, float* out_utt_dev, float* out_chunk_dev, int32_t* out_lens_host,
                              float* const* stages_dev, void* stream);
/* tests: the front alone -> out_dev [B, ceil(ceil(Tin / 2) / s2), d_model] */
int pf_chunkconformer_front(pf_chunkconformer* h, const float* feats_dev, int32_t B, int32_t Tin, int32_t chunk, float* out_dev, void* stream);
/* tests: fill every workspace buffer with 0xff bytes (a forward must not read what it did not write) */
int pf_chunkconformer_debug_poison(pf_chunkconformer* h);
/* single-kernel hooks (csrc/chunk_conformer.h). pf_k_cc_window_attention: pf_k_relpos_attention's "latest" form where query i sees keys
 * [start_i, end_i) of (chunk, left) below klens_dev[b] only (chunk == 0: no chunk mask); rows without a visible key are zeros.
 * pf_k_cc_glu_dw: pf_k_conformer_glu_dw with causal != 0 padding taps - 1 rows on the left only. pf_k_cc_copy_rows:
 * y[b, t] = x[b, t * step], t < To, x of Ti rows per sequence. */
int pf_k_cc_window_attention(const float* qkv_dev, const float* P_dev, const float* u_dev, const float* v_dev, const int32_t* klens_dev,
                             int32_t B, int32_t T, int32_t H, int32_t chunk, int32_t left, float* out_dev, void* stream);
int pf_k_cc_glu_dw(const float* g_dev, const float* dw_dev, const float* dw_bias_dev, const float* bn_scale_dev, const float* bn_shift_dev,
                   int32_t B, int32_t T, int32_t D, int32_t taps, int32_t causal, float* y_dev, void* stream);
int pf_k_cc_copy_rows(const float* x_dev, int32_t Ti, int32_t step, float* y_dev, int32_t B, int32_t To, int32_t D, void* stream);

/* ---- E-Branchformer encoder (funasr/models/e_branchformer/encoder.py EBranchformerEncoder: Conv2dSubsampling, then blocks of two
 * parallel branches -- relative-position self-attention ("latest" or "legacy", head dim 64) and the convolutional gating MLP
 * (branchformer/cgmlp.py: Linear + exact GELU, LayerNorm + depthwise conv gate, Linear) -- merged by a depthwise conv over their
 * concatenation and a Linear, with optional (macaron) Swish feed-forwards around them). Tensor names are the reference's keys below
 * `encoder.`: "embed.conv.0.weight", "encoders.0.attn.linear_pos.weight", "encoders.0.attn.pos_bias_u",
 * "encoders.0.cgmlp.channel_proj1.0.weight", "encoders.0.cgmlp.csgu.norm.weight", "encoders.0.cgmlp.csgu.conv.weight",
 * "encoders.0.cgmlp.channel_proj2.bias", "encoders.0.depthwise_conv_fusion.weight", "encoders.0.merge_proj.weight",
 * "encoders.0.norm_mlp.weight", "after_norm.bias", ... plus "pos_table" as for pf_conformer.
 * Shapes, lengths and precisions are pf_conformer's: the ZERO-PADDED batch in, every row computed, lengths by the mask rule. Neither
 * depthwise conv is masked (the reference's are not): a clip's frames depend on the rows behind its end, i.e. on its batch.
 * precision 3 runs the block GEMMs on the fp16 MFMA with two-plane operands except merge_proj, which stays exact fp32 (its operand's
 * a-priori bound is too loose); the subsampling GEMMs, linear_pos, attention, convs and LayerNorms are fp32 in both.
 * cgmlp_units % 64 == 0 (the gate has cgmlp_units / 2 channels), conv kernels odd <= 31; ffn_dim is read only with use_ffn. */
typedef struct pf_ebranchformer pf_ebranchformer;
typedef struct pf_ebranchformer_config {
    int32_t input_dim, d_model, n_heads, ffn_dim, n_blocks;
    int32_t cgmlp_units, cgmlp_kernel, merge_kernel;
    int32_t use_ffn;              /* 1: a Swish feed-forward behind the merge */
    int32_t macaron;              /* 1 (with use_ffn): a second feed-forward in front of the branches, both scaled by 0.5 */
    int32_t legacy;               /* 1: rel_pos_type "legacy" */
    int32_t precision;            /* 0 fp32, 3 f16x2 */
    float ln_eps;
} pf_ebranchformer_config;
pf_ebranchformer* pf_ebranchformer_create(const pf_ebranchformer_config* cfg);
void pf_ebranchformer_destroy(pf_ebranchformer* h);
int pf_ebranchformer_set_tensor(pf_ebranchformer* h, const char* name, const float* data, int64_t numel);
int pf_ebranchformer_missing(const pf_ebranchformer* h);
int pf_ebranchformer_set_precision(pf_ebranchformer* h, int32_t precision);
int32_t pf_ebranchformer_num_frames(const pf_ebranchformer* h, int32_t n_frames, int32_t padded_frames);
/* as pf_conformer_forward. Fails when Tin < 7 or T > 5000. No sync. */
int pf_ebranchformer_forward(pf_ebranchformer* h, const float* feats_dev, const int32_t* lens_host, int32_t B, int32_t Tin, float* out_dev,
                             int32_t* out_lens_host, void* stream);
/* single-kernel hooks (tests) of the block: the exact GELU in place (n % 4 == 0); the gating unit h_dev [B T, 2 C] -> y_dev [B T, C] =
 * x_r * (dwconv(LayerNorm(x_g)) + bias) with stats_dev [B T, 2] as workspace; the merge x1_dev, x2_dev [B T, D] (separate buffers) ->
 * y_dev [B T, 2 D] = c + dwconv(c) + bias over c = [x1 | x2]. Convs over time within a sequence's T rows, zeros outside. */
int pf_k_eb_gelu(float* x_dev, int64_t n, void* stream);
int pf_k_eb_csgu(const float* h_dev, const float* gamma_dev, const float* beta_dev, float eps, const float* dw_dev, const float* dw_bias_dev,
                 int32_t B, int32_t T, int32_t C, int32_t taps, float* stats_dev, float* y_dev, void* stream);
int pf_k_eb_merge(const float* x1_dev, const float* x2_dev, const float* dw_dev, const float* dw_bias_dev, int32_t B, int32_t T, int32_t D,
                  int32_t taps, float* y_dev, void* stream);

/* ---- Transformer decoder, one autoregressive step for all running hypotheses of a beam (funasr/models/transformer/decoder.py
 * TransformerDecoder.forward_one_step / batch_score: embed x sqrt(D) + sinusoid, pre-LN self-attention over the hypothesis' own
 * prefix, cross-attention over the utterance's encoder memory, ReLU feed-forward, after_norm, output layer, log-softmax; head dim 64).
 * Tensor names are the reference's keys below `decoder.` ("embed.0.weight", "decoders.0.src_attn.linear_k.weight", "after_norm.weight",
 * "output_layer.bias", ...) plus "pos_table" [5000, D] (row p = the sinusoid of position p, built on the host as the reference does).
 * State on the device: the cross-attention K / V of every layer (computed once by begin) and a self-attention K / V cache per layer
 * and hypothesis slot. All GEMMs of a step are the fp32 small-M weight-streaming kernel. */
typedef struct pf_tdecoder pf_tdecoder;
typedef struct pf_tdecoder_config {
    int32_t vocab_size, d_model, n_heads, ffn_dim, n_blocks;
    float ln_eps;
} pf_tdecoder_config;
pf_tdecoder* pf_tdecoder_create(const pf_tdecoder_config* cfg);
void pf_tdecoder_destroy(pf_tdecoder* h);
int pf_tdecoder_set_tensor(pf_tdecoder* h, const char* name, const float* data, int64_t numel);
int pf_tdecoder_missing(const pf_tdecoder* h);
/* a new utterance: memory_dev [T, d_model]; caches for max_hyp slots of max_len positions are (re)set. No sync. */
int pf_tdecoder_begin(pf_tdecoder* h, const float* memory_dev, int32_t T, int32_t max_len, int32_t max_hyp, void* stream);
/* slot k < n_hyp gets token tokens_host[k] at position pos (positions are appended in order: pos <= positions filled so far)
 * -> logp_dev [n_hyp, vocab_size] log-probabilities of the next token. No sync. */
int pf_tdecoder_step(pf_tdecoder* h, const int32_t* tokens_host, int32_t pos, int32_t n_hyp, float* logp_dev, void* stream);
/* slot k < n_hyp takes the cache of slot parents_host[k] (a gather on the device; a parent may repeat or be dropped). No sync. */
int pf_tdecoder_reorder(pf_tdecoder* h, const int32_t* parents_host, int32_t n_hyp, void* stream);

/* ---- SAN-M autoregressive decoder (funasr/models/sanm/decoder.py FsmnDecoder.forward_one_step), the same stepper for a beam search
 * on the host. Tensor names are the module's state_dict keys: "embed.0.weight" (a bare embedding: no scale, no positional row),
 * "decoders.{i}.*" for i < att_layer_num (norm1, feed_forward.{w_1, norm, w_2} with w_2 without bias, norm2,
 * self_attn.fsmn_block.weight [D, 1, K], norm3, src_attn.{linear_q, linear_k_v, linear_out}), "decoders2.{j}.*" for the
 * n_blocks - att_layer_num layers without cross-attention, "decoders3.0.*" (norm1 and feed_forward only; applied WITHOUT a residual),
 * "after_norm.*", "output_layer.*".
 * Limits (create refuses with a message naming the field): head dim 64 or 128, d_model <= 2048, ffn_dim % 32 == 0 and <= 2048,
 * 1 <= kernel_size <= 32, sanm_shift >= 0 with a right padding kernel_size - 1 - (kernel_size - 1) / 2 - sanm_shift >= 0,
 * 1 <= att_layer_num <= n_blocks. sanm_shift is the RESOLVED value (the module's default None is (kernel_size - 1) / 2).
 * State on the device: K | V of every cross-attention layer (one GEMM through linear_k_v per layer, by begin) and, per FSMN layer and
 * hypothesis slot, the K-column window of the memory block in two buffers: the window at step n is the last K columns of
 * [0] * L + [x_0] + [0] * R + [x_1 .. x_n] with L = (K - 1) / 2 + sanm_shift and R = K - 1 - L -- the reference's cache rule, which
 * is the causal memory only when R == 0. All GEMMs of a step are the fp32 small-M weight-streaming kernel. */
typedef struct pf_fsmndecoder pf_fsmndecoder;
typedef struct pf_fsmndecoder_config {
    int32_t vocab_size, d_model, n_heads, ffn_dim, n_blocks, att_layer_num, kernel_size, sanm_shift;
    float ln_eps;
} pf_fsmndecoder_config;
pf_fsmndecoder* pf_fsmndecoder_create(const pf_fsmndecoder_config* cfg);
void pf_fsmndecoder_destroy(pf_fsmndecoder* h);
int pf_fsmndecoder_set_tensor(pf_fsmndecoder* h, const char* name, const float* data, int64_t numel);
int pf_fsmndecoder_missing(const pf_fsmndecoder* h);
/* a new utterance: memory_dev [T, d_model]; the windows of max_hyp slots are zeroed (max_len <= 5000, max_hyp <= 256). No sync. */
int pf_fsmndecoder_begin(pf_fsmndecoder* h, const float* memory_dev, int32_t T, int32_t max_len, int32_t max_hyp, void* stream);
/* slot k < n_hyp gets token tokens_host[k] at position pos (every position once, in order: pos == positions run so far); its window
 * continues the one of slot parents[k] of the last reorder(), or its own when no reorder() came since the last step
 * -> logp_dev [n_hyp, vocab_size] log-probabilities of the next token. No sync. */
int pf_fsmndecoder_step(pf_fsmndecoder* h, const int32_t* tokens_host, int32_t pos, int32_t n_hyp, float* logp_dev, void* stream);
/* slot k < n_hyp of the NEXT step takes the window of slot parents_host[k] of the last one (a parent may repeat or be dropped; every
 * parent ran at the last position). Records the parents only: the next step's FSMN kernel reads the parent's window. No sync. */
int pf_fsmndecoder_reorder(pf_fsmndecoder* h, const int32_t* parents_host, int32_t n_hyp, void* stream);
/* single-kernel hooks of the step (tests; see csrc/conformer.h): the fused norm2 + FSMN window + residual (+ norm3) kernel over
 * windows win_in_dev / win_out_dev [slots, K, D] (parents_dev NULL: slot k continues its own), and the few-query cross-attention
 * over kv_dev [T, 2 H dk] (K | V) for dk 64 or 128 */
int pf_k_fsmn_step(const float* t_dev, const float* x_dev, const float* g2_dev, const float* b2_dev, const float* w_dev,
                   const float* win_in_dev, float* win_out_dev, const int32_t* parents_dev, int32_t pos, int32_t n, int32_t D, int32_t K,
                   int32_t left_pad, const float* g3_dev, const float* b3_dev, float eps, float* x_out_dev, float* xn_out_dev, void* stream);
int pf_k_cross_attention_step(const float* q_dev, const float* kv_dev, int32_t T, int32_t n, int32_t H, int32_t dk, float* out_dev,
                              void* stream);

/* ---- UniASR two-pass ASR (funasr/models/uniasr/model.py): the offline chunked SAN-M encoder, `stride_conv`, the SCAMA decoder step.
 * Chunked encoder (SANMEncoderChunkOpt.forward with `ind`, scama/encoder.py:393-478): the caller lays the frames out as overlap_chunk
 * does (scama/chunk_utilis.py: per chunk `shift` FSMN shift rows, then `chunk` frames; pf_uniasr_gather_rows with the host's index
 * map, -1 for a zero row, for the features AND for the positional table) and runs pf_encoder_forward over those rows after
 * pf_encoder_set_chunk_mask(e, chunk, stride, shift, look_back): every block's attention then takes mask_att_chunk_encoder -- a row
 * sees its own chunk and, when it is one of the chunk's first `stride` frames, the first `stride` frames of each of the `look_back`
 * chunks before -- and its FSMN memory mask_shfit_chunk, both worked out from the geometry on the device (no [Tc, Tc] mask).
 * chunk == 0 switches the masks off. fp32 mode only (pf_encoder_set_precision(e, 0)); not together with pf_encoder_set_vad_mask. */
int pf_encoder_set_chunk_mask(pf_encoder* e, int32_t chunk, int32_t stride, int32_t shift, int32_t look_back);
/* out_dev[r] = idx_dev[r] >= 0 ? src_dev[idx_dev[r]] : 0 for r < n: rows of D floats (D % 4 == 0), source rows ld_src floats apart,
 * n_src of them (an index at or past n_src reads as a zero row). split_chunk and remove_chunk as gathers. No sync. */
int pf_uniasr_gather_rows(const float* src_dev, int32_t ld_src, int32_t n_src, const int32_t* idx_dev, float* out_dev, int32_t n, int32_t D,
                          void* stream);
/* Conv1dSubsampling (transformer/utils/subsampling.py:332-388) over the concatenation [a | b] along the features, read from its two
 * sources: out_dev [Tout, Cout] = relu(conv1d(pad(x, (pad_left, pad_right)), w [Cout, Da + Db, taps], stride) + bias), x = [a [T, Da] |
 * b [T, Db]]; Tout at most (T + pad_left + pad_right - taps) / stride + 1. taps <= 8, taps (Da + Db) floats within 48 KiB. No sync. */
int pf_uniasr_stride_conv(const float* a_dev, int32_t Da, const float* b_dev, int32_t Db, int32_t T, const float* w_dev, const float* bias_dev,
                          int32_t Cout, int32_t taps, int32_t stride, int32_t pad_left, int32_t pad_right, float* out_dev, int32_t Tout,
                          void* stream);
/* SCAMA decoder step (scama/decoder.py FsmnDecoderSCAMAOpt.forward_one_step without concat_embeds): pf_fsmndecoder's stepper -- the
 * same config, tensor names, limits, begin and reorder -- whose step restricts the softmax of every `decoders.{i}` cross-attention to
 * the keys j with key_lo <= j < key_hi and mask_row_dev[j] != 0 (mask_row_dev [T] floats on the device, NULL: the whole window); no
 * other K / V row is read. A position without a visible key gets a zero context (the reference fills the scores with the dtype's
 * minimum, takes the softmax and fills the masked probabilities with 0). */
typedef struct pf_scamadecoder pf_scamadecoder;
pf_scamadecoder* pf_scamadecoder_create(const pf_fsmndecoder_config* cfg);
void pf_scamadecoder_destroy(pf_scamadecoder* h);
int pf_scamadecoder_set_tensor(pf_scamadecoder* h, const char* name, const float* data, int64_t numel);
int pf_scamadecoder_missing(const pf_scamadecoder* h);
int pf_scamadecoder_begin(pf_scamadecoder* h, const float* memory_dev, int32_t T, int32_t max_len, int32_t max_hyp, void* stream);
int pf_scamadecoder_step(pf_scamadecoder* h, const int32_t* tokens_host, int32_t pos, int32_t n_hyp, const float* mask_row_dev,
                         int32_t key_lo, int32_t key_hi, float* logp_dev, void* stream);
int pf_scamadecoder_reorder(pf_scamadecoder* h, const int32_t* parents_host, int32_t n_hyp, void* stream);
/* single-kernel hooks (tests; see csrc/uniasr.h): the chunk-masked attention over qkv_dev [B T, 3 H dk] (q | k | v), the chunk-masked
 * FSMN memory, and the masked few-query cross-attention over kv_dev [T, 2 H dk] */
int pf_k_chunk_attention(const float* qkv_dev, const int32_t* klens_dev, int32_t B, int32_t T, int32_t H, int32_t dk, int32_t chunk,
                         int32_t stride, int32_t shift, int32_t look_back, float* out_dev, void* stream);
int pf_k_chunk_fsmn(const float* in_dev, int32_t ldin, const float* w_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t C, int32_t K,
                    int32_t left_pad, int32_t chunk, int32_t stride, int32_t shift, float* out_dev, void* stream);
int pf_k_scama_attention(const float* q_dev, const float* kv_dev, int32_t T, const float* mask_row_dev, int32_t key_lo, int32_t key_hi,
                         int32_t n, int32_t H, int32_t dk, float* out_dev, void* stream);

/* single-kernel hooks of the two above (tests): the relative-position attention (qkv_dev [B T, 3 D] q | k | v, P_dev [T or 2 T - 1, D],
 * u_dev / v_dev [H, 64], klens_dev [B] -> out_dev [B T, D]; see csrc/conformer.h) and the GLU + depthwise conv + BatchNorm + Swish
 * row kernel (g_dev [B T, 2 D], dw_dev [D, taps], BatchNorm folded to scale / shift [D] -> y_dev [B T, D]) */
int pf_k_relpos_attention(const float* qkv_dev, const float* P_dev, const float* u_dev, const float* v_dev, const int32_t* klens_dev, int32_t B,
                          int32_t T, int32_t H, int32_t legacy, float* out_dev, void* stream);
int pf_k_conformer_glu_dw(const float* g_dev, const float* dw_dev, const float* dw_bias_dev, const float* bn_scale_dev,
                          const float* bn_shift_dev, int32_t B, int32_t T, int32_t D, int32_t taps, float* y_dev, void* stream);
/* single-kernel hooks of the Transformer encoder (tests): the plain masked attention (qkv_dev [B T, 3 D] q | k | v, klens_dev [B]
 * -> out_dev [B T, D]; keys >= klens_dev[b] masked, no row at or past them read) and the embedding rows
 * y[b T + t] = x[b NE + t] * scale + pe[t] for t < T <= NE (pe_dev [>= T, D] or NULL: the scale alone) */
int pf_k_tf_attention(const float* qkv_dev, const int32_t* klens_dev, int32_t B, int32_t T, int32_t H, float* out_dev, void* stream);
int pf_k_tf_embed_rows(const float* x_dev, int32_t NE, const float* pe_dev, int32_t B, int32_t T, int32_t D, float scale, float* y_dev,
                       void* stream);

/* ---- LCB-Net (funasr/models/lcbnet: long-context biasing ASR, audio plus the OCR text of the slides). The audio side is pf_tfencoder /
 * pf_tdecoder / pf_ctc; these two handles are the text side. Both run exact-fp32 GEMMs: the rows are few, run once per utterance, and no
 * a-priori bound crosses the handles (the text encoder's output feeds the fusion layer's K / V projections).
 *
 * pf_textencoder: TransformerTextEncoder (lcbnet/encoder.py:130-241): Embedding x sqrt(D) + pe[t], pre-LayerNorm blocks of masked
 * self-attention and a ReLU feed-forward (the block loop of pf_tfencoder behind another front), after_norm. Tensor names: the reference's
 * keys below `text_encoder.` -- "embed.0.weight" [vocab, D], "encoders.<i>.self_attn.linear_{q,k,v,out}.{weight,bias}",
 * "encoders.<i>.feed_forward.w_{1,2}.{weight,bias}", "encoders.<i>.norm{1,2}.{weight,bias}", "after_norm.{weight,bias}" -- plus
 * "pos_table" [5000, D]. */
typedef struct pf_textencoder pf_textencoder;
typedef struct pf_textencoder_config {
    int32_t vocab_size, d_model, n_heads, ffn_dim, n_blocks;
    float ln_eps;
} pf_textencoder_config;
pf_textencoder* pf_textencoder_create(const pf_textencoder_config* cfg);
void pf_textencoder_destroy(pf_textencoder* h);
int pf_textencoder_set_tensor(pf_textencoder* h, const char* name, const float* data, int64_t numel);
int pf_textencoder_missing(const pf_textencoder* h);
/* ids_host [B, L] (every id in [0, vocab_size), checked here before any launch), lens_host [B] (keys at or past lens_host[b] are
 * masked; every row is computed) -> out_dev [B, L, D]. Fails unless 1 <= L <= 5000. No sync. */
int pf_textencoder_forward(pf_textencoder* h, const int32_t* ids_host, const int32_t* lens_host, int32_t B, int32_t L, float* out_dev,
                           void* stream);

/* pf_fusion: FusionSANEncoder = ONE SelfSrcAttention layer (lcbnet/encoder.py:244-370):
 *   x += self_attn(norm1 x); x += src_attn(norm2 x, mem, mem); x += feed_forward(norm3 x)
 * Tensor names: the reference's keys below `fusion_encoder.` ("self_attn.*", "src_attn.*", "feed_forward.w_{1,2}.*", "norm{1,2,3}.*"). */
typedef struct pf_fusion pf_fusion;
typedef struct pf_fusion_config {
    int32_t d_model, n_heads, ffn_dim;
    float ln_eps;
} pf_fusion_config;
pf_fusion* pf_fusion_create(const pf_fusion_config* cfg);
void pf_fusion_destroy(pf_fusion* h);
int pf_fusion_set_tensor(pf_fusion* h, const char* name, const float* data, int64_t numel);
int pf_fusion_missing(const pf_fusion* h);
/* x_dev [B, T, D], mem_dev [B, L, D] -> out_dev [B, T, D] (another buffer than x_dev). x_lens_host / mem_lens_host [B] or NULL: NULL
 * means every row / every key (what the reference's inference passes: both masks None). add_input != 0: out = x + layer(x, mem), the
 * model's `encoder_out + fusion_out`, the addend riding in the last GEMM. 1 <= T <= 12000, 1 <= L <= 5000. No sync. */
int pf_fusion_forward(pf_fusion* h, const float* x_dev, const int32_t* x_lens_host, const float* mem_dev, const int32_t* mem_lens_host,
                      int32_t B, int32_t T, int32_t L, int32_t add_input, float* out_dev, void* stream);
/* single-kernel hooks (tests): the cross-attention of many queries over a second sequence (q_dev [B Tq, >= 64 H] rows ldq floats apart,
 * kv_dev [B L, 128 H] K | V, klens_dev [B] -> out_dev [B Tq, 64 H]; keys >= klens_dev[b] masked, no row at or past them read) and
 * the token rows y[b L + t] = table[ids[b L + t]] * scale + pe[t] (ids_dev inside the table: not checked on the device) */
int pf_k_tf_cross_attention(const float* q_dev, int32_t ldq, const float* kv_dev, const int32_t* klens_dev, int32_t B, int32_t Tq, int32_t L,
                            int32_t H, float* out_dev, void* stream);
int pf_k_text_embed_rows(const float* table_dev, const int32_t* ids_dev, const float* pe_dev, int32_t B, int32_t L, int32_t D, float scale,
                         float* y_dev, void* stream);

/* ---- E-Paraformer (funasr/models/e_paraformer): the parallel integrate-and-fire predictor and the one-pass SAN decoder. The encoder
 * is pf_conformer.
 * pf_pif: PifPredictor.forward (pif_predictor.py:84-130), inference path. Tensor names are the reference's keys below `predictor.`:
 * "cif_conv1d.weight" [D, 1, l_order + r_order + 1], "cif_conv1d.bias" [D], "cif_output.weight" [1, D], "cif_output.bias" [1], "sigma"
 * [sigma_heads], "bias" [sigma_heads] (constant over the frames: it cancels in the softmax and is never read). Exact fp32 in every
 * mode, fixed summation orders, no atomics. Two calls around ONE host read of the B token sums:
 *   pf_pif_alphas: x_dev [B, T, D] rows of the padded batch, lens_host [B] -> alphas_dev [B, T] (exactly 0 at t >= lens[b]) and
 *     token_num_dev [B], their sums. The depthwise conv is not masked (the reference's is not): it reads the clip's own padded rows and
 *     zeros outside [0, T), never another clip's.
 *   the caller rounds the sums half to even (on the fp32 value) -> counts_host [B], Lmax = their maximum (>= 1; a batch without any
 *     token needs no second call)
 *   pf_pif_embeds: alphas_dev is normalised IN PLACE by counts[b] / token_num[b] (all zero for a clip with a zero sum or count: no
 *     division), align_dev [B, T] receives its inclusive prefix sums, embeds_dev [B, Lmax, D] the Gaussian-kernel attention from the
 *     fire positions l + 0.5 to the frames t < lens[b], per sigma head over its D / sigma_heads channels. Every clip gets all Lmax rows
 *     (rows at or past its own count are the reference's too); a clip with lens[b] == 0 gets zero rows; rows of x_dev at or past
 *     lens[b] are not read.
 * Limits: D <= 1024, 1 .. 8 sigma heads with D / sigma_heads a multiple of 32, l_order / r_order 0 .. 15, T <= 5000, Lmax <= 2048. No sync. */
typedef struct pf_pif pf_pif;
typedef struct pf_pif_config {
    int32_t d_model, l_order, r_order, sigma_heads;
    float threshold;              /* carried for the record: the inference path does not read it */
    float smooth_factor, noise_threshold;
} pf_pif_config;
pf_pif* pf_pif_create(const pf_pif_config* cfg);
void pf_pif_destroy(pf_pif* h);
int pf_pif_set_tensor(pf_pif* h, const char* name, const float* data, int64_t numel);
int pf_pif_missing(const pf_pif* h);
int pf_pif_alphas(pf_pif* h, const float* x_dev, const int32_t* lens_host, int32_t B, int32_t T, float* alphas_dev, float* token_num_dev,
                  void* stream);
int pf_pif_embeds(pf_pif* h, const float* x_dev, float* alphas_dev, const float* token_num_dev, const int32_t* counts_host,
                  const int32_t* lens_host, int32_t B, int32_t T, int32_t Lmax, float* align_dev, float* embeds_dev, void* stream);
/* pf_sandecoder: ParaformerSANDecoder.forward (decoder.py:1201-1251) + log-softmax + row arg-max, ONE pass over all B x L token rows:
 * the rows are the predictor's embeddings (no lookup, no positional row); per layer x += self_attn(norm1 x) (keys at or past the
 * clip's token count masked, not causal), x += src_attn(norm2 x, memory) (keys at or past the clip's encoder length masked),
 * x += w_2(relu(w_1(norm3 x))); then after_norm, output_layer. Tensor names: the reference's keys below `decoder.` without the unused
 * `embed.*` ("decoders.0.self_attn.linear_q.weight", "decoders.0.src_attn.linear_k.bias", "decoders.0.feed_forward.w_1.weight",
 * "decoders.0.norm3.weight", "after_norm.bias", "output_layer.weight", ...). Head dim 64, ffn_dim % 32.
 * precision 3 runs self_attn q / k / v / linear_out, src_attn.linear_q, w_1 and w_2 from two-plane fp16 operands at a-priori
 * exponents; src_attn.linear_k / linear_v / linear_out (no bound on the caller's memory) and output_layer stay exact fp32.
 * memory_dev [B, T, D], embeds_dev [B, L, D] -> logp_dev [B, L, V] (log-softmax; may be NULL), ids_dev / best_dev [B, L]: each row's
 * arg-max (first maximum) and its log-probability. A clip with tok_lens_host[b] == 0 has no self-attention key: its attention output
 * is zero, its rows stay finite and no other clip reads them. 1 <= T <= 12000, 1 <= L <= 2048. No sync. */
typedef struct pf_sandecoder pf_sandecoder;
typedef struct pf_sandecoder_config {
    int32_t d_model, n_heads, ffn_dim, n_blocks, vocab_size;
    int32_t precision;            /* 0 fp32, 3 f16x2 */
    float ln_eps;
} pf_sandecoder_config;
pf_sandecoder* pf_sandecoder_create(const pf_sandecoder_config* cfg);
void pf_sandecoder_destroy(pf_sandecoder* h);
int pf_sandecoder_set_tensor(pf_sandecoder* h, const char* name, const float* data, int64_t numel);
int pf_sandecoder_missing(const pf_sandecoder* h);
int pf_sandecoder_set_precision(pf_sandecoder* h, int32_t precision);
int pf_sandecoder_forward(pf_sandecoder* h, const float* memory_dev, const int32_t* mem_lens_host, const float* embeds_dev,
                          const int32_t* tok_lens_host, int32_t B, int32_t T, int32_t L, float* logp_dev, int32_t* ids_dev, float* best_dev,
                          void* stream);
/* single-kernel hooks (tests) of the predictor: the alphas and their per-clip sums (lens_dev [B] on the device); the normalisation +
 * prefix sum (n_dev [B] counts; an_dev may be a_dev); the embeddings. Out-of-range arguments return an error and launch nothing. */
int pf_k_pif_alphas(const float* h_dev, const float* conv_w_dev, const float* conv_b_dev, const float* out_w_dev, const float* out_b_dev,
                    const int32_t* lens_dev, int32_t B, int32_t T, int32_t D, int32_t l_order, int32_t r_order, float smooth, float noise,
                    float* a_dev, float* token_num_dev, void* stream);
int pf_k_pif_align(const float* a_dev, const float* token_num_dev, const int32_t* n_dev, int32_t B, int32_t T, float* an_dev, float* align_dev,
                   void* stream);
int pf_k_pif_embed(const float* align_dev, const float* h_dev, const float* sigma_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t L,
                   int32_t D, int32_t H, float* embeds_dev, void* stream);

/* ---- Transducer (RNN-T) search (funasr/models/transducer: RNNTDecoder + JointNetwork + BeamSearchTransducer.default_beam_search,
 * the one decoding path the reference's Transducer builds: one utterance, is_final, no LM, no length normalisation). One handle
 * holds the prediction network (embedding, n_layers LSTM cells) and the joint network; the search loop runs on the host side of the
 * library: a prediction step (one launch per layer + lin_dec) only for a label prefix not seen in this utterance, two launches per
 * joint evaluation, one small read-back. All of it exact fp32 on the VALU; scores accumulate in double on the host.
 * Tensor names are the reference's keys: "decoder.embed.weight" [vocab, embed_dim], "decoder.rnn.<l>.weight_ih_l0" [4 hidden, in],
 * "decoder.rnn.<l>.weight_hh_l0" [4 hidden, hidden], "decoder.rnn.<l>.bias_ih_l0" / "bias_hh_l0" [4 hidden] (gates i, f, g, o),
 * "joint_network.lin_enc.weight" [joint_dim, enc_dim] / ".bias", "joint_network.lin_dec.weight" [joint_dim, hidden],
 * "joint_network.lin_out.weight" [vocab, joint_dim] / ".bias".
 * Limits: vocab >= 2, blank_id 0, embed_dim / hidden / joint_dim multiples of 4 and <= 1024, enc_dim a multiple of 32 (the K step of
 * the fp32 GEMM that projects the frames) and <= 1024, 1 <= n_layers <= 4, beam <= 16. */
typedef struct pf_transducer pf_transducer;
typedef struct pf_transducer_config {
    int32_t vocab, enc_dim, embed_dim, hidden, n_layers, joint_dim, blank_id;
} pf_transducer_config;
pf_transducer* pf_transducer_create(const pf_transducer_config* cfg);
void pf_transducer_destroy(pf_transducer* h);
int pf_transducer_set_weights(pf_transducer* h, const char* name, const float* data, int64_t numel);
int pf_transducer_missing(const pf_transducer* h);
/* the message of this handle's last failed search ("" after a good one); the string lives until the next search on the handle */
const char* pf_transducer_last_error(const pf_transducer* h);
/* what pf_transducer_search returns beside 0 and the negative statuses of every entry point */
#define PF_TRANSDUCER_NONFINITE 2     /* a joint record held a non-finite value (NaN / inf weights or encoder output) */
#define PF_TRANSDUCER_CAP 3           /* a frame needed more than max_expansions_per_frame joint evaluations */
/* enc_out_dev [T, enc_dim] of ONE utterance -> the min(nbest, found) best hypotheses, best first: ids_out [nbest, max_len] (row i:
 * lens_out[i] labels, the leading blank of the reference's yseq included), scores_out [nbest], *n_out rows.
 * max_expansions_per_frame <= 0: 64 * beam. stats_out (optional) int64 [3]: joint evaluations, prediction steps, the largest
 * number of joint evaluations of one frame -- written on failure too. Synchronises the stream (one read-back per evaluation). */
int pf_transducer_search(pf_transducer* h, const float* enc_out_dev, int32_t T, int32_t beam, int32_t nbest,
                         int32_t max_expansions_per_frame, int32_t* ids_out, int32_t* lens_out, double* scores_out, int32_t max_len,
                         int32_t* n_out, int64_t* stats_out, void* stream);
/* single-kernel hooks of the above (tests), on caller-supplied device buffers.
 * pf_k_rnnt_pred_step: one prediction step for `label`. weights_dev: per layer l, back to back, weight_ih [4 H, in_l] (in_0 = E,
 * else H), weight_hh [4 H, H], bias_ih [4 H], bias_hh [4 H]. state_dev [n_slots][L][2][H] (h then c), dec_proj_dev [n_slots][J].
 * Reads slot src, writes slot dst (state and dec_proj = lin_dec . h' of the last layer) and nothing else; src == dst is refused.
 * pf_k_rnnt_joint_topk: log-softmax(lin_out . tanh(enc_proj + dec_proj) + bias) -> record_dev [1 + 2 k] 4-byte words: logp of row 0,
 * the k best logp among rows >= 1 (equal values: lower row first), their rows as int32. k <= min(16, V - 1). partials_dev: scratch of
 * pf_k_rnnt_joint_partial_floats(V, k) floats, fully rewritten. */
int pf_k_rnnt_pred_step(const float* embed_dev, const float* weights_dev, const float* lin_dec_dev, float* state_dev, float* dec_proj_dev,
                        int32_t n_slots, int32_t V, int32_t E, int32_t H, int32_t L, int32_t J, int32_t label, int32_t src, int32_t dst,
                        void* stream);
int64_t pf_k_rnnt_joint_partial_floats(int32_t V, int32_t k);
int pf_k_rnnt_joint_topk(const float* enc_proj_dev, const float* dec_proj_dev, const float* w_out_dev, const float* b_out_dev, int32_t V,
                         int32_t J, int32_t k, float* partials_dev, float* record_dev, void* stream);

typedef struct pf_ctc pf_ctc;
pf_ctc* pf_ctc_create(int32_t d_model, int32_t vocab_size);
void pf_ctc_destroy(pf_ctc* c);
int pf_ctc_set_tensor(pf_ctc* c, const char* name, const float* data, int64_t numel);   /* "ctc_lo.weight|bias" */
int pf_ctc_missing(const pf_ctc* c);
/* hidden_dev: [M, d_model]; ids_dev: int32 [M] frame-wise argmax; logits_dev (nullable): [M, vocab]. No sync. */
int pf_ctc_greedy(pf_ctc* c, const float* hidden_dev, int32_t M, int32_t* ids_dev, float* logits_dev, void* stream);
/* 0 = fp32 MFMA (default), 3 = the arg-max route (logits_dev == NULL) from two-plane fp16 operands on the fp16 MFMA
 * (fp32-class logits; the modes of pf_encoder_set_precision) */
int pf_ctc_set_precision(pf_ctc* c, int32_t mode);

/* ---- Paraformer-v2 posterior embedder (funasr/models/paraformer_v2_community/model.py:451-482,545-574, decoder.py:318-325): the
 * decoder input made from the CTC head instead of a CIF predictor. Per clip: frame-wise softmax of the CTC logits, greedy path,
 * maximal runs of one non-blank label over the clip's valid frames (the same label on both sides of a blank: two runs; sos / eos are
 * ordinary labels), the mean posterior of each run, then the decoder's input layer Linear(V -> D), LayerNorm(eps 1e-5), ReLU,
 * x * sqrt(D) + pe[token index]. Computed in the frame domain: E = probs . embed.0.weight^T per frame (row chunks whose logits /
 * probabilities stay under 256 MB), then mean over the run + bias per token. The CTC weights are BORROWED from a pf_ctc handle of the
 * same d_model / vocab. Tensor names: "embed.0.weight" [D, V], "embed.0.bias", "embed.1.weight", "embed.1.bias" [D] (the reference's
 * keys below `decoder.`) and "pos_table" [5000, D] (row p = the sinusoid of position p, built on the host as the reference does). */
typedef struct pf_posterior_embed pf_posterior_embed;
pf_posterior_embed* pf_posterior_embed_create(int32_t vocab_size, int32_t d_model, int32_t blank_id);   /* d_model % 32 == 0, <= 2048 */
void pf_posterior_embed_destroy(pf_posterior_embed* h);
int pf_posterior_embed_set_tensor(pf_posterior_embed* h, const char* name, const float* data, int64_t numel);
int pf_posterior_embed_missing(const pf_posterior_embed* h);
/* 0 = both GEMMs on the exact-fp32 MFMA; 3 (default) = two-plane fp16 operands on the fp16 MFMA, fp32-class results (of the logits,
 * the last vocab_size % 4 columns come from the fp32 MFMA). Other modes are refused with a message. */
int pf_posterior_embed_set_precision(pf_posterior_embed* h, int32_t mode);
/* rows of [B * T] per chunk; 0 (default) = as many as the 256 MB workspace cap admits. A row's result does not depend on it. */
int pf_posterior_embed_set_chunk_rows(pf_posterior_embed* h, int32_t rows);
/* test hook like pf_decoder_debug_poison: fills the handle's activation workspaces with `byte`; a pf_posterior_embed_embeds then
 * needs a new pf_posterior_embed_runs. Synchronises. */
int pf_posterior_embed_debug_poison(pf_posterior_embed* h, int32_t byte);
/* hidden_dev [B, T, d_model] (encoder output), lens_host[b] in 1 .. T valid frames. Enqueues logits / softmax / arg-max / E and the
 * run scan, then waits ONCE for the run counts: counts_host[b] = runs of clip b. path_dev (nullable): int32 [B, T] greedy path.
 * Returns N = the largest count (0: every clip is blank), negative on error (pf_last_error). */
int pf_posterior_embed_runs(pf_posterior_embed* h, pf_ctc* ctc, const float* hidden_dev, const int32_t* lens_host, int32_t B, int32_t T,
                            int32_t* counts_host, int32_t* path_dev, void* stream);
/* after pf_posterior_embed_runs with the same B / T: embeds_dev [B, N, d_model] (rows >= counts[b] zero; runs past N dropped),
 * run_ranges_dev (nullable) int32 [B, N, 2] = first and one-past-last frame of each run (zero behind). N == 0 writes nothing. No sync. */
int pf_posterior_embed_embeds(pf_posterior_embed* h, int32_t B, int32_t T, int32_t N, float* embeds_dev, int32_t* run_ranges_dev,
                              void* stream);

/* ----------------------------------------------------------------------------------------------- streaming
 * Chunked online decoding (ParaformerStreaming, funasr/models/paraformer_streaming/model.py:552-763): one handle =
 * a lock-step batch of n_streams independent streams (the reference: exactly 1) with all caches in HBM
 * (encoder K/V rings funasr/models/sanm/attention.py:343-361, overlap window funasr/models/scama/encoder.py:480-494,
 * CIF remainder cif_predictor.py:347-392, decoder FSMN / cross-attention caches attention.py:606-625,829-841).
 * The steady-state step is captured in a hipGraph per (n_frames, is_final, tail_chunk) and replayed. */
typedef struct pf_stream pf_stream;

typedef struct pf_stream_config {
    int32_t n_streams;        /* streams advanced together (>= 1) */
    int32_t chunk_left;       /* chunk_size[0] = 0 */
    int32_t chunk_cur;        /* chunk_size[1] = 10 LFR frames = 600 ms */
    int32_t chunk_right;      /* chunk_size[2] = 5 look-ahead frames */
    int32_t enc_look_back;    /* encoder_chunk_look_back (chunks), 4 */
    int32_t dec_look_back;    /* decoder_chunk_look_back (chunks), 1 */
    int32_t max_frames;       /* most feature frames a step may bring (>= chunk_cur) */
    int32_t max_tokens;       /* token rows decoded per stream per step (<= 96) */
    int32_t use_graph;        /* 1: capture + replay the step as a hipGraph */
} pf_stream_config;

/* the three handles must outlive the stream and carry all their tensors */
pf_stream* pf_stream_create(pf_encoder* e, pf_predictor* p, pf_decoder* d, const pf_stream_config* cfg);
void pf_stream_destroy(pf_stream* s);
/* sinusoidal position table, row r = position r+1 (StreamSinusoidalPositionEncoder, embedding.py:468-482); host or
 * device pointer, [rows, input_dim]. Default: 4096 rows computed with libm. */
int pf_stream_set_pe(pf_stream* s, const float* pe, int32_t rows);
int pf_stream_reset(pf_stream* s, void* stream);
/* "gemm_mode": 0 (default) = the step's GEMMs on the fp32 kernels (weight-streaming GEMM for a few rows: the latency path of
 * one or a few streams); 3 = on the fp16 matrix cores with two-plane fp16 operands and fp32 results (the offline f16x2 mode's
 * arithmetic, pf_encoder_set_precision 3: the throughput path of many lock-step streams). Attention, FSMN, CIF and the caches
 * stay fp32 in both. The reference has one arithmetic (torch fp32, paraformer_streaming/model.py:552-763); both modes meet
 * its parity bars. Synchronises, prepares the weight planes, drops captured graphs.
 * A/B switches of the step's launch fusions (defaults in brackets; all but "ln_carry" return the bits of the
 * separate launches): "ln_carry" [2] fp32 step: LayerNorms carried between the small-M GEMMs (0 never, 1 steps of <= 32 rows,
 * 2 always; one-pass variance: fp32-class, not the bits of the stand-alone LayerNorm); "fsmn_rides" [1] the encoder's FSMN memory
 * block inside the attention launch; "kv_batched" [1] fp32 step: the decoder's key/value projections of the step's encoder rows
 * and the ring appends as one launch each; "ln_folded" [1] f16x2 step: LayerNorms in the second launch of the split-K
 * projections, attention writing the out-projection's operand planes; "short_k" [3] f16x2 step of a small handle (<= 2048 rows):
 * linear_out in the four-slice split-K form with norm2 in its second launch (0 never, 1 / 2 every K = d_model projection: break-even);
 * "wide_k" [0] four workgroups per tile for the long-K
 * projections of a <= 32-row step (bitwise, slower: measured and kept off). */
int pf_stream_set_option(pf_stream* s, const char* key, int32_t value);
/* One chunk for every stream. feats_dev: [n_streams, n_frames, input_dim] un-scaled online features (ignored for a
 * tail chunk, which re-feeds the cached window, model.py:715-720). Outputs: ids_host int32 [n_streams, max_tokens]
 * (raw arg-max ids incl. sos/eos/blank), n_tokens_host int32 [n_streams]; optional enc_out_dev
 * [n_streams, W, d_model] (W = chunk_left + chunk_right + n_frames, or chunk_left + chunk_right for a tail chunk).
 * SYNCHRONISES (returns host values). */
int pf_stream_step(pf_stream* s, const float* feats_dev, int32_t n_frames, int32_t is_final, int32_t tail_chunk,
                   int32_t* ids_host, int32_t* n_tokens_host, float* enc_out_dev, void* stream);
/* pf_stream_step in two halves: _begin enqueues the step on the handle's own HIP stream and returns at once, _end waits for it and
 * fills ids_host / n_tokens_host. Handles built over DIFFERENT encoder / predictor / decoder handles may each have a step in
 * flight: steps of a few dozen streams leave most of the chip idle and overlap there (tools/bench_streaming.py --replicas). */
int pf_stream_step_begin(pf_stream* s, const float* feats_dev, int32_t n_frames, int32_t is_final, int32_t tail_chunk,
                         float* enc_out_dev, void* stream);
int pf_stream_step_end(pf_stream* s, int32_t* ids_host, int32_t* n_tokens_host);
/* debug / parity: carried CIF state and position counter (any pointer may be NULL) */
int pf_stream_peek(pf_stream* s, float* cif_alpha_host, float* cif_hidden_host, int32_t* start_idx_host);

/* ------------------------------------------------------------------------------------------------------------------
 * Utterance-level data parallelism over the GPUs of one node (dp_rccl.hip): ONE PROCESS PER GPU, RCCL over xGMI.
 * Replaces the reference's multi-GPU recipe -- one inference process per GPU over a split wav.scp, the outputs concatenated
 * (examples/aishell/paraformer/run.sh:135-190) -- for hosts that bind this header directly; funasr_amd/dp.py is the same
 * split on torch.distributed. The path shards over independent clips: there is NO collective on the data path. The two
 * exchanges: the weights once (rank `root` -> every rank, written straight into the handles' device storage) and a gather of
 * fixed-stride int32 hypotheses per batch.
 *   rank 0:      n = pf_dp_unique_id(id, 128)            -> ship the 128 bytes to the other ranks (any channel: a file, MPI, a socket)
 *   every rank:  hipSetDevice(local_rank); dp = pf_dp_create(id, 128, world, rank)     (collective: all ranks call it)
 *                pf_dp_broadcast_encoder(dp, enc, 0, stream) ... _predictor / _decoder / _ctc   (collective; handles built from
 *                                                                  the same config on every rank, tensors set on the root only)
 *                per batch: pf_dp_gather_ids(dp, my_ids_dev, n, all_ids_dev_on_root, 0, stream)
 * RCCL is loaded on first use (dlopen): without it every pf_dp_* call fails with pf_last_error() and nothing else changes. */
typedef struct pf_dp pf_dp;
/* rank 0 only: fills the 128-byte RCCL unique id; returns 128, or < 0 */
int pf_dp_unique_id(void* id_out, int32_t cap);
/* communicator of `world` ranks on the CURRENT device (one rank per device; collective). NULL on failure. */
pf_dp* pf_dp_create(const void* unique_id, int32_t id_bytes, int32_t world, int32_t rank);
int pf_dp_destroy(pf_dp* dp);
int pf_dp_world(const pf_dp* dp);
int pf_dp_rank(const pf_dp* dp);
/* rank `root`'s weights -> the same handle on every rank, in place in library-owned HBM (one grouped broadcast over the
 * handle's tensors); every tensor must be set on the root; on return (stream synchronised) the handle is ready on all ranks */
int pf_dp_broadcast_encoder(pf_dp* dp, pf_encoder* e, int32_t root, void* stream);
int pf_dp_broadcast_predictor(pf_dp* dp, pf_predictor* p, int32_t root, void* stream);
int pf_dp_broadcast_decoder(pf_dp* dp, pf_decoder* d, int32_t root, void* stream);
int pf_dp_broadcast_ctc(pf_dp* dp, pf_ctc* c, int32_t root, void* stream);
/* any device buffer (parameters that live outside the module handles): rank `root`'s bytes -> every rank, in place. Enqueued on
 * `stream`; does not synchronise. */
int pf_dp_broadcast_raw(pf_dp* dp, void* buf_dev, int64_t bytes, int32_t root, void* stream);
/* ids_dev: `count` int32 on this rank's device (e.g. [B, 1 + n_pad]: token count, then ids); out_dev (root only):
 * world * count int32, rank r's block at r * count. Enqueued on `stream`; does not synchronise. */
int pf_dp_gather_ids(pf_dp* dp, const int32_t* ids_dev, int64_t count, int32_t* out_dev, int32_t root, void* stream);

/* online frontend pieces (WavFrontendOnline, wav_frontend.py:395-505): log-mel of one buffer, and LFR + CMVN over a
 * frame buffer that already carries its left context */
int pf_frontend_fbank(pf_frontend* f, const float* wav_dev, int64_t n_samples, float* fbank_dev, void* stream);
int pf_frontend_lfr_cmvn(pf_frontend* f, const float* frames_dev, int32_t T, int32_t rows, float* out_dev, void* stream);

/* Test hooks: fill every activation workspace of the handle with `byte` (use 0x7B: huge finite fp16 / fp32 patterns). A
 * forward must not depend on what earlier batches left there (tests/test_stateless_gpu.py). Synchronise. */
int pf_encoder_debug_poison(pf_encoder* e, int32_t byte);
int pf_decoder_debug_poison(pf_decoder* d, int32_t byte);
int pf_predictor_debug_poison(pf_predictor* p, int32_t byte);
/* -------------------------------------------------------------------------------- single kernels (tests / bench)
 * Thin wrappers over the individual gfx950 kernels so that parity tests and the roofline bench can drive one
 * kernel at a time through the same ABI. All pointers are device pointers. */
/* small-M GEMM with a LayerNorm carried between GEMMs (the streaming step's fused LayerNorms): see gemm_skinny.hip.
 * stats_out [M][N / 16][2]: the block partials (sum, sum of squares) of the finished outputs; out_gamma [N] (with stats_out): the
 * stored values are C * out_gamma. stats_in [M][K / 16][2] + ln_c (2 N floats from pf_k_ln_consts): C = W LayerNorm(A) + bias
 * evaluated as rstd (W (gamma A) - mean c1) + c2; ln_g = gamma, or NULL when A already holds gamma A.
 * ws_part (>= tiles * 16 * 512 floats) + ws_count (one zeroed int32 per tile; tiles = ceil(N / 16) * ceil(M / 16 or 32)), M <= 32:
 * the four-workgroups-per-tile form for long K, the same bits */
int pf_k_gemm_skinny_ln(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, const float* R2, int32_t ldr2,
                        float* Cout, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t relu, float* stats_out,
                        const float* stats_in, const float* ln_g, const float* ln_c, float ln_eps, const float* out_gamma, float* ws_part,
                        int32_t* ws_count, void* stream);
int pf_k_ln_consts(const float* W, int32_t ldw, int32_t N, int32_t K, const float* gamma, const float* beta, const float* bias, float* c,
                   void* stream);
/* test hook: pf_k_gemm_f32 takes the small-M weight-streaming kernel (the streaming step's GEMM) for M <= m;
 * default 0 = the 128x128 tile kernel (the offline path's GEMM) */
int pf_set_skinny_max_m(int32_t m);
/* read-only: rows of the block tile (64 or 128) the tile kernel takes for an M x N problem, fp32 and bf16 operands alike: the
 * launcher's own rule, so that a test can tell which form a shape reaches; both forms give a row the same bits */
int pf_k_gemm_f32_block_rows(int32_t M, int32_t N);
int pf_k_gemm_f32(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, const float* R1,
                  int32_t ldr1, const float* R2, int32_t ldr2, float* C, int32_t ldc, int32_t M, int32_t N,
                  int32_t K, int32_t relu, void* stream);
/* 1 if the library holds the measured-and-off kernel shapes and ablation builds (libparaformer_hip_measure.so, `make -C funasr_amd/csrc
 * measure`: what tools/bench_*.py and the records under profiles/ were made with); 0 for the product library, in which the option keys
 * and tile ids of those shapes return an error. */
int pf_measurement_build(void);
/* Conv1d over time as one exact-fp32 GEMM whose im2col is gathered by the operand loads (the predictor's cif_conv1d,
 * funasr/models/paraformer/cif_predictor.py:275-278): hidden [B, T, D], W [N, taps * D] (column tap * D + c = weight[n, c, tap]),
 * C [B * T, N]; rows t + tap - left outside [0, T) read as zero; zero_dev: >= 128 B of zeros; D % 32 == 0. Bitwise pf_k_gemm_f32
 * on the materialised column matrix. */
int pf_k_conv1d_gemm_f32(const float* hidden, const float* W, const float* bias, float* C, int32_t B, int32_t T, int32_t D,
                         int32_t N, int32_t taps, int32_t left, int32_t relu, const float* zero_dev, void* stream);
/* bf16-operand GEMM of the throughput mode: A [M,K] bf16, W [N,K] bf16 (strides in elements), fp32 accumulate on
 * v_mfma_f32_32x32x16_bf16, fp32 bias / residuals, C fp32 (c_bf16 = 0) or bf16 (1). K % 64 == 0. */
int pf_k_gemm_bf16(const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias, const float* R1,
                   int32_t ldr1, const float* R2, int32_t ldr2, void* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                   int32_t relu, int32_t c_bf16, void* stream);
int pf_k_gemm_bf16_time(const void* A, int32_t lda, const void* W, int32_t ldw, const float* bias, void* C, int32_t ldc,
                        int32_t M, int32_t N, int32_t K, int32_t c_bf16, int32_t iters, float* ms_out, void* stream);
/* fp32-accurate GEMM on the bf16 matrix cores (gemm_split3.hip): both operands as three bf16 planes
 * (x = hi + mid + lo exactly; plane p of a matrix starts `*_plane` elements after plane p-1), six bf16 MFMA products
 * per operand pair, fp32 accumulate / bias / residuals. Output fp32 C, or (C3 != NULL) the three planes of the result.
 * K % 32 == 0 (planes zero-padded), N % 4 == 0, strides in elements. */
int pf_k_split3(const float* x, int32_t ldx, void* y3, int32_t ldy, int64_t plane, int32_t M, int32_t N, void* stream);
int pf_k_gemm_split3(const void* A3, int32_t lda, int64_t a_plane, const void* W3, int32_t ldw, int64_t w_plane,
                     const float* bias, const float* R1, int32_t ldr1, const float* R2, int32_t ldr2, float* C,
                     int32_t ldc, void* C3, int32_t ldc3, int64_t c_plane, int32_t M, int32_t N, int32_t K,
                     int32_t relu, int32_t iters, float* ms_out, void* stream);
/* the kernels of the headline mode, one at a time (tests/test_kernels_f16x2_gpu.py):
 * full-row form of the N = 512 projections with the residual adds and the following LayerNorm in the epilogue
 * (gemm_f16x2_row.hip; replaces linear_out / w_2 + LayerNorm of funasr/models/sanm/encoder.py:120-146) */
int pf_k_gemm_f16x2_row(const void* A2, int32_t lda, int64_t a_plane, const void* W2, int32_t ldw, int64_t w_plane, float oscale,
                        const float* bias, const float* R1, int32_t ldr1, const float* R2, int32_t ldr2, float* C, int32_t ldc,
                        const float* ln_g, const float* ln_b, float ln_eps, void* Y2, int64_t y_plane, float yscale, float* Yf,
                        int32_t M, int32_t K, int32_t relu, int32_t a_nt, int32_t iters, float* ms_out, void* stream);
/* The encoder block's position-wise feed-forward in ONE launch (gemm_f16x2_ffn.hip; funasr/models/transformer/
 * positionwise_feed_forward.py:14-34 with the residual add of sanm/encoder.py:141-146 and, optionally, the next LayerNorm):
 * Cout = R + (relu(X W1^T + b1) W2^T + b2); with ln_g: Y2 (planes of LayerNorm(Cout) * yscale) or Yf (fp32). X2 [2][M, 512],
 * W1 [2][F, 512], W2 [2][512, F] are two-plane fp16 operands (hi plane, then lo plane); oscale1 = 2^-(e_x + e_w1), hscale = the
 * hidden activations' plane scale 2^e_h, oscale2 = 2^-(e_h + e_w2). F % 128 == 0. Cout may alias R. */
int pf_k_ffn_f16x2(const void* X2, const void* W1, const void* W2, const float* b1, const float* b2, float oscale1, float hscale,
                   float oscale2, const float* R, float* Cout, const float* ln_g, const float* ln_b, float ln_eps, void* Y2,
                   float yscale, float* Yf, int32_t M, int32_t F, int32_t iters, float* ms_out, void* stream);
/* FSMN form of the full-row kernel: the first addend is the FSMN memory block (11 taps [512, 11], left padding 5;
 * funasr/models/sanm/attention.py:216-239) of the fp32 rows fs_v [M, 512], computed in the epilogue; fs_lo / fs_hi (device
 * int32 [M / 16]): valid input rows [lo, hi) of the sequence that owns each 16-row group. M % 16 == 0; ln_g / ln_b required */
int pf_k_gemm_f16x2_row_fsmn(const void* A2, int32_t lda, int64_t a_plane, const void* W2, int32_t ldw, int64_t w_plane, float oscale,
                             const float* bias, const float* fs_v, int32_t ldfv, const float* fs_w, const int32_t* fs_lo,
                             const int32_t* fs_hi, const float* R2, int32_t ldr2, float* C, int32_t ldc, const float* ln_g,
                             const float* ln_b, float ln_eps, void* Y2, int64_t y_plane, float yscale, float* Yf, int32_t M, int32_t K,
                             int32_t a_nt, int32_t iters, float* ms_out, void* stream);
/* LayerNorm writing the two fp16 planes of y * scale (what the f16x2 GEMMs read) */
int pf_k_layernorm_planes(const float* x, int32_t ldx, const float* gamma, const float* beta, void* y2, int32_t ldy, int64_t plane,
                          float scale, int32_t M, int32_t D, float eps, int32_t iters, float* ms_out, void* stream);
/* QKV form (kv_form 0, N = 3 D: Q planes, K planes, fp32 V, V^T planes) / KV form (kv_form 1, N = 2 D: K planes, V^T planes) */
int pf_k_gemm_f16x2_qkv(const void* A2, int32_t lda, int64_t a_plane, const void* W2, int32_t ldw, int64_t w_plane, float oscale,
                        const float* bias, int32_t M, int32_t D, int32_t K, int32_t kv_form, void* Qp, void* Kp, int64_t qk_plane,
                        float* Vf, void* VT, int32_t ldvt, int64_t vt_plane, float q_mul, float k_mul, float v_mul, int32_t tile,
                        int32_t iters, float* ms_out, void* stream);
/* fused arg-max form (vocabulary / CTC projection): ids[row] = argmax_n, lowest index on ties; scratch [M, 2 ceil(N / 256)] */
int pf_k_gemm_f16x2_argmax(const void* A2, int32_t lda, int64_t a_plane, const void* W2, int32_t ldw, int64_t w_plane, float oscale,
                           const float* bias, int32_t M, int32_t N, int32_t K, int32_t* ids, float* scratch_val,
                           int32_t* scratch_idx, void* stream);
/* two-plane fp16 split operands (x * scale = hi + lo) and the fp32-accurate three-product GEMM on them (gemm_f16x2.hip) */
int pf_k_split2(const float* x, int32_t ldx, void* y2, int32_t ldy, int64_t plane, int32_t M, int32_t N, float scale,
                void* stream);
int pf_k_gemm_f16x2(const void* A2, int32_t lda, int64_t a_plane, const void* W2, int32_t ldw, int64_t w_plane,
                    float oscale, const float* bias, const float* R1, int32_t ldr1, const float* R2, int32_t ldr2,
                    float* C, int32_t ldc, void* C2, int32_t ldc2, int64_t c_plane, float cscale, int32_t M, int32_t N,
                    int32_t K, int32_t relu, int32_t tile, int32_t iters, float* ms_out, void* stream);
/* attention on two-plane fp16 operands (attention_f16x2.hip; the layouts the QKV / KV forms of gemm_f16x2.hip write) */
int pf_k_attention_f16x2(const void* Q2, int64_t q_plane, const void* K2, int64_t k_plane, const void* VT2, int32_t ldvt,
                         int64_t vt_plane, void* O2, int64_t o_plane, const int32_t* klens_dev, int32_t B, int32_t H,
                         int32_t Tp, int32_t Tq, float sscale, float oscale, int32_t variant, int32_t iters, float* ms_out,
                         void* stream);
/* fp32 -> bf16 (round to nearest even), n % 4 == 0 */
int pf_k_cast_bf16(const float* x, void* y, int64_t n, void* stream);
int pf_k_gemm_argmax_f32(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, int32_t M,
                         int32_t N, int32_t K, int32_t* ids, float* scratch_val, int32_t* scratch_idx, void* stream);
/* row-wise log-softmax over N columns (the scores the beam search of paraformer/search.py consumes); in place allowed */
int pf_k_log_softmax(const float* x, int32_t ldx, float* y, int32_t ldy, int32_t M, int32_t N, void* stream);
int pf_k_layernorm(const float* x, int32_t ldx, const float* gamma, const float* beta, float* y, int32_t ldy,
                   int32_t M, int32_t D, int32_t Dpad, float eps, void* stream);
int pf_k_fsmn(const float* in, int32_t ldin, const float* w, const float* R, int32_t ldr, float* out, int32_t ldo,
              const int32_t* lens_dev, int32_t B, int32_t T, int32_t C, int32_t K, int32_t left_pad, void* stream);
/* The attention hooks and an EMPTY key sequence (klens_dev[b] < 1); none of them checks the device-side lengths.
 * pf_k_attention_f32 (attention_f32.hip: the LDS-DMA, the register-staged and the few-query kernel) writes zero rows for that
 * sequence, as the reference's masked_fill(0) after the softmax does, and reads none of its K / V rows; the other sequences of the
 * batch are unaffected. pf_k_attention_f32_two_source always has n2 >= 1 keys. pf_k_attention_f32_dk (attention_mid.hip) also
 * writes zero rows, outside its stated contract. The Conformer / Transformer / LCB-Net attentions (attention_relpos.hip,
 * attention_abs.hip, lcbnet.hip) write zero rows. Every other hook REQUIRES klens_dev[b] >= 1 and the caller has to guarantee it, as
 * pf_encoder_forward, pf_decoder_forward and their kin do by refusing lens < 1: pf_k_attention_split3 would read the K / V row in
 * front of the sequence's first one, pf_k_attention_bf16 and pf_k_attention_small would store NaN rows, pf_k_attention_f16x2 takes
 * klens in 1 .. Tp. emotion2vec's ALiBi attention works on packed rows, where a sequence without rows has no query either. */
int pf_k_attention_f32(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                       float* O, int32_t ldo, const int32_t* klens_dev, int32_t B, int32_t H, int32_t Tq,
                       int32_t Tk, float scale, void* stream);
/* the same with two key/value sources (the streaming step's [cached ring | this chunk]): sequence b takes keys
 * [0, n1_dev[b * n1_stride]) from (K, V; Tk rows per sequence) and then n2 keys from (K2, V2; T2 rows per sequence) */
int pf_k_attention_f32_two_source(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                                  const float* K2, int32_t ldk2, const float* V2, int32_t ldv2, float* O, int32_t ldo,
                                  const int32_t* n1_dev, int32_t n1_stride, int32_t B, int32_t H, int32_t Tq,
                                  int32_t Tk, int32_t T2, int32_t n2, float scale, void* stream);
/* small heads (d_k <= 64, multiple of 4; the CT-Transformer's 8 x 32), Tk <= 1024: rows hold H heads of d_k columns */
int pf_k_attention_small(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                         float* O, int32_t ldo, const int32_t* klens_dev, int32_t B, int32_t H, int32_t d_k,
                         int32_t Tq, int32_t Tk, float scale, void* stream);
/* heads of d_k = 80 or 96 (MonotonicAligner's 4 x 80), any Tk, exact fp32 on the matrix cores (attention_mid.hip): rows hold H
 * heads of d_k columns; one key/value source, key-padding mask (klens_dev[b] >= 1), fp32 output; columns >= H * d_k of O untouched */
int pf_k_attention_f32_dk(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                          float* O, int32_t ldo, const int32_t* klens_dev, int32_t B, int32_t H, int32_t Tq,
                          int32_t Tk, int32_t d_k, float scale, void* stream);
/* embedding lookup: out[i, :] = table[ids_dev[i], :] (ids clamped to [0, rows)); D % 4 == 0 */
int pf_k_gather_rows(const float* table, int32_t ld, int32_t rows, const int32_t* ids_dev, float* out, int32_t n,
                     int32_t D, void* stream);
/* same contract, both products on the bf16 MFMA from three-plane split operands (fp32-class results; mode bf16x3) */
int pf_k_attention_split3(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                          float* O, int32_t ldo, const int32_t* klens_dev, int32_t B, int32_t H, int32_t Tq,
                          int32_t Tk, float scale, void* stream);
/* bf16 twin of pf_k_attention_f32: Q/K/V/O bf16, strides in elements */
int pf_k_attention_bf16(const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, void* O,
                        int32_t ldo, const int32_t* klens_dev, int32_t B, int32_t H, int32_t Tq, int32_t Tk, float scale,
                        void* stream);
/* torch.nn.LSTM (one layer, ndir = 1 | 2, zero initial state) on device tensors in torch's layouts: x [B, T, D],
 * w_ih [ndir][4H][D], w_hh [ndir][4H][H], b_ih / b_hh [ndir][4H] -> out [B, T, ndir * H]; H % 16 == 0, H <= 512, D % 32 == 0.
 * Synchronises (lstm.hip). */
int pf_k_lstm(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t B, int32_t T,
              int32_t D, int32_t H, int32_t ndir, float* out, void* stream);
/* CIF integrate-and-fire on caller-provided weights (cif_v1, cif_predictor.py:853-908): alphas [B, T], hidden
 * [B, T, D] -> peaks [B, T] (= "fires"), n_fires int32 [B], embeds [B, N, D] (rows >= n_fires[b] zero). */
int pf_k_cif(const float* alphas, const float* hidden, int32_t B, int32_t T, int32_t D, int32_t N, float* peaks,
             int32_t* n_fires, float* embeds, void* stream);
/* the same with the utterance lengths and the tail of the predictors (tail_process_fn, cif_predictor.py:414-446), through the
 * launches the predictor handles make after their alpha kernel: alphas [B, T] with zeros at t >= lens_host[b] (host int32, 1 ..
 * T), tail_threshold > 0 adds it at index lens[b] (tail_mask) or T. loop = 0: the prefix-sum scan of CifPredictorV2 (any T);
 * loop = 1: the sequential fp32 `cif` of CifPredictorV3 (bicif_paraformer/cif_predictor.py:39-86; T <= 4095, refused beyond).
 * -> alphas_out [B, T+1] as the scan leaves them, peaks [B, T+1], n_fires int32 [B], n_tok int32 [B] (loop form only:
 * floor(sum alphas); may be NULL otherwise), embeds [B, N, D] (fires past N dropped, rows >= n_fires[b] zero). Synchronises. */
int pf_k_cif_tail(const float* alphas, const float* hidden, const int32_t* lens_host, int32_t B, int32_t T, int32_t D, int32_t N,
                  float tail_threshold, int32_t tail_mask, int32_t loop, float* alphas_out, float* peaks, int32_t* n_fires,
                  int32_t* n_tok, float* embeds, void* stream);
/* the run scan of the posterior embedder alone, on caller-provided greedy paths: ids_dev int32 [B, T], lens_host[b] in 0 .. T ->
 * counts_dev int32 [B], ranges_dev int32 [B, ld, 2] (first and one-past-last frame of run j < min(count, ld); entries behind are
 * left as they were). Synchronises. */
int pf_k_ctc_runs(const int32_t* ids_dev, const int32_t* lens_host, int32_t B, int32_t T, int32_t blank, int32_t* counts_dev,
                  int32_t* ranges_dev, int32_t ld, void* stream);
/* ids[row] = first column of the largest of x[row, 0 .. N) (row stride ldx >= N), as torch.argmax (a row of -inf only: 0; NaN
 * unspecified): the arg-max of the streaming decoder and of the vocabulary projection when logits are requested */
int pf_k_argmax_rows(const float* x, int32_t ldx, int32_t M, int32_t N, int32_t* ids, void* stream);
/* the row statistics of pf_k_log_softmax without its output: lse[row] = logsumexp(x[row, 0 .. N)) by the same reduction (x - lse is
 * bit for bit what pf_k_log_softmax stores), pred[row] = first column of the largest fl(x[row][j] - lse[row]), i.e. torch.argmax of the
 * rounded log-probabilities */
int pf_k_log_softmax_stats(const float* x, int32_t ldx, int32_t M, int32_t N, float* lse, int32_t* pred, void* stream);
/* batched CTC forced alignment, the arithmetic of funasr/models/sense_voice/utils/ctc_alignment.py comparison by comparison. Clip b
 * of B reads the in_lens_host[b] (0 .. 4096) rows b * T + t0 + t of emis [B, T, V] (row stride ld) and its tgt_lens_host[b]
 * (1 .. 1024) labels targets_dev[b * ldt + l] (device int32, ignore ids already mapped to `blank`; a label outside [0, V) emits
 * -inf); labels [B, T_out] (device int32) receives the label or `blank` aligned to every frame, -1 behind the clip's frames.
 * lse (may be NULL, device [B * T]): emis holds logits and the emission is fl(x - lse[row]). pred (may be NULL, device int32
 * [B * T]): rows with pred == blank take 0 as their blank emission. scratch: device memory of at least
 * pf_k_ctc_align_scratch_bytes(B, max in_lens, max tgt_lens) bytes, contents irrelevant. Anything outside these limits is refused
 * before the first launch. The host arrays are copied before the call returns; it does not synchronise. */
int64_t pf_k_ctc_align_scratch_bytes(int32_t B, int32_t T_max, int32_t L_max);
int pf_k_ctc_align(const float* emis, int32_t ld, int32_t T, int32_t V, int32_t t0, const float* lse, const int32_t* pred,
                   const int32_t* targets_dev, int32_t ldt, const int32_t* in_lens_host, const int32_t* tgt_lens_host, int32_t B,
                   int32_t blank, int32_t* labels, int32_t T_out, void* scratch, int64_t scratch_bytes, void* stream);
/* average kernel time in milliseconds of `iters` back-to-back launches of the GEMM above, measured with
 * hipEvents on `stream` (used by bench.py for the roofline line) */
int pf_k_gemm_f32_time(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float* C,
                       int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t iters, float* ms_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PARAFORMER_HIP_H_ */
