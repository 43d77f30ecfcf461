"""Drop the HIP classes into the reference's own registry.

`funasr.register.tables.register(table, key)` overwrites an existing key (funasr/register.py:172-177); calling
`funasr_amd.install()` after `import funasr` therefore re-points "WavFrontend", "SANMEncoder", "CifPredictorV2" / "V3",
"ParaformerSANMDecoder", "Paraformer", "BiCifParaformer", "SeacoParaformer", "ContextualParaformer" (+ its decoder),
"ParaformerStreaming", "Paraformer_v2_community" (+ "ParaformerSANMDecoder_v2_community"), "SenseVoiceSmall",
"FsmnVADStreaming", "CTTransformer", "CTTransformerStreaming", "CAMPPlus", "ERes2NetV2" (+ "iic/speech_eres2netv2_sv_zh-cn_16k-common"), "Emotion2vec", "Conformer", "Transformer", "EBranchformer" / "Branchformer" (+ "EBranchformerEncoder"), "EParaformer" (+ "PifPredictor", "ParaformerSANDecoder"), "Transducer" (+ "RWKVEncoder", "ChunkConformerEncoder", "rnnt_decoder", "joint_network"), "SANM" (+ "FsmnDecoder"), "UniASR" (+ "FsmnDecoderSCAMAOpt"), "MonotonicAligner", "LCBNet" (+ "TransformerTextEncoder", "FusionSANEncoder", "ConvBiasPredictor"), "FunASRNano" (+ the adaptor_classes "Transformer", and "Linear" / "QFormer" as names that refuse) (and their encoders / decoders / frontends) at the gfx950 implementations,
and `funasr.AutoModel(model=<dir>, device="cuda")` builds them by name (funasr/auto/auto_model.py:591-646) with no
other change. Without the `funasr` package pass any object with a compatible `register(table, key)` method.
"""
from __future__ import annotations


def hip_classes():
    """(table, key, class) triples of everything this package provides: every class the package's own registry
    (funasr_amd.register.tables) holds after its modules are imported -- frontends, encoders, predictors (V2, V3), decoder,
    the model classes (Paraformer, BiCifParaformer, SeacoParaformer, ParaformerStreaming, Paraformer_v2_community, SenseVoiceSmall,
    FsmnVADStreaming, CTTransformer, CTTransformerStreaming, CAMPPlus, ERes2NetV2, Emotion2vec, Conformer, Transformer, EBranchformer, EParaformer, Transducer (with the RWKVEncoder of its template and the ChunkConformerEncoder), SANM, UniASR, MonotonicAligner, LCBNet, FunASRNano with its adaptor_classes) and the tokenizers (CharTokenizer, SentencepiecesTokenizer,
    HuggingfaceTokenizer)."""
    from . import (bicif_paraformer, campplus, chunk_conformer, cif_predictor, conformer, contextual_paraformer, ct_transformer, e_paraformer, ebranchformer, emotion2vec, eres2net, fsmn_vad, lcbnet, monotonic_aligner, normalize,  # noqa: F401
                   paraformer, paraformer_decoder, paraformer_streaming, paraformer_v2, fun_asr_nano, rwkv_encoder, sanm, sanm_encoder, seaco_paraformer, sense_voice, tokenizer, transducer, transformer, uniasr, wav_frontend)
    from .register import TABLE_NAMES, tables as own

    out = []
    for table in TABLE_NAMES:
        for key, cls in sorted(getattr(own, table, {}).items()):
            out.append((table, key, cls))
    return out


def install(tables=None, include_tokenizer: bool = False):
    """Register the HIP classes into `tables` (default: funasr.register.tables). Returns the list of (table, key)."""
    if tables is None:
        from funasr.register import tables as _tables      # the reference package

        tables = _tables
    done = []
    for table, key, cls in hip_classes():
        if table == "tokenizer_classes" and not include_tokenizer:
            continue                                        # the reference tokenizers are host-only and reused as-is
        tables.register(table, key)(cls)
        done.append((table, key))
    return done
