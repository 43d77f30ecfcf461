"""Seeded synthetic checkpoints and audio with the reference's state_dict key names and shapes.

There are no real weights or corpora in the build environment (no network), so parity tests and bench.py run on
random-initialised models of the exact Paraformer-large / SenseVoiceSmall architecture. Scales are chosen
"trained-like": residual stream O(1-5) after 50 blocks, CIF weights summing to ~4 tokens per second
(SURVEY.md section 8d). Key names follow funasr/models/{sanm/encoder.py,paraformer/cif_predictor.py,
paraformer/decoder.py,sense_voice/model.py}; a real model.pt uses the same keys.

Everything is generated with a CPU torch.Generator, so the same seed gives the same tensors on every machine.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

PARAFORMER_LARGE = dict(
    frontend=dict(fs=16000, window="hamming", n_mels=80, frame_length=25, frame_shift=10, lfr_m=7, lfr_n=6,
                  dither=0.0),
    encoder=dict(input_size=560, output_size=512, attention_heads=4, linear_units=2048, num_blocks=50,
                 kernel_size=11, sanm_shfit=0),
    predictor=dict(idim=512, threshold=1.0, l_order=1, r_order=1, tail_threshold=0.45, smooth_factor=1.0,
                   noise_threshold=0.0, tail_mask=True),
    decoder=dict(vocab_size=8404, encoder_output_size=512, attention_heads=4, linear_units=2048, num_blocks=16,
                 att_layer_num=16, kernel_size=11, sanm_shfit=0),
)

SENSEVOICE_SMALL = dict(
    frontend=dict(fs=16000, window="hamming", n_mels=80, frame_length=25, frame_shift=10, lfr_m=7, lfr_n=6,
                  dither=0.0),
    encoder=dict(input_size=560, output_size=512, attention_heads=4, linear_units=2048, num_blocks=50, tp_blocks=20,
                 kernel_size=11, sanm_shfit=0),
    vocab_size=25055,
)


def tiny(cfg: dict, enc_blocks: int = 2, dec_blocks: int = 2, vocab: int = 97, tp_blocks: int | None = None) -> dict:
    """Same architecture with fewer blocks / smaller vocabulary, for tests the CPU oracle finishes in seconds."""
    import copy

    c = copy.deepcopy(cfg)
    c["encoder"]["num_blocks"] = enc_blocks
    if "tp_blocks" in c["encoder"] and tp_blocks is not None:
        c["encoder"]["tp_blocks"] = tp_blocks
    if "decoder" in c:
        c["decoder"]["num_blocks"] = dec_blocks
        c["decoder"]["att_layer_num"] = dec_blocks
        c["decoder"]["vocab_size"] = vocab
    if "vocab_size" in c:
        c["vocab_size"] = vocab
    return c


class _Rng:
    def __init__(self, seed: int):
        self.g = torch.Generator(device="cpu").manual_seed(seed)

    def normal(self, *shape, std=1.0, mean=0.0):
        return torch.randn(*shape, generator=self.g, dtype=torch.float32) * std + mean


def _linear(sd, rng, name, out_f, in_f, gain=1.0, bias=True, bias_std=0.02):
    sd[name + ".weight"] = rng.normal(out_f, in_f, std=gain / math.sqrt(in_f))
    if bias:
        sd[name + ".bias"] = rng.normal(out_f, std=bias_std)


def _ln(sd, rng, name, dim):
    sd[name + ".weight"] = rng.normal(dim, std=0.1, mean=1.0)
    sd[name + ".bias"] = rng.normal(dim, std=0.05)


def encoder_state_dict(cfg: dict, seed: int = 0, prefix: str = "") -> Dict[str, torch.Tensor]:
    """Keys of SANMEncoder (sanm/encoder.py:351-377) / SenseVoiceEncoderSmall (sense_voice/model.py:575-621)."""
    rng = _Rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    D, F, Din, K = cfg["output_size"], cfg["linear_units"], cfg["input_size"], cfg["kernel_size"]
    blocks = [("encoders0.0", Din)] + [(f"encoders.{i}", D) for i in range(cfg["num_blocks"] - 1)]
    blocks += [(f"tp_encoders.{i}", D) for i in range(cfg.get("tp_blocks", 0))]
    for name, in_dim in blocks:
        p = prefix + name
        _ln(sd, rng, p + ".norm1", in_dim)
        _linear(sd, rng, p + ".self_attn.linear_q_k_v", 3 * D, in_dim, gain=1.0)
        sd[p + ".self_attn.fsmn_block.weight"] = rng.normal(D, 1, K, std=0.15)
        _linear(sd, rng, p + ".self_attn.linear_out", D, D, gain=0.5)
        _ln(sd, rng, p + ".norm2", D)
        _linear(sd, rng, p + ".feed_forward.w_1", F, D, gain=1.0)
        _linear(sd, rng, p + ".feed_forward.w_2", D, F, gain=0.5)
    _ln(sd, rng, prefix + "after_norm", D)
    if cfg.get("tp_blocks", 0) > 0:
        _ln(sd, rng, prefix + "tp_norm", D)
    return sd


def predictor_state_dict(cfg: dict, seed: int = 1, prefix: str = "", cif_bias: float = -1.5) -> Dict[str, torch.Tensor]:
    """Keys of CifPredictorV2 (paraformer/cif_predictor.py:241-243)."""
    rng = _Rng(seed)
    D = cfg["idim"]
    taps = cfg["l_order"] + cfg["r_order"] + 1
    w_out = rng.normal(1, D, std=2.0 / math.sqrt(D))
    w_out = w_out - w_out.mean()      # no seed-dependent offset: z ~ N(bias, ~1.4^2) for unit-variance hidden
    sd = {
        prefix + "cif_conv1d.weight": rng.normal(D, D, taps, std=1.0 / math.sqrt(D * taps)),
        prefix + "cif_conv1d.bias": rng.normal(D, std=0.02),
        prefix + "cif_output.weight": w_out,
        # -1.5 (the value the golden fixtures were made with) gives ~1.3 tokens/s on speech_like() clips through the
        # 50-block synthetic encoder; bench.py passes -0.1 = mean alpha ~0.24 = ~4 tokens/s (N ~ 120 per 30 s clip,
        # SURVEY.md 8d), measured with tools/calibrate_alpha.py
        prefix + "cif_output.bias": torch.tensor([cif_bias], dtype=torch.float32),
    }
    return sd


def decoder_state_dict(cfg: dict, seed: int = 2, prefix: str = "", with_embed: bool = False) -> Dict[str, torch.Tensor]:
    """Keys of ParaformerSANMDecoder (paraformer/decoder.py:329-392)."""
    rng = _Rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    D, F, K, V = cfg["encoder_output_size"], cfg["linear_units"], cfg["kernel_size"], cfg["vocab_size"]

    def ffn(p):
        _ln(sd, rng, p + ".norm1", D)
        _linear(sd, rng, p + ".feed_forward.w_1", F, D)
        _ln(sd, rng, p + ".feed_forward.norm", F)
        _linear(sd, rng, p + ".feed_forward.w_2", D, F, gain=0.5, bias=False)

    for i in range(cfg["att_layer_num"]):
        p = prefix + f"decoders.{i}"
        ffn(p)
        _ln(sd, rng, p + ".norm2", D)
        sd[p + ".self_attn.fsmn_block.weight"] = rng.normal(D, 1, K, std=0.15)
        _ln(sd, rng, p + ".norm3", D)
        _linear(sd, rng, p + ".src_attn.linear_q", D, D)
        _linear(sd, rng, p + ".src_attn.linear_k_v", 2 * D, D)
        _linear(sd, rng, p + ".src_attn.linear_out", D, D, gain=0.5)
    for i in range(max(cfg.get("num_blocks", cfg["att_layer_num"]) - cfg["att_layer_num"], 0)):   # decoders2 (decoder.py:363-380)
        p = prefix + f"decoders2.{i}"
        ffn(p)
        _ln(sd, rng, p + ".norm2", D)
        sd[p + ".self_attn.fsmn_block.weight"] = rng.normal(D, 1, K, std=0.15)
    ffn(prefix + "decoders3.0")
    _ln(sd, rng, prefix + "after_norm", D)
    _linear(sd, rng, prefix + "output_layer", V, D)
    if with_embed:
        sd[prefix + "embed.0.weight"] = rng.normal(V, D, std=0.02)   # training-only (decoder.py:314-317)
    return sd


BENCH_CIF_BIAS = -0.1


def paraformer_state_dict(cfg: dict = PARAFORMER_LARGE, seed: int = 0, cif_bias: float = -1.5) -> Dict[str, torch.Tensor]:
    sd = {}
    sd.update(encoder_state_dict(cfg["encoder"], seed * 3 + 0, "encoder."))
    sd.update(predictor_state_dict(cfg["predictor"], seed * 3 + 1, "predictor.", cif_bias=cif_bias))
    sd.update(decoder_state_dict(cfg["decoder"], seed * 3 + 2, "decoder."))
    return sd


def paraformer_v2_conf(d_model: int = 256, heads: int = 2, ffn: int = 512, enc_blocks: int = 2, dec_blocks: int = 2, vocab: int = 261,
                       kernel_size: int = 11, input_size: int = 560) -> dict:
    """constructor arguments of a Paraformer_v2_community model (the layout of funasr/models/paraformer_v2_community/template.yaml)
    at a chosen size"""
    enc = {"output_size": d_model, "attention_heads": heads, "linear_units": ffn, "num_blocks": enc_blocks, "dropout_rate": 0.1,
           "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.1, "input_layer": "pe", "pos_enc_class": "SinusoidalPositionEncoder",
           "normalize_before": True, "kernel_size": kernel_size, "sanm_shfit": 0, "selfattention_layer_type": "sanm"}
    dec = {"attention_heads": heads, "linear_units": ffn, "num_blocks": dec_blocks, "dropout_rate": 0.1, "positional_dropout_rate": 0.1,
           "self_attention_dropout_rate": 0.1, "src_attention_dropout_rate": 0.1, "att_layer_num": dec_blocks, "kernel_size": kernel_size,
           "sanm_shfit": 0, "input_layer": "linear"}
    return {"encoder": "SANMEncoder", "encoder_conf": enc, "decoder": "ParaformerSANMDecoder_v2_community", "decoder_conf": dec,
            "ctc_conf": {"dropout_rate": 0.0, "ctc_type": "builtin", "reduce": True, "ignore_nan_grad": True}, "ctc_weight": 0.3,
            "lsm_weight": 0.1, "length_normalized_loss": True, "input_size": input_size, "vocab_size": vocab, "blank_id": 0, "sos": 1, "eos": 2}


def paraformer_v2_state_dict(cfg: dict, seed: int = 0, ctc_gain: float = 8.0, blank_bias: float = 0.0) -> Dict[str, torch.Tensor]:
    """Keys of Paraformer_v2_community (paraformer_v2_community/model.py): encoder.*, decoder.* with the input layer
    decoder.embed.{0,1}.{weight,bias}, ctc.ctc_lo.*. `cfg` in the layout of paraformer_v2_conf(). A CONFIDENT CTC head: logits of
    order `ctc_gain` on unit-variance encoder output (a random head of order 1 has a flat density of top-2 gaps near zero, so a
    greedy path on it cannot be compared id for id); `blank_bias` is added to the blank's bias and sets the share of blank frames.
    The output layer gets the same gain."""
    ec, dc, V, Din = cfg["encoder_conf"], cfg["decoder_conf"], cfg["vocab_size"], cfg["input_size"]
    D = ec["output_size"]
    enc_cfg = dict(output_size=D, linear_units=ec["linear_units"], input_size=Din, kernel_size=ec["kernel_size"], num_blocks=ec["num_blocks"])
    dec_cfg = dict(encoder_output_size=D, linear_units=dc["linear_units"], kernel_size=dc["kernel_size"], vocab_size=V,
                   att_layer_num=dc["att_layer_num"], num_blocks=dc["num_blocks"])
    sd = {}
    sd.update(encoder_state_dict(enc_cfg, seed * 4 + 0, "encoder."))
    sd.update(decoder_state_dict(dec_cfg, seed * 4 + 1, "decoder."))
    rng = _Rng(seed * 4 + 2)
    sd["decoder.output_layer.weight"] = sd["decoder.output_layer.weight"] * ctc_gain
    sd["decoder.embed.0.weight"] = rng.normal(D, V, std=1.0)
    sd["decoder.embed.0.bias"] = rng.normal(D, std=0.02)
    _ln(sd, rng, "decoder.embed.1", D)
    _linear(sd, rng, "ctc.ctc_lo", V, D, gain=ctc_gain)
    sd["ctc.ctc_lo.bias"][cfg.get("blank_id", 0)] += blank_bias
    return sd


def sensevoice_state_dict(cfg: dict = SENSEVOICE_SMALL, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Keys of SenseVoiceSmall (sense_voice/model.py:702-737): encoder.*, embed.weight, ctc.ctc_lo.*"""
    sd = {}
    sd.update(encoder_state_dict(cfg["encoder"], seed * 3 + 0, "encoder."))
    rng = _Rng(seed * 3 + 1)
    D = cfg["encoder"]["output_size"]
    sd["embed.weight"] = rng.normal(16, cfg["encoder"]["input_size"], std=0.5)
    _linear(sd, rng, "ctc.ctc_lo", cfg["vocab_size"], D)
    return sd


def synthetic_cmvn(dim: int = 560, seed: int = 7):
    """Stand-in for am.mvn rows (<AddShift>, <Rescale>): shift ~ -mean(log-mel), scale ~ 1/std."""
    rng = _Rng(seed)
    shift = -(8.0 + rng.normal(dim, std=1.0))
    scale = 0.2 + 0.05 * torch.rand(dim, generator=rng.g)
    return shift.float(), scale.float()


def speech_like(n_samples: int, seed: int, fs: int = 16000) -> torch.Tensor:
    """Deterministic speech-like clip: harmonics of a slowly varying f0, syllable-rate amplitude
    modulation, a little noise, peak 0.3. float32 in [-1, 1]."""
    g = torch.Generator(device="cpu").manual_seed(1234 + seed)
    t = torch.arange(n_samples, dtype=torch.float64) / fs
    r = torch.rand(8, generator=g, dtype=torch.float64)
    f0 = 80.0 + 220.0 * r[0] + 20.0 * torch.sin(2 * math.pi * (0.3 + r[1]) * t)
    phase = 2 * math.pi * torch.cumsum(f0, 0) / fs
    nh = 3 + int(r[2] * 3)
    x = torch.zeros(n_samples, dtype=torch.float64)
    for h in range(1, nh + 1):
        x += torch.sin(h * phase + 6.28 * r[3] * h) / h
    am = 0.55 + 0.45 * torch.sin(2 * math.pi * (3.0 + 3.0 * r[4]) * t + 6.28 * r[5])
    x = x * am
    x = x + 0.01 * torch.randn(n_samples, generator=g, dtype=torch.float64)
    x = x / x.abs().max() * 0.3
    return x.float()


def confident_output_layer(weight: torch.Tensor, bias: torch.Tensor, hidden: torch.Tensor, margin: float = 4.0,
                           merge_cos: float = 0.98, chunk: int = 2048):
    """A "trained-like" output layer from a random one. A random Linear over 8404 classes puts the top two logits of a
    position ~0.24 sigma apart on average with a FLAT density of gaps near zero: about one position in 10^4 is a near-tie
    that any fp32 summation order flips, so id-level parity on random weights cannot tell a benign near-tie from a small
    systematic error. A trained model is confident on in-distribution speech. This is the closed-form stand-in for that
    training, on the hidden states `hidden` [n, D] the layer actually sees (the decoder's after_norm output at the token
    positions of a calibration batch; the encoder output at valid frames for a CTC head), in ONE step (no iteration):
      * position k is labelled with the class the random layer prefers for its CENTRED hidden state hc_k = h_k - mean (as
        diverse a label sequence as before); positions whose centred states nearly coincide (cosine > merge_cos) take the
        label of the first of them;
      * W_c += M hc_k / |hc_k|^2 and b_c -= M hc_k . mean / |hc_k|^2 for every position k labelled c: adds exactly M to
        position k's own logit of class c and M cos(hc_k, hc_j) |hc_j| / |hc_k| at any other position j. With
        M = margin / (1 - merge_cos) a position's own class leads every class labelled at a non-merged position by >= ~margin.
    Pure torch, runs on the tensors' device. Returns (weight, bias, stats); stats: min / median top-2 gap, the share of
    positions with a top-2 gap above 1e-3, distinct classes, merged positions."""
    W, b = weight.detach().clone().float(), bias.detach().clone().float()
    H = hidden.detach().float()
    n = H.shape[0]
    mean = H.mean(0)
    Hc = H - mean
    nrm2 = (Hc * Hc).sum(1, keepdim=True).clamp_min(1e-12)
    Hn = Hc / nrm2.sqrt()
    blocks = [slice(r0, min(n, r0 + chunk)) for r0 in range(0, n, chunk)]
    cls = torch.cat([(Hc[r] @ W.T).argmax(1) for r in blocks])
    rep = torch.cat([((Hn[r] @ Hn.T) > merge_cos).float().argmax(1) for r in blocks])     # first near-duplicate (<= own index)
    for _ in range(64):
        nxt = rep[rep]
        if bool(torch.equal(nxt, rep)):
            break
        rep = nxt
    cls = cls[rep]
    M = margin / (1.0 - merge_cos)
    d = Hc / nrm2
    W.index_add_(0, cls, M * d)
    b.index_add_(0, cls, -M * (d @ mean))
    gaps = []
    for r in blocks:
        v = (H[r] @ W.T + b).topk(2, dim=1).values
        gaps.append(v[:, 0] - v[:, 1])
    gaps = torch.cat(gaps)
    ar = torch.arange(n, device=H.device)
    stats = dict(min_gap=float(gaps.min()), median_gap=float(gaps.median()), frac_gap_above_1e3=float((gaps > 1e-3).float().mean()),
                 distinct_classes=int(cls.unique().numel()), merged_positions=int((rep != ar).sum()), positions=int(n), boost=M)
    return W, b, stats


def make_paraformer_confident(model, feats: torch.Tensor, flens, margin: float = 4.0):
    """Calibrate the output layer of a (synthetic) Paraformer mirror on one batch of features with confident_output_layer:
    runs the model's own device path up to the decoder's hidden states at the token positions, rewrites
    `decoder.output_layer.{weight,bias}` in place and returns ({state_dict key: cpu tensor} for the CPU oracle, stats)."""
    enc, olens = model.encode(feats, flens)
    embeds, token_num, _, _ = model.calc_predictor(enc, olens)
    tok = [int(round(v)) for v in token_num.tolist()]
    hid, _ = model.decoder(enc, olens, embeds, torch.tensor(tok), return_hidden=True)
    H = torch.cat([hid[b, : tok[b]] for b in range(len(tok)) if tok[b] > 0])
    lay = model.decoder.output_layer
    W, b, stats = confident_output_layer(lay.weight.to(H.device), lay.bias.to(H.device), H, margin=margin)
    with torch.no_grad():
        lay.weight.copy_(W.to(lay.weight.device))
        lay.bias.copy_(b.to(lay.bias.device))
    model.decoder.mark_dirty()
    return {"decoder.output_layer.weight": W.cpu(), "decoder.output_layer.bias": b.cpu()}, stats


def campplus_state_dict(seed: int = 0, embedding_size: int = 192) -> Dict[str, torch.Tensor]:
    """A CAM++ state dict in the reference's layout (funasr/models/campplus/model.py; 937 keys) with He-scaled conv weights and
    NON-trivial BatchNorm statistics (weight near 1, bias / running_mean off zero, running_var in [0.5, 2]), so that folding a
    BatchNorm into the conv before it is exercised and every layer still sees activations of order one."""
    from .campplus import CAMPPlus

    g = torch.Generator().manual_seed(seed)
    shapes = {k: tuple(v.shape) for k, v in CAMPPlus(embedding_size=embedding_size).state_dict().items()}
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + 1.5 * torch.rand(shp, generator=g)
        elif ".bn" in k or "batchnorm" in k or "shortcut.1" in k:
            sd[k] = (1.0 + 0.2 * torch.randn(shp, generator=g)) if k.endswith("weight") else 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            sd[k] = torch.randn(shp, generator=g) * (2.0 / fan_in) ** 0.5
    return sd


def eres2net_conf(feat_dim: int = 16, embedding_size: int = 32, m_channels: int = 16, num_blocks=(1, 1, 2, 1)) -> dict:
    """an ERes2NetV2 model_conf at a chosen size (default: the tiny configuration of the tests; the published model is
    feat_dim 80, embedding_size 192, m_channels 64, num_blocks [3, 4, 6, 3])"""
    return {"feat_dim": feat_dim, "embedding_size": embedding_size, "m_channels": m_channels, "baseWidth": 26, "scale": 2,
            "expansion": 2, "num_blocks": list(num_blocks), "pooling_func": "TSTP", "two_emb_layer": False}


def eres2net_state_dict(seed: int = 0, module_or_shapes=None, gain: float = 1.1) -> Dict[str, torch.Tensor]:
    """An ERes2NetV2 state dict in the reference's layout (funasr/models/eres2net/model.py: "model."-prefixed keys, 557 at the default
    configuration) for a module, a {name: shape} mapping, or (None) the default configuration. Conv weights are He-scaled times
    `gain` and the BatchNorm statistics are non-trivial (weight near 1, bias / running_mean off zero, running_var in [0.5, 2]), so
    that folding is exercised and the block outputs reach both ends of their clamp(0, 20) (a plain ReLU then fails the parity tests)."""
    if module_or_shapes is None:
        from .eres2net import ERes2NetV2SV

        module_or_shapes = ERes2NetV2SV()
    shapes = module_or_shapes if isinstance(module_or_shapes, dict) else {k: tuple(v.shape) for k, v in module_or_shapes.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in shapes.items():
        shp = tuple(shp)
        bn = len(shp) <= 1 and not k.endswith("seg_1.bias") and not (k.endswith(("local_att.0.bias", "local_att.3.bias")))
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + 1.5 * torch.rand(shp, generator=g)
        elif bn:
            sd[k] = (1.0 + 0.2 * torch.randn(shp, generator=g)) if k.endswith("weight") else 0.3 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            # layer3_ds has no BatchNorm behind it and seg_1 sums thousands of statistics of order 10: scaled down so that
            # fuse34's two inputs are of one size and the embedding is of order one
            scale = 0.02 if k.endswith("seg_1.weight") else (0.25 if k.endswith("layer3_ds.weight") else gain)
            sd[k] = torch.randn(shp, generator=g) * scale * (2.0 / fan_in) ** 0.5
    return sd


def emotion2vec_conf(embed_dim: int = 256, num_heads: int = 4, prenet_depth: int = 1, depth: int = 2, num_alibi_heads: int = None,
                     per_head: bool = True) -> dict:
    """an emotion2vec model_conf (template.yaml's layout) at a chosen size; the conv encoder is the real 512-channel stack"""
    return {"embed_dim": embed_dim, "num_heads": num_heads, "depth": depth, "mlp_ratio": 4.0, "norm_eps": 1e-05, "norm_affine": True,
            "layer_norm_first": False, "normalize": True, "extractor_mode": "layer_norm",
            "encoder_dropout": 0.0, "post_mlp_drop": 0.0, "attention_dropout": 0.0, "activation_dropout": 0.0, "dropout_input": 0.0,
            "layerdrop": 0.0, "start_drop_path_rate": 0.0, "end_drop_path_rate": 0.0, "end_of_block_targets": False,
            "modalities": {"audio": {"prenet_depth": prenet_depth, "num_extra_tokens": 10, "init_extra_token_zero": True,
                                     "use_alibi_encoder": True, "alibi_scale": 1.0, "learned_alibi": False, "learned_alibi_scale": True,
                                     "learned_alibi_scale_per_head": per_head, "learned_alibi_scale_per_layer": False,
                                     "num_alibi_heads": num_alibi_heads or num_heads, "model_depth": depth, "extractor_mode": "layer_norm",
                                     "feature_encoder_spec": "[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512,2,2)] + [(512,2,2)]",
                                     "conv_pos_width": 95, "conv_pos_groups": 16, "conv_pos_depth": 5, "conv_pos_pre_ln": False,
                                     "prenet_layerdrop": 0.0, "prenet_dropout": 0.0, "start_drop_path_rate": 0.0,
                                     "end_drop_path_rate": 0.0, "local_grad_mult": 1.0, "decoder": None}}}


def emotion2vec_state_dict(seed: int, model) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (an Emotion2vec module): fan-in scaled convs / linears, LayerNorms near
    identity, random extra tokens, per-head ALiBi scales around 1 with one negative entry (clamped to 0 by the model)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        shp = tuple(v.shape)
        if k.endswith("alibi_scale"):
            t = 0.5 + torch.rand(shp, generator=g)
            t.view(-1)[min(1, t.numel() - 1)] = -0.3
            sd[k] = t
        elif k.endswith("extra_tokens"):
            sd[k] = torch.randn(shp, generator=g)
        elif len(shp) == 1:
            is_ln = any(s in k for s in ("norm", ".2.1.", "project_features.1."))
            sd[k] = (1.0 + 0.2 * torch.randn(shp, generator=g)) if (is_ln and k.endswith("weight")) else 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            sd[k] = torch.randn(shp, generator=g) * (1.0 / fan_in) ** 0.5
    return sd


def conformer_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 256, enc_blocks: int = 2, dec_blocks: int = 2,
                   kernel: int = 15, macaron: bool = True, rel_pos_type: str = "legacy", vocab: int = 60, input_size: int = 80) -> dict:
    """constructor arguments of a Conformer model (the layout of funasr/models/conformer/template.yaml) at a chosen size"""
    enc = {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": enc_blocks,
           "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.0, "input_layer": "conv2d",
           "normalize_before": True, "pos_enc_layer_type": "rel_pos", "selfattention_layer_type": "rel_selfattn",
           "activation_type": "swish", "macaron_style": macaron, "use_cnn_module": True, "cnn_module_kernel": kernel}
    if rel_pos_type != "legacy":                       # the AISHELL yaml leaves it out: "legacy" is the constructor's default
        enc["rel_pos_type"] = rel_pos_type
    dec = {"attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": dec_blocks, "dropout_rate": 0.1,
           "positional_dropout_rate": 0.1, "self_attention_dropout_rate": 0.0, "src_attention_dropout_rate": 0.0}
    return {"encoder": "ConformerEncoder", "encoder_conf": enc, "decoder": "TransformerDecoder", "decoder_conf": dec,
            "ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False, "input_size": input_size, "vocab_size": vocab}


CONFORMER_AISHELL = dict(output_size=256, attention_heads=4, linear_units=2048, enc_blocks=12, dec_blocks=6, kernel=15, macaron=True,
                         rel_pos_type="legacy", vocab=4234)


def transformer_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 256, enc_blocks: int = 2, dec_blocks: int = 2,
                     vocab: int = 60, input_size: int = 80) -> dict:
    """constructor arguments of a Transformer model (the layout of examples/aishell/transformer/conf/*.yaml) at a chosen size"""
    enc = {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": enc_blocks,
           "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.0, "input_layer": "conv2d",
           "normalize_before": True}
    dec = {"attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": dec_blocks, "dropout_rate": 0.1,
           "positional_dropout_rate": 0.1, "self_attention_dropout_rate": 0.0, "src_attention_dropout_rate": 0.0}
    return {"encoder": "TransformerEncoder", "encoder_conf": enc, "decoder": "TransformerDecoder", "decoder_conf": dec,
            "ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False, "input_size": input_size, "vocab_size": vocab}


TRANSFORMER_AISHELL = dict(output_size=256, attention_heads=4, linear_units=2048, enc_blocks=12, dec_blocks=6, vocab=4234)


def transformer_state_dict(seed: int, model) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (a Transformer module or the reference's), drawn as conformer_state_dict draws them"""
    return conformer_state_dict(seed, model)


def ebranchformer_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 256, cgmlp_linear_units: int = 256,
                       enc_blocks: int = 2, dec_blocks: int = 2, cgmlp_kernel: int = 31, merge_kernel: int = 31, use_ffn: bool = True,
                       macaron: bool = True, rel_pos_type: str = "latest", vocab: int = 40, input_size: int = 80,
                       dec_linear_units: int = None, attention_dropout_rate: float = 0.1) -> dict:
    """constructor arguments of an E-Branchformer model (the layout of funasr/models/e_branchformer/template.yaml) at a chosen size"""
    enc = {"output_size": output_size, "attention_heads": attention_heads, "attention_layer_type": "rel_selfattn",
           "pos_enc_layer_type": "rel_pos", "rel_pos_type": rel_pos_type, "cgmlp_linear_units": cgmlp_linear_units,
           "cgmlp_conv_kernel": cgmlp_kernel, "use_linear_after_conv": False, "gate_activation": "identity", "num_blocks": enc_blocks,
           "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": attention_dropout_rate, "input_layer": "conv2d",
           "layer_drop_rate": 0.0, "linear_units": linear_units, "positionwise_layer_type": "linear", "use_ffn": use_ffn,
           "macaron_ffn": macaron, "merge_conv_kernel": merge_kernel}
    dec = {"attention_heads": attention_heads, "linear_units": dec_linear_units or linear_units, "num_blocks": dec_blocks, "dropout_rate": 0.1,
           "positional_dropout_rate": 0.1, "self_attention_dropout_rate": 0.0, "src_attention_dropout_rate": 0.0}
    return {"encoder": "EBranchformerEncoder", "encoder_conf": enc, "decoder": "TransformerDecoder", "decoder_conf": dec,
            "ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False, "input_size": input_size, "vocab_size": vocab}


# funasr/models/e_branchformer/template.yaml (the ESPnet AISHELL recipe)
EBRANCHFORMER_TEMPLATE = dict(output_size=256, attention_heads=4, linear_units=1024, cgmlp_linear_units=1024, enc_blocks=12, dec_blocks=6,
                              cgmlp_kernel=31, merge_kernel=31, use_ffn=True, macaron=True, rel_pos_type="latest", vocab=4234,
                              dec_linear_units=2048)


def ebranchformer_state_dict(seed: int, model) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (an EBranchformer module or the reference's), drawn as conformer_state_dict draws
    them (the two depthwise convs fan-in scaled with a bias of order 0.1: neither near the identity nor negligible beside it)"""
    return conformer_state_dict(seed, model)


def eparaformer_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 256, enc_blocks: int = 2, dec_blocks: int = 2,
                     kernel: int = 15, l_order: int = 1, r_order: int = 1, sigma_heads: int = 4, vocab: int = 40, input_size: int = 80,
                     ctc_weight: float = 0.0) -> dict:
    """constructor arguments of an E-Paraformer model (the layout of examples/aishell/e_paraformer/conf/
    e_paraformer_conformer_12e_6d_2048_256.yaml) at a chosen size"""
    c = conformer_conf(output_size=output_size, attention_heads=attention_heads, linear_units=linear_units, enc_blocks=enc_blocks,
                       dec_blocks=dec_blocks, kernel=kernel, macaron=True, vocab=vocab, input_size=input_size)
    pred = {"idim": output_size, "threshold": 1.0, "l_order": l_order, "r_order": r_order, "sigma": 0.5, "bias": 0.0, "sigma_heads": sigma_heads}
    return {"encoder": "ConformerEncoder", "encoder_conf": c["encoder_conf"], "decoder": "ParaformerSANDecoder", "decoder_conf": c["decoder_conf"],
            "predictor": "PifPredictor", "predictor_conf": pred, "ctc_weight": ctc_weight, "lsm_weight": 0.1, "length_normalized_loss": False,
            "predictor_weight": 1.0, "predictor_bias": 2, "sampling_ratio": 0.4, "use_1st_decoder_loss": True, "input_size": input_size,
            "vocab_size": vocab}


# examples/aishell/e_paraformer/conf/e_paraformer_conformer_12e_6d_2048_256.yaml
EPARAFORMER_TEMPLATE = dict(output_size=256, attention_heads=4, linear_units=2048, enc_blocks=12, dec_blocks=6, kernel=15, l_order=1, r_order=1,
                            sigma_heads=4, vocab=4234)


def eparaformer_state_dict(seed: int, model, cif_bias: float = -1.0) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (an EParaformer module or the reference's), drawn as conformer_state_dict draws them,
    then the predictor's own: a DISTINCT sigma per head (0.6 .. 1.8: the heads must not be interchangeable), a small distinct bias per
    head (it cancels in the softmax; a result that moved with it would show), and a negative `cif_output.bias` so that the alphas sum
    to a fraction of the frame count (about a token per four frames). The decoder's attention output projections are drawn at 0.3 of
    the fan-in scale: untrained attention is near uniform, its output the same at every token position, and at full scale that common
    part drowns what tells the positions apart"""
    sd = conformer_state_dict(seed, model)
    for k in sd:
        if k.startswith("decoder.decoders.") and "_attn.linear_out." in k:
            sd[k] = sd[k] * 0.3
    H = sd["predictor.sigma"].numel()
    sd["predictor.sigma"] = torch.linspace(0.6, 1.8, H) if H > 1 else torch.tensor([0.9])
    sd["predictor.bias"] = 0.25 * torch.arange(H, dtype=torch.float32) - 0.3
    sd["predictor.cif_output.bias"] = torch.full_like(sd["predictor.cif_output.bias"], cif_bias)
    return sd


def lcbnet_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 256, enc_blocks: int = 2, dec_blocks: int = 2,
                text_blocks: int = 2, vocab: int = 300, input_size: int = 80) -> dict:
    """constructor arguments of an LCBNet model at a chosen size: transformer_conf plus the text encoder, the one fusion layer and the
    bias predictor (funasr/models/lcbnet/model.py; every width is the audio encoder's). The default ids of a decode without text
    need a vocabulary of at least 296 tokens."""
    c = transformer_conf(output_size, attention_heads, linear_units, enc_blocks, dec_blocks, vocab, input_size)
    c.update({
        "text_encoder": "TransformerTextEncoder",
        "text_encoder_conf": {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units,
                              "num_blocks": text_blocks, "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.0},
        "fusion_encoder": "FusionSANEncoder",
        "fusion_encoder_conf": {"size": output_size, "attention_heads": attention_heads, "attention_dim": output_size,
                                "linear_units": linear_units, "self_attention_dropout_rate": 0.0, "src_attention_dropout_rate": 0.0,
                                "positional_dropout_rate": 0.1, "dropout_rate": 0.1},
        "bias_predictor": "ConvBiasPredictor",
        "bias_predictor_conf": {"size": output_size, "l_order": 3, "r_order": 3, "attention_heads": attention_heads,
                                "attention_dropout_rate": 0.1, "linear_units": linear_units},
        "select_num": 2, "select_length": 3, "insert_blank": True})
    return c


LCBNET_ZOO_LIKE = dict(output_size=256, attention_heads=4, linear_units=2048, enc_blocks=12, dec_blocks=6, text_blocks=6, vocab=5000)


def lcbnet_state_dict(seed: int, model, ctc_gain: float = 0.5, blank_bias: float = 18.0, eos_bias: float = 12.0,
                      fusion_gain: float = 1.5) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (an LCBNet module or the reference's), drawn like sanm_state_dict in the sorted order
    of the keys, then made "trained-like" in the three places where plain random weights leave the joint search of a 300-token
    vocabulary without a usable answer (no hypothesis ever ends on its own, every hypothesis runs to the frame count, and the CTC
    prefix scores of such hypotheses are the infeasible -1e10):
      * the CTC head is confident and mostly blank: its logits x `ctc_gain`, the blank's bias + `blank_bias`, as after training;
      * the decoder keeps `eos` (= vocab - 1) among its candidates: the output layer's bias of that row + `eos_bias`, so that a
        hypothesis can end where the CTC prefix score says the sequence is complete;
      * the text matters: the output projection of the fusion layer's cross-attention x `fusion_gain`."""
    sd = sanm_state_dict(seed, model)
    V = sd["ctc.ctc_lo.weight"].shape[0]
    sd["ctc.ctc_lo.weight"] = sd["ctc.ctc_lo.weight"] * ctc_gain
    sd["ctc.ctc_lo.bias"][0] += blank_bias
    sd["decoder.output_layer.bias"][V - 1] += eos_bias
    sd["fusion_encoder.src_attn.linear_out.weight"] = sd["fusion_encoder.src_attn.linear_out.weight"] * fusion_gain
    return sd


def sanm_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 64, enc_blocks: int = 2, dec_blocks: int = 3,
              att_layer_num: int = 2, kernel: int = 11, sanm_shfit="default", enc_kernel: int = 11, ctc_weight: float = 0.3, vocab: int = 60,
              input_size: int = 80) -> dict:
    """constructor arguments of a SANM model (the layout of funasr/models/sanm/template.yaml) at a chosen size. sanm_shfit "default"
    leaves the decoder's key out: the constructor's (kernel - 1) // 2, the causal memory for an odd kernel"""
    enc = {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": enc_blocks,
           "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.1, "input_layer": "pe",
           "pos_enc_class": "SinusoidalPositionEncoder", "normalize_before": True, "kernel_size": enc_kernel, "sanm_shfit": 0,
           "selfattention_layer_type": "sanm"}
    dec = {"attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": dec_blocks, "dropout_rate": 0.1,
           "positional_dropout_rate": 0.1, "self_attention_dropout_rate": 0.1, "src_attention_dropout_rate": 0.1,
           "att_layer_num": att_layer_num, "kernel_size": kernel}
    if sanm_shfit != "default":
        dec["sanm_shfit"] = sanm_shfit
    return {"encoder": "SANMEncoder", "encoder_conf": enc, "decoder": "FsmnDecoder", "decoder_conf": dec, "ctc_weight": ctc_weight,
            "lsm_weight": 0.1, "length_normalized_loss": True, "input_size": input_size, "vocab_size": vocab}


# funasr/models/sanm/template.yaml: D 512, 4 heads (d_k 128), FFN 2048, 50 encoder and 16 decoder blocks (all with cross-attention),
# kernel 11 with sanm_shfit 0 (five zero columns between the first token and the second), no CTC head; 7 x 80 LFR features
SANM_TEMPLATE = dict(output_size=512, attention_heads=4, linear_units=2048, enc_blocks=50, dec_blocks=16, att_layer_num=16, kernel=11,
                     sanm_shfit=0, ctc_weight=0.0, vocab=8404, input_size=560)


def sanm_state_dict(seed: int, model) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (a SANM module or the reference's): the tensors of conformer_state_dict (the FSMN
    taps [D, 1, K] fan-in scaled like every other convolution), drawn in the SORTED order of the keys -- this package's modules and
    the reference's list the same keys in different orders"""
    g = torch.Generator().manual_seed(seed)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    return {k: _synthetic_tensor(k, shapes[k], g) for k in sorted(shapes)}


def uniasr_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 64, enc_blocks: int = 2, enc2_blocks: int = 1,
                dec_blocks: int = 2, att_layer_num: int = 2, att_layer_num2: int = 1, kernel: int = 11, chunk_size=(4, 6), stride=(2, 4),
                pad_left=(1, 2), encoder_att_look_back_factor=(0, 1), decoder_att_look_back_factor=(1, 2), conv_kernel: int = 2,
                conv_stride: int = 2, conv_pad=(0, 1), vocab: int = 30, input_size: int = 80) -> dict:
    """constructor arguments of a UniASR model (the layout of the model zoo's 2-pass config.yaml files) at a chosen size: both
    encoders SANMEncoderChunkOpt with the same chunk geometries, both decoders FsmnDecoderSCAMAOpt -- the first with sanm_shfit 0 as
    the zoo has it and cross-attention in `att_layer_num` layers, the second with the constructor's default shift and
    `att_layer_num2` -- both predictors CifPredictorV2 without a tail"""
    def enc(blocks):
        return {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": blocks,
                "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.1, "input_layer": "pe",
                "pos_enc_class": "SinusoidalPositionEncoder", "normalize_before": True, "kernel_size": 11, "sanm_shfit": 0,
                "selfattention_layer_type": "sanm", "chunk_size": list(chunk_size), "stride": list(stride), "pad_left": list(pad_left),
                "encoder_att_look_back_factor": list(encoder_att_look_back_factor),
                "decoder_att_look_back_factor": list(decoder_att_look_back_factor)}

    def dec(att, **extra):
        return dict({"attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": dec_blocks, "dropout_rate": 0.1,
                     "positional_dropout_rate": 0.1, "self_attention_dropout_rate": 0.1, "src_attention_dropout_rate": 0.1,
                     "att_layer_num": att, "kernel_size": kernel}, **extra)

    pred = {"idim": output_size, "threshold": 1.0, "l_order": 1, "r_order": 1}
    return {"encoder": "SANMEncoderChunkOpt", "encoder_conf": enc(enc_blocks), "encoder2": "SANMEncoderChunkOpt",
            "encoder2_conf": enc(enc2_blocks), "decoder": "FsmnDecoderSCAMAOpt", "decoder_conf": dec(att_layer_num, sanm_shfit=0),
            "decoder2": "FsmnDecoderSCAMAOpt", "decoder2_conf": dec(att_layer_num2), "predictor": "CifPredictorV2",
            "predictor_conf": dict(pred), "predictor2": "CifPredictorV2", "predictor2_conf": dict(pred),
            "stride_conv": "stride_conv1d", "stride_conv_conf": {"kernel_size": conv_kernel, "stride": conv_stride, "pad": list(conv_pad)},
            "ctc_weight": 0.0, "ctc2_weight": 0.0, "lsm_weight": 0.1, "length_normalized_loss": True, "input_size": input_size,
            "vocab_size": vocab}


def uniasr_state_dict(seed: int, model) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (a UniASR module or the reference's), drawn like sanm_state_dict in the sorted order
    of the keys. The alpha heads' biases are set to 0.5 so that a frame weighs about 0.6: the predictor's mask keeps `stride` frames
    of a chunk, and a clip of a few dozen frames should still fire a handful of tokens"""
    sd = sanm_state_dict(seed, model)
    for k in sd:
        if k.endswith("cif_output.bias"):
            sd[k] = torch.full_like(sd[k], 0.5)
    return sd


def aligner_conf(output_size: int = 320, attention_heads: int = 4, linear_units: int = 1280, num_blocks: int = 30, idim: int = None,
                 upsample_type: str = "cnn_blstm", use_cif1_cnn: bool = False, input_size: int = 560) -> dict:
    """constructor arguments of a MonotonicAligner (the layout of funasr/models/monotonic_aligner/template.yaml, which the
    defaults are: D 320, 4 heads of d_k 80, FFN 1280, 30 blocks, the BLSTM timestamp head on the raw encoder output)"""
    enc = {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": num_blocks,
           "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.1, "input_layer": "pe",
           "pos_enc_class": "SinusoidalPositionEncoder", "normalize_before": True, "kernel_size": 11, "sanm_shfit": 0,
           "selfattention_layer_type": "sanm"}
    pred = {"idim": output_size if idim is None else idim, "threshold": 1.0, "l_order": 1, "r_order": 1, "tail_threshold": 0.45,
            "smooth_factor2": 0.25, "noise_threshold2": 0.01, "upsample_times": 3, "use_cif1_cnn": use_cif1_cnn,
            "upsample_type": upsample_type}
    return {"encoder": "SANMEncoder", "encoder_conf": enc, "predictor": "CifPredictorV3", "predictor_conf": pred,
            "length_normalized_loss": False, "predictor_bias": 1, "input_size": input_size}


def aligner_state_dict(seed: int, model) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (a MonotonicAligner module or the reference's), drawn like sanm_state_dict in the
    sorted order of the keys. The second alpha head's weight is drawn 4x wider than fan-in scaling and its bias set to -0.5, so that
    the upsampled weights vary from frame to frame and the scaled integral crosses its threshold well inside a frame"""
    g = torch.Generator().manual_seed(seed)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = {k: _synthetic_tensor(k, shapes[k], g) for k in sorted(shapes)}
    sd["predictor.cif_output2.weight"] = sd["predictor.cif_output2.weight"] * 4.0
    sd["predictor.cif_output2.bias"] = torch.full(shapes["predictor.cif_output2.bias"], -0.5)
    return sd


def _synthetic_tensor(k: str, shp: tuple, g: torch.Generator) -> torch.Tensor:
    """one tensor of conformer_state_dict, by the name and shape of its key"""
    if k.endswith("num_batches_tracked"):
        return torch.tensor(0, dtype=torch.long)
    if k.endswith("running_mean"):
        return 0.2 * torch.randn(shp, generator=g)
    if k.endswith("running_var"):
        return 0.5 + 1.5 * torch.rand(shp, generator=g)
    if k.endswith("pos_bias_u") or k.endswith("pos_bias_v"):
        return 0.1 * torch.randn(shp, generator=g)
    if k.endswith("embed.0.weight") and len(shp) == 2:
        return torch.randn(shp, generator=g) * (1.0 / shp[1]) ** 0.5
    if k.endswith("ctc_lo.weight") or k.endswith("output_layer.weight"):      # logits of order 4: few near-ties between classes
        return torch.randn(shp, generator=g) * 4.0 * (1.0 / shp[1]) ** 0.5
    if len(shp) == 1:
        is_norm = "norm" in k
        return (1.0 + 0.2 * torch.randn(shp, generator=g)) if (is_norm and k.endswith("weight")) else 0.1 * torch.randn(shp, generator=g)
    fan_in = 1
    for d in shp[1:]:
        fan_in *= d
    return torch.randn(shp, generator=g) * (1.0 / fan_in) ** 0.5


def conformer_state_dict(seed: int, model) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (a Conformer module or the reference's): fan-in scaled convs / linears, LayerNorms
    near identity, NON-trivial BatchNorm statistics (weight near 1, bias / running_mean off zero, running_var in [0.5, 2]),
    relative-position biases of order 0.1, a token embedding of order 1 / sqrt(D); drawn in the order of the module's state dict"""
    g = torch.Generator().manual_seed(seed)
    return {k: _synthetic_tensor(k, tuple(v.shape), g) for k, v in model.state_dict().items()}


def transducer_conf(encoder: str = "ConformerEncoder", output_size: int = 128, attention_heads: int = 2, linear_units: int = 256,
                    enc_blocks: int = 2, embed_size: int = 48, hidden_size: int = 64, num_layers: int = 2, joint_space_size: int = 96,
                    vocab: int = 61, input_size: int = 80) -> dict:
    """constructor arguments of a Transducer model (the layout of funasr/models/rwkv_bat/template.yaml's prediction and joint
    networks over one of the built encoders) at a chosen size. For RWKVEncoder `linear_units` is its linear_size and
    `attention_heads` is unused; the template's time_reduction_factor 2 is kept. ChunkConformerEncoder gets chunk_conformer_conf's
    dynamic mode"""
    if encoder == "RWKVEncoder":
        enc = rwkv_encoder_conf(output_size=output_size, linear_size=linear_units, num_blocks=enc_blocks)
    elif encoder == "ChunkConformerEncoder":
        enc = chunk_conformer_conf(output_size=output_size, attention_heads=attention_heads, linear_units=linear_units, num_blocks=enc_blocks)
    else:
        enc = (conformer_conf if encoder == "ConformerEncoder" else transformer_conf)(
            output_size=output_size, attention_heads=attention_heads, linear_units=linear_units, enc_blocks=enc_blocks)["encoder_conf"]
    return {"encoder": encoder, "encoder_conf": enc, "decoder": "rnnt_decoder",
            "decoder_conf": {"embed_size": embed_size, "hidden_size": hidden_size, "num_layers": num_layers, "embed_dropout_rate": 0.1,
                             "dropout_rate": 0.1, "use_embed_mask": False},
            "joint_network": "joint_network", "joint_network_conf": {"joint_space_size": joint_space_size},
            "auxiliary_ctc_weight": 0.0, "input_size": input_size, "vocab_size": vocab}


TRANSDUCER_TEMPLATE = dict(embed_size=512, hidden_size=512, num_layers=1, joint_space_size=512, vocab=4234)

# funasr/models/rwkv_bat/template.yaml: D 512, 18 blocks, every second frame kept; linear_size and context_size are the constructor's
# defaults (4 D, 1024)
RWKV_TEMPLATE = dict(output_size=512, num_blocks=18, time_reduction_factor=2)


def rwkv_encoder_conf(output_size: int = 64, linear_size: int = 160, num_blocks: int = 3, time_reduction_factor: int = 2,
                      context_size: int = None) -> dict:
    """the encoder_conf of an RWKVEncoder in the layout of funasr/models/rwkv_bat/template.yaml at a chosen size (linear_size None:
    the constructor's 4 x output_size)"""
    conf = {"kernel": 3, "subsampling_factor": 4, "output_size": output_size, "num_blocks": num_blocks,
            "time_reduction_factor": time_reduction_factor, "att_dropout_rate": 0.1, "ffn_dropout_rate": 0.1, "dropout_rate": 0.1}
    if linear_size is not None:
        conf["linear_size"] = linear_size
    if context_size is not None:
        conf["context_size"] = context_size
    return conf


def chunk_conformer_conf(output_size: int = 64, attention_heads: int = 1, linear_units: int = 128, num_blocks: int = 2,
                         cnn_module_kernel: int = 15, subsampling_factor: int = 4, time_reduction_factor: int = 2, mode: str = "dynamic",
                         default_chunk_size: int = 4, left_chunk_size: int = 1, **more) -> dict:
    """the encoder_conf of a ChunkConformerEncoder (funasr/models/conformer/encoder.py:914) at a chosen size, in one of its three
    forward modes: "full" (neither flag), "dynamic" (dynamic_chunk_training) or "unified" (unified_model_training). Its synthetic
    weights are drawn by conformer_state_dict's rule."""
    if mode not in ("full", "dynamic", "unified"):
        raise ValueError(f"chunk_conformer_conf: mode {mode!r} (full, dynamic or unified)")
    conf = {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": num_blocks,
            "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.1, "embed_vgg_like": False,
            "normalize_before": True, "activation_type": "swish", "cnn_module_kernel": cnn_module_kernel,
            "subsampling_factor": subsampling_factor, "time_reduction_factor": time_reduction_factor,
            "dynamic_chunk_training": mode == "dynamic", "unified_model_training": mode == "unified",
            "default_chunk_size": default_chunk_size, "left_chunk_size": left_chunk_size, "jitter_range": 2}
    conf.update(more)
    return conf


def rwkv_encoder_state_dict(seed: int, model, prefix: str = "") -> Dict[str, torch.Tensor]:
    """synthetic weights of the RWKVEncoder `model` (this package's or the reference's) under `prefix`, drawn in the sorted order of the
    keys: He-scaled convs (six ReLUs in a row keep their scale), LayerNorms near identity, time_decay uniform over [-5, 3] (the span of
    the reference's initialisation: w = -exp(.) from -0.007 to -20), time_first of order 0.5, token-shift mixes uniform over [0, 1],
    fan-in scaled linears with the time mix's proj_key three times wider, so that |k| reaches about 12 and stays within a few tens"""
    g = torch.Generator().manual_seed(seed)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = {}
    for k in sorted(shapes):
        shp = shapes[k]
        if k.endswith("time_decay"):
            t = -5.0 + 8.0 * torch.rand(shp, generator=g)
        elif k.endswith("time_first"):
            t = 0.5 * torch.randn(shp, generator=g)
        elif "time_mix_" in k:
            t = torch.rand(shp, generator=g)
        elif len(shp) == 1:
            t = (1.0 + 0.2 * torch.randn(shp, generator=g)) if ("norm" in k and k.endswith("weight")) else 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            gain = 2.0 ** 0.5 if len(shp) == 4 else (3.0 if k.endswith("att.proj_key.weight") else 1.0)
            t = torch.randn(shp, generator=g) * gain * (1.0 / fan_in) ** 0.5
        sd[prefix + k] = t
    return sd


def transducer_state_dict(seed: int, model, n_planted: int = 10, threshold: float = 0.7) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (a Transducer module or the reference's). The encoder is drawn as
    conformer_state_dict draws it. Plain random search networks do not make a search that SETTLES (an output layer that rarely
    prefers blank expands without end), so the tokens are planted over a random background:
      * background: an embedding of order 1, LSTMs with a strong input and a weak recurrent part, small `lin_enc` / `lin_dec`, an
        output layer with logit noise of order 1 over a STAIRCASE of biases: blank at +3, the unplanted labels in a random order at
        -2, -5, -8, ... (3 apart, level at -26 from rank 8 on). Blank takes ~ 99 %, and neither the rank k / k + 1 boundary of the
        label scores nor two copies of one hypothesis made at different frames come close to a tie;
      * planted label i < n_planted owns joint dimension i, embedding dimension i and hidden unit i of every LSTM layer.
        `lin_enc` row i is a random direction of gain 3 with bias -3 threshold: tanh is ~ +1 on the few frames whose projection
        exceeds `threshold` sigma by ~ 0.6 and ~ -1 elsewhere; `lin_out` maps +1 to a logit of blank + 5 and -1 to -28 (magnitudes stay small: float32 resolves a log-probability of 30 to 2e-6);
      * hidden unit i passes "the LAST label is label i" up the stack (input and output gates open, forget gate shut, the cell input
        reads dimension i only): ~ 0.74 then, ~ 0 otherwise, whatever came before. `lin_dec` row i turns it into -12, so a label is
        not emitted twice in a row and the frame falls back to blank."""
    sd = conformer_state_dict(seed, model)
    if "encoder.rwkv_blocks.0.att.time_decay" in sd:                 # an RWKV encoder has its own drawing rule
        sd.update(rwkv_encoder_state_dict(seed, model.encoder, prefix="encoder."))
    g = torch.Generator().manual_seed(seed + 7919)
    gains = {"weight_ih_l0": 2.0, "weight_hh_l0": 0.5, "joint_network.lin_enc.weight": 0.5, "joint_network.lin_dec.weight": 0.5,
             "joint_network.lin_out.weight": 1.5}
    for k, v in model.state_dict().items():
        if not (k.startswith("decoder.") or k.startswith("joint_network.")):
            continue
        shp = tuple(v.shape)
        if k == "decoder.embed.weight":
            sd[k] = torch.randn(shp, generator=g)
        elif len(shp) == 1:
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        else:
            gain = [x for n, x in gains.items() if k.endswith(n)][0]
            sd[k] = torch.randn(shp, generator=g) * gain * (1.0 / shp[1]) ** 0.5
    V, J = sd["joint_network.lin_out.weight"].shape
    D = sd["joint_network.lin_enc.weight"].shape[1]
    E = sd["decoder.embed.weight"].shape[1]
    H = sd["decoder.rnn.0.weight_hh_l0"].shape[1]
    P = min(n_planted, V - 3, J // 2 - 1, E // 2, H // 2)
    blank, off = 4.0, -19.0
    labels = (3 + torch.randperm(V - 3, generator=g)[:P]).tolist()
    others = [v for v in range(1, V) if v not in set(labels)]
    rank = torch.randperm(len(others), generator=g).tolist()
    sd["joint_network.lin_out.bias"][0] += blank
    for v, r in zip(others, rank):
        sd["joint_network.lin_out.bias"][v] += -2.0 - 2.4 * min(r, 5) - (5.0 if r > 5 else 0.0)
    # joint dimension P: a frame-dependent level shared by all unplanted labels (two copies of a hypothesis made at different frames
    # then differ by units, not by the noise alone); it moves no rank among them
    sd["joint_network.lin_enc.weight"][P] = 1.5 * torch.randn(D, generator=g) * (1.0 / D) ** 0.5
    sd["joint_network.lin_enc.bias"][P] = 0.0
    sd["joint_network.lin_dec.weight"][P] = 0.0
    sd["joint_network.lin_out.weight"][:, P] = 0.0
    sd["joint_network.lin_out.weight"][others, P] = 3.0
    sd["decoder.embed.weight"][:, :P] = 0.0
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("decoder.rnn."))
    for i, v in enumerate(labels):
        sd["decoder.embed.weight"][v, i] = 3.0
        for l in range(layers):
            p = f"decoder.rnn.{l}."
            for gate, bias in enumerate((4.0, -4.0, 0.0, 4.0)):                             # i, f, g, o
                row = gate * H + i
                sd[p + "weight_ih_l0"][row] = 0.0
                sd[p + "weight_hh_l0"][row] = 0.0
                sd[p + "bias_ih_l0"][row] = bias
                sd[p + "bias_hh_l0"][row] = 0.0
            sd[p + "weight_ih_l0"][2 * H + i, i] = 4.0
        sd["joint_network.lin_enc.weight"][i] = 3.0 * torch.randn(D, generator=g) * (1.0 / D) ** 0.5
        sd["joint_network.lin_enc.bias"][i] = -3.0 * threshold
        sd["joint_network.lin_dec.weight"][i] = 0.0
        sd["joint_network.lin_dec.weight"][i, i] = -12.0 / 0.74
        sd["joint_network.lin_out.weight"][:, i] = 0.0
        sd["joint_network.lin_out.weight"][v, i] = (blank + 5.0 - off) / 2
        sd["joint_network.lin_out.bias"][v] += (blank + 5.0 + off) / 2
    return sd


def kws_fsmn_conf(input_dim: int = 40, input_affine_dim: int = 24, fsmn_layers: int = 2, linear_dim: int = 32, proj_dim: int = 16,
                  lorder: int = 4, rorder: int = 2, lstride: int = 1, rstride: int = 1, output_affine_dim: int = 24, vocab: int = 67) -> dict:
    """constructor arguments of an FsmnKWS model (the layout of examples/industrial_data_pretraining/fsmn_kws/conf/*.yaml) at a
    chosen size"""
    enc = {"input_dim": input_dim, "input_affine_dim": input_affine_dim, "fsmn_layers": fsmn_layers, "linear_dim": linear_dim,
           "proj_dim": proj_dim, "lorder": lorder, "rorder": rorder, "lstride": lstride, "rstride": rstride,
           "output_affine_dim": output_affine_dim, "output_dim": vocab, "use_softmax": False}
    return {"encoder": "FSMN", "encoder_conf": enc, "ctc_conf": {"dropout_rate": 0.0, "ctc_type": "builtin", "reduce": True,
                                                                 "ignore_nan_grad": True, "extra_linear": False},
            "ctc_weight": 1.0, "input_size": input_dim, "vocab_size": vocab}


KWS_FSMN_RECIPE = dict(input_dim=400, input_affine_dim=140, fsmn_layers=4, linear_dim=250, proj_dim=128, lorder=10, rorder=2,
                       output_affine_dim=140, vocab=2599)                       # fsmn_4e_l10r2_250_128_fdim80_t2599


def kws_sanm_conf(output_size: int = 128, attention_heads: int = 2, linear_units: int = 64, num_blocks: int = 2, vocab: int = 67,
                  input_size: int = 40) -> dict:
    """constructor arguments of a SanmKWS model (examples/industrial_data_pretraining/sanm_kws/conf/*.yaml) at a chosen size"""
    enc = {"output_size": output_size, "attention_heads": attention_heads, "linear_units": linear_units, "num_blocks": num_blocks,
           "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "attention_dropout_rate": 0.1, "input_layer": "pe",
           "pos_enc_class": "SinusoidalPositionEncoder", "normalize_before": True, "kernel_size": 11, "sanm_shfit": 0,
           "selfattention_layer_type": "sanm"}
    return {"encoder": "SANMEncoder", "encoder_conf": enc, "ctc_conf": {"dropout_rate": 0.0, "ctc_type": "builtin", "reduce": True},
            "ctc_weight": 1.0, "input_size": input_size, "vocab_size": vocab}


KWS_SANM_RECIPE = dict(output_size=256, attention_heads=4, linear_units=320, num_blocks=6, vocab=2602, input_size=280)  # sanm_6e_320_256_fdim40_t2602


def kws_state_dict(seed: int, model, planted=(), gain: float = 6.0, blank: float = 2.0, floor: float = -3.0) -> Dict[str, torch.Tensor]:
    """synthetic weights in the layout of `model` (an FsmnKWS / SanmKWS module or the reference's). Everything but the output
    layer is drawn by conformer_state_dict's rules (fan-in scaled matrices, LayerNorm weights near 1, other vectors of order 0.1), key
    by key in NAME order. Plain random weights give a near-uniform posterior that never crosses the
    search's 0.05 (a probe at 67 tokens: 0.02 at most), so the output layer -- `encoder.out_linear2.linear` where the model has no
    `ctc_lo`, `ctc.ctc_lo` otherwise -- is planted over a quiet background:
      * every row is a random direction with logit noise of order 1; the bias of blank is `blank`, of every other unplanted
        token `floor`: blank holds most of the mass on most frames;
      * the rows of the `planted` token ids have `gain` times the background's scale and bias 0: each of them overtakes blank on
        the few frames whose hidden vector points its way, and two of them now and then share a frame."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in sorted(model.state_dict().items()):            # by NAME: the reference's modules register their parameters in another order
        shp = tuple(v.shape)
        if len(shp) == 1:
            sd[k] = (1.0 + 0.2 * torch.randn(shp, generator=g)) if ("norm" in k and k.endswith("weight")) else 0.1 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            sd[k] = torch.randn(shp, generator=g) * (1.0 / fan_in) ** 0.5
    g = torch.Generator().manual_seed(seed + 104729)
    wkey = [k for k in sd if k.endswith("ctc_lo.weight")] or [k for k in sd if k.endswith("out_linear2.linear.weight")]
    wkey = wkey[0]
    bkey = wkey[: -len("weight")] + "bias"
    V, K = sd[wkey].shape
    sd[wkey] = torch.randn(V, K, generator=g) * (1.0 / K) ** 0.5
    sd[bkey] = torch.full((V,), float(floor)) + 0.1 * torch.randn(V, generator=g)
    sd[bkey][0] = float(blank)
    for v in planted:
        sd[wkey][int(v)] *= float(gain)
        sd[bkey][int(v)] = 0.0
    return sd
