"""Restatement of the reference's UniASR inference (funasr/models/uniasr/model.py over scama/chunk_utilis.py, scama/encoder.py,
scama/decoder.py, paraformer/cif_predictor.py, transformer/utils/subsampling.py) in plain torch, dtype-generic (float64 for the bars,
float32 for the gap), one sequence at a time. Written from the formulas, with the masks as DENSE tensors the way the reference holds
them (the package works from the chunk geometry instead, so the two are independent statements of the same masks):
    chunk layout    chunk c = `shift` zero rows + `chunk` rows holding the frames c stride - pad_left ...; split = add_mask @ pad(x),
                    remove = rm_mask @ x_chunk; everything cut to Tc = (n - 1)(chunk + shift) + shift + pad_left + T - (n - 1) stride rows
    encoder         x sqrt(D) + PE(frame index) BEFORE the split; per block x = [x +] att(LN1 x) ; x = x + FFN(LN2 x); after_norm
    att             softmax over the keys of mask_att (all-masked rows: zero context) . V -> linear_out, + FSMN memory of the V
                    projection: m (conv(m v) + m v) with m = mask_shift
    stride_conv     relu(conv1d(pad([features | remove(pass 1)]))) cut to (T - 1) // stride + 1 rows
    predictor       alphas = relu(sigmoid(cif_output(relu(conv(x mask_shift)))) smooth - noise) mask_predictor; tokens = sum
    decoder step    tests/_sanm_oracle.FsmnStepper with the position's mask row in every `decoders` cross-attention
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as Fn

from funasr_amd.transformer_search import BeamSearchTransformer

from . import _sanm_oracle as S
from ._conformer_oracle import _lin, _ln, cast, to_np  # noqa: F401


# ------------------------------------------------------------------------------------------------ chunk layout
def geometry(T: int, chunk: int, stride: int, pad_left: int, shift: int, look_back: int) -> dict:
    """the dense masks of overlap_chunk.gen_chunk_mask for one sequence, built chunk by chunk and cut like the reference's"""
    n = math.ceil(T / stride)
    P = chunk + shift
    Tc = (n - 1) * P + shift + pad_left + T - (n - 1) * stride
    W = max(chunk, T + pad_left)
    add = np.zeros((n * P, W + chunk + n * stride), np.float32)
    rm = np.zeros((W + n * stride + stride, n * P), np.float32)
    m_shift, m_pred, att = np.zeros(n * P, np.float32), np.zeros(n * P, np.float32), np.zeros((n * P, n * P), np.float32)
    for c in range(n):
        r0 = c * P + shift
        for i in range(chunk):
            if c * stride + i < W:
                add[r0 + i, c * stride + i] = 1.0
        for k in range(stride):
            rm[c * stride + k, r0 + pad_left + k] = 1.0
        m_shift[r0: r0 + chunk] = 1.0
        m_pred[r0 + pad_left: r0 + pad_left + stride] = 1.0
        att[r0: r0 + chunk, r0: r0 + chunk] = 1.0
        for cb in range(max(c - look_back, 0), c):
            att[r0: r0 + stride, cb * P + shift: cb * P + shift + stride] = 1.0
    return dict(T=T, Tc=Tc, P=P, chunk=chunk, stride=stride, pad_left=pad_left, shift=shift, look_back=look_back,
                add=add[:Tc, : T + pad_left], rm=rm[:T, :Tc], mask_shift=m_shift[:Tc], mask_predictor=m_pred[:Tc], mask_att=att[:Tc, :Tc])


def geometry_of(enc_conf: dict, T: int, ind: int) -> dict:
    n = len(enc_conf["chunk_size"])
    pick = lambda key: (list(enc_conf[key]) if len(enc_conf[key]) >= n else [enc_conf[key][0]] * n)[ind]    # noqa: E731
    return geometry(T, enc_conf["chunk_size"][ind], enc_conf["stride"][ind], pick("pad_left"), (enc_conf.get("kernel_size", 11) - 1) // 2,
                    pick("encoder_att_look_back_factor"))


def index_maps(geo: dict):
    """(add_index [Tc], rm_index [T]) of the dense masks: every row holds at most one 1"""
    add, rm = geo["add"], geo["rm"]
    assert add.sum(1).max() <= 1 and (rm.sum(1) == 1).all()
    src = add.argmax(1) - geo["pad_left"]                            # (a row that picks one of the pad_left zero rows is a zero row)
    return np.where((add.sum(1) > 0) & (src >= 0), src, -1).astype(np.int32), rm.argmax(1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ encoder
def position_table(T: int, depth: int, dtype):
    pos = torch.arange(1, T + 1, dtype=dtype)[:, None]
    inc = math.log(10000.0) / (depth / 2 - 1)
    inv = torch.exp(torch.arange(depth // 2, dtype=dtype) * (-inc))
    return torch.cat([torch.sin(pos * inv), torch.cos(pos * inv)], 1)


def masked_attention(q, k, v, H: int, mask):
    """q, k, v [T, D], mask [Tq, Tk] 0 / 1 -> [Tq, D]; a row without a visible key gives zeros"""
    T, D = q.shape
    dk = D // H
    s = torch.einsum("qhd,khd->hqk", q.view(T, H, dk), k.view(-1, H, dk)) / math.sqrt(dk)
    dead = (mask == 0)[None]
    p = torch.softmax(s.masked_fill(dead, -float("inf")), dim=-1)
    p = torch.nan_to_num(p, nan=0.0).masked_fill(dead, 0.0)
    return torch.einsum("hqk,khd->qhd", p, v.view(-1, H, dk)).reshape(T, D)


def fsmn_memory(v, taps, m, left: int):
    """v [T, D], taps [D, 1, K], m [T] 0 / 1"""
    K = taps.shape[-1]
    vm = v * m[:, None]
    conv = Fn.conv1d(Fn.pad(vm.t()[None], (left, K - 1 - left)), taps, groups=v.shape[1])[0].t()
    return (conv + vm) * m[:, None]


def encoder_chunked(sd, prefix: str, conf: dict, x, geo: dict):
    """SANMEncoderChunkOpt.forward(x [T, F], ind) -> [Tc, D]"""
    dt = x.dtype
    D, H, K = conf["output_size"], conf["attention_heads"], conf.get("kernel_size", 11)
    left = (K - 1) // 2 + max(conf.get("sanm_shfit", 0), 0)
    T = x.shape[0]
    x = x * D ** 0.5 + position_table(T, x.shape[1], dt)
    x = torch.as_tensor(geo["add"], dtype=dt) @ Fn.pad(x, (0, 0, geo["pad_left"], 0))
    m_att, m_shift = torch.as_tensor(geo["mask_att"], dtype=dt), torch.as_tensor(geo["mask_shift"], dtype=dt)
    blocks = [prefix + "encoders0.0."] + [prefix + f"encoders.{i}." for i in range(conf["num_blocks"] - 1)]
    for p in blocks:
        xn = _ln(x, sd, p + "norm1.")
        q, k, v = _lin(xn, sd, p + "self_attn.linear_q_k_v.").split(D, dim=-1)
        att = _lin(masked_attention(q, k, v, H, m_att), sd, p + "self_attn.linear_out.") + \
            fsmn_memory(v, sd[p + "self_attn.fsmn_block.weight"], m_shift, left)
        x = x + att if x.shape[1] == D else att
        x = x + _lin(torch.relu(_lin(_ln(x, sd, p + "norm2."), sd, p + "feed_forward.w_1.")), sd, p + "feed_forward.w_2.")
    return _ln(x, sd, prefix + "after_norm.")


def remove_chunk(x_chunk, geo: dict):
    return torch.as_tensor(geo["rm"], dtype=x_chunk.dtype) @ x_chunk


def stride_conv(w, b, x, stride: int, pad):
    """Conv1dSubsampling.forward over x [T, C] -> [(T - 1) // stride + 1, Cout]"""
    pad = tuple(pad) if isinstance(pad, (list, tuple)) else (pad, pad)
    y = torch.relu(Fn.conv1d(Fn.pad(x.t()[None], pad), w, b, stride=stride))[0].t()
    n = (x.shape[0] - 1) // stride + 1
    assert y.shape[0] >= n
    return y[:n]


# ------------------------------------------------------------------------------------------------ predictor, alignments, scama mask
def predictor_alphas(sd, prefix: str, conf: dict, enc_out, geo: dict):
    dt = enc_out.dtype
    h = enc_out * torch.as_tensor(geo["mask_shift"], dtype=dt)[:, None]
    lo, ro = conf["l_order"], conf["r_order"]
    y = torch.relu(Fn.conv1d(Fn.pad(h.t()[None], (lo, ro)), sd[prefix + "cif_conv1d.weight"], sd[prefix + "cif_conv1d.bias"]))[0].t()
    a = torch.sigmoid(_lin(y, sd, prefix + "cif_output."))[:, 0]
    a = torch.relu(a * conf.get("smooth_factor", 1.0) - conf.get("noise_threshold", 0))
    return a * torch.as_tensor(geo["mask_predictor"], dtype=dt)


def frame_alignments(alphas):
    """gen_frame_alignments in eval mode, one sequence, in the reference's tensor form"""
    L = alphas.shape[0]
    n = int(torch.floor(alphas.sum()))
    cum = torch.floor(torch.cumsum(alphas, 0)).to(torch.int32)
    if n == 0:
        return np.zeros(L, np.int32)
    idx = torch.arange(1, n + 1, dtype=torch.int32)[:, None]
    count = (torch.floor(torch.true_divide(cum[None].repeat(n, 1), idx)).to(torch.int32) == 0).sum(-1) + 1
    count = torch.clamp(count, 0, L)
    return (count[:, None] == torch.arange(1, L + 1)[None]).sum(0).to(torch.int32).numpy()


def scama_mask(alignments, geo: dict, dec_look_back: int):
    """build_scama_mask_for_cross_attention_decoder with chunk_size 1, encoder_chunk_size = attention_chunk_size = P, eval mode,
    in the reference's tensor form -> [N, Tc]"""
    al = torch.as_tensor(np.asarray(alignments), dtype=torch.int32)
    L, P = al.shape[0], geo["P"]
    N = int(al.sum())
    if N == 0:
        return np.zeros((0, L), np.float32)
    cum = torch.cumsum(al, 0)[None].repeat(N, 1)
    idx = torch.arange(1, N + 1, dtype=torch.int32)[:, None]
    cnt = (torch.floor(torch.divide(cum, idx)).to(torch.int32) == 0).sum(-1) + 1
    cnt = torch.clip(torch.clip(cnt, 1, L) - 1, 0, L)
    end = (torch.floor(cnt / P) + 1) * P
    mlc = math.ceil(L / P) * P
    cols = torch.arange(mlc)[None]
    seq = lambda n: (cols < n[:, None]).float()                                    # noqa: E731
    flip = 1 - seq(torch.clip(end - P, 0, mlc))
    flip2 = 1 - seq(torch.clip(end - P * (dec_look_back + 1), 0, mlc))
    mask = seq(end)
    hop = Fn.pad(torch.as_tensor(geo["mask_predictor"]), (0, mlc - L))[None]
    shifted = torch.cat([mask[:, P:], torch.zeros(N, P)], 1)
    mask = (flip * mask + shifted * hop) * flip2
    return (mask[:, :L] * torch.as_tensor(geo["mask_shift"])[None]).numpy().astype(np.float32)


# ------------------------------------------------------------------------------------------------ decoder step
def masked_cross_attention(q, kv, H: int, row):
    """_sanm_oracle.cross_attention under a memory mask row [T] (MultiHeadedAttentionCrossAtt.forward_attention: fill with the dtype's
    minimum, softmax, fill with 0 -- an empty row gives a zero context)"""
    n, D = q.shape
    dk = D // H
    k, v = kv[:, :D].reshape(-1, H, dk), kv[:, D:].reshape(-1, H, dk)
    s = torch.einsum("nhd,thd->nht", q.view(n, H, dk), k) / math.sqrt(dk)
    dead = (torch.as_tensor(row) == 0)[None, None].to(s.device)
    p = torch.softmax(s.masked_fill(dead, torch.finfo(s.dtype).min), dim=-1).masked_fill(dead, 0.0)
    return torch.einsum("nht,thd->nhd", p, v).reshape(n, D)


class ScamaStepper(S.FsmnStepper):
    """FsmnDecoderSCAMAOpt.forward_one_step for all running hypotheses; mask [N, T]: position i takes row min(i, N - 1)
    (uniasr/beam_search.py:391-394); None: no mask; N == 0: nothing visible"""

    def __init__(self, sd, conf: dict, memory, mask=None, prefix="decoder."):
        super().__init__(sd, conf, memory, prefix)
        self.mask = None if mask is None else np.asarray(mask, np.float32).reshape(-1, memory.shape[0])

    def row(self, pos: int):
        if self.mask is None:
            return np.ones(self.memory.shape[0], np.float32)
        return self.mask[min(pos, self.mask.shape[0] - 1)] if self.mask.shape[0] else np.zeros(self.memory.shape[0], np.float32)

    def step(self, tokens, pos):
        sd, p = self.sd, self.p
        row = self.row(pos)
        x = sd[p + "embed.0.weight"][torch.as_tensor(tokens, device=self.memory.device)]
        for q, fsmn, cross in self.layers:
            q = p + q
            t = S.ffn(_ln(x, sd, q + "norm1."), sd, q + "feed_forward.")
            if not fsmn:
                x = t
                continue
            key = q[len(p):]
            x, xn, self.hist[key] = S.fsmn_step(t, x, self.hist[key], sd[q + "norm2.weight"], sd[q + "norm2.bias"],
                                                sd[q + "self_attn.fsmn_block.weight"], self.K, self.left,
                                                sd[q + "norm3.weight"] if cross else None, sd[q + "norm3.bias"] if cross else None)
            if cross:
                x = x + _lin(masked_cross_attention(_lin(xn, sd, q + "src_attn.linear_q."), self.kv[key], self.H, row), sd,
                             q + "src_attn.linear_out.")
        return torch.log_softmax(_lin(_ln(x, sd, p + "after_norm."), sd, p + "output_layer."), dim=-1)


# ------------------------------------------------------------------------------------------------ search with its margins
class MarginSearch(BeamSearchTransformer):
    """the package's host search, recording the smallest gap between neighbours among the best beam + 1 candidates of every position
    (what decides which hypotheses survive and in which order) and among the ended hypotheses at the end"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.margin = float("inf")

    def _search(self, running, logp, ctc, dtype):
        cand = torch.cat([self.w_dec * logp[k].double() + self.w_len + h.score for k, h in enumerate(running)])
        top = torch.sort(cand, descending=True)[0][: self.beam_size + 1]
        if top.numel() > 1:
            self.margin = min(self.margin, float((top[:-1] - top[1:]).min()))
        return super()._search(running, logp, ctc, dtype)

    def __call__(self, *a, **k):
        nbest = super().__call__(*a, **k)
        s = [h.score for h in nbest]
        if len(s) > 1:
            self.margin = min(self.margin, min(x - y for x, y in zip(s[:-1], s[1:])))
        return nbest


MODES = {"fast": (0, 1), "normal": (0, 2), "offline": (1, 2)}


def recognize(sd, conf: dict, feats, decoding_model: str = "normal", beam_size: int = 5, token_num_relax: int = 5, penalty: float = 0.0,
              decoding_ctc_weight: float = 0.0):
    """UniASR.inference for the features of one utterance (no normalisation) -> every stage and the n-best. sd in the dtype of feats."""
    ind, which = MODES[decoding_model]
    out = {}
    geo1 = geometry_of(conf["encoder_conf"], feats.shape[0], ind)
    enc = out["enc1"] = encoder_chunked(sd, "encoder.", conf["encoder_conf"], feats, geo1)
    geo, dconf, pconf, dp, pp, econf = geo1, conf["decoder_conf"], conf["predictor_conf"], "decoder.", "predictor.", conf["encoder_conf"]
    if which == 2:
        sc = conf["stride_conv_conf"]
        x2 = out["stride_conv"] = stride_conv(sd["stride_conv.conv.weight"], sd["stride_conv.conv.bias"],
                                              torch.cat([feats, remove_chunk(enc, geo1)], 1), sc["stride"], sc["pad"])
        geo = geometry_of(conf["encoder2_conf"], x2.shape[0], ind)
        enc = out["enc2"] = encoder_chunked(sd, "encoder2.", conf["encoder2_conf"], x2, geo)
        dconf, pconf, dp, pp, econf = conf["decoder2_conf"], conf["predictor2_conf"], "decoder2.", "predictor2.", conf["encoder2_conf"]
    alphas = out["alphas"] = predictor_alphas(sd, pp, pconf, enc, geo)
    out["token_num"] = float(alphas.sum())
    cum = torch.cumsum(alphas, 0)[alphas > 0]                        # (a masked frame repeats the sum before it)
    out["cumsum_margin"] = float((cum - torch.round(cum)).abs().min()) if cum.numel() else 1.0
    align = out["alignments"] = frame_alignments(alphas)
    n = len(econf["chunk_size"])
    lb = (list(econf["decoder_att_look_back_factor"]) * n)[:n][ind] if len(econf["decoder_att_look_back_factor"]) < n else \
        econf["decoder_att_look_back_factor"][ind]
    mask = out["scama_mask"] = scama_mask(align, geo, lb)
    out["geo"], out["memory"] = geo, enc
    maxlen = int(out["token_num"] + token_num_relax)
    search = MarginSearch(beam_size=beam_size, vocab_size=conf["vocab_size"], sos=1, eos=2, ctc_weight=0.0, length_bonus_weight=penalty,
                          blank=0, pre_beam=False)
    search.w_dec = 1.0 - decoding_ctc_weight
    stepper = ScamaStepper(sd, dconf, enc, mask, prefix=dp)
    out["nbest"] = search(stepper, maxlen, None, 0.0, 0.0, dtype=feats.dtype) if maxlen >= 1 else []
    out["margin"] = search.margin
    return out
