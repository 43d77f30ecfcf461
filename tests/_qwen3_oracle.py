"""torch restatement (float64 or float32, CPU) of what funasr_amd.qwen3 / funasr_amd.fun_asr_nano compute on the device: the Qwen3
decoder -- RMSNorm, per-head q/k norm, rotate-half RoPE, causal grouped-query attention, SwiGLU, (tied) head --, greedy generation over
it, and the FunASRNano `Transformer` adaptor. Written from the upstream definitions; shared by tools/make_golden_funasr_nano.py and the
tests."""
from __future__ import annotations

import math

import torch

TINY = {      # the LMs of the goldens: 2 layers, hidden 128, vocabulary 97
    "hd64_g2": dict(head_dim=64, num_attention_heads=4, num_key_value_heads=2, tie_word_embeddings=True),
    "hd128_g1": dict(head_dim=128, num_attention_heads=4, num_key_value_heads=4, tie_word_embeddings=False),
    "hd128_g4": dict(head_dim=128, num_attention_heads=4, num_key_value_heads=1, tie_word_embeddings=True),
}
EOS, PAD = 3, 0


def tiny_config(name: str) -> dict:
    c = dict(model_type="qwen3", architectures=["Qwen3ForCausalLM"], vocab_size=97, hidden_size=128, intermediate_size=96, num_hidden_layers=2,
             rms_norm_eps=1e-6, rope_theta=1000000.0, hidden_act="silu", attention_bias=False, attention_dropout=0.0,
             max_position_embeddings=8192, eos_token_id=EOS, pad_token_id=None, bos_token_id=None, use_sliding_window=False,
             sliding_window=None, use_cache=True)
    c.update(TINY[name])
    return c


def state_dict_keys(c: dict) -> list:
    keys = ["model.embed_tokens.weight"]
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        keys += [p + n for n in ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                                 "self_attn.q_norm.weight", "self_attn.k_norm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight",
                                 "mlp.down_proj.weight", "input_layernorm.weight", "post_attention_layernorm.weight")]
    return keys + ["model.norm.weight", "lm_head.weight"]


def seeded_state_dict(c: dict, seed: int) -> dict:
    """float32 weights with enough spread for a decisive arg-max (the upstream init, std 0.02, leaves every logit within 1e-2)"""
    g = torch.Generator().manual_seed(seed)
    H, I, V = c["hidden_size"], c["intermediate_size"], c["vocab_size"]
    hd, nh, nkv = c["head_dim"], c["num_attention_heads"], c["num_key_value_heads"]

    def lin(o, i, gain=1.5):
        return torch.randn(o, i, generator=g) * (gain / math.sqrt(i))

    def norm(n):
        return 1.0 + 0.2 * torch.randn(n, generator=g)

    sd = {"model.embed_tokens.weight": torch.randn(V, H, generator=g)}
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        sd[p + "self_attn.q_proj.weight"] = lin(nh * hd, H)
        sd[p + "self_attn.k_proj.weight"] = lin(nkv * hd, H)
        sd[p + "self_attn.v_proj.weight"] = lin(nkv * hd, H)
        sd[p + "self_attn.o_proj.weight"] = lin(H, nh * hd)
        sd[p + "self_attn.q_norm.weight"] = norm(hd)
        sd[p + "self_attn.k_norm.weight"] = norm(hd)
        sd[p + "mlp.gate_proj.weight"] = lin(I, H)
        sd[p + "mlp.up_proj.weight"] = lin(I, H)
        sd[p + "mlp.down_proj.weight"] = lin(H, I)
        sd[p + "input_layernorm.weight"] = norm(H)
        sd[p + "post_attention_layernorm.weight"] = norm(H)
    sd["model.norm.weight"] = norm(H)
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"] if c["tie_word_embeddings"] else torch.randn(V, H, generator=g)
    return sd


def seeded_prompt(c: dict, seed: int, rows: int) -> torch.Tensor:
    """[rows, hidden] float32 inputs_embeds"""
    return torch.randn(rows, c["hidden_size"], generator=torch.Generator().manual_seed(1000 + seed))


# ---------------------------------------------------------------------------------------------------------------- pieces
def rope_cos_sin(head_dim: int, theta: float, positions, dtype=torch.float64):
    """float32 tables as upstream computes them (inv_freq, angle, cos / sin all float32), cast to `dtype`: [n, head_dim / 2]"""
    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float) / head_dim))
    pos = torch.as_tensor(positions, dtype=torch.int64).float()
    freqs = pos[:, None] * inv_freq[None, :]
    return freqs.cos().to(dtype), freqs.sin().to(dtype)


def rmsnorm(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


def qk_rope(x, w, eps, cos, sin):
    """x [rows, heads, hd], cos / sin [rows, hd / 2] -> normed and rotated"""
    x = rmsnorm(x, w, eps)
    c, s = torch.cat((cos, cos), -1)[:, None, :], torch.cat((sin, sin), -1)[:, None, :]
    return x * c + rotate_half(x) * s


def gqa_attention(q, k, v, p0: int):
    """q [M, Hq, hd] at positions p0 .. p0 + M - 1, k / v [L, Hkv, hd] with L >= p0 + M: row i attends to keys 0 .. p0 + i"""
    M, Hq, hd = q.shape
    L, Hkv = k.shape[0], k.shape[1]
    G = Hq // Hkv
    kk, vv = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    s = torch.einsum("mhd,lhd->hml", q, kk) * (hd ** -0.5)
    mask = torch.arange(L)[None, :] > (p0 + torch.arange(M))[:, None]
    s = s.masked_fill(mask[None], float("-inf"))
    return torch.einsum("hml,lhd->mhd", torch.softmax(s, -1), vv)


def swiglu(gate, up):
    return gate / (1.0 + torch.exp(-gate)) * up


def forward(sd: dict, c: dict, embeds: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """logits [T, V] of every row of inputs_embeds [T, H] (one sequence from position 0)"""
    w = {k: v.to(dtype) for k, v in sd.items()}
    x = embeds.to(dtype)
    T = x.shape[0]
    hd, nh, nkv, eps = c["head_dim"], c["num_attention_heads"], c["num_key_value_heads"], c["rms_norm_eps"]
    cos, sin = rope_cos_sin(hd, c["rope_theta"], range(T), dtype)
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        h = rmsnorm(x, w[p + "input_layernorm.weight"], eps)
        q = (h @ w[p + "self_attn.q_proj.weight"].T).reshape(T, nh, hd)
        k = (h @ w[p + "self_attn.k_proj.weight"].T).reshape(T, nkv, hd)
        v = (h @ w[p + "self_attn.v_proj.weight"].T).reshape(T, nkv, hd)
        q = qk_rope(q, w[p + "self_attn.q_norm.weight"], eps, cos, sin)
        k = qk_rope(k, w[p + "self_attn.k_norm.weight"], eps, cos, sin)
        a = gqa_attention(q, k, v, 0).reshape(T, nh * hd)
        x = x + a @ w[p + "self_attn.o_proj.weight"].T
        h = rmsnorm(x, w[p + "post_attention_layernorm.weight"], eps)
        x = x + swiglu(h @ w[p + "mlp.gate_proj.weight"].T, h @ w[p + "mlp.up_proj.weight"].T) @ w[p + "mlp.down_proj.weight"].T
    x = rmsnorm(x, w["model.norm.weight"], eps)
    head = w["model.embed_tokens.weight"] if c["tie_word_embeddings"] else w["lm_head.weight"]
    return x @ head.T


def greedy(sd: dict, c: dict, embeds: torch.Tensor, max_new_tokens: int, eos=(EOS,), dtype=torch.float64):
    """(ids, logits [len(ids), V]): greedy ids of one sequence up to and including its first eos, the logits each was taken from"""
    emb = sd["model.embed_tokens.weight"]
    x, ids, rows = embeds.to(torch.float32), [], []
    for _ in range(max_new_tokens):
        lg = forward(sd, c, x, dtype)[-1]
        t = int(torch.argmax(lg))
        ids.append(t)
        rows.append(lg)
        if t in eos:
            break
        x = torch.cat((x, emb[t][None]), 0)
    return ids, torch.stack(rows)


def top2_gap(logits: torch.Tensor) -> float:
    """smallest best-minus-second over the rows of logits [n, V]"""
    top = torch.topk(logits, 2, -1).values
    return float((top[:, 0] - top[:, 1]).min())


# --------------------------------------------------------------------------------------------------------------- adaptor
def layer_norm(x, g, b, eps=1e-12):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def adaptor(sd: dict, x: torch.Tensor, ilen: int, k: int, heads: int, dtype=torch.float64):
    """the `Transformer` adaptor (llm_asr/adaptor.py) on one clip: x [T, encoder_dim] with ilen valid frames -> ([ceil(T / k), llm_dim],
    olen). Frames are zero-padded to a multiple of k and stacked; linear1, ReLU, linear2; then pre-norm encoder layers whose attention
    masks the chunks at or past olen = (ilen - 1) // k + 1."""
    w = {n: v.to(dtype) for n, v in sd.items()}
    x = x.to(dtype)
    T, D = x.shape
    n = (T - 1) // k + 1
    x = torch.cat((x, x.new_zeros(n * k - T, D)), 0).reshape(n, D * k)
    x = torch.relu(x @ w["linear1.weight"].T + w["linear1.bias"]) @ w["linear2.weight"].T + w["linear2.bias"]
    olen = (ilen - 1) // k + 1
    L = x.shape[-1]
    dk = L // heads
    i = 0
    while f"blocks.{i}.norm1.weight" in w:
        p = f"blocks.{i}."
        h = layer_norm(x, w[p + "norm1.weight"], w[p + "norm1.bias"])
        q = (h @ w[p + "self_attn.linear_q.weight"].T + w[p + "self_attn.linear_q.bias"]).reshape(n, heads, dk)
        kk = (h @ w[p + "self_attn.linear_k.weight"].T + w[p + "self_attn.linear_k.bias"]).reshape(n, heads, dk)
        v = (h @ w[p + "self_attn.linear_v.weight"].T + w[p + "self_attn.linear_v.bias"]).reshape(n, heads, dk)
        s = torch.einsum("qhd,khd->hqk", q, kk) / math.sqrt(dk)
        s = s.masked_fill((torch.arange(n) >= olen)[None, None, :], float("-inf"))
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(n, L)
        x = x + a @ w[p + "self_attn.linear_out.weight"].T + w[p + "self_attn.linear_out.bias"]
        h = layer_norm(x, w[p + "norm2.weight"], w[p + "norm2.bias"])
        h = torch.relu(h @ w[p + "feed_forward.w_1.weight"].T + w[p + "feed_forward.w_1.bias"])
        x = x + h @ w[p + "feed_forward.w_2.weight"].T + w[p + "feed_forward.w_2.bias"]
        i += 1
    return x, olen
