"""What tools/make_golden_funasr_nano.py and the FunASRNano tests share: the tiny model configuration, a synthetic `transformers`
tokenizer (a `tokenizers` WordLevel model over single characters with the ChatML and speech special tokens, at most 97 ids -- the tiny
LM's vocabulary), a stand-in frontend whose frame count is all the prompt assembly looks at, seeded weights, and the writer of a
synthetic model directory (config.yaml, configuration.json, model.pt, the LM's config / tokenizer sub-directory)."""
from __future__ import annotations

import json
import math
import os

import torch

from . import _qwen3_oracle as O

SPECIALS = ["<|endoftext|>", "<unk>", "<|im_start|>", "<|im_end|>", "<|startofspeech|>", "<|endofspeech|>"]      # id 3 = <|im_end|> = eos
CHARS = list("\n :,[]!.01abcdefghijklmnopqrstuvwxyzAY") + list("请结合上下文信息更加准确地完成语音转写任务如果没有相关我们会留空热词列表不进行本规整，。：*中英")
assert len(SPECIALS) + len(CHARS) <= 97 and len(set(CHARS)) == len(CHARS)

ENCODER_CONF = dict(output_size=128, attention_heads=1, linear_units=128, num_blocks=2, tp_blocks=1, dropout_rate=0.0, kernel_size=11,
                    sanm_shfit=0, input_layer="pe", normalize_before=True)
ADAPTOR_CONF = dict(downsample_rate=2, ffn_dim=64, n_layer=2, attention_heads=2, encoder_dim=128, llm_dim=128)
INPUT_SIZE = 560          # 80 mel bins x lfr_m 7
STUB_DIM = 80
FRAME_SAMPLES = 960


def _load_transformers() -> bool:
    """Import what these tests use of `transformers` when this module is imported, i.e. while pytest collects and before any test
    runs. The package loads its modules lazily and probes optional packages (torchaudio, soundfile, ..) as it does; a probe that first
    runs after another test has put a stand-in module without a __spec__ into sys.modules raises instead of answering. Loaded up
    front -- down to one tiny model and one tokenizer round trip -- nothing is probed later, and nothing global is touched."""
    try:
        import transformers
        from transformers import AutoConfig, AutoModelForCausalLM, AutoTokenizer, PreTrainedTokenizerFast  # noqa: F401
    except ImportError:
        return False
    if hasattr(transformers, "Qwen3Config"):
        import tempfile
        import transformers.models.qwen3.modeling_qwen3  # noqa: F401
        m = AutoModelForCausalLM.from_config(transformers.Qwen3Config(vocab_size=8, hidden_size=16, intermediate_size=16, num_hidden_layers=1,
                                                                      num_attention_heads=2, num_key_value_heads=1, head_dim=8, eos_token_id=1))
        m.generate(inputs_embeds=torch.zeros(1, 2, 16), max_new_tokens=1, do_sample=False, pad_token_id=1)
        with tempfile.TemporaryDirectory() as d:
            AutoTokenizer.from_pretrained(write_llm_dir(d), local_files_only=True)
    return True


def model_conf(llm_dir: str, low_frame_rate: bool = False, lm: str = "hd64_g2") -> dict:
    """constructor arguments of FunASRNano (the reference's and this package's) at tiny size"""
    return dict(audio_encoder="SenseVoiceEncoderSmall", audio_encoder_conf=dict(ENCODER_CONF), audio_adaptor="Transformer",
                audio_adaptor_conf=dict(ADAPTOR_CONF, use_low_frame_rate=low_frame_rate), llm="Qwen3",
                llm_conf=dict(hub="hf", freeze=True, llm_dtype="fp32", init_param_path=llm_dir), input_size=INPUT_SIZE)


def write_llm_config(path: str, lm: str = "hd64_g2") -> str:
    """the LM's config.json alone in `path` (all that building the model needs)"""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
        json.dump(O.tiny_config(lm), f, indent=1)
    return path


class CharTokenizer:
    """the synthetic tokenizer's `encode` in plain Python (special tokens first, then one id per character, <unk> otherwise): what the
    prompt assembly needs, without the `transformers` package; tested equal to the saved tokenizer where that package exists"""

    def __init__(self):
        self.vocab = {t: i for i, t in enumerate(SPECIALS + CHARS)}

    def encode(self, s: str) -> list:
        ids, i = [], 0
        while i < len(s):
            sp = next((t for t in SPECIALS if s.startswith(t, i)), None)
            ids.append(self.vocab[sp] if sp else self.vocab.get(s[i], self.vocab["<unk>"]))
            i += len(sp) if sp else 1
        return ids


def write_llm_dir(path: str, lm: str = "hd64_g2") -> str:
    """the LM's config.json and the synthetic tokenizer's files in `path`"""
    write_llm_config(path, lm)
    from tokenizers import Regex, Tokenizer, decoders, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    vocab = {t: i for i, t in enumerate(SPECIALS + CHARS)}
    tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Split(Regex("(?m:.)"), "isolated")
    tok.decoder = decoders.Fuse()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", eos_token="<|im_end|>", pad_token="<|endoftext|>",
                                   additional_special_tokens=["<|im_start|>", "<|startofspeech|>", "<|endofspeech|>"])
    fast.save_pretrained(path)
    return path


class StubFrontend:
    """fs / frame_shift / lfr_n and a call that turns N samples into N // 960 frames of 80 features: the prompt assembly reads the
    frame count only, and the end-to-end test wants features that are a fixed function of the samples"""
    fs, frame_shift, lfr_n = 16000, 10, 6

    def output_size(self):
        return STUB_DIM

    def __call__(self, data, data_len, **kwargs):
        data = torch.as_tensor(data, dtype=torch.float32)
        if data.dim() < 2:
            data = data[None]
        n = int(data_len[0]) // FRAME_SAMPLES
        x = data[:, : n * FRAME_SAMPLES].reshape(data.shape[0], n, FRAME_SAMPLES)
        feats = torch.stack([x[..., j::STUB_DIM].mean(-1) for j in range(STUB_DIM)], -1) * 8.0
        return feats, torch.tensor([n], dtype=torch.int32)


def clip(seed: int, n_frames: int) -> torch.Tensor:
    return torch.randn(n_frames * FRAME_SAMPLES + 17, generator=torch.Generator().manual_seed(500 + seed))


def encoder_state_dict(model, seed: int) -> dict:
    """seeded weights for every key of model.audio_encoder / model.audio_adaptor (by shape: matrices ~ 1 / sqrt(fan-in), norm weights
    near 1, everything else small)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.startswith("llm."):
            continue
        if v.dim() >= 2:
            fan = v[0].numel()
            sd[k] = torch.randn(v.shape, generator=g) / math.sqrt(fan)
        elif "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
    return sd


def adaptor_state_dict(seed: int, conf: dict = None) -> dict:
    """the `Transformer` adaptor's keys (reference names) with seeded weights"""
    c = dict(ADAPTOR_CONF if conf is None else conf)
    g = torch.Generator().manual_seed(seed)
    L, D, Fd, k = c["llm_dim"], c["encoder_dim"], c["ffn_dim"], c["downsample_rate"]

    def lin(sd, name, o, i):
        sd[name + ".weight"] = torch.randn(o, i, generator=g) / math.sqrt(i)
        sd[name + ".bias"] = 0.05 * torch.randn(o, generator=g)

    sd = {}
    lin(sd, "linear1", Fd, D * k)
    lin(sd, "linear2", L, Fd)
    for i in range(c["n_layer"]):
        p = f"blocks.{i}."
        for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
            lin(sd, p + "self_attn." + n, L, L)
        lin(sd, p + "feed_forward.w_1", L // 4, L)
        lin(sd, p + "feed_forward.w_2", L, L // 4)
        for n in ("norm1", "norm2"):
            sd[p + n + ".weight"] = 1.0 + 0.1 * torch.randn(L, generator=g)
            sd[p + n + ".bias"] = 0.05 * torch.randn(L, generator=g)
    return sd


def write_model_dir(path: str, state_dict: dict, low_frame_rate: bool = False, lm: str = "hd64_g2") -> str:
    """config.yaml + configuration.json + model.pt + llm/ (LM config and tokenizer): what AutoModel(model=path) builds FunASRNano from"""
    import yaml

    os.makedirs(path, exist_ok=True)
    write_llm_dir(os.path.join(path, "llm"), lm)
    conf = model_conf("llm", low_frame_rate, lm)
    conf.update(model="FunASRNano", tokenizer="HuggingfaceTokenizer", tokenizer_conf=dict(init_param_path="llm"), frontend="WavFrontend",
                frontend_conf=dict(fs=16000, window="hamming", n_mels=80, frame_length=25, frame_shift=10, lfr_m=7, lfr_n=6))
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    with open(os.path.join(path, "configuration.json"), "w", encoding="utf-8") as f:
        json.dump({"framework": "pytorch", "task": "auto-speech-recognition",
                   "file_path_metas": {"init_param": "model.pt", "config": "config.yaml", "llm_conf": {"init_param_path": "llm"},
                                       "tokenizer_conf": {"init_param_path": "llm"}}}, f, indent=1)
    torch.save(state_dict, os.path.join(path, "model.pt"))
    return path


HAVE_TRANSFORMERS = _load_transformers()
