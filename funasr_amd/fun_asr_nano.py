"""Fun-ASR-Nano on gfx950: `FunASRNano` (model_classes; funasr/models/fun_asr_nano/model.py) -- an audio encoder, an adaptor and a
Qwen3 causal LM that writes the transcript token by token -- and the `Transformer` adaptor (adaptor_classes;
funasr/models/llm_asr/adaptor.py:125-202).

  * `audio_encoder` is looked up by name in encoder_classes (`SenseVoiceEncoderSmall`, funasr_amd/sanm_encoder.py).
  * `TransformerAdaptor`: frames zero-padded to a multiple of `downsample_rate` and stacked, linear1 + ReLU, linear2, then `n_layer`
    pre-norm Transformer encoder layers (`attention_heads`, feed-forward width llm_dim // 4) masked by olens = (ilens - 1) // k + 1.
    Every product runs on the kernels the Transformer family has: the exact-fp32 GEMM with bias / ReLU / residual epilogues, the
    row LayerNorm, and the masked attention of csrc/attention_abs.hip (heads of 64) or csrc/attention_f32.hip (heads of 128).
  * `Qwen3Decoder` (funasr_amd/qwen3.py) is the LM: prefill, KV cache and the greedy loop inside the library.

The inference path is the reference's, step by step: `get_prompt` (hotwords, language, itn), `generate_chatml`, `data_template`, the
ChatML source string and its split at <|startofspeech|>..<|endofspeech|> (`data_load_speech`), both `fake_token_len` formulas, the
embedding lookup on the device, the first `fake_token_len` adaptor rows spliced in at `fbank_beg`, greedy generation with
max_new_tokens = `max_length` (512), pad = pad_token_id or eos_token_id, `tokenizer.batch_decode`, the `prev_text` prefix, the record
{"key", "text", "text_tn", "label"} and the 1best_recog writers. A list of inputs is one batch of the LM (slices of 16), every clip at
its own length: no left padding, and every clip's ids are what it gets alone.

Not built (each refused by name): `hub: ms`, `llm_dtype` / `fp16` / `bf16` other than fp32, `use_lora`, `teacherforcing`, `llm_kwargs`
that change the search (do_sample, num_beams > 1, penalties, ..), the `Linear` and `QFormer` adaptors, adaptor heads other than 64 /
128. A configured `ctc_decoder` is not built either: its `ctc_decoder.*` / `ctc.*` checkpoint keys are skipped and no `ctc_text` or
timestamps are produced (one log line says so).
"""
from __future__ import annotations

import logging
import random
import re
import string
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from . import sanm_encoder as _sanm_encoder  # noqa: F401  (registers SenseVoiceEncoderSmall, the audio encoder of this model's configurations)
from . import tokenizer as _tokenizer  # noqa: F401  (registers HuggingfaceTokenizer, the tokenizer of this model's configurations)
from .audio import load_audio
from .datadir_writer import DatadirWriter
from .hip_module import Holder, _truthy, device_lens, layer_norm, linear
from .qwen3 import Qwen3Decoder
from .register import tables

SPEECH_SPAN = re.compile(r"(<\|startofspeech\|>.*?<\|endofspeech\|>)")
# generate() arguments that leave a greedy search what it is (value -> allowed)
_NEUTRAL_LLM_KWARGS = {"do_sample": (False, None), "num_beams": (1, None), "num_beam_groups": (1, None), "repetition_penalty": (1.0, None),
                       "length_penalty": (1.0, None), "no_repeat_ngram_size": (0, None), "temperature": (1.0, None), "top_k": (None, 50),
                       "top_p": (1.0, None), "penalty_alpha": (None,), "num_return_sequences": (1, None), "use_cache": (True, None)}


def _refuse(what: str):
    raise NotImplementedError(f"FunASRNano(HIP): {what} is not built")


# =============================================================================================================== adaptors
@tables.register("adaptor_classes", "Transformer")
class TransformerAdaptor(nn.Module):
    def __init__(self, downsample_rate=2, encoder_dim=1280, llm_dim=4096, ffn_dim: int = 2048, **kwargs):
        super().__init__()
        self.k, self.encoder_dim, self.llm_dim, self.ffn_dim = int(downsample_rate), int(encoder_dim), int(llm_dim), int(ffn_dim)
        self.n_layer, self.heads = int(kwargs.get("n_layer", 2)), int(kwargs.get("attention_heads", 8))
        who = "TransformerAdaptor(HIP)"
        dk = self.llm_dim // max(self.heads, 1)
        refusals = [
            (self.k < 1, f"downsample_rate: {downsample_rate}"),
            (self.n_layer > 0 and (self.heads < 1 or self.llm_dim != dk * self.heads or dk not in (64, 128)),
             f"attention_heads: {self.heads} with llm_dim {self.llm_dim} (heads of 64 or 128)"),
            ((self.encoder_dim * self.k) % 32 != 0, f"encoder_dim x downsample_rate: {self.encoder_dim * self.k} (a multiple of 32)"),
            (self.ffn_dim % 32 != 0, f"ffn_dim: {self.ffn_dim} (a multiple of 32)"),
            (self.llm_dim % 128 != 0, f"llm_dim: {self.llm_dim} (a multiple of 128, so that llm_dim // 4 is one of 32)"),
        ]
        for bad, why in refusals:
            if bad:
                raise NotImplementedError(f"{who}: {why} is not built")
        self.dk = dk
        self.linear1, self.linear2 = linear(self.ffn_dim, self.encoder_dim * self.k), linear(self.llm_dim, self.ffn_dim)
        self.blocks = None
        if self.n_layer > 0:
            blocks = nn.ModuleList()
            L = self.llm_dim
            for _ in range(self.n_layer):
                b = Holder()
                a = Holder()
                a.linear_q, a.linear_k, a.linear_v, a.linear_out = linear(L, L), linear(L, L), linear(L, L), linear(L, L)
                f = Holder()
                f.w_1, f.w_2 = linear(L // 4, L), linear(L, L // 4)
                b.self_attn, b.feed_forward, b.norm1, b.norm2 = a, f, layer_norm(L), layer_norm(L)
                blocks.append(b)
            self.blocks = blocks
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, x: torch.Tensor, ilens=None):
        """x [B, T, encoder_dim], ilens [B] -> ([B, ceil(T / k), llm_dim], olens int64 [B])"""
        dev = self.linear1.weight.device
        if dev.type != "cuda":
            raise RuntimeError("TransformerAdaptor runs only on an AMD GPU through libparaformer_hip.so (there is no CPU fallback by design)")
        x = x.to(device=dev, dtype=torch.float32)
        B, T, D = x.shape
        n = (T - 1) // self.k + 1
        lens = [int(v) for v in (ilens.tolist() if isinstance(ilens, torch.Tensor) else ilens)]
        olens = [(v - 1) // self.k + 1 for v in lens]
        with torch.cuda.device(dev):
            x = F.pad(x, (0, 0, 0, n * self.k - T)).reshape(B * n, D * self.k).contiguous()
            h = ops.gemm(x, self.linear1.weight, self.linear1.bias, relu=True)
            y = ops.gemm(h, self.linear2.weight, self.linear2.bias)
            klens = device_lens(olens, dev)
            L, H = self.llm_dim, self.heads
            for b in self.blocks or ():
                a, f = b.self_attn, b.feed_forward
                xn = ops.layernorm(y, b.norm1.weight, b.norm1.bias, 1e-12)
                qkv = torch.empty(B * n, 3 * L, device=dev)
                for j, lin in enumerate((a.linear_q, a.linear_k, a.linear_v)):
                    ops.gemm(xn, lin.weight, lin.bias, out=qkv[:, j * L:(j + 1) * L])
                if self.dk == 64:
                    att = torch.empty(B * n, L, device=dev)
                    _lib.check(_lib.load().pf_k_tf_attention(qkv.data_ptr(), klens.data_ptr(), B, n, H, att.data_ptr(),
                                                             torch.cuda.current_stream().cuda_stream), "pf_k_tf_attention")
                else:
                    v3 = qkv.reshape(B, n, 3 * L)
                    att = ops.attention(v3[:, :, :L], v3[:, :, L:2 * L], v3[:, :, 2 * L:], klens, H, self.dk ** -0.5).reshape(B * n, L)
                y = ops.gemm(att, a.linear_out.weight, a.linear_out.bias, add1=y)
                xn = ops.layernorm(y, b.norm2.weight, b.norm2.bias, 1e-12)
                h = ops.gemm(xn, f.w_1.weight, f.w_1.bias, relu=True)
                y = ops.gemm(h, f.w_2.weight, f.w_2.bias, add1=y)
        return y.reshape(B, n, self.llm_dim), torch.tensor(olens, dtype=torch.int64, device=dev)


@tables.register("adaptor_classes", "Linear")
class LinearAdaptor(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("audio_adaptor: Linear is not built (the HIP adaptor is audio_adaptor: Transformer)")


@tables.register("adaptor_classes", "QFormer")
class QFormerAdaptor(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("audio_adaptor: QFormer is not built (the HIP adaptor is audio_adaptor: Transformer)")


# ================================================================================================================== model
def check_llm_kwargs(llm_kwargs) -> None:
    """refuse every `llm_kwargs` entry that would change the search: the library's loop is greedy"""
    for k, v in (llm_kwargs or {}).items():
        if k not in _NEUTRAL_LLM_KWARGS or v not in _NEUTRAL_LLM_KWARGS[k]:
            _refuse(f"llm_kwargs.{k}: {v!r} (greedy search only)")


def check_llm_dtype(conf: dict) -> None:
    dt = conf.get("llm_dtype", "fp32")
    if dt != "fp32":
        _refuse(f"llm_dtype: {dt} (only fp32)")
    for k in ("fp16", "bf16"):
        if _truthy(conf.get(k, False)):
            _refuse(f"{k}: true for the LM (only fp32)")


@tables.register("model_classes", "FunASRNano")
class FunASRNano(nn.Module):
    def __init__(self, audio_encoder: str = None, audio_encoder_conf: dict = None, audio_adaptor: str = None, audio_adaptor_conf: dict = None,
                 llm: str = None, llm_conf: dict = None, input_size: int = 80, length_normalized_loss: bool = False, **kwargs):
        super().__init__()
        audio_encoder_conf, audio_adaptor_conf, llm_conf = dict(audio_encoder_conf or {}), dict(audio_adaptor_conf or {}), dict(llm_conf or {})
        if audio_encoder_conf.get("hub", None) == "ms":
            _refuse("audio_encoder_conf.hub: ms (the encoder is built by name from encoder_classes; nothing is downloaded)")
        check_llm_dtype(llm_conf)
        if _truthy(llm_conf.get("use_lora", False)):
            _refuse("llm_conf.use_lora: true")
        encoder_class = tables.encoder_classes.get(audio_encoder)
        if encoder_class is None:
            raise KeyError(f"audio_encoder {audio_encoder!r} is not registered in encoder_classes: {sorted(tables.encoder_classes)}")
        self.audio_encoder = encoder_class(input_size=input_size, **audio_encoder_conf)
        encoder_dim = self.audio_encoder.output_size()
        init_param_path = llm_conf.get("init_param_path", None)
        if not init_param_path:
            raise ValueError("FunASRNano: llm_conf.init_param_path (the directory of the LM's config.json) is required")
        self.llm = Qwen3Decoder.from_config_dir(str(init_param_path))
        self.llm_dtype = "fp32"
        adaptor_class = tables.adaptor_classes.get(audio_adaptor)
        if adaptor_class is None:
            raise KeyError(f"audio_adaptor {audio_adaptor!r} is not registered in adaptor_classes: {sorted(tables.adaptor_classes)}")
        if encoder_dim > 0:
            audio_adaptor_conf["encoder_dim"] = encoder_dim
        audio_adaptor_conf["llm_dim"] = self.llm.hidden_size
        self.audio_adaptor = adaptor_class(**audio_adaptor_conf)
        self.use_low_frame_rate = _truthy(audio_adaptor_conf.get("use_low_frame_rate", False))
        self.ctc_decoder = None
        if kwargs.get("ctc_decoder", None) is not None:
            logging.warning("FunASRNano(HIP): ctc_decoder %r is not built: its ctc_decoder.* / ctc.* weights are skipped, no ctc_text and no "
                            "timestamps are produced", kwargs.get("ctc_decoder"))
        self.length_normalized_loss = length_normalized_loss
        for p in self.parameters():
            p.requires_grad_(False)

    # ---------------------------------------------------------------------------------------------- prompt and ChatML
    def get_prompt(self, hotwords, language: str = None, itn: bool = True) -> str:
        prompt = ""
        if len(hotwords) > 0:
            prompt = ("请结合上下文信息，更加准确地完成语音转写任务。如果没有相关信息，我们会留空。\n\n\n**上下文信息：**\n\n\n"
                      f"热词列表：[{', '.join(hotwords)}]\n")
        prompt += "语音转写" if language is None else f"语音转写成{language}"
        if not itn:
            prompt += "，不进行文本规整"
        return prompt + "："

    def generate_chatml(self, prompt: str, data):
        turn = [{"role": "system", "content": "You are a helpful assistant."}]
        if isinstance(data, str):
            turn.append({"role": "user", "content": f"{prompt}<|startofspeech|>!{data}<|endofspeech|>"})
        elif isinstance(data, torch.Tensor):
            turn.append({"role": "user", "content": f"{prompt}<|startofspeech|>!!<|endofspeech|>", "audio": data})
        else:
            return None
        turn.append({"role": "assistant", "content": "null"})
        return turn

    def data_template(self, data) -> dict:
        out = {"system": [], "user": [], "assistant": []}
        for item in data:
            role, content = item["role"], item["content"]
            if role == "user" and "audio" in item:
                content = [content, item["audio"]]
            if role in out:
                out[role].append(content)
        out["system"] = out["system"] * len(out["user"])
        return out

    def fake_token_len(self, n_frames: int) -> int:
        """speech placeholders of a clip of n_frames feature frames"""
        if not self.use_low_frame_rate:
            return int(n_frames)
        olens = 1 + (int(n_frames) - 3 + 2 * 1) // 2
        olens = 1 + (olens - 3 + 2 * 1) // 2
        return (olens - 1) // 2 + 1

    def _speech_features(self, item, frontend, meta_data, kwargs):
        """one speech span's source -> (features [1, T, F], lengths int32 [1, 1])"""
        t1 = time.perf_counter()
        if kwargs.get("data_type", "sound") == "fbank":
            if not isinstance(item, torch.Tensor):
                raise TypeError("FunASRNano: data_type fbank takes feature tensors [T, F]")
            speech = item if item.dim() == 3 else item[None]
            return speech.to(torch.float32), torch.tensor([[speech.shape[1]]], dtype=torch.int32)
        wav = load_audio(item, fs=frontend.fs, audio_fs=kwargs.get("fs", 16000))
        t2 = time.perf_counter()
        meta_data["load_data"] = f"{t2 - t1:0.3f}"
        device = kwargs.get("device", None)
        wav = wav[None] if device is None else wav[None].to(device)
        speech, lens = frontend(wav, [int(wav.shape[1])])
        meta_data["extract_feat"] = f"{time.perf_counter() - t2:0.3f}"
        lens = torch.as_tensor(lens).reshape(1, -1).to(dtype=torch.int32, device="cpu")
        meta_data["batch_data_time"] = int(lens.sum()) * frontend.frame_shift * frontend.lfr_n / 1000
        return speech.to(torch.float32), lens

    def data_load_speech(self, contents: dict, tokenizer, frontend, meta_data=None, **kwargs) -> dict:
        meta_data = {} if meta_data is None else meta_data
        conf = kwargs.get("dataset_conf") or {}
        do_think, sys_prompt = conf.get("do_think", True), conf.get("sys_prompt", True)
        open_turn = _truthy(kwargs.get("infer_with_assistant_input", False))
        input_ids, labels, fbank, fbank_lens, fbank_mask, fbank_beg, fake_lens = [], [], [], [], [], [], []
        input_source_ids, target_ids = [], []
        for i, (system_prompt, user_prompt, target_out) in enumerate(zip(contents["system"], contents["user"], contents["assistant"])):
            if i >= kwargs.get("multiturn_num_max", 5) or len(input_ids) > kwargs.get("max_token_length", 1500):
                break
            audio = None
            if isinstance(user_prompt, (list, tuple)):
                user_prompt, audio = user_prompt
            source = f"<|im_start|>user\n{user_prompt}"
            if i == 0 and sys_prompt:
                source = f"<|im_start|>system\n{system_prompt}<|im_end|>\n" + source
            if not open_turn:
                source += "<|im_end|>\n<|im_start|>assistant\n"
            if not do_think:
                source += "<think>\n\n</think>\n\n"
            if kwargs.get("prev_text", None) is not None:
                source += kwargs["prev_text"]
            source_ids, mask_i, fake_i, beg_i = [], [], 0, -1
            speech, speech_lengths = [], []
            for piece in SPEECH_SPAN.split(source):
                if not piece.startswith("<|startofspeech|>"):
                    ids = tokenizer.encode(piece)
                    source_ids += ids
                    mask_i += [0] * len(ids)
                    continue
                piece = piece.replace("<|startofspeech|>", "").replace("<|endofspeech|>", "")
                if not piece.startswith("!"):
                    continue
                piece = piece[1:]
                item = audio if piece.startswith("!") else piece            # "!!": the samples ride beside the prompt
                speech, speech_lengths = self._speech_features(item, frontend, meta_data, kwargs)
                fake_i = self.fake_token_len(int(speech_lengths[0, 0]))
                beg_i = len(source_ids)
                source_ids += [0] * fake_i
                mask_i += [1] * fake_i
            fbank_beg.append(beg_i + len(input_ids))
            fake_lens.append(fake_i)
            target_ids = tokenizer.encode(f"{target_out}<|im_end|>")
            input_source_ids = input_ids + source_ids
            input_ids = input_ids + source_ids + target_ids
            labels += [-100] * len(source_ids) + target_ids
            fbank_mask += mask_i
            if len(speech) > 0:
                fbank.append(speech[0])
                fbank_lens.append(speech_lengths[0])
        out = {
            "speech": torch.nn.utils.rnn.pad_sequence(fbank, batch_first=True, padding_value=0.0) if fbank else [],
            "speech_lengths": torch.nn.utils.rnn.pad_sequence(fbank_lens, batch_first=True, padding_value=-1) if fbank else [],
            "fbank_mask": torch.tensor(fbank_mask, dtype=torch.float32)[None],
            "fbank_beg": torch.tensor(fbank_beg, dtype=torch.int32)[None],
            "fake_token_len": torch.tensor(fake_lens, dtype=torch.int32)[None],
            "input_ids": torch.tensor(input_ids, dtype=torch.int64)[None],
            "attention_mask": torch.ones(1, len(input_ids), dtype=torch.int32),
            "labels_ids": torch.tensor(labels, dtype=torch.int64),
            "source_ids": torch.tensor(input_source_ids, dtype=torch.int64)[None],
            "target_ids": torch.tensor(target_ids, dtype=torch.int64)[None],
        }
        return out

    # ------------------------------------------------------------------------------------------------------ inference
    def encode(self, speech, speech_lengths):
        out = self.audio_encoder(speech, speech_lengths)
        return out[0], out[1]

    def inference_prepare(self, data_in, data_lengths=None, key=None, tokenizer=None, frontend=None, **kwargs):
        """one clip (a ChatML turn list) -> (inputs_embeds [1, rows, hidden] on the device, contents, batch, source_ids, meta_data)"""
        if len(data_in) > 1:
            raise NotImplementedError("inference_prepare takes one clip; FunASRNano.inference batches a list through the LM")
        if _truthy(kwargs.get("teacherforcing", False)):
            _refuse("teacherforcing: true")
        meta_data = {}
        contents = self.data_template(data_in[0])
        batch = self.data_load_speech(contents, tokenizer, frontend, meta_data=meta_data, **kwargs)
        source_ids = batch["source_ids"].clamp(min=0)
        embeds = self.llm.embed(source_ids[0])
        if len(batch["speech"]) > 0:
            lens = batch["speech_lengths"][:, 0]
            encoder_out, encoder_out_lens = self.encode(batch["speech"], lens)
            adaptor_out, adaptor_out_lens = self.audio_adaptor(encoder_out, encoder_out_lens)
            meta_data.update(encoder_out=encoder_out, encoder_out_lens=encoder_out_lens, audio_adaptor_out=adaptor_out,
                             audio_adaptor_out_lens=adaptor_out_lens)
            speech_idx = 0
            for turn, beg in enumerate(batch["fbank_beg"][0].clamp(min=0).tolist()):
                if beg <= 0:
                    continue
                n = max(int(batch["fake_token_len"][0, turn]), 0)
                if beg + n > embeds.shape[0] or n > adaptor_out.shape[1]:      # (the reference falls back to the adaptor's own length)
                    n = min(int(adaptor_out_lens[speech_idx]), embeds.shape[0] - beg)
                embeds[beg:beg + n] = adaptor_out[speech_idx, :n]
                speech_idx += 1
        return embeds[None], contents, batch, source_ids, meta_data

    def inference(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        if isinstance(data_in, torch.Tensor) and kwargs.get("data_type", "sound") == "fbank":
            data_in = [data_in] if data_in.dim() < 3 else list(data_in)
        prompt = self.get_prompt(kwargs.get("hotwords", []), kwargs.get("language", None), kwargs.get("itn", True))
        turns = [self.generate_chatml(prompt, data) for data in data_in]
        if key is None:
            chars = string.ascii_letters + string.digits
            key = ["rand_key_" + "".join(random.choice(chars) for _ in range(13)) for _ in turns]
        return self.inference_llm(turns, data_lengths=data_lengths, key=key, tokenizer=tokenizer, frontend=frontend, **kwargs)

    def inference_llm(self, data_in, data_lengths=None, key: list = None, tokenizer=None, frontend=None, **kwargs):
        if _truthy(kwargs.get("teacherforcing", False)):
            _refuse("teacherforcing: true")
        check_llm_dtype(kwargs)
        check_llm_kwargs(kwargs.get("llm_kwargs", {}))
        if key is not None and len(key) > 0 and isinstance(key[0], (list, tuple)):
            key = list(key[0])
        embeds, labels, meta_data = [], [], {}
        for i, turn in enumerate(data_in):
            emb, contents, _batch, _src, meta_i = self.inference_prepare([turn], data_lengths, None, tokenizer, frontend, **kwargs)
            embeds.append(emb[0])
            labels.append(contents["assistant"][-1])
            for name, value in meta_i.items():
                if isinstance(value, (int, float)) and not isinstance(value, bool):
                    meta_data[name] = meta_data.get(name, 0.0) + value
                elif name not in meta_data:
                    meta_data[name] = value
        cfg = self.llm.config
        pad = cfg.get("pad_token_id") or (self.llm.eos_token_ids[0] if self.llm.eos_token_ids else 0)
        ids = self.llm.generate(embeds, max_new_tokens=int(kwargs.get("max_length", 512)), pad_token_id=pad)
        texts = tokenizer.batch_decode(ids, skip_special_tokens=kwargs.get("skip_special_tokens", True))
        writer = None
        if kwargs.get("output_dir") is not None:
            if not hasattr(self, "writer"):
                self.writer = DatadirWriter(kwargs.get("output_dir"))
            writer = self.writer["1best_recog"]
        results = []
        for i, response in enumerate(texts):
            response = kwargs.get("prev_text", "") + response if kwargs.get("prev_text") else response
            k = key[i] if key is not None and i < len(key) else f"rand_{i}"
            clean = re.sub(r"[^\w\s\u3000\u4e00-\u9fff]+", "", response)
            results.append({"key": k, "text": re.sub(r"\s+", " ", response.replace("/sil", " ")), "text_tn": clean, "label": labels[i]})
            if writer is not None:
                writer["text"][k] = response.replace("\n", " ")
                writer["label"][k] = labels[i].replace("\n", " ")
                writer["text_tn"][k] = clean
        return results, meta_data
