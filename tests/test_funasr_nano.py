"""Fun-ASR-Nano without a GPU: registry entries, state-dict keys, prompt and ChatML assembly against what the reference recorded
(tests/golden/funasr_nano.json, written by tools/make_golden_funasr_nano.py), the float64 oracle against upstream Qwen3ForCausalLM, the
goldens' close-call condition, every refusal by name, the synthetic tokenizer, and AutoModel on a synthetic model directory up to the
point where the device is needed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from funasr_amd.fun_asr_nano import FunASRNano, TransformerAdaptor, check_llm_kwargs
from funasr_amd.qwen3 import Qwen3Decoder, read_lm_config, rope_table
from funasr_amd.register import tables

from . import _funasr_nano_fixtures as X
from . import _qwen3_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "funasr_nano.json"), encoding="utf-8") as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "funasr_nano.npz"))


needs_transformers = pytest.mark.skipif(not X.HAVE_TRANSFORMERS, reason="the transformers package is not installed")


@pytest.fixture(scope="module")
def llm_dir(tmp_path_factory):
    """the LM's config.json alone: building the model needs nothing else, and no `transformers`"""
    return X.write_llm_config(str(tmp_path_factory.mktemp("llm")))


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return X.write_llm_dir(str(tmp_path_factory.mktemp("llm_tok")))


@pytest.fixture(scope="module")
def model(llm_dir):
    return FunASRNano(**X.model_conf(llm_dir))


def test_registry_entries_and_install():
    from funasr_amd.install import hip_classes, install
    assert tables.model_classes["FunASRNano"] is FunASRNano and tables.adaptor_classes["Transformer"] is TransformerAdaptor
    assert {"Linear", "QFormer"} <= set(tables.adaptor_classes) and "HuggingfaceTokenizer" in tables.tokenizer_classes
    have = {(t, k) for t, k, _ in hip_classes()}
    assert {("model_classes", "FunASRNano"), ("adaptor_classes", "Transformer"), ("tokenizer_classes", "HuggingfaceTokenizer")} <= have

    class Sink:
        def __init__(self):
            self.got = set()

        def register(self, table, key=None):
            self.got.add((table, key))
            return lambda cls: cls

    s = Sink()
    install(s)
    assert ("adaptor_classes", "Transformer") in s.got and ("model_classes", "FunASRNano") in s.got
    assert not any(t == "tokenizer_classes" for t, _ in s.got)


def test_state_dict_keys_and_shapes_are_the_references(model, golden):
    meta, _ = golden
    mine = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert mine == meta["state_dict"]
    assert list(Qwen3Decoder(O.tiny_config("hd128_g1")).state_dict()) == O.state_dict_keys(O.tiny_config("hd128_g1"))


class _Recording:
    def __init__(self, tok):
        self.tok, self.calls = tok, []

    def encode(self, s):
        self.calls.append(s)
        return self.tok.encode(s)


def test_prompt_and_chatml_assembly_against_the_reference(model, golden):
    meta, _ = golden
    tok = X.CharTokenizer()                                  # the synthetic tokenizer's encode (test_tokenizer_class checks that it is)
    fe = X.StubFrontend()
    assert len(meta["prompts"]) >= 5
    for n, case in enumerate(meta["prompts"]):
        model.use_low_frame_rate = case["low_frame_rate"]
        assert model.get_prompt(case["hotwords"], case["language"], case["itn"]) == case["prompt"]
        turns = model.generate_chatml(case["prompt"], X.clip(n, case["frames"]))
        contents = model.data_template(turns)
        assert contents["assistant"][-1] == case["label"] and contents["system"] == ["You are a helpful assistant."]
        rt = _Recording(tok)
        kw = {} if case["prev_text"] is None else {"prev_text": case["prev_text"]}
        b = model.data_load_speech(contents, rt, fe, meta_data={}, **kw)
        assert rt.calls == case["encode_calls"]
        assert b["input_ids"][0].tolist() == case["input_ids"] and b["source_ids"][0].tolist() == case["source_ids"]
        assert b["labels_ids"].tolist() == case["labels_ids"] and [int(v) for v in b["fbank_mask"][0].tolist()] == case["fbank_mask"]
        assert b["fbank_beg"][0].tolist() == case["fbank_beg"] and b["fake_token_len"][0].tolist() == case["fake_token_len"]
        assert b["speech_lengths"].reshape(-1).tolist() == case["speech_lengths"] == [case["frames"]]
        assert b["attention_mask"].shape == b["input_ids"].shape and b["speech"].shape[:2] == (1, case["frames"])
    path_turn = model.generate_chatml("p", "/some/clip.wav")
    assert path_turn[1]["content"] == "p<|startofspeech|>!/some/clip.wav<|endofspeech|>" and "audio" not in path_turn[1]
    model.use_low_frame_rate = False


def _upstream(c, sd):
    if not X.HAVE_TRANSFORMERS:
        pytest.skip("the transformers package is not installed")
    import transformers
    if not hasattr(transformers, "Qwen3Config"):
        pytest.skip("this transformers has no Qwen3")
    cfg = transformers.Qwen3Config(**{k: v for k, v in c.items() if k not in ("model_type", "architectures")})
    m = transformers.AutoModelForCausalLM.from_config(cfg).float().eval()
    m.load_state_dict(sd, strict=True)
    return m


@pytest.mark.parametrize("name", list(O.TINY))
def test_oracle_against_upstream_and_the_close_call_condition(golden, name):
    meta, arr = golden
    rec, e_ref = meta["lm"][name], meta["e_ref"]
    c = O.tiny_config(name)
    c["eos_token_id"] = rec["eos_token_id"]
    sd = O.seeded_state_dict(c, rec["seed"])
    m = _upstream(c, sd)
    emb = sd["model.embed_tokens.weight"]
    for i, n in enumerate(rec["rows"]):
        x = O.seeded_prompt(c, rec["seed"] * 10 + i, n)
        ids, logits = O.greedy(sd, c, x, rec["max_new_tokens"], eos=(rec["eos_token_id"],))
        assert ids == rec["ids"][i]
        gold = torch.from_numpy(arr[f"{name}_logits_{i}"])
        assert torch.equal(logits, gold), "the stored logits are the oracle's, bit for bit"
        assert O.top2_gap(gold) >= 64 * e_ref, "a golden step is too close a call"
        full = torch.cat([x] + [emb[t][None] for t in ids[:-1]], 0)
        with torch.no_grad():
            up = m(inputs_embeds=full[None]).logits[0, n - 1:].double()
            gen = m.generate(inputs_embeds=x[None], max_new_tokens=rec["max_new_tokens"], do_sample=False, pad_token_id=rec["eos_token_id"])
        d = float((up - gold).abs().max())
        print(f"{name} prompt {i}: |upstream fp32 - oracle| {d:.3e}, e_ref {e_ref:.3e}")
        assert d <= 4 * e_ref and gen[0].tolist() == ids
        d32 = float((O.forward(sd, c, full, torch.float32)[n - 1:].double() - gold).abs().max())
        assert d32 <= 4 * e_ref


@needs_transformers
def test_rope_table_is_upstreams(llm_dir):
    import transformers
    if not hasattr(transformers, "Qwen3Config"):
        pytest.skip("this transformers has no Qwen3")
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RotaryEmbedding
    cfg = transformers.AutoConfig.from_pretrained(llm_dir)
    pos = torch.tensor([[0, 1, 77, 4095]])
    cos, sin = Qwen3RotaryEmbedding(cfg)(torch.zeros(1, 4, 128), pos)
    mine_c, mine_s = rope_table(64, 1000000.0, 4096)
    assert torch.equal(cos[0, :, :32], mine_c[pos[0]]) and torch.equal(sin[0, :, 32:], mine_s[pos[0]])


def test_lm_config_reading(llm_dir, tmp_path):
    conf = read_lm_config(llm_dir)
    m = Qwen3Decoder(conf)
    assert (m.head_dim, m.num_heads, m.num_kv_heads, m.rope_theta, m.eos_token_ids) == (64, 4, 2, 1000000.0, [3])
    for where in ("rope_parameters", "rope_scaling"):       # theta inside a sub-dict, none at the top level
        c = {k: v for k, v in O.tiny_config("hd64_g2").items() if k != "rope_theta"}
        c[where] = {"rope_theta": 5000.0, "rope_type": "default"}
        assert Qwen3Decoder(c).rope_theta == 5000.0
    with pytest.raises(FileNotFoundError, match="config.json"):
        read_lm_config(str(tmp_path / "nothing"))


@pytest.mark.parametrize("change,match", [
    (dict(model_type="qwen2"), "model_type: qwen2"),
    (dict(attention_bias=True), "attention_bias: true"),
    (dict(use_sliding_window=True, sliding_window=128), "sliding window"),
    (dict(layer_types=["full_attention", "sliding_attention"]), "sliding window"),
    (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), "rope type: yarn"),
    (dict(hidden_act="gelu"), "hidden_act: gelu"),
    (dict(head_dim=96), "head_dim: 96"),
    (dict(hidden_size=120), "hidden_size: 120"),
    (dict(intermediate_size=100), "intermediate_size: 100"),
    (dict(num_key_value_heads=3), "num_key_value_heads: 3"),
])
def test_lm_refusals_by_name(change, match):
    with pytest.raises(NotImplementedError, match=match):
        Qwen3Decoder(dict(O.tiny_config("hd64_g2"), **change))


def test_model_refusals_by_name(llm_dir, model):
    def conf(**over):
        c = X.model_conf(llm_dir)
        for k, v in over.items():
            c[k] = dict(c[k], **v) if isinstance(v, dict) and isinstance(c.get(k), dict) else v
        return c

    for over, match in ((dict(audio_encoder_conf=dict(hub="ms")), "hub: ms"), (dict(llm_conf=dict(llm_dtype="bf16")), "llm_dtype: bf16"),
                        (dict(llm_conf=dict(use_lora=True)), "use_lora"), (dict(audio_adaptor="Linear"), "Linear"),
                        (dict(audio_adaptor="QFormer"), "QFormer"), (dict(audio_adaptor_conf=dict(attention_heads=4)), "attention_heads: 4")):
        with pytest.raises(NotImplementedError, match=match):
            FunASRNano(**conf(**over))
    for kwargs, match in ((dict(teacherforcing=True), "teacherforcing"), (dict(llm_dtype="fp16"), "llm_dtype: fp16"), (dict(bf16=True), "bf16"),
                          (dict(fp16=True), "fp16"), (dict(llm_kwargs=dict(do_sample=True)), "llm_kwargs.do_sample"),
                          (dict(llm_kwargs=dict(num_beams=4)), "llm_kwargs.num_beams"),
                          (dict(llm_kwargs=dict(repetition_penalty=1.2)), "llm_kwargs.repetition_penalty")):
        with pytest.raises(NotImplementedError, match=match):
            model.inference([torch.zeros(4000)], tokenizer=None, frontend=X.StubFrontend(), **kwargs)
    check_llm_kwargs(dict(do_sample=False, num_beams=1))                # what leaves the search greedy passes


def test_ctc_decoder_is_announced_and_not_built(llm_dir, caplog):
    import logging
    with caplog.at_level(logging.WARNING):
        m = FunASRNano(**X.model_conf(llm_dir), ctc_decoder="Transformer", ctc_vocab_size=50)
    assert m.ctc_decoder is None and any("ctc_decoder" in r.message and "not built" in r.message for r in caplog.records)
    assert not any(k.startswith(("ctc_decoder.", "ctc.")) for k in m.state_dict())


def test_fake_token_len_formulas(model):
    model.use_low_frame_rate = True
    assert [model.fake_token_len(n) for n in (1, 2, 3, 8, 9, 100)] == [((1 + (1 + (n - 1) // 2 - 1) // 2) - 1) // 2 + 1 for n in (1, 2, 3, 8, 9, 100)]
    model.use_low_frame_rate = False
    assert model.fake_token_len(37) == 37


@needs_transformers
def test_tokenizer_class(tok_dir, tmp_path, monkeypatch, golden):
    llm_dir = tok_dir
    make = tables.tokenizer_classes["HuggingfaceTokenizer"]
    tok = make(init_param_path=llm_dir)
    for case in golden[0]["prompts"]:                        # the plain-Python encode of the assembly test is this tokenizer's
        for text in case["encode_calls"] + ["<unk>?\t<|endoftext|>"]:
            assert X.CharTokenizer().encode(text) == tok.encode(text)
    ids = tok.encode("<|im_start|>user\n语音转写：<|im_end|>")
    assert ids[0] == X.SPECIALS.index("<|im_start|>") and ids[-1] == 3 and max(ids) < 97
    assert tok.batch_decode([ids], skip_special_tokens=True) == ["user\n语音转写："]
    with pytest.raises(FileNotFoundError, match="local directory"):
        make(init_param_path="Qwen/Qwen3-0.6B")                          # a hub name: refused, never looked up
    monkeypatch.setitem(sys.modules, "transformers", None)
    with pytest.raises(ImportError, match="transformers"):
        make(init_param_path=llm_dir)


@needs_transformers
def test_auto_model_builds_from_a_model_directory_up_to_the_device(tmp_path, model):
    from funasr_amd.auto_model import AutoModel, load_model_dir
    sd = X.encoder_state_dict(model, 3)
    sd.update({"llm." + k: v for k, v in O.seeded_state_dict(O.tiny_config("hd64_g2"), 1).items()})
    sd["ctc.ctc_lo.weight"] = torch.zeros(2, 2)                          # keys of a CTC head: skipped on load
    path = X.write_model_dir(str(tmp_path / "model"), sd, low_frame_rate=True)
    kw = load_model_dir(path)
    assert kw["llm_conf"]["init_param_path"] == os.path.join(path, "llm") == kw["tokenizer_conf"]["init_param_path"]
    am = AutoModel(model=path, device="cpu")
    assert isinstance(am.model, FunASRNano) and am.model.use_low_frame_rate and am.kwargs["tokenizer"].eos_token == "<|im_end|>"
    got = am.model.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items() if not k.startswith("ctc."))
    with pytest.raises(RuntimeError, match="no GPU visible|AMD GPU"):       # the frontend without a GPU, else the model on the cpu
        am.generate(input=torch.zeros(8000), max_length=4)
