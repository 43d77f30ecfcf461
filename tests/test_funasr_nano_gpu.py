"""Fun-ASR-Nano on the MI355X: the `Transformer` adaptor against its golden, the Qwen3 decoder handle (prefill, decode steps over the KV
cache, the greedy loop, ragged batches) against the float64 oracle and the goldens of tools/make_golden_funasr_nano.py, and
`FunASRNano.inference` / `AutoModel.generate` end to end on a synthetic model directory.

Bars: logits within 4 x e_ref, the largest |upstream Qwen3ForCausalLM in float32 - oracle in float64| over all golden steps (stored by
the tool); the adaptor within 4 x gap_adaptor, the reference adaptor's own float32 - float64 gap. Ids are compared for equality: the tool
only stores cases whose every step has a best-minus-second gap of at least 64 x e_ref."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd.qwen3 import Qwen3Decoder

from . import _funasr_nano_fixtures as X
from . import _qwen3_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "funasr_nano.json"), encoding="utf-8") as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "funasr_nano.npz"))


def _lm(name, rec, cuda):
    """(config, weights, prompts, device module) of one golden LM"""
    c = O.tiny_config(name)
    c["eos_token_id"] = rec["eos_token_id"]
    sd = O.seeded_state_dict(c, rec["seed"])
    prompts = [O.seeded_prompt(c, rec["seed"] * 10 + i, n) for i, n in enumerate(rec["rows"])]
    m = Qwen3Decoder(c)
    m.load_state_dict(sd, strict=True)
    return c, sd, prompts, m.to(cuda)


def _close(tag, got, ref, bar):
    d = float((got.double().cpu() - ref).abs().max())
    print(f"{tag}: max |d| {d:.3e}, bar {bar:.3e}, ratio {d / bar:.3f}")
    assert torch.isfinite(got).all() and d <= bar, (tag, d, bar)


def test_adaptor_against_its_golden(cuda, golden):
    from funasr_amd.fun_asr_nano import TransformerAdaptor
    meta, arr = golden
    a = TransformerAdaptor(**meta["adaptor_conf"])
    a.load_state_dict(X.adaptor_state_dict(meta["adaptor_seed"], meta["adaptor_conf"]), strict=True)
    a = a.to(cuda)
    out, olens = a(torch.from_numpy(arr["adaptor_x"]).to(cuda), torch.from_numpy(arr["adaptor_ilens"]))
    assert olens.tolist() == arr["adaptor_olens"].tolist()
    ref = torch.from_numpy(arr["adaptor_out"])
    for b, n in enumerate(olens.tolist()):
        _close(f"adaptor clip {b}", out[b, :n], ref[b, :n], 4 * meta["gap_adaptor"])


@pytest.mark.parametrize("name", list(O.TINY))
def test_prefill_logits_and_stepwise_decoding(cuda, golden, name):
    meta, arr = golden
    rec, bar = meta["lm"][name], 4 * meta["e_ref"]
    c, sd, prompts, m = _lm(name, rec, cuda)
    # one ragged batch: every row's logits against the oracle's forward, the last rows against the golden step 0
    first, logits = m.prefill(prompts, rec["max_new_tokens"], return_logits=True)
    for i, x in enumerate(prompts):
        _close(f"{name} prefill clip {i}", logits[i], O.forward(sd, c, x), bar)
        _close(f"{name} prefill clip {i} last row vs golden", logits[i][-1], torch.from_numpy(arr[f"{name}_logits_{i}"][0]), bar)
        assert first[i] == rec["ids"][i][0]
    # decode steps of the batch over the cache: each step's logits are those of one prefill over the whole sequence
    emb = sd["model.embed_tokens.weight"]
    ids, seqs = list(first), [[t] for t in first]
    step_logits = []
    for _ in range(4):
        ids, lg = m.step(ids, return_logits=True)
        step_logits.append(lg.clone())
        for b, t in enumerate(ids):
            seqs[b].append(t)
    full = [torch.cat([x] + [emb[t][None] for t in seqs[b][:-1]], 0) for b, x in enumerate(prompts)]
    _, whole = m.prefill(full, 0, return_logits=True)
    for b, x in enumerate(prompts):
        ref = O.forward(sd, c, full[b])
        for k, lg in enumerate(step_logits):
            row = x.shape[0] + k
            _close(f"{name} clip {b} step {k} vs one prefill", lg[b], whole[b][row].double().cpu(), bar)
            _close(f"{name} clip {b} step {k} vs oracle", lg[b], ref[row], bar)


@pytest.mark.parametrize("name", list(O.TINY))
def test_greedy_ids_equal_the_goldens_alone_and_batched(cuda, golden, name):
    meta, _ = golden
    rec = meta["lm"][name]
    c, sd, prompts, m = _lm(name, rec, cuda)
    n_max, eos = rec["max_new_tokens"], rec["eos_token_id"]
    assert any(ids[-1] == eos and len(ids) < n_max for ids in rec["ids"]), "no golden run stops at eos"
    assert any(len(ids) == n_max and eos not in ids for ids in rec["ids"]), "no golden run stops at max_new_tokens"
    alone = []
    for i, x in enumerate(prompts):
        m.prefill([x], n_max)
        out = m.greedy(n_max)
        assert out.shape == (1, len(rec["ids"][i])), "the loop ends with its only sequence, or at max_new_tokens"
        assert out[0].tolist() == rec["ids"][i], (name, i)
        alone.append(out[0].tolist())
    m.debug_poison()
    m.prefill(prompts, n_max)                                # B = 3, three lengths; clip 0 finishes first and is frozen
    out = m.greedy(n_max, pad_token_id=96)
    assert out.shape == (3, max(len(a) for a in alone))
    for i, a in enumerate(alone):
        assert out[i, :len(a)].tolist() == a, (name, i)
        assert (out[i, len(a):] == 96).all(), "a finished sequence emits the pad id"
    assert m.generate(prompts, n_max) == alone
    short = m.generate(prompts[1:], 3)                       # stops at max_new_tokens
    assert short == [a[:3] for a in alone[1:]]


def test_handle_refuses_what_it_cannot_hold(cuda, golden):
    from funasr_amd import _lib
    meta, _ = golden
    _, _, prompts, m = _lm("hd64_g2", meta["lm"]["hd64_g2"], cuda)
    m.prefill(prompts[:1], 1)
    m.greedy(1)
    with pytest.raises(_lib.HipRuntimeError, match="reserved"):
        m.greedy(5)
    with pytest.raises(ValueError, match="1 .. 16"):
        m.prefill([prompts[0]] * 17, 1)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    if not X.HAVE_TRANSFORMERS:
        pytest.skip("the transformers package is not installed (the tokenizer of the model directory)")
    from funasr_amd.fun_asr_nano import FunASRNano
    root = tmp_path_factory.mktemp("funasr_nano")
    llm_dir = X.write_llm_dir(str(root / "probe_llm"))
    probe = FunASRNano(**X.model_conf(llm_dir))
    sd = X.encoder_state_dict(probe, 21)
    c = O.tiny_config("hd64_g2")
    lm_sd = O.seeded_state_dict(c, 1)
    sd.update({"llm." + k: v for k, v in lm_sd.items()})
    sd["ctc_decoder.linear.weight"] = torch.zeros(3, 3)      # a checkpoint of a model with a CTC decoder: skipped on load
    assert sorted(k for k in sd if not k.startswith("ctc_decoder.")) == sorted(probe.state_dict())
    return X.write_model_dir(str(root / "model"), sd, low_frame_rate=True), c, lm_sd


def _expected_records(am, c, lm_sd, feats_list, keys, max_length, prev_text=None, hotwords=()):
    """records assembled from the ORACLE's ids: the device encoder's output (tested elsewhere) through the float64 adaptor and LM"""
    import re
    model, tok = am.model, am.kwargs["tokenizer"]
    ad_sd = {k[len("audio_adaptor."):]: v.cpu() for k, v in model.state_dict().items() if k.startswith("audio_adaptor.")}
    prompt = model.get_prompt(list(hotwords), None, True)
    out = []
    for feats, key in zip(feats_list, keys):
        enc, _ = model.encode(feats[None], [feats.shape[0]])
        ad, olen = O.adaptor(ad_sd, enc[0].cpu(), feats.shape[0], X.ADAPTOR_CONF["downsample_rate"], X.ADAPTOR_CONF["attention_heads"])
        source = f"<|im_start|>system\nYou are a helpful assistant.<|im_end|>\n<|im_start|>user\n{prompt}"
        head = tok.encode(source)
        tail = tok.encode("<|im_end|>\n<|im_start|>assistant\n" + (prev_text or ""))
        emb = lm_sd["model.embed_tokens.weight"].double()
        fake = model.fake_token_len(feats.shape[0])             # placeholders in the prompt; the first `fake` adaptor rows replace them
        if fake <= ad.shape[0]:
            speech = ad[:fake]
        else:                                                   # more placeholders than adaptor rows: the reference's fallback writes
            speech = torch.cat((ad[:olen], emb[[0] * (fake - olen)]), 0)      # the adaptor's own length, the rest stay token 0
        x = torch.cat((emb[head], speech, emb[tail]), 0)
        ids, logits = O.greedy(lm_sd, c, x, max_length, eos=(c["eos_token_id"],))
        assert O.top2_gap(logits) > 1e-2, "this clip's arg-max is too close a call for an equality test: change its seed"
        text = (prev_text or "") + tok.batch_decode([ids], skip_special_tokens=True)[0]
        out.append({"key": key, "text": re.sub(r"\s+", " ", text.replace("/sil", " ")), "text_tn": re.sub(r"[^\w\s\u3000\u4e00-\u9fff]+", "", text),
                    "label": "null"})
    return out


def test_auto_model_end_to_end_sound_and_fbank(cuda, model_dir, tmp_path):
    from funasr_amd.auto_model import AutoModel
    path, c, lm_sd = model_dir
    am = AutoModel(model=path, device="cuda:0", disable_update=True)
    assert type(am.model).__name__ == "FunASRNano" and am.model.audio_adaptor.linear1.weight.is_cuda
    fe = am.kwargs["frontend"]
    waves = [torch.randn(16000 + 1600 * i, generator=torch.Generator().manual_seed(40 + i)) * 0.1 for i in range(3)]
    feats = []
    for w in waves:
        f, n = fe(w[None].to(cuda), [w.shape[0]])
        feats.append(f[0, : int(torch.as_tensor(n).reshape(-1)[0])])
    keys = ["a", "b", "c"]
    want = _expected_records(am, c, lm_sd, feats, keys, 6)
    out_dir = str(tmp_path / "out")
    got = am.generate(input=waves, key=keys, batch_size=3, max_length=6, output_dir=out_dir)       # one batch of three lengths
    assert got == want
    assert am.generate(input=waves[1], key=["b"], max_length=6) == want[1:2]                        # each clip is what it gets alone
    assert am.generate(input=feats[2].cpu(), key=["c"], data_type="fbank", max_length=6) == want[2:]
    for name, field in (("text", "text"), ("label", "label"), ("text_tn", "text_tn")):
        with open(os.path.join(out_dir, "1best_recog", name), encoding="utf-8") as f:
            lines = f.read().splitlines()
        assert len(lines) == 3 and lines[0].startswith("a")
    # FunASRNano.inference itself, with prev_text and hotwords in the prompt, and one placeholder per frame (use_low_frame_rate off)
    am.model.use_low_frame_rate = False
    want2 = _expected_records(am, c, lm_sd, feats[:2], keys[:2], 5, prev_text="ab", hotwords=["中文"])
    got2, _ = am.model.inference(waves[:2], key=keys[:2], tokenizer=am.kwargs["tokenizer"], frontend=fe, device="cuda:0", max_length=5,
                                 prev_text="ab", hotwords=["中文"])
    assert got2 == want2
