"""Writes tests/golden/funasr_nano.json and tests/golden/funasr_nano.npz (CPU; needs the reference tree and `transformers`).

From the reference's own `FunASRNano` and `Transformer` adaptor (imported read-only through oracle.ref_import) at the tiny size of
tests/_funasr_nano_fixtures.py:
  state_dict         key -> shape of FunASRNano (SenseVoiceEncoderSmall + Transformer adaptor + the tiny Qwen3)
  prompts            per case (hotwords, language, itn, prev_text, use_low_frame_rate, clip frames): what get_prompt / generate_chatml /
                     data_template / data_load_speech return -- the prompt, the strings handed to tokenizer.encode in order (the
                     source string around the speech span, then the target), input_ids, source_ids, labels_ids, fbank_mask,
                     fbank_beg, fake_token_len, speech_lengths -- with the synthetic tokenizer and the stand-in frontend
  adaptor_*          the adaptor on a tiny input in float64, gap_adaptor = max |float32 - float64| of the reference itself
From upstream `Qwen3ForCausalLM` (float32, CPU) and the float64 oracle (tests/_qwen3_oracle.py), per tiny LM (head_dim 64 with groups of 2,
head_dim 128 with groups of 1 and of 4), seeded weights (the seed is stored, never the weights) and three seeded prompts:
  lm.<name>          seed, eos_token_id, prompt rows, max_new_tokens, the oracle's greedy ids per prompt
  <name>_logits_<p>  the oracle's float64 logits of every generated step
  e_ref              the largest |upstream float32 - oracle float64| logit over all golden steps
The eos id of an LM is one the first prompt's free run emits after a few steps, so one golden run stops at eos and the others at
max_new_tokens. Seeds are probed until EVERY generated step of every case has a best-minus-second logit gap of at least 64 x e_ref
and every run holds at least three distinct ids."""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _funasr_nano_fixtures as X  # noqa: E402
from tests import _qwen3_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PROMPT_ROWS = (9, 5, 14)
MAX_NEW = 12
MIN_DISTINCT = 3          # distinct ids every golden run must hold
PROMPT_CASES = [
    dict(hotwords=[], language=None, itn=True, prev_text=None, low_frame_rate=False, frames=7),
    dict(hotwords=["中文", "语音"], language=None, itn=True, prev_text=None, low_frame_rate=False, frames=12),
    dict(hotwords=[], language="中文", itn=False, prev_text=None, low_frame_rate=True, frames=23),
    dict(hotwords=["a", "b c"], language="英文", itn=True, prev_text="上文 ", low_frame_rate=True, frames=40),
    dict(hotwords=[], language=None, itn=False, prev_text="ab", low_frame_rate=False, frames=3),
]


class RecordingTokenizer:
    def __init__(self, tok):
        self.tok, self.calls = tok, []

    def encode(self, s):
        self.calls.append(s)
        return self.tok.encode(s)


def upstream(c: dict, sd: dict):
    from transformers import AutoModelForCausalLM, Qwen3Config
    cfg = Qwen3Config(**{k: v for k, v in c.items() if k not in ("model_type", "architectures")})
    m = AutoModelForCausalLM.from_config(cfg).float().eval()
    m.load_state_dict(sd, strict=True)
    return m


def lm_case(name: str, seed: int):
    """-> (record, arrays, e_ref, smallest gap) of one tiny LM at one seed"""
    c = O.tiny_config(name)
    sd = O.seeded_state_dict(c, seed)
    prompts = [O.seeded_prompt(c, seed * 10 + i, n) for i, n in enumerate(PROMPT_ROWS)]
    free, _ = O.greedy(sd, c, prompts[0], MAX_NEW, eos=())
    eos = next((t for i, t in enumerate(free) if i >= 3 and t not in free[:i]), None)
    if eos is None:
        return None
    c["eos_token_id"] = eos
    m = upstream(c, sd)
    rec, arrays, e_ref, gap = dict(seed=seed, eos_token_id=eos, rows=list(PROMPT_ROWS), max_new_tokens=MAX_NEW, ids=[]), {}, 0.0, float("inf")
    for i, x in enumerate(prompts):
        ids, logits = O.greedy(sd, c, x, MAX_NEW, eos=(eos,))
        emb = sd["model.embed_tokens.weight"]
        full = torch.cat([x] + [emb[t][None] for t in ids[:-1]], 0)
        with torch.no_grad():
            up = m(inputs_embeds=full[None]).logits[0, x.shape[0] - 1:].double()
            gen = m.generate(inputs_embeds=x[None], max_new_tokens=MAX_NEW, do_sample=False, pad_token_id=eos)[0].tolist()
        assert gen == ids, (name, seed, i, gen, ids)
        e_ref = max(e_ref, float((up - logits).abs().max()))
        gap = min(gap, O.top2_gap(logits))
        if len(set(ids)) < MIN_DISTINCT:      # a run that repeats one id would not notice a step that reads a stale position
            return None
        rec["ids"].append(ids)
        arrays[f"{name}_logits_{i}"] = logits.numpy()
    return rec, arrays, e_ref, gap


def reference_parts(tmp: str):
    # transformers loads its modules lazily and probes optional packages as it does: everything the reference will touch is loaded
    # BEFORE the stand-in modules of ref_import (torchaudio, soundfile, ..) exist
    from transformers import AutoConfig, AutoModelForCausalLM, AutoTokenizer
    llm_dir = X.write_llm_dir(os.path.join(tmp, "llm"))
    AutoModelForCausalLM.from_config(AutoConfig.from_pretrained(llm_dir))
    tok = AutoTokenizer.from_pretrained(llm_dir)
    from oracle import ref_import
    ref_import.install()
    if "torchaudio.functional" not in sys.modules:      # the model file imports it for its CTC timestamps, which nothing here runs
        import types
        sys.modules["torchaudio.functional"] = types.ModuleType("torchaudio.functional")
        sys.modules["torchaudio"].functional = sys.modules["torchaudio.functional"]
    import funasr.models.llm_asr.adaptor  # noqa: F401  (registers the adaptors)
    import funasr.models.sense_voice.model  # noqa: F401  (registers SenseVoiceEncoderSmall)
    from funasr.models.fun_asr_nano.model import FunASRNano
    from funasr.register import tables

    out, arrays = {}, {}
    model = FunASRNano(**X.model_conf(llm_dir))
    out["state_dict"] = {k: list(v.shape) for k, v in model.state_dict().items()}
    fe = X.StubFrontend()
    out["prompts"] = []
    for n, case in enumerate(PROMPT_CASES):
        model.use_low_frame_rate = case["low_frame_rate"]
        rt = RecordingTokenizer(tok)
        prompt = model.get_prompt(case["hotwords"], case["language"], case["itn"])
        contents = model.data_template(model.generate_chatml(prompt, X.clip(n, case["frames"])))
        kw = {} if case["prev_text"] is None else {"prev_text": case["prev_text"]}
        b = model.data_load_speech(contents, rt, fe, meta_data={}, **kw)
        out["prompts"].append(dict(case, prompt=prompt, encode_calls=rt.calls, input_ids=b["input_ids"][0].tolist(),
                                   source_ids=b["source_ids"][0].tolist(), labels_ids=b["labels_ids"].tolist(),
                                   fbank_mask=[int(v) for v in b["fbank_mask"][0].tolist()], fbank_beg=b["fbank_beg"][0].tolist(),
                                   fake_token_len=b["fake_token_len"][0].tolist(), speech_lengths=b["speech_lengths"].reshape(-1).tolist(),
                                   label=contents["assistant"][-1]))
    # the adaptor on a tiny input: two clips of 9 and 6 encoder frames (an odd count: one zero frame is stacked on)
    conf = dict(X.ADAPTOR_CONF)
    adaptor = tables.adaptor_classes.get("Transformer")(**conf).eval()
    sd = X.adaptor_state_dict(7)
    assert sorted(sd) == sorted(adaptor.state_dict()), "the fixture's adaptor keys are not the reference's"
    adaptor.load_state_dict(sd, strict=True)
    x = torch.randn(2, 9, conf["encoder_dim"], generator=torch.Generator().manual_seed(9))
    x[1, 6:] = 0.0
    ilens = torch.tensor([9, 6])
    with torch.no_grad():
        y32, olens = adaptor(x, ilens)
        y64, _ = adaptor.double()(x.double(), ilens)
    for b in range(2):
        mine, ol = O.adaptor(sd, x[b], int(ilens[b]), conf["downsample_rate"], conf["attention_heads"])
        assert ol == int(olens[b]) and float((mine[:ol] - y64[b, :ol]).abs().max()) < 1e-10, "the oracle's adaptor is not the reference's"
    arrays.update(adaptor_x=x.numpy(), adaptor_ilens=ilens.numpy(), adaptor_olens=olens.numpy(), adaptor_out=y64.numpy())
    out["gap_adaptor"] = float((y32.double() - y64).abs().max())
    out["adaptor_seed"], out["adaptor_conf"] = 7, conf
    return out, arrays


def main():
    out, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        ref, ref_arrays = reference_parts(tmp)
    out.update(ref)
    arrays.update(ref_arrays)
    out["lm"], e_ref, picked = {}, 0.0, {}
    for name in O.TINY:
        for seed in range(1, 400):
            got = lm_case(name, seed)
            if got is None:
                continue
            picked[name] = got
            if got[3] >= 64 * max(e_ref, got[2]):
                break
        else:
            raise SystemExit(f"{name}: no seed below 400 gives decisive logits")
        e_ref = max(e_ref, picked[name][2])
    for name, (rec, arr, e, gap) in picked.items():      # against the FINAL e_ref: no case may be left out
        assert gap >= 64 * e_ref, (name, gap, e_ref)
        out["lm"][name] = dict(rec, min_gap=gap)
        arrays.update(arr)
    out["e_ref"] = e_ref
    os.makedirs(GOLDEN, exist_ok=True)
    with open(os.path.join(GOLDEN, "funasr_nano.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, indent=1)
    np.savez_compressed(os.path.join(GOLDEN, "funasr_nano.npz"), **arrays)
    print(f"e_ref {e_ref:.3e}; " + ", ".join(f"{n}: seed {r['seed']} eos {r['eos_token_id']} gap {r['min_gap']:.3f}" for n, r in out["lm"].items()))


if __name__ == "__main__":
    main()
