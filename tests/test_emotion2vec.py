"""load_model_dir's token list, as download_model_from_hub.py:87-90 resolves it: a `tokens.txt` beside config.yaml (emotion2vec
ships its label list that way) becomes tokenizer_conf.token_list, a `tokens.json` wins over it, and a directory with neither keeps
its config's tokenizer_conf untouched."""
import json
import os

from funasr_amd.auto_model import load_model_dir
from funasr_amd.tokenizer import CharTokenizer

LABELS = ["angry", "disgusted", "fearful", "happy", "neutral", "other", "sad", "surprised", "unuse_0"]


def _model_dir(path, txt=False, js=False):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        f.write("model: Emotion2vec\ntokenizer: CharTokenizer\ntokenizer_conf:\n  unk_symbol: <unk>\n  split_with_space: true\n")
    if txt:
        with open(os.path.join(path, "tokens.txt"), "w", encoding="utf-8") as f:
            f.write("\n".join(LABELS) + "\n")
    if js:
        with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
            json.dump(LABELS[:3], f)
    return str(path)


def test_tokens_txt_is_the_token_list(tmp_path):
    kw = load_model_dir(_model_dir(tmp_path, txt=True))
    conf = kw["tokenizer_conf"]
    assert conf["token_list"] == os.path.join(str(tmp_path), "tokens.txt")
    assert conf["unk_symbol"] == "<unk>" and conf["split_with_space"] is True       # the config's own keys are kept
    assert CharTokenizer(**conf).token_list == LABELS


def test_tokens_json_wins_over_tokens_txt(tmp_path):
    kw = load_model_dir(_model_dir(tmp_path, txt=True, js=True))
    assert kw["tokenizer_conf"]["token_list"] == os.path.join(str(tmp_path), "tokens.json")
    assert CharTokenizer(**kw["tokenizer_conf"]).token_list == LABELS[:3]


def test_no_token_file_leaves_the_config_alone(tmp_path):
    kw = load_model_dir(_model_dir(tmp_path))
    assert kw["tokenizer_conf"] == {"unk_symbol": "<unk>", "split_with_space": True}


# ---------------------------------------------------------------------------------------------- the model, CPU side
import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

from funasr_amd import synth  # noqa: E402
from funasr_amd.emotion2vec import Emotion2vec, get_slopes, parse_feature_encoder_spec  # noqa: E402
from funasr_amd.register import tables  # noqa: E402

from . import _emotion2vec_oracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "emotion2vec.npz"))


def _tiny(golden=None):
    m = Emotion2vec(model_conf=synth.emotion2vec_conf(), vocab_size=9)
    return m, synth.emotion2vec_state_dict(int(golden["seed"]) if golden is not None else 7, m)


def test_oracle_equals_the_reference_in_float64(golden):
    m, sd = _tiny(golden)
    labels = list(golden["labels"])
    for i in range(len(golden["lens"])):
        fr = O.features(torch.from_numpy(golden[f"wav_{i}"]), sd, O.cfg_of(m), reference_casts=True)
        pooled, probs = O.head(fr, sd, labels)
        for name, got in (("frames", fr), ("pooled", pooled), ("probs", probs)):
            ref = golden[f"{name}64_{i}"]
            rel = np.abs(got.numpy() - ref).max() / np.abs(ref).max()
            assert rel <= 1e-9, (name, i, rel)


def test_slopes_are_the_reference_slopes(golden):
    for h in (4, 12, 16):
        np.testing.assert_array_equal(np.array(get_slopes(h), np.float32), golden[f"slopes_{h}"])
        assert O.slopes(h) == get_slopes(h)


def test_state_dict_is_the_reference_layout():
    with open(os.path.join(GOLDEN, "emotion2vec_state_dict.json")) as f:
        ref = json.load(f)
    m = Emotion2vec(model_conf=synth.emotion2vec_conf(768, 12, 4, 8), vocab_size=9)
    mine = {k: list(v.shape) for k, v in m.state_dict().items()}
    dec = "modality_encoders.AUDIO.decoder."
    assert mine == {k: v for k, v in ref.items() if not k.startswith(dec)}
    assert any(k.startswith(dec) for k in ref)
    full = {k: torch.zeros(v) for k, v in ref.items()}
    m.load_state_dict(full, strict=True)                       # the training-only decoder keys are accepted and dropped
    assert sum(v.numel() for v in m.state_dict().values()) > 90e6
    assert tables.model_classes["Emotion2vec"] is Emotion2vec


def test_feature_encoder_spec_is_parsed_without_eval():
    tmpl = "[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512,2,2)] + [(512,2,2)]"
    assert parse_feature_encoder_spec(tmpl) == [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
    with pytest.raises(ValueError):
        parse_feature_encoder_spec("__import__('os').getcwd()")
    with pytest.raises(ValueError):
        parse_feature_encoder_spec("[(512, 10, 5)] - [(1, 2, 3)]")


def test_numeric_fields_are_coerced():
    conf = synth.emotion2vec_conf()
    conf["norm_eps"] = "1e-05"                                # what yaml.safe_load gives for `norm_eps: 1e-05`
    conf["mlp_ratio"] = "4.0"
    m = Emotion2vec(**conf, vocab_size=9)                     # the flattened form build_model passes
    assert m.norm_eps == 1e-5 and isinstance(m.norm_eps, float) and m.ffn_dim == 1024
    assert m.conv_pos_kernel == 19 and m.spec[0] == (512, 10, 5)


@pytest.mark.parametrize("where,key,value,match", [
    ("top", "layer_norm_first", True, "layer_norm_first"),
    ("audio", "extractor_mode", "default", "extractor_mode"),
    ("audio", "learned_alibi", True, "learned_alibi"),
    ("audio", "conv_pos_pre_ln", True, "conv_pos_pre_ln"),
    ("audio", "use_alibi_encoder", False, "use_alibi_encoder"),
    ("top", "num_heads", 8, "head dim"),
])
def test_unbuilt_options_are_refused(where, key, value, match):
    conf = synth.emotion2vec_conf()
    (conf if where == "top" else conf["modalities"]["audio"])[key] = value
    with pytest.raises(NotImplementedError, match=match):
        Emotion2vec(model_conf=conf, vocab_size=9)
    with pytest.raises(NotImplementedError, match="precision"):
        Emotion2vec(model_conf=synth.emotion2vec_conf(), precision="bf16")


def test_records_drop_unuse_labels(golden):
    labels = list(golden["labels"])
    probs = np.stack([golden[f"probs64_{i}"] for i in range(3)])
    recs = O.records(["a", "b", "c"], probs, labels)
    for r in recs:
        assert r["labels"] == labels[:-1] and len(r["scores"]) == 8
        assert abs(sum(r["scores"]) - 1.0) < 1e-9
    assert golden["probs64_0"][-1] == 0.0


def test_no_cpu_fallback():
    m, sd = _tiny()
    m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        m.forward_packed(torch.zeros(16000), [16000])
    with pytest.raises(ValueError, match="at least 400"):
        m.forward_packed(torch.zeros(300), [300])
