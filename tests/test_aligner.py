"""MonotonicAligner, CPU side: registry, the reference's state-dict names and shapes, refused options, the float64 restatement of the
encoder and the timestamp head against the reference's recorded float64 outputs (tests/golden/aligner.npz, written by
tools/make_golden_aligner.py), the host half (`cif_timestamps` + `sentence_postprocess`) on the recorded weights against the recorded
records, and the two-input route: `prepare_data_iterator` and the loader on (sound, text) inputs.

Bar of the float64 oracle against the recorded float64 run: 4 x the recorded fp32 - fp64 gap of the same quantity (the rule of
tests/test_sanm.py; the two float64 computations actually agree to 1e-7 or better, which is printed)."""
import json
import os

import numpy as np
import pytest
import torch

from funasr_amd import synth
from funasr_amd.audio import load_audio_text, load_text
from funasr_amd.auto_model import prepare_data_iterator
from funasr_amd.monotonic_aligner import MonotonicAligner
from funasr_amd.register import tables
from funasr_amd.timestamps import cif_timestamps
from funasr_amd.tokenizer import CharTokenizer, sentence_postprocess

from ._model_dir import write_wav

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INPUT_SIZE = 560
CONFIGS = {
    "A": dict(output_size=320, attention_heads=4, linear_units=64, num_blocks=2, upsample_type="cnn_blstm", use_cif1_cnn=False),
    "B": dict(output_size=96, attention_heads=1, linear_units=64, num_blocks=2, upsample_type="cnn_blstm", use_cif1_cnn=True),
}


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "aligner.npz"), allow_pickle=False))


def golden_model(g, name):
    conf = synth.aligner_conf(input_size=INPUT_SIZE, **CONFIGS[name])
    model = MonotonicAligner(**conf)
    sd = synth.aligner_state_dict(int(g["seed"]), model)
    model.load_state_dict(sd, strict=True)
    return model, sd, conf


def golden_batch(g):
    """the two clips zero-padded into one batch -> (speech [2, 41, 560], lens)"""
    lens = [int(v) for v in g["lens"]]
    speech = torch.zeros(len(lens), max(lens), INPUT_SIZE)
    for i, n in enumerate(lens):
        speech[i, :n] = torch.from_numpy(g[f"feats_{i}"])
    return speech, lens


def golden_tokens(g, i):
    return [str(g["tokens"][int(t)]) for t in g[f"transcript_{i}"]]


def records_from(g, name, i, us_alphas, us_peaks):
    """the host half of `inference` for clip i -> (timestamp_str, text, timestamp)"""
    n = int(g["lens"][i]) * 3
    token = golden_tokens(g, i)
    ts_str, ts = cif_timestamps(us_alphas[:n], us_peaks[:n], list(token))
    text, stamps, _ = sentence_postprocess(token, ts)
    return ts_str, text, stamps


def assert_records_equal(g, name, i, got):
    ts_str, text, stamps = got
    assert ts_str == str(g[f"{name}_timestamp_str_{i}"])
    assert text == str(g[f"{name}_text_{i}"])
    assert stamps == g[f"{name}_timestamp_{i}"].tolist()


# ------------------------------------------------------------------------------------------------------ registry, state dict
def test_registry_and_install():
    from funasr_amd.install import hip_classes, install

    assert tables.model_classes["MonotonicAligner"] is MonotonicAligner
    assert ("model_classes", "MonotonicAligner", MonotonicAligner) in hip_classes()

    class Tables:
        def __init__(self):
            self.seen = {}

        def register(self, table, key):
            def deco(cls):
                self.seen[(table, key)] = cls
                return cls
            return deco

    t = Tables()
    install(t)
    assert t.seen[("model_classes", "MonotonicAligner")] is MonotonicAligner


def test_state_dict_names_and_shapes_are_the_references_at_the_template():
    ref = json.load(open(os.path.join(GOLDEN, "aligner_state_dict.json")))
    model = MonotonicAligner(encoder="SANMEncoder", encoder_conf=ref["encoder_conf"], predictor="CifPredictorV3",
                             predictor_conf=ref["predictor_conf"], input_size=ref["input_size"], **ref["model_conf"])
    own = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert own == ref["shapes"]
    assert all(k.startswith(("encoder.", "predictor.")) for k in own)
    # the template's geometry is the one the new attention kernel exists for, and it defaults to the only mode it has
    assert model.encoder.output_size() // model.encoder.attention_heads == 80 and model.encoder._mode() == "fp32"
    # the defaults of synth.aligner_conf are the template
    conf = synth.aligner_conf()
    assert {k: conf["encoder_conf"][k] for k in ref["encoder_conf"]} == ref["encoder_conf"]
    assert {k: conf["predictor_conf"][k] for k in ref["predictor_conf"]} == ref["predictor_conf"]


def test_strict_load_and_constructor_arguments():
    g = load_golden()
    model, sd, conf = golden_model(g, "A")
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in sd.items() if k != "predictor.cif_output2.bias"}, strict=True)
    # specaug*, length_normalized_loss and predictor_bias are accepted
    MonotonicAligner(specaug="SpecAugLFR", specaug_conf={"lfr_rate": 6}, **dict(conf, length_normalized_loss=True, predictor_bias=0))


@pytest.mark.parametrize("change,named", [
    (dict(encoder="ConformerEncoder"), "encoder: ConformerEncoder"),
    (dict(predictor="CifPredictorV2"), "predictor: CifPredictorV2"),
    (dict(predictor_conf=dict(upsample_type="cnn_attn")), "upsample_type: cnn_attn"),
    (dict(encoder_conf=dict(output_size=160, attention_heads=2), predictor_conf=dict(idim=160)), "idim: 160"),
    (dict(encoder_conf=dict(output_size=224, attention_heads=2), predictor_conf=dict(idim=224, upsample_type="cnn")), "attention_heads: 2"),
    (dict(precision="f16x2"), "precision: f16x2"),
    (dict(precision="bf16"), "precision: bf16"),
    (dict(precision="bf16x3"), "precision: bf16x3"),
])
def test_refusals_name_the_option(change, named):
    conf = synth.aligner_conf(input_size=INPUT_SIZE, **CONFIGS["A"])
    for k, v in change.items():
        conf[k] = dict(conf[k], **v) if isinstance(v, dict) else v
    with pytest.raises(NotImplementedError) as e:
        MonotonicAligner(**conf)
    assert named in str(e.value)


def test_precision_and_training_forward_are_refused_after_construction():
    model, _, _ = golden_model(load_golden(), "A")
    for mode in ("f16x2", "bf16", "bf16x3"):
        with pytest.raises(NotImplementedError, match="80"):
            model.set_precision(mode)
        with pytest.raises(NotImplementedError, match="d_k = 80"):
            model.encoder.set_precision(mode)
    model.set_precision("fp32").set_precision(None)
    with pytest.raises(NotImplementedError, match="training"):
        model(torch.zeros(1, 4, INPUT_SIZE), torch.tensor([4]), torch.zeros(1, 2), torch.tensor([2]))


# ------------------------------------------------------------------------------------------------------ float64 restatement
@pytest.mark.parametrize("name", ["A", "B"])
def test_float64_oracle_equals_the_references_recorded_run(name):
    from oracle import bicif_oracle as BO
    from oracle import paraformer_oracle as PO

    g = load_golden()
    _, sd, conf = golden_model(g, name)
    speech, lens = golden_batch(g)
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                           # (the oracles allocate their states in the default dtype)
    try:
        sd64 = {k: v.double() for k, v in sd.items()}
        enc, olens = PO.sanm_encoder(speech.double(), torch.tensor(lens), sd64, conf["encoder_conf"], "encoder.")
        tok = torch.tensor([int(n) + 1 for n in g["n_tokens"]])
        usa, usp = BO.upsample_timestamp(enc, olens, tok, sd64, conf["predictor_conf"], "predictor.")
    finally:
        torch.set_default_dtype(before)
    for i, n in enumerate(lens):
        for key, got in (("enc", enc[i, :n]), ("us_alphas", usa[i, : 3 * n]), ("us_peaks", usp[i, : 3 * n])):
            d = float(np.abs(got.numpy() - g[f"{name}_{key}_{i}"][: got.shape[0]]).max())
            gap = float(g[f"{name}_gap_{key}"])
            print(f"{name} clip {i} {key}: max |d| {d:.3e} (recorded fp32 - fp64 gap {gap:.3e})")
            assert d <= 4.0 * gap
        assert_records_equal(g, name, i, records_from(g, name, i, usa[i].float(), usp[i].float()))


@pytest.mark.parametrize("name", ["A", "B"])
def test_host_half_on_the_golden_weights_gives_the_golden_records(name):
    g = load_golden()
    counts = []
    for i in range(len(g["lens"])):
        usa, usp = torch.from_numpy(g[f"{name}_us_alphas_{i}"]).float(), torch.from_numpy(g[f"{name}_us_peaks_{i}"]).float()
        got = records_from(g, name, i, usa, usp)
        assert_records_equal(g, name, i, got)
        assert len(got[2]) == int(g["n_tokens"][i])
        assert int((usp >= 1.0 - 1e-4).sum()) == int(g["n_tokens"][i]) + 1
        assert float(g[f"{name}_margin_{i}"]) > 2e-4                 # the fire margin the generator asserts
        counts.append(got[0].count("<sil>"))
    assert counts[0] > 0 and counts[1] == 0                          # gaps above 12 frames in the 3-token clip only


def test_empty_transcript_returns_like_the_reference():
    g = load_golden()
    assert str(g["empty_transcript"]) == "returns"
    usa, usp = torch.from_numpy(g["A_us_alphas_0"]).float(), torch.from_numpy(g["A_us_peaks_0"]).float()
    ts_str, ts = cif_timestamps(usa, usp, [])
    assert (ts_str, ts) == ("", []) and sentence_postprocess([], ts) == ("", [], [])


# ------------------------------------------------------------------------------------------------------ the two-input route
TOKENS = ["<blank>", "<s>", "</s>", "欢", "迎", "大", "家", "<unk>"]


@pytest.fixture()
def pair_files(tmp_path):
    paths = []
    for i, n in enumerate((1600, 2400)):
        p = str(tmp_path / f"utt{i}.wav")
        write_wav(p, synth.speech_like(n, seed=i))
        paths.append(p)
    scp, txt = str(tmp_path / "wav.scp"), str(tmp_path / "text.txt")
    with open(scp, "w", encoding="utf-8") as f:
        f.write(f"first {paths[0]}\nsecond {paths[1]}\n")
    with open(txt, "w", encoding="utf-8") as f:
        f.write("one 欢 迎\ntwo 大 家 欢 迎\n")
    return paths, scp, txt


def test_prepare_data_iterator_on_tuple_inputs(pair_files):
    paths, scp, txt = pair_files
    dt = ("sound", "text")
    # one pair: the key is the LAST input's, a random one for a raw string
    keys, data = prepare_data_iterator((paths[0], "欢 迎 大 家"), data_type=dt)
    assert data == [(paths[0], "欢 迎 大 家")] and len(keys) == 1 and keys[0].startswith("rand_key_")
    # scp + text file: zipped line by line, the keys of text.txt
    keys, data = prepare_data_iterator((scp, txt), data_type=dt)
    assert keys == ["one", "two"] and data == [(paths[0], "欢 迎"), (paths[1], "大 家 欢 迎")]
    # two lists: the reference's one-key-variable loop over the last list (the first random key labels every string)
    keys, data = prepare_data_iterator((paths, ["欢 迎", "大 家"]), data_type=dt)
    assert data == [(paths[0], "欢 迎"), (paths[1], "大 家")] and len(keys) == 2 and keys[0] == keys[1] and keys[0].startswith("rand_key_")
    # key rule: with the sound LAST the file names are the keys
    keys, data = prepare_data_iterator((["欢 迎", "大 家"], paths), data_type=("text", "sound"))
    assert keys == ["utt0", "utt1"] and data == [("欢 迎", paths[0]), ("大 家", paths[1])]


def test_tuple_inputs_that_do_not_pair_up_are_an_error(pair_files):
    paths, scp, _ = pair_files
    dt = ("sound", "text")
    with pytest.raises(ValueError, match="0 inputs"):
        prepare_data_iterator((), data_type=dt)
    with pytest.raises(ValueError, match="1 inputs"):
        prepare_data_iterator((paths[0],), data_type=dt)
    with pytest.raises(ValueError, match="2, 1 items"):
        prepare_data_iterator((paths, ["only one"]), data_type=dt)
    with pytest.raises(ValueError, match="2, 1 items"):
        prepare_data_iterator((scp, "a raw string"), data_type=dt)


def test_inputs_without_a_tuple_data_type_behave_as_before(pair_files):
    paths, scp, _ = pair_files
    assert prepare_data_iterator(paths[0]) == (["utt0"], [paths[0]])
    assert prepare_data_iterator(paths, data_type="sound") == (["utt0", "utt1"], paths)
    assert prepare_data_iterator(tuple(paths)) == (["utt0", "utt1"], paths)
    assert prepare_data_iterator(scp, data_type="sound") == (["first", "second"], paths)
    keys, data = prepare_data_iterator("欢迎", data_type="text")
    assert data == ["欢迎"] and keys[0].startswith("rand_key_")
    keys, data = prepare_data_iterator((paths[0], "not a file"))        # a tuple without a tuple data_type: a plain list of two inputs
    assert data == [paths[0], "not a file"] and keys == ["utt0", "utt0"]


def test_loader_on_tuple_inputs_and_text_from_string_and_file(pair_files, tmp_path):
    paths, _, _ = pair_files
    tok = CharTokenizer(token_list=TOKENS)
    assert load_text("欢 迎 大 家", tok) == [3, 4, 5, 6]
    assert load_text("欢迎x", tok) == [3, 4, 7]                          # unknown characters -> <unk>
    one = str(tmp_path / "one.txt")
    with open(one, "w", encoding="utf-8") as f:
        f.write(" 大 家 \n")
    assert load_text(one, tok) == [5, 6]
    assert load_text([5, 6], tok) == [5, 6]                              # ready token ids pass through
    audio, text = load_audio_text([(paths[0], "欢 迎"), (paths[1], one)], data_type=("sound", "text"), tokenizer=tok)
    assert [int(a.shape[0]) for a in audio] == [1600, 2400] and all(a.dtype == torch.float32 for a in audio)
    assert text == [[3, 4], [5, 6]]
    with pytest.raises(ValueError, match="tokenizer"):
        load_text("欢 迎", None)
    with pytest.raises(ValueError, match="2 inputs"):
        load_audio_text([(paths[0],)], data_type=("sound", "text"), tokenizer=tok)
    with pytest.raises(NotImplementedError, match="image"):
        load_audio_text([(paths[0], "x")], data_type=("sound", "image"), tokenizer=tok)
