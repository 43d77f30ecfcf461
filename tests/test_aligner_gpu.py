"""MonotonicAligner on the MI355X: the d_k = 80 / 96 attention kernel (csrc/attention_mid.hip) against float64 softmax attention, its
guard band, masked rows and repeatability; the SAN-M encoder at those head sizes against the reference's recorded float64 outputs
(tests/golden/aligner.npz); the refused precisions and masks; the timestamp head, the records, `AutoModel` on a synthetic model
directory with (sound, text) inputs, and one run at the template's geometry.

Bars: the kernel 2e-5 (the bar of test_attention_f32 for the d_k = 128 kernel on the same input distribution); the encoder 4 x the
reference's recorded fp32 - fp64 gap (FACTOR["fp32"] of tests/test_sanm_gpu.py); the timestamp head 1e-5 on us_alphas and 1e-4 on
us_peaks with the same fire frames (tests/test_bicif.py)."""
import json
import os
import shutil

import pytest
import torch
import yaml

from funasr_amd import _lib, ops, synth
from funasr_amd.monotonic_aligner import MonotonicAligner

from ._model_dir import write_wav
from .test_aligner import CONFIGS, GOLDEN, INPUT_SIZE, assert_records_equal, golden_batch, golden_model, golden_tokens, load_golden, records_from

pytestmark = pytest.mark.gpu
FIRE = 1.0 - 1e-4
HEADS = [(80, 4), (96, 2)]
SHAPES = [(1, 1, 1, [1]), (2, 33, 33, [33, 32]), (2, 83, 83, [83, 40]), (3, 37, 150, [150, 1, 33]), (2, 130, 64, [64, 31]),
          (2, 129, 129, [129, 128]), (1, 500, 500, [500])]


def _maxd(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _qkv(B, Tq, Tk, D, seed):
    """Q / K / V as the encoder passes them: column blocks of [B, T, 3 D] projections (one buffer where Tq == Tk)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, Tq, 3 * D, generator=g)
    b = a if Tq == Tk else torch.randn(B, Tk, 3 * D, generator=g)
    return a, b


def _reference(a, b, lens, H, dk):
    B, Tq, Tk, D = a.shape[0], a.shape[1], b.shape[1], H * dk
    klens = torch.tensor(lens)
    qh = a[:, :, :D].double().reshape(B, Tq, H, dk).transpose(1, 2) * dk ** -0.5
    kh = b[:, :, D: 2 * D].double().reshape(B, Tk, H, dk).transpose(1, 2)
    vh = b[:, :, 2 * D:].double().reshape(B, Tk, H, dk).transpose(1, 2)
    m = (torch.arange(Tk)[None, :] >= klens[:, None])[:, None, None, :]
    p = torch.softmax((qh @ kh.transpose(-1, -2)).masked_fill(m, float("-inf")), -1).masked_fill(m, 0.0)
    return (p @ vh).transpose(1, 2).reshape(B, Tq, D)


def _run(cuda, a, b, lens, H, dk, out=None):
    D = H * dk
    ad = a.to(cuda)
    bd = ad if b is a else b.to(cuda)
    got = ops.attention_mid(ad[:, :, :D], bd[:, :, D: 2 * D], bd[:, :, 2 * D:], torch.tensor(lens, dtype=torch.int32).to(cuda), H, dk ** -0.5,
                            out=out)
    torch.cuda.synchronize()
    return got


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dk,H", HEADS)
@pytest.mark.parametrize("B,Tq,Tk,lens", SHAPES)
def test_attention_mid_against_float64_softmax_attention(cuda, dk, H, B, Tq, Tk, lens):
    """one key; one tile and one key over; a partial third tile; Tq != Tk either way with a one-key sequence; two query blocks; a
    full last tile beside one key more; 500 x 500"""
    a, b = _qkv(B, Tq, Tk, H * dk, Tq * 13 + Tk + dk)
    d = _maxd(_run(cuda, a, b, lens, H, dk), _reference(a, b, lens, H, dk))
    print(f"attention_mid d_k {dk} H {H} B {B} Tq {Tq} Tk {Tk}: max |d| {d:.3e} (bar 2e-5)")
    assert d < 2e-5


@pytest.mark.parametrize("dk,H", HEADS)
def test_attention_mid_guard_band_is_untouched(cuda, dk, H):
    """ldo = D + 32 and a sentinel everywhere: the last head's padded channels (the third 32-channel block past d_k = 80) go nowhere"""
    D, (B, Tq, Tk, lens) = H * dk, SHAPES[4]
    a, b = _qkv(B, Tq, Tk, D, 77 + dk)
    buf = torch.full((B, Tq, D + 32), -12345.0, device=cuda)
    _run(cuda, a, b, lens, H, dk, out=buf)
    assert bool((buf[:, :, D:] == -12345.0).all())
    assert _maxd(buf[:, :, :D], _reference(a, b, lens, H, dk)) < 2e-5
    # ... and at the end of the allocation: the last row of the last sequence is followed by the sentinel row only
    flat = torch.full((B * Tq + 1, D), -12345.0, device=cuda)
    _run(cuda, a, b, lens, H, dk, out=flat[: B * Tq].view(B, Tq, D))
    assert bool((flat[B * Tq] == -12345.0).all()) and bool(torch.equal(flat[: B * Tq].view(B, Tq, D), buf[:, :, :D]))


@pytest.mark.parametrize("dk,H", HEADS)
def test_attention_mid_never_reads_masked_rows_and_repeats_bit_for_bit(cuda, dk, H):
    D = H * dk
    for B, Tq, Tk, lens in (SHAPES[2], SHAPES[3], SHAPES[5]):
        a, b = _qkv(B, Tq, Tk, D, 5 * Tq + Tk + dk)
        if b is a:
            b = a.clone()                                                # poison the keys only: padded QUERY rows are computed
        zero, nan = b.clone(), b.clone()
        for i, n in enumerate(lens):
            zero[i, n:, D:] = 0.0
            nan[i, n:, D:] = float("nan")
        got_zero, got_nan = _run(cuda, a, zero, lens, H, dk), _run(cuda, a, nan, lens, H, dk)
        assert bool(torch.isfinite(got_nan).all()) and bool(torch.equal(got_zero, got_nan))
        assert bool(torch.equal(got_nan, _run(cuda, a, nan, lens, H, dk)))   # a call repeats bit for bit


def test_attention_dispatch_refuses_other_head_sizes_at_the_new_entry(cuda):
    q = torch.zeros(1, 4, 2 * 112, device=cuda)
    with pytest.raises(RuntimeError, match="80 or 96"):
        ops.attention_mid(q, q, q, torch.tensor([4], dtype=torch.int32).to(cuda), 2, 1.0)


# ------------------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("name", ["A", "B"])
def test_encoder_equals_the_references_recorded_output(cuda, name):
    g = load_golden()
    model, _, _ = golden_model(g, name)
    model = model.to(cuda)
    speech, lens = golden_batch(g)
    gap = float(g[f"{name}_gap_enc"])
    assert model.encoder._mode() == "fp32"
    batch, olens = model.encode(speech.to(cuda), lens)
    assert [int(v) for v in olens.tolist()] == lens
    for i, n in enumerate(lens):
        alone, _ = model.encode(speech[i: i + 1, :n].to(cuda), [n])
        want = g[f"{name}_enc_{i}"][:n]
        for tag, got in (("alone", alone[0]), ("batch", batch[i, :n])):
            d = _maxd(got, want)
            print(f"{name} clip {i} {tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / gap:.2f} (bar 4)")
            assert d <= 4.0 * gap, (name, i, tag, d, gap)


def test_other_precisions_and_masks_are_refused_at_d_k_80(cuda):
    from funasr_amd.sanm_encoder import SANMEncoder, SANMVadEncoder

    conf = synth.aligner_conf(input_size=INPUT_SIZE, **CONFIGS["A"])["encoder_conf"]
    enc = SANMEncoder(input_size=INPUT_SIZE, **conf).to(cuda)
    for mode in ("f16x2", "bf16", "bf16x3"):
        with pytest.raises(NotImplementedError, match="d_k = 80"):
            enc.set_precision(mode)
    lib, h = enc._ensure_handle()                                      # ... and at the C ABI, every mode but fp32
    for mode in (1, 2, 3):
        assert lib.pf_encoder_set_precision(h, mode) != 0 and "d_k = 80" in lib.pf_last_error().decode()
    assert lib.pf_encoder_set_precision(h, 0) == 0
    vad = SANMVadEncoder(input_size=INPUT_SIZE, **conf)
    vad.load_state_dict(synth.sanm_state_dict(1, vad))
    with pytest.raises(RuntimeError, match="d_k = 80"):                # the masked call, by name
        vad.to(cuda)(torch.zeros(1, 8, INPUT_SIZE, device=cuda), [8], [3])


def test_the_streaming_handle_refuses_an_encoder_with_heads_of_80(cuda):
    """the chunk step, by name: the guard comes before every other check of pf_stream_create, so handles without weights and a
    predictor / decoder of another width do"""
    import ctypes as C

    lib = _lib.load()
    ecfg = _lib.pf_encoder_config(INPUT_SIZE, 320, 4, 1280, 1, 0, 11, 0, 1e-12)
    pcfg = _lib.pf_predictor_config(512, 1, 1, 1.0, 1.0, 0.0, 0.45, 1)
    dcfg = _lib.pf_decoder_config(31, 512, 4, 2048, 1, 11, 5, 1e-12)
    scfg = _lib.pf_stream_config(1, 0, 10, 5, 4, 1, 10, 32, 0)
    e, p, d = lib.pf_encoder_create(C.byref(ecfg)), lib.pf_predictor_create(C.byref(pcfg)), lib.pf_decoder_create(C.byref(dcfg))
    assert e and p and d, _lib.last_error()
    try:
        assert not lib.pf_stream_create(e, p, d, C.byref(scfg))
        assert "d_k = 80" in _lib.last_error() and "chunk step" in _lib.last_error()
    finally:
        lib.pf_decoder_destroy(d)
        lib.pf_predictor_destroy(p)
        lib.pf_encoder_destroy(e)


# ------------------------------------------------------------------------------------------------------------ head, records
@pytest.mark.parametrize("name", ["A", "B"])
def test_timestamp_head_and_records_equal_the_references(cuda, name):
    g = load_golden()
    model, _, _ = golden_model(g, name)
    model = model.to(cuda)
    speech, lens = golden_batch(g)
    tok = [int(n) + 1 for n in g["n_tokens"]]
    # the head alone, on the reference's recorded encoder output (padding rows included: the reverse LSTM pass starts there)
    hidden = torch.stack([torch.from_numpy(g[f"{name}_enc_{i}"]).float() for i in range(len(lens))]).to(cuda)
    _, _, usa, usp = model.calc_predictor_timestamp(hidden, lens, tok)
    # ... and behind the GPU encoder: what `inference` computes
    enc, olens = model.encode(speech.to(cuda), lens)
    _, _, usa2, usp2 = model.calc_predictor_timestamp(enc, lens, tok)
    for i, n in enumerate(lens):
        wa, wp = torch.from_numpy(g[f"{name}_us_alphas_{i}"]), torch.from_numpy(g[f"{name}_us_peaks_{i}"])
        da, dp = _maxd(usa[i, : 3 * n], wa), _maxd(usp[i, : 3 * n], wp)
        print(f"{name} clip {i}: us_alphas {da:.3e} (bar 1e-5), us_peaks {dp:.3e} (bar 1e-4)")
        assert da < 1e-5 and dp < 1e-4
        assert torch.nonzero(usp[i, : 3 * n].cpu() >= FIRE).reshape(-1).tolist() == g[f"{name}_fires_{i}"].tolist()
        assert_records_equal(g, name, i, records_from(g, name, i, usa[i].cpu(), usp[i].cpu()))
        assert_records_equal(g, name, i, records_from(g, name, i, usa2[i].cpu(), usp2[i].cpu()))


# ------------------------------------------------------------------------------------------------------------ AutoModel
VOCAB = ["<blank>", "<s>", "</s>"] + list("欢迎大家来到这里我们一起") + ["<unk>"]


def write_aligner_dir(path):
    os.makedirs(path, exist_ok=True)
    conf = synth.aligner_conf(input_size=INPUT_SIZE, **CONFIGS["A"])
    model = MonotonicAligner(**conf)
    cfg = {"model": "MonotonicAligner", "model_conf": {"length_normalized_loss": False, "predictor_bias": 1},
           "encoder": conf["encoder"], "encoder_conf": conf["encoder_conf"], "predictor": conf["predictor"],
           "predictor_conf": conf["predictor_conf"],
           "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                        "lfr_m": 7, "lfr_n": 6},
           "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(cfg, f, allow_unicode=True)
    torch.save(synth.aligner_state_dict(11, model), os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(VOCAB, f, ensure_ascii=False)
    shutil.copy(os.path.join(GOLDEN, "am.mvn"), os.path.join(path, "am.mvn"))


def test_auto_model_end_to_end_on_sound_text_pairs(cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel

    mdir = str(tmp_path / "fa")
    write_aligner_dir(mdir)
    wavs, texts = [], ["欢 迎 大 家", "我 们 一 起 来 到 这 里"]
    for i, seconds in enumerate((1.3, 2.1)):
        wavs.append(str(tmp_path / f"clip{i}.wav"))
        write_wav(wavs[-1], synth.speech_like(int(16000 * seconds), seed=40 + i))
    scp, txt = str(tmp_path / "wav.scp"), str(tmp_path / "text.txt")
    with open(scp, "w", encoding="utf-8") as f:
        f.write("".join(f"utt{i} {w}\n" for i, w in enumerate(wavs)))
    with open(txt, "w", encoding="utf-8") as f:
        f.write("".join(f"utt{i} {t}\n" for i, t in enumerate(texts)))
    dt = ("sound", "text")
    am = AutoModel(model=mdir, device=str(cuda), disable_update=True)
    assert isinstance(am.model, MonotonicAligner)
    alone = [am.generate(input=(w, t), data_type=dt)[0] for w, t in zip(wavs, texts)]                    # a single pair
    for rec, t in zip(alone, texts):
        n = len(t.split())
        assert rec["text"] == t and len(rec["timestamp"]) == n
        flat = [v for span in rec["timestamp"] for v in span]
        assert flat == sorted(flat) and flat[0] >= 0
    out_dir = str(tmp_path / "out")
    batch = am.generate(input=(scp, txt), data_type=dt, batch_size=2, output_dir=out_dir)                 # scp + text file, one batch
    assert [r["key"] for r in batch] == ["utt0", "utt1"]
    for a, b in zip(alone, batch):                                                                        # a clip's record does not depend on its batch mates
        assert a["text"] == b["text"] and a["timestamp"] == b["timestamp"]
    for name in ("timestamp_list", "timestamp_str"):
        lines = open(os.path.join(out_dir, "tp_res", name), encoding="utf-8").read().splitlines()
        assert [ln.split()[0] for ln in lines] == ["utt0", "utt1"]
    lists = am.generate(input=(wavs, texts), data_type=dt, batch_size=2)                                  # two lists
    one_by_one = am.generate(input=(scp, txt), data_type=dt, batch_size=1)                                # scp + text file, batches of one
    for got in (lists, one_by_one):
        assert [(r["text"], r["timestamp"]) for r in got] == [(r["text"], r["timestamp"]) for r in alone]


def test_template_geometry_smoke(cuda):
    """30 blocks, D 320 (4 heads of d_k 80), F 1280: one 10-second clip of 167 frames with a 40-token transcript"""
    conf = synth.aligner_conf(input_size=INPUT_SIZE)
    assert conf["encoder_conf"]["num_blocks"] == 30 and conf["encoder_conf"]["output_size"] == 320 and conf["encoder_conf"]["linear_units"] == 1280
    model = MonotonicAligner(**conf)
    model.load_state_dict(synth.aligner_state_dict(2, model), strict=True)
    model = model.to(cuda)
    T, n_tok = 167, 40
    speech = torch.randn(1, T, INPUT_SIZE, generator=torch.Generator().manual_seed(9)).to(cuda)
    enc, olens = model.encode(speech, [T])
    _, _, usa, usp = model.calc_predictor_timestamp(enc, [T], [n_tok + 1])
    assert bool(torch.isfinite(enc).all()) and bool(torch.isfinite(usa).all()) and bool(torch.isfinite(usp).all())
    assert usa.shape == (1, 3 * T) and int((usp[0] >= FIRE).sum()) == n_tok + 1
    from funasr_amd.timestamps import cif_timestamps
    _, spans = cif_timestamps(usa[0].cpu(), usp[0].cpu(), [f"t{i}" for i in range(n_tok)])
    flat = [v for span in spans for v in span]
    assert len(spans) == n_tok and flat == sorted(flat)
