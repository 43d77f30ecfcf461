"""Paraformer-v2 on the GPU: the run-scan kernel at its edges, the posterior embedder against the float64 restatement
(tests/_paraformer_v2_oracle.py), and the model against what the reference recorded (tests/golden/paraformer_v2.npz).

Bounds. Embedder: e_ref = max |torch fp32 - float64| of the reference's own order on the same inputs (recorded in the golden by
tools/make_golden_paraformer_v2.py); the HIP result must stay within 4 e_ref + 1e-6. Encoder / decoder hidden: the bounds
tests/test_parity_gpu.py applies to the same quantities of Paraformer (read from that file's text, see _parity_bounds)."""
import functools
import os
import re
import sys

import pytest
import torch

from funasr_amd import _lib, ops, synth
from funasr_amd.register import tables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _paraformer_v2_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = PO.load_golden()
SOS, EOS, BLANK = 1, 2, 0


# ------------------------------------------------------------------------------------------------------ run scan
def _scan_rows(T):
    """the edge patterns as full-length rows [T]; each is scanned at lens 1, T - 1 and T"""
    r = torch.Generator().manual_seed(T)
    rows = {
        "all_blank": torch.zeros(T, dtype=torch.int32),
        "no_blank": torch.randint(3, 6, (T,), generator=r).int(),                     # equal and different neighbours, never blank
        "one_run": torch.full((T,), 9, dtype=torch.int32),                            # (at len T - 1 the padding ids equal the run's label)
        "same_label_around_a_blank": torch.tensor([5, 5, 0, 5] * (T // 4 + 1), dtype=torch.int32)[:T],
        "adjacent_different": (torch.arange(T) % 7 + 3).int(),
        "sos_eos": torch.tensor([SOS, SOS, EOS, 0, EOS, SOS] * (T // 6 + 1), dtype=torch.int32)[:T],
        "blank_runs": torch.tensor([0, 0, 4, 4, 4, 0, 0, 0, 6] * (T // 9 + 1), dtype=torch.int32)[:T],
    }
    return rows


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_run_scan_equals_a_python_loop(cuda, T):
    rows = _scan_rows(T)
    names, ids, lens = [], [], []
    for name, row in rows.items():
        for n in (1, T - 1, T):
            names.append((name, n)); ids.append(row); lens.append(n)
    ids = torch.stack(ids).to(cuda)
    counts, ranges = ops.ctc_runs(ids, lens, blank=BLANK)
    counts, ranges = counts.cpu().tolist(), ranges.cpu()
    for i, (name, n) in enumerate(names):
        want = PO.runs_of(ids[i, :n].cpu(), BLANK)
        assert counts[i] == len(want), (name, n)
        assert ranges[i, : len(want)].tolist() == [list(w) for w in want], (name, n)
        assert bool((ranges[i, len(want):] == -1).all()), (name, n)               # nothing written behind the clip's runs


def test_run_scan_batch_of_three_with_different_lens_and_a_short_table(cuda):
    T = 257
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 4, (3, T), generator=g).int().to(cuda)
    lens = [257, 100, 1]
    counts, ranges = ops.ctc_runs(ids, lens, blank=BLANK)
    for b in range(3):
        want = PO.runs_of(ids[b, : lens[b]].cpu(), BLANK)
        assert int(counts[b]) == len(want) and ranges[b, : len(want)].cpu().tolist() == [list(w) for w in want]
    counts2, short = ops.ctc_runs(ids, lens, blank=BLANK, ld=8)                     # a table shorter than the runs: counted, not written
    assert torch.equal(counts2, counts) and torch.equal(short[0].cpu(), ranges[0, :8].cpu())
    counts3, _ = ops.ctc_runs(ids, lens, blank=3)                                   # another blank id
    assert counts3.cpu().tolist() == [len(PO.runs_of(ids[b, : lens[b]].cpu(), 3)) for b in range(3)]


# ------------------------------------------------------------------------------------------------------ embedder
@functools.lru_cache(maxsize=None)
def _embedder_ref(V):
    hid, lens, w = PO.embedder_case(V, int(GOLD[f"embed.V{V}.seed"]))
    ref, gap = PO.embedder_reference(hid, lens, w, torch.float64)
    assert gap >= 0.02
    return hid, lens, w, ref


def _embedder_modules(V, w, cuda, blank_bias_extra=0.0):
    from funasr_amd.ctc import CTC
    from funasr_amd.paraformer_v2 import PosteriorEmbed
    ctc = CTC(odim=V, encoder_output_size=PO.EMBED_D)
    cb = w["ctc_b"].clone()
    cb[BLANK] += blank_bias_extra
    ctc.load_state_dict({"ctc_lo.weight": w["ctc_w"], "ctc_lo.bias": cb}, strict=True)
    emb = PosteriorEmbed(V, PO.EMBED_D, BLANK)
    emb.load_state_dict({"0.weight": w["w0"], "0.bias": w["b0"], "1.weight": w["g"], "1.bias": w["b"]}, strict=True)
    return ctc.to(cuda), emb.to(cuda)


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
@pytest.mark.parametrize("V", PO.EMBED_V)
def test_embedder_against_the_float64_restatement(cuda, V, mode):
    hid, lens, w, ref = _embedder_ref(V)
    ctc, emb = _embedder_modules(V, w, cuda)
    x = hid.to(cuda)
    runs = emb.runs(ctc, x, lens, mode, want_path=True)
    N, counts, path = runs.N, runs.counts, runs.path
    out, ranges = emb.embeds(runs, want_ranges=True)
    assert counts == [len(r[1]) for r in ref] and N == max(counts)
    e_ref = float(GOLD[f"embed.V{V}.e_ref"])
    worst = 0.0
    for b, (rpath, rruns, remb) in enumerate(ref):
        assert path[b, : lens[b]].cpu().tolist() == rpath.tolist()
        assert ranges[b, : len(rruns)].cpu().tolist() == [list(r) for r in rruns]
        assert bool((out[b, len(rruns):] == 0).all()) and bool((ranges[b, len(rruns):] == 0).all())     # rows j >= n_b: exactly zero
        worst = max(worst, float((out[b, : len(rruns)].cpu().double() - remb).abs().max()))
    print(f"embedder V={V} {mode}: max |hip - float64| {worst:.3e}, e_ref {e_ref:.3e}, bound {4 * e_ref + 1e-6:.3e}")
    assert worst <= 4 * e_ref + 1e-6, (worst, e_ref)
    # several row chunks (64 rows of the 195): bitwise the single-chunk result
    runs2 = emb.runs(ctc, x, lens, mode, want_path=True, chunk_rows=64)
    out2, ranges2 = emb.embeds(runs2, want_ranges=True)
    assert runs2.N == N and runs2.counts == counts and torch.equal(runs2.path, path) and torch.equal(ranges2, ranges) and torch.equal(out2, out)
    # a poisoned workspace changes nothing
    _lib.check(_lib.load().pf_posterior_embed_debug_poison(emb._handle, 0x7B), "pf_posterior_embed_debug_poison")
    runs3 = emb.runs(ctc, x, lens, mode)
    out3, _ = emb.embeds(runs3)
    assert runs3.counts == counts and torch.equal(out3, out)


def test_embedder_all_blank_returns_zero_and_touches_nothing(cuda):
    V = 261
    hid, lens, w, _ = _embedder_ref(V)
    ctc, emb = _embedder_modules(V, w, cuda, blank_bias_extra=1000.0)
    runs = emb.runs(ctc, hid.to(cuda), lens, "fp32", want_path=True)
    path = runs.path
    assert runs.N == 0 and runs.counts == [0, 0, 0]
    for b, n in enumerate(lens):
        assert bool((path[b, :n] == BLANK).all())
    sentinel = torch.full((3, 4, PO.EMBED_D), 7.0, device=cuda)
    lib = _lib.load()
    assert lib.pf_posterior_embed_embeds(emb._handle, 3, PO.EMBED_T, 0, sentinel.data_ptr(), None, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
    assert lib.pf_posterior_embed_set_precision(emb._handle, 1) != 0 and "mode must be" in _lib.last_error()      # bf16: refused with a message


# ------------------------------------------------------------------------------------------------------ model level
def _parity_bounds():
    """The bounds tests/test_parity_gpu.py asserts for Paraformer in every fp32-class mode (its f32_mode fixture): encoder output
    `(res["enc"].cpu() - t(g["enc"])).abs().max().item() < 1e-4` (test_pipeline_token_ids_equal_reference) and decoder hidden states
    `(hidden[b, :n].cpu() - ref_hidden[b, :n]).abs().max().item() < 2e-4` (test_decoder_with_decoders2_vs_reference_golden)."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_parity_gpu.py"), encoding="utf-8").read()
    enc = re.search(r'assert \(res\["enc"\]\.cpu\(\) - t\(g\["enc"\]\)\)\.abs\(\)\.max\(\)\.item\(\) < ([0-9.e-]+)', text)
    hid = re.search(r"assert \(hidden\[b, :n\]\.cpu\(\) - ref_hidden\[b, :n\]\)\.abs\(\)\.max\(\)\.item\(\) < ([0-9.e-]+)", text)
    return float(enc.group(1)), float(hid.group(1))


MODES = {"A": "fp32", "B": "f16x2"}


@functools.lru_cache(maxsize=None)
def _model(shape, blank_bias_key="blank_bias"):
    conf, sd = PO.model_state(shape, int(GOLD[f"{shape}.seed"]), float(GOLD["ctc_gain"]), float(GOLD[blank_bias_key]))
    model = tables.model_classes.get("Paraformer_v2_community")(**dict(conf, precision=MODES[shape]))
    model.load_state_dict(sd, strict=True)
    return model.to("cuda:0"), conf


def _feats(shape, T):
    return PO.clip_features(T, int(GOLD[f"{shape}.seed"]))


@functools.lru_cache(maxsize=None)
def _single(shape, T):
    model, _ = _model(shape)
    return model.recognize_features(_feats(shape, T)[None].to("cuda:0"), [T], return_intermediate=True)


@pytest.mark.parametrize("shape", sorted(PO.SHAPES))
@pytest.mark.parametrize("T", PO.CLIP_T)
def test_model_against_the_reference_records(cuda, shape, T):
    enc_tol, hid_tol = _parity_bounds()
    res = _single(shape, T)
    p = f"{shape}.T{T}."
    assert res["path"][0].cpu().tolist() == GOLD[p + "path"].tolist()
    assert res["ids"][0] == GOLD[p + "token_int"].tolist()
    assert res["raw_ids"][0] == GOLD[p + "raw_ids"].tolist()
    d_enc = float((res["enc"][0].cpu() - torch.from_numpy(GOLD[p + "enc"])).abs().max())
    n = res["token_num"][0]
    d_emb = float((res["embeds"][0, :n].cpu() - torch.from_numpy(GOLD[p + "embed"])).abs().max())
    d_hid = float((res["hidden"][0, :n].cpu() - torch.from_numpy(GOLD[p + "hidden"])).abs().max())
    print(f"shape {shape} ({MODES[shape]}) T={T}: encoder {d_enc:.2e} (< {enc_tol}), embed {d_emb:.2e}, decoder hidden {d_hid:.2e} (< {hid_tol})")
    assert d_enc < enc_tol and d_hid < hid_tol


@pytest.mark.parametrize("shape", sorted(PO.SHAPES))
def test_ragged_batch_equals_the_batch_of_one_runs(cuda, shape):
    """divergence (a): one ragged batch of all clips gives, clip by clip, bitwise the ids of the batch-of-one runs"""
    _, hid_tol = _parity_bounds()
    model, _ = _model(shape)
    Ts = list(PO.CLIP_T)
    x = torch.zeros(len(Ts), max(Ts), 560)
    for b, T in enumerate(Ts):
        x[b, :T] = _feats(shape, T)
    res = model.recognize_features(x.to(cuda), Ts, return_intermediate=True)
    fast = model.recognize_features(x.to(cuda), Ts)                                     # the production call: no intermediates
    for b, T in enumerate(Ts):
        one = _single(shape, T)
        assert res["raw_ids"][b] == one["raw_ids"][0] == fast["raw_ids"][b] and res["ids"][b] == GOLD[f"{shape}.T{T}.token_int"].tolist()
        assert res["path"][b, :T].cpu().tolist() == GOLD[f"{shape}.T{T}.path"].tolist()
        n = res["token_num"][b]
        d = float((res["hidden"][b, :n].cpu() - torch.from_numpy(GOLD[f"{shape}.T{T}.hidden"])).abs().max())
        assert d < hid_tol, (T, d)


class _Tok:
    bpemodel = None                                  # (skips the character-level post-processing: ids -> "12 7 ...")

    def ids2tokens(self, ids):
        return [str(i) for i in ids]

    def tokens2text(self, tokens):
        return " ".join(tokens)


@pytest.mark.parametrize("shape", sorted(PO.SHAPES))
def test_all_blank_clip_gives_the_empty_record_between_its_neighbours(cuda, shape):
    """divergence (b): the reference appends no record for an all-blank clip, which shifts every later key"""
    model, _ = _model(shape)
    Ts = [31, PO.SHORT_BLANK_T, 7]
    clips = [_feats(shape, 31), PO.clip_features(PO.SHORT_BLANK_T, int(GOLD[f"{shape}.blank_clip_seed"])), _feats(shape, 7)]
    x = torch.zeros(3, 31, 560)
    for b, c in enumerate(clips):
        x[b, : c.shape[0]] = c
    recs, _ = model.inference(x.to(cuda), data_lengths=Ts, key=["first", "silent", "last"], tokenizer=_Tok(), data_type="fbank", device="cuda:0")
    assert [r["key"] for r in recs] == ["first", "silent", "last"]
    assert recs[1] == {"key": "silent", "token_int": [], "text": ""}
    for r, T in ((recs[0], 31), (recs[2], 7)):
        want = GOLD[f"{shape}.T{T}.token_int"].tolist()
        assert r["token_int"] == want and r["text"] == " ".join(str(i) for i in want)
    # the second state dict (large blank bias): the recorded all-blank clip, alone in its batch -> N == 0, no decoder call
    blank_model, _ = _model(shape, "all_blank_bias")
    res = blank_model.recognize_features(_feats(shape, PO.BLANK_T)[None].to(cuda), [PO.BLANK_T], return_intermediate=True)
    assert res["path"][0].cpu().tolist() == GOLD[f"{shape}.blank.path"].tolist() and res["ids"] == [[]] and res["token_num"] == [0]
    recs, _ = blank_model.inference(_feats(shape, PO.BLANK_T)[None].to(cuda), key=["k"], data_type="fbank", device="cuda:0")
    assert recs == [{"key": "k", "token_int": []}]


@pytest.mark.parametrize("shape", sorted(PO.SHAPES))
def test_poisoned_workspaces_give_identical_ids(cuda, shape):
    model, _ = _model(shape)
    Ts = [65, 7, 31]
    x = torch.zeros(3, 65, 560)
    for b, T in enumerate(Ts):
        x[b, :T] = _feats(shape, T)
    a = model.recognize_features(x.to(cuda), Ts)
    lib = _lib.load()
    for mod, fn in ((model.encoder, lib.pf_encoder_debug_poison), (model.decoder, lib.pf_decoder_debug_poison),
                    (model.decoder.embed, lib.pf_posterior_embed_debug_poison)):
        _lib.check(fn(mod._handle, 0x7B), "debug_poison")
    b = model.recognize_features(x.to(cuda), Ts)
    assert a["raw_ids"] == b["raw_ids"] and a["token_num"] == b["token_num"]


def test_decoder_forward_follows_the_reference_contract(cuda):
    """forward(hs_pad, hlens, merged posteriors [B, N, V], lens) -> logits: the `embed` layers on the given tensor, then the parent"""
    shape, T = "A", 31
    model, _ = _model(shape)
    p = f"{shape}.T{T}."
    merged = torch.from_numpy(GOLD[p + "merged"])[None].to(cuda)
    _, hid_tol = _parity_bounds()
    logits, hidden, _ = model.decoder(torch.from_numpy(GOLD[p + "enc"])[None].to(cuda), [T], merged, [merged.shape[1]], return_both=True)
    assert logits.shape == (1, merged.shape[1], 261)
    assert float((hidden[0].cpu() - torch.from_numpy(GOLD[p + "hidden"])).abs().max()) < hid_tol
    assert logits[0].argmax(-1).cpu().tolist() == GOLD[p + "raw_ids"].tolist()


def test_automodel_generate_on_speech_like_audio(cuda, tmp_path):
    import json
    import shutil
    import yaml
    from _model_dir import VOCAB, write_wav
    from funasr_amd.auto_model import AutoModel

    conf = synth.paraformer_v2_conf(**dict(PO.SHAPES["B"], vocab=len(VOCAB)))
    sd = synth.paraformer_v2_state_dict(conf, seed=3, ctc_gain=8.0, blank_bias=12.0)
    d = str(tmp_path / "v2")
    os.makedirs(d)
    cfg = {"model": "Paraformer_v2_community",
           "model_conf": {k: conf[k] for k in ("ctc_weight", "lsm_weight", "length_normalized_loss", "blank_id", "sos", "eos")},
           "encoder": conf["encoder"], "encoder_conf": conf["encoder_conf"], "decoder": conf["decoder"], "decoder_conf": conf["decoder_conf"],
           "ctc_conf": conf["ctc_conf"], "frontend": "WavFrontend",
           "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10, "lfr_m": 7, "lfr_n": 6},
           "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(d, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(cfg, f, allow_unicode=True)
    torch.save(sd, os.path.join(d, "model.pt"))
    with open(os.path.join(d, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(VOCAB, f, ensure_ascii=False)
    shutil.copy(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "am.mvn"), os.path.join(d, "am.mvn"))
    wavs = []
    for i, secs in enumerate((1.3, 0.8, 2.1, 0.5)):
        path = str(tmp_path / f"clip{i}.wav")
        write_wav(path, synth.speech_like(int(16000 * secs), seed=i))
        wavs.append(path)
    am = AutoModel(model=d, device="cuda:0", disable_update=True)
    assert type(am.model).__name__ == "Paraformer_v2_community"
    res = am.generate(input=wavs, batch_size=3)
    assert sorted(r["key"] for r in res) == [f"clip{i}" for i in range(4)]
    for r in res:
        assert isinstance(r["token_int"], list) and isinstance(r["text"], str)
        assert all(t not in (0, 1, 2) for t in r["token_int"])
    assert any(r["token_int"] for r in res)
