"""Transducer on the MI355X through the C ABI: the prediction step and the two-launch joint step against the float64 oracle on random
inputs, the search (`pf_transducer_search`) on the goldens' recorded encoder outputs -- ids, n-best order and evaluation counts exact,
scores within 8 x gap_score --, its two guards, independence of back-to-back searches, and AutoModel end to end in both encoder
precisions.

Bars are the project's fp32 rules (tests/test_transformer_gpu.py): 4 x the reference's own fp32 - fp64 gap stored beside the recorded
outputs; where no recorded gap exists (random-input kernel tests) 4 x max |oracle fp32 - oracle fp64| on the same inputs -- another
valid fp32 summation order may be that far off -- with the floor 1e-7."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from funasr_amd import _lib, synth
from funasr_amd.transducer import Transducer, TransducerSearchError

from . import _transducer_oracle as O
from ._model_dir import write_wav
from .test_conformer import pin_positional_rows
from .test_transducer import golden_model, golden_searches, load_golden

pytestmark = pytest.mark.gpu
FACTOR = {"fp32": 4.0, "f16x2": 8.0}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _maxd(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _check(tag, got, want64, gap, factor=4.0):
    d = _maxd(got, want64)
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / max(gap, 1e-30):.2f} (bar {factor:g})")
    assert d <= factor * gap, (tag, d, gap)


# ------------------------------------------------------------------------------------------------ rnnt_pred_step
def _pred_weights(V, E, H, L, J, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {"decoder.embed.weight": torch.randn(V, E, generator=g), "joint_network.lin_dec.weight": torch.randn(J, H, generator=g) / H ** 0.5}
    for l in range(L):
        n = E if l == 0 else H
        sd[f"decoder.rnn.{l}.weight_ih_l0"] = torch.randn(4 * H, n, generator=g) * (1.5 / n ** 0.5)
        sd[f"decoder.rnn.{l}.weight_hh_l0"] = torch.randn(4 * H, H, generator=g) * (1.5 / H ** 0.5)
        sd[f"decoder.rnn.{l}.bias_ih_l0"] = 0.3 * torch.randn(4 * H, generator=g)
        sd[f"decoder.rnn.{l}.bias_hh_l0"] = 0.3 * torch.randn(4 * H, generator=g)
    return sd


def _pack(sd, L):
    return torch.cat([sd[f"decoder.rnn.{l}.{n}"].reshape(-1) for l in range(L)
                      for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]).contiguous()


class _Pred:
    """the hook on caller-supplied buffers: n_slots slots, slot 0 zero, every other slot NaN"""

    def __init__(self, cuda, sd, V, E, H, L, J, n_slots):
        self.dims = (V, E, H, L, J)
        self.n_slots = n_slots
        self.embed = sd["decoder.embed.weight"].contiguous().to(cuda)
        self.weights = _pack(sd, L).to(cuda)
        self.lin_dec = sd["joint_network.lin_dec.weight"].contiguous().to(cuda)
        self.state = torch.full((n_slots, L, 2, H), float("nan"), device=cuda)
        self.state[0] = 0
        self.proj = torch.full((n_slots, J), float("nan"), device=cuda)

    def step(self, label, src, dst):
        V, E, H, L, J = self.dims
        rc = _lib.load().pf_k_rnnt_pred_step(self.embed.data_ptr(), self.weights.data_ptr(), self.lin_dec.data_ptr(), self.state.data_ptr(),
                                             self.proj.data_ptr(), self.n_slots, V, E, H, L, J, label, src, dst, _stream())
        torch.cuda.synchronize()
        return rc


def _oracle_chain(sd, labels, dt):
    s = O.cast(sd, dt)
    state, out = O.init_state(s), []
    for lab in labels:
        d, state = O.pred_step(s, lab, state)
        out.append((state[0], state[1], O.dec_proj(s, d)))
    return out


@pytest.mark.parametrize("E,H,L", [(48, 64, 2), (20, 20, 1), (512, 512, 1), (64, 36, 4)])
def test_pred_step_chain_against_the_oracle(cuda, E, H, L):
    """label 0 and label V - 1 among a chain of 5 steps through distinct slots; every slot but slot 0 starts as NaN, and after the
    chain exactly the written slots are finite: a step writes dst and nothing else"""
    V, J = 37, 24 if H < 512 else 512
    sd = _pred_weights(V, E, H, L, J, seed=E + H + L)
    labels = [0, V - 1, 5, 0, 11]
    p = _Pred(cuda, sd, V, E, H, L, J, n_slots=8)
    slots = [3, 1, 6, 2, 5]                                           # distinct, not in order; slots 4 and 7 stay untouched
    src = 0
    for lab, dst in zip(labels, slots):
        assert p.step(lab, src, dst) == 0
        src = dst
    r64, r32 = _oracle_chain(sd, labels, torch.float64), _oracle_chain(sd, labels, torch.float32)
    for n, dst in enumerate(slots):
        for name, got, k in (("h", p.state[dst, :, 0], 0), ("c", p.state[dst, :, 1], 1), ("dec_proj", p.proj[dst], 2)):
            _check(f"pred_step E={E} H={H} L={L} step {n} {name}", got, r64[n][k], max(_maxd(r32[n][k], r64[n][k]), 1e-7))
    assert bool((p.state[0] == 0).all())
    for s in (4, 7):
        assert bool(torch.isnan(p.state[s]).all()) and bool(torch.isnan(p.proj[s]).all()), s
    assert bool(torch.isnan(p.proj[0]).all())                         # slot 0 is only ever read


def test_pred_step_refuses_src_equal_dst_and_bad_arguments(cuda):
    """every workgroup of a layer reads all of h of the source slot, so a step in place would race: refused, like a label or a slot
    outside its range; nothing is written"""
    V, E, H, L, J = 11, 20, 20, 1, 8
    p = _Pred(cuda, _pred_weights(V, E, H, L, J, seed=1), V, E, H, L, J, n_slots=3)
    before = p.state.clone()
    for label, src, dst, word in ((1, 1, 1, "src == dst"), (V, 0, 1, "label"), (-1, 0, 1, "label"), (1, 0, 3, "slot"), (1, -1, 1, "slot")):
        assert p.step(label, src, dst) != 0
        assert word in _lib.last_error(), (word, _lib.last_error())
    assert torch.equal(torch.nan_to_num(p.state, nan=7.0), torch.nan_to_num(before, nan=7.0))


# ------------------------------------------------------------------------------------------------ rnnt_joint_topk
def _joint(cuda, enc_p, dec_p, W, b, k, poison=True):
    V, J = W.shape
    lib = _lib.load()
    n = int(lib.pf_k_rnnt_joint_partial_floats(V, k))
    part = torch.full((n + 8,), float("nan"), device=cuda)
    if not poison:
        part[:n] = 0.0
    rec = torch.full((1 + 2 * k + 4,), float("nan"), device=cuda)
    dev = [t.contiguous().to(cuda) for t in (enc_p, dec_p, W, b)]
    _lib.check(lib.pf_k_rnnt_joint_topk(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), V, J, k, part.data_ptr(),
                                        rec.data_ptr(), _stream()), "pf_k_rnnt_joint_topk")
    torch.cuda.synchronize()
    assert bool(torch.isnan(rec[1 + 2 * k:]).all()) and bool(torch.isnan(part[n:]).all())      # nothing behind the record / the scratch
    assert bool(torch.isfinite(part[:n].view(-1, 4 + 2 * k)[:, :3]).all())
    rec = rec.cpu()
    return rec[: 1 + k].clone(), rec[1 + k: 1 + 2 * k].view(torch.int32).tolist()


def _joint_inputs(V, J, seed, top_row):
    g = torch.Generator().manual_seed(seed)
    enc_p, dec_p = torch.randn(J, generator=g), torch.randn(J, generator=g)
    W = torch.randn(V, J, generator=g) * (2.0 / J ** 0.5)
    b = 0.5 * torch.randn(V, generator=g)
    b[top_row] += 9.0                                                 # the maximum: row 0 (the blank), row 1 or row V - 1
    return enc_p, dec_p, W, b


def _joint_against_the_oracle(cuda, enc_p, dec_p, W, b, k, tag):
    sd = {"joint_network.lin_out.weight": W, "joint_network.lin_out.bias": b}
    lp64 = O.joint_logp(O.cast(sd, torch.float64), enc_p.double(), dec_p.double())
    lp32 = O.joint_logp(O.cast(sd, torch.float32), enc_p, dec_p)
    gap = max(_maxd(lp32, lp64), 1e-7)
    vals, ids = _joint(cuda, enc_p, dec_p, W, b, k)
    assert all(1 <= i < W.shape[0] for i in ids) and len(set(ids)) == k, ids
    want_v, want_i = O.topk_lower_index_first(lp64, min(k + 1, W.shape[0] - 1))
    _check(f"{tag} blank", vals[0], lp64[0], gap)
    _check(f"{tag} top-{k} values", vals[1:], want_v[:k], gap)
    _check(f"{tag} values at the returned ids", vals[1:], lp64[ids], gap)
    for r in range(k):                                                # ids exact where float64 separates the ranks by > 1000 x gap
        lo = float(want_v[r] - want_v[r + 1]) if r + 1 < want_v.shape[0] else float("inf")
        hi = float(want_v[r - 1] - want_v[r]) if r > 0 else float("inf")
        if min(lo, hi) > 1000 * gap:
            assert ids[r] == int(want_i[r]), (tag, r, ids, want_i.tolist())
    return vals, ids


@pytest.mark.parametrize("V,J,k", [(2, 4, 1), (3, 36, 2), (61, 96, 5), (61, 4, 16), (257, 36, 16), (257, 512, 1), (4234, 512, 2),
                                   (4234, 96, 16), (33, 96, 5), (65, 36, 16)])
@pytest.mark.parametrize("top_row", ["blank", "row1", "last"])
def test_joint_topk_against_the_oracle(cuda, V, J, k, top_row):
    """one workgroup and many, a last workgroup of one row (V = 33, 65, 257), k clipped to V - 1; the maximum at the blank (which
    stays out of the top-k), at row 1 and at row V - 1; partial buffers poisoned with NaN"""
    k = min(k, V - 1)
    top = {"blank": 0, "row1": 1, "last": V - 1}[top_row]
    enc_p, dec_p, W, b = _joint_inputs(V, J, seed=V + J + k, top_row=top)
    vals, ids = _joint_against_the_oracle(cuda, enc_p, dec_p, W, b, k, f"joint V={V} J={J} k={k} max at {top_row}")
    if top != 0:
        assert ids[0] == top
    assert 0 not in ids


def test_joint_topk_all_inside_one_workgroup_ties_and_a_floor_row(cuda):
    """the 16 best all in the rows of the third workgroup; two exactly equal logits there (rows of zero weights, equal biases) come
    lower index first; one row of -1e30"""
    V, J, k = 257, 96, 16
    enc_p, dec_p, W, b = _joint_inputs(V, J, seed=5, top_row=0)
    rows = list(range(64, 96))
    b[rows[:20]] += 20.0 + torch.arange(20, dtype=torch.float32)      # ranks 0 .. 19 inside workgroup 2, one unit apart
    W[70] = 0.0
    W[77] = 0.0
    b[70] = b[77] = 31.25                                             # an exact tie among the 16 best
    b[100] = -1e30
    vals, ids = _joint_against_the_oracle(cuda, enc_p, dec_p, W, b, k, "joint one-workgroup")
    assert all(64 <= i < 96 for i in ids), ids
    assert ids.index(70) + 1 == ids.index(77) and float(vals[1 + ids.index(70)]) == float(vals[1 + ids.index(77)])
    vals2, ids2 = _joint(cuda, enc_p, dec_p, W, b, k, poison=False)
    assert ids2 == ids and torch.equal(vals2, vals)                   # deterministic, whatever the scratch held


# ------------------------------------------------------------------------------------------------ the search on the goldens
@pytest.fixture(scope="module")
def golden(cuda):
    g = load_golden()
    model, sd, conf = golden_model(g)
    return g, model.to(cuda), sd, conf


@pytest.mark.parametrize("name,clip,frames,beam", golden_searches())
def test_search_on_the_recorded_encoder_outputs(golden, cuda, name, clip, frames, beam):
    """T = 1 and the three clips at beam 1, 2, 5 with nbest = beam: ids, order and counts exact, scores within 8 x gap_score"""
    g, model, _, _ = golden
    enc = torch.from_numpy(g[f"enc_{clip}"]).float()[:frames]
    hyps, info = model.search(enc.to(cuda), beam_size=beam, nbest=beam)
    n = int(g[f"search_{name}_n"])
    assert [h[0] for h in hyps] == [g[f"search_{name}_ids_{r}"].tolist() for r in range(n)]
    for c in ("joint_evals", "pred_steps", "max_frame_evals"):
        assert info[c] == int(g[f"search_{name}_{c}"]), (c, info)
    d = float(np.abs(np.asarray([h[1] for h in hyps]) - g[f"search_{name}_scores"]).max())
    print(f"search {name}: {info}, scores max |d| {d:.3e} (bar {8 * float(g['gap_score']):.3e})")
    assert d <= 8 * float(g["gap_score"])


def test_search_guards_and_independence(golden, cuda):
    """a NaN planted in enc_out ends the search with the non-finite error (it must not hang); max_expansions_per_frame = 1 on a clip
    that needs more ends it with the cap error; both are the error path, no GPU fault. Then two searches back to back on the same
    handle give what each gives alone: the prefix cache and the slots do not leak between utterances."""
    g, model, _, _ = golden
    enc = [torch.from_numpy(g[f"enc_{i}"]).float().to(cuda) for i in range(3)]
    alone = [model.search(e, beam_size=2, nbest=2) for e in enc[:2]]
    bad = enc[1].clone()
    bad[3, 5] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite") as e:
        model.search(bad, beam_size=2)
    assert isinstance(e.value, TransducerSearchError) and e.value.stats["max_frame_evals"] >= 1
    assert int(g["search_c1_b2_max_frame_evals"]) > 1
    with pytest.raises(RuntimeError, match="max_expansions_per_frame = 1"):
        model.search(enc[1], beam_size=2, max_expansions_per_frame=1)
    again = [model.search(e, beam_size=2, nbest=2) for e in (enc[0], enc[1], enc[0])]
    assert again[0] == alone[0] and again[1] == alone[1] and again[2] == alone[0]


def test_search_refuses_what_is_not_built(golden, cuda):
    g, model, _, _ = golden
    enc = torch.from_numpy(g["enc_0"]).float().to(cuda)
    with pytest.raises(NotImplementedError, match="beam_size"):
        model.search(enc, beam_size=17)
    with pytest.raises(ValueError, match="max_expansions_per_frame"):
        model.search(enc, beam_size=2, max_expansions_per_frame=0)


# ------------------------------------------------------------------------------------------------ AutoModel
def _model_dir(path, g, precision):
    os.makedirs(path, exist_ok=True)
    tokens = g["tokens"].tolist()
    c = synth.transducer_conf(vocab=len(tokens))
    conf = {"model": "Transducer", "model_conf": {"auxiliary_ctc_weight": 0.0, "precision": precision},
            "encoder": c["encoder"], "encoder_conf": c["encoder_conf"], "decoder": c["decoder"], "decoder_conf": c["decoder_conf"],
            "joint_network": c["joint_network"], "joint_network_conf": c["joint_network_conf"],
            "frontend": "WavFrontend", "frontend_conf": {"fs": 16000, "window": "hamming", "n_mels": 80, "frame_length": 25, "frame_shift": 10,
                                                         "lfr_m": 1, "lfr_n": 1},
            "tokenizer": "CharTokenizer", "tokenizer_conf": {"unk_symbol": "<unk>", "split_with_space": True}}
    with open(os.path.join(path, "config.yaml"), "w", encoding="utf-8") as f:
        yaml.safe_dump(conf, f, allow_unicode=True)
    torch.save({"state_dict": synth.transducer_state_dict(int(g["seed"]), Transducer(**c))}, os.path.join(path, "model.pt"))
    with open(os.path.join(path, "tokens.json"), "w", encoding="utf-8") as f:
        json.dump(tokens, f, ensure_ascii=False)
    return tokens


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_automodel_decodes_the_golden_clips_to_the_golden_tokens(golden, cuda, tmp_path, precision):
    """a model directory on disk -> AutoModel -> the recorded features of the three clips decode to the recorded 1-best (beam 2, the
    reference's default), one record whatever nbest is passed; the encoder output meets the encoder bars on the way"""
    from funasr_amd.auto_model import AutoModel

    g = golden[0]
    tokens = _model_dir(str(tmp_path / "transducer"), g, precision)
    am = AutoModel(model=str(tmp_path / "transducer"), device="cuda", disable_update=True)
    assert isinstance(am.model, Transducer) and am.model.encoder.precision == precision
    pin_positional_rows(am.model, g)                                  # the recording host's table is part of the recording
    for i in range(3):
        feats = torch.from_numpy(g[f"feats_{i}"])
        enc, _ = am.model.encode(feats[None].to(cuda), [feats.shape[0]])
        _check(f"clip {i} encoder {precision}", enc[0], g[f"enc_{i}"], float(g[f"gap_enc_{i}"]), FACTOR[precision])
        res = am.generate(input=feats, data_type="fbank", key=f"clip{i}", nbest=3, output_dir=str(tmp_path / "out"))
        assert len(res) == 1 and set(res[0]) >= {"key", "token", "text", "text_postprocessed"}
        want = [tokens[t] for t in g[f"search_c{i}_b2_ids_0"].tolist() if t not in (0, 1, 2)]
        assert res[0]["token"] == want, (i, res[0]["token"], want)
    for name in ("token", "text", "text_postprocessed"):
        assert os.path.exists(str(tmp_path / "out" / "1best_recog" / name))
    with pytest.raises(NotImplementedError, match="batch decoding is not implemented"):
        am.model.inference(torch.zeros(2, 50, 80), batch_size=2)


def test_wav_input_through_automodel(golden, cuda, tmp_path):
    from funasr_amd.auto_model import AutoModel

    _model_dir(str(tmp_path / "transducer"), golden[0], "f16x2")
    p = str(tmp_path / "utt0.wav")
    write_wav(p, synth.speech_like(16000, seed=20))
    am = AutoModel(model=str(tmp_path / "transducer"), device="cuda", disable_update=True)
    res = am.generate(input=p, beam_size=5)
    assert len(res) == 1 and res[0]["key"] == "utt0" and isinstance(res[0]["token"], list)
