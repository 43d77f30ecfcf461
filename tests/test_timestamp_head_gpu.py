"""The LSTM recurrence of csrc/lstm.hip and the BLSTM timestamp head of CifPredictorV3 at their edges.

Reached only through `ops.lstm` (pf_k_lstm -> lstm_forward) and `CifPredictorV3.get_upsample_timestamp`
(pf_predictor_timestamp), compared with oracle/bicif_oracle.py (`lstm`, `upsample_timestamp`, `cif_wo_hidden`) evaluated in
float64: the oracle allocates in torch's default dtype, which `_oracle` switches inside a try / finally.

Paths reached here and nowhere else in the suite:
  * lstm_step_kernel<1>, <6>, <16>, <20> (H = 16, 96, 256, 320), and <32> (H = 512) beyond B = 3;
  * a second and a third 64-utterance workgroup tile (blockIdx.z > 0) with both directions, in the row-major output of
    `ops.lstm` and in the unit-major [T][C][Bs] output that us_alpha_t_kernel reads with stride Bs; the same at H = 512 (a
    hotword list of more than 64 entries, two stacked layers, the rows at len - 1);
  * 16-utterance wave tiles that are full, one short, one over (B = 15, 16, 17, 63, 64, 65);
  * T = 1, 2, 3 (the ping-pong of h_a / h_b), 2048 and 12285 steps, T x B odd (ld_pre rounded up), a one-column input GEMM;
  * saturated gates (|pre-activation| > 50);
  * more than 4096 upsampled frames: the chunk loop and the carry of us_scale_scan_kernel, up to the 12285 frames that the
    V3 predictor admits, and the sizes around one chunk (4095, 4096, 4097, 4098, 8192, 8193);
  * upsample_times 1, 2 and 8, use_cif1_cnn on, the plain `cnn` head beside the BLSTM head;
  * one predictor handle across batch sizes (h_a, h_b, cell, pre and lstm_out hold another call's contents);
  * the refusal of H = 80, D = 48, ndir = 3 by the launchers, and of idim = 160 by the BLSTM head of a handle whose
    `forward` works.

Bars (the convention of tests/test_conformer_gpu.py, FACTOR["fp32"] = 4): `gap` is the oracle's own float32-vs-float64
difference on the same case, and the device must lie within 4 x max(gap, 2^-24 x max |want64|) of the float64 result; the
second term is the rounding of storing the result in float32. Every check prints its ratio d / max(gap, 2^-24 max |want64|).

Two checks of the head need no tolerance, because us_scale_scan_kernel stores the scaled weights it integrates:
  * us_peaks is BITWISE cif_wo_hidden(us_alphas from the device, float32(1 - 1e-4)), the sequential float32 loop on the CPU;
  * the float64 row sums of us_alphas equal token_num within 4 x 2^-24 x token_num x sqrt(frames): the kernel rounds the
    total to float32, divides and multiplies once per frame, 3 roundings = 3 x 2^-24 relative at the worst, whatever the
    number of frames (frames = U x len, the number of non-zero terms).
No fire position is compared with the float64 oracle's peaks: the float32 and float64 integrals differ by up to 6e-5 at
12285 frames, so an integral can sit that close to the threshold; the bitwise check carries that burden.

Measured on the MI355X (ratio per group, smallest .. largest; the bar is 4 and stays 4: expf / tanhf cost nothing visible):
  every instantiation     1.03 .. 3.03   (H <= 128: at most 1.59; H = 256, 320, 512: 2.64, 3.03, 2.34 -- the MFMA chain adds the
                                          H products of a gate one after the other, the CPU oracle in blocks)
  batch tiles             1.14 .. 1.89
  hotword shape           1.62 (whole output), 2.32 (rows len - 1, against their own gap)
  step counts             0.93 (T = 2048) .. 1.76
  saturated gates         1.03
  alone / batched         1.19 .. 1.56 against float64; alone against batched 0.00 (bitwise on this shape, not promised)
  head, B cases           0.27 .. 2.07
  scan, cnn head          0.56 .. 1.33;  behind the BLSTM 0.97 (4098 frames), 1.04 (12285 frames)
  row sums / token_num    0.00 .. 1.00 of 2^-24 x token_num x sqrt(frames)
The 12285-step case takes 0.2 s on the device and one to four seconds of CPU oracle (cached for the GPU test), so it is kept.

Without a GPU the `test_*_inputs_*` tests still build every input and reference and assert what the GPU assertions rest on.
"""
import functools
import math
import zlib

import pytest
import torch

from oracle import bicif_oracle as BO

FACTOR = 4.0                     # FACTOR["fp32"] of tests/test_conformer_gpu.py
EPS = 2.0 ** -24                 # unit roundoff of float32
THRESHOLD = 1.0 - 1e-4           # get_upsample_timestamp's cif_wo_hidden threshold (cfg["threshold"] = 1.0)
HIDDEN_SIZES = (16, 32, 48, 64, 96, 128, 256, 320, 512)
BATCH_TILES = (1, 15, 16, 17, 63, 64, 65, 129)


def _oracle(dtype, fn, *args, **kwargs):
    """the oracle allocates in torch's default dtype: evaluate it in `dtype`"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return fn(*args, **kwargs)
    finally:
        torch.set_default_dtype(old)


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _maxd(a, b):
    return float((a.double() - b.double()).abs().max())


def _unit(want64, gap):
    return max(gap, EPS * float(want64.abs().max()))


def _check(tag, got, want64, gap):
    assert got.shape == want64.shape, (tag, got.shape, want64.shape)
    assert bool(torch.isfinite(got).all()), tag
    d, unit = _maxd(got, want64), _unit(want64, gap)
    print(f"{tag}: max |d| {d:.3e}, gap {gap:.3e}, ratio {d / unit:.2f} (bar {FACTOR:g})")
    assert d <= FACTOR * unit, (tag, d, gap, unit)


# ------------------------------------------------------------------------------------------------ inputs: recurrence
def _sfx(ndir):
    return ("", "_reverse")[:ndir]


@functools.lru_cache(maxsize=None)
def lstm_case(B, T, D, H, ndir, layers=1, ih_scale=1.0):
    """weights scaled as in BO.predictor_v3_state_dict: w_ih ~ 1/sqrt(D), w_hh ~ 0.7/sqrt(H), biases 0.1"""
    g = _gen("lstm", B, T, D, H, ndir, layers, ih_scale)
    x = torch.randn(B, T, D, generator=g)
    sd = {}
    for k in range(layers):
        d_in = D if k == 0 else ndir * H
        for s in _sfx(ndir):
            sd[f"weight_ih_l{k}{s}"] = torch.randn(4 * H, d_in, generator=g) * (ih_scale / d_in ** 0.5)
            sd[f"weight_hh_l{k}{s}"] = torch.randn(4 * H, H, generator=g) * (0.7 / H ** 0.5)
            sd[f"bias_ih_l{k}{s}"] = torch.randn(4 * H, generator=g) * 0.1
            sd[f"bias_hh_l{k}{s}"] = torch.randn(4 * H, generator=g) * 0.1
    want64 = _oracle(torch.float64, BO.lstm, x.double(), _cast(sd, torch.float64), "", layers, ndir == 2)
    want32 = _oracle(torch.float32, BO.lstm, x, sd, "", layers, ndir == 2)
    assert want64.dtype == torch.float64 and want32.dtype == torch.float32
    return dict(x=x, sd=sd, want64=want64, want32=want32, gap=_maxd(want32, want64), ndir=ndir, layers=layers,
                tag=f"lstm B={B} T={T} D={D} H={H} ndir={ndir} layers={layers} ih x{ih_scale:g}")


def instantiation_case(H):
    return lstm_case(17, 5, 32, H, 2)        # both 16-row wave tiles in use, lanes 1..15 of the second are padding


def batch_tile_case(B):
    return lstm_case(B, 4, 32, 64, 2)        # B = 129: Bs = 192, a third workgroup tile


HOTWORD_B, HOTWORD_T = 130, 10


def hotword_case():
    return lstm_case(HOTWORD_B, HOTWORD_T, 512, 512, 1, layers=2)


def hotword_rows(y):
    """the rows `_hotword_representation` keeps: index len - 1, ragged lengths 1..10"""
    lens = torch.arange(HOTWORD_B) % HOTWORD_T + 1
    return y[torch.arange(HOTWORD_B), lens - 1]


STEP_CASES = {
    "T=1": (3, 1, 32, 32, 2), "T=2": (3, 2, 32, 32, 2), "T=3": (3, 3, 32, 32, 2),      # state in h_b, h_a, h_b at the end
    "T=2048": (2, 2048, 32, 32, 2),
    "TxB odd": (5, 7, 32, 48, 2),             # 35 columns of `pre` in a row stride of 36
    "one column": (1, 1, 32, 64, 2),
}


def saturated_case():
    return lstm_case(4, 6, 32, 64, 2, ih_scale=64.0)


def largest_preactivation(c):
    """max |W_ih x + b_ih + b_hh| over the first layer: a lower bound of what the gates see at step 0 (h = 0)"""
    m = 0.0
    for s in _sfx(c["ndir"]):
        pre = c["x"].double() @ c["sd"][f"weight_ih_l0{s}"].double().T + (c["sd"][f"bias_ih_l0{s}"] + c["sd"][f"bias_hh_l0{s}"]).double()
        m = max(m, float(pre.abs().max()))
    return m


def alone_case():
    return lstm_case(5, 6, 32, 64, 2)


def all_lstm_cases():
    cases = [instantiation_case(H) for H in HIDDEN_SIZES] + [batch_tile_case(B) for B in BATCH_TILES]
    cases += [lstm_case(*a) for a in STEP_CASES.values()]
    return cases + [hotword_case(), saturated_case(), alone_case()]


# ------------------------------------------------------------------------------------------------------ inputs: head
def head_cfg(idim, U, kind, cif1):
    return dict(idim=idim, threshold=1.0, l_order=1, r_order=1, tail_threshold=0.45, smooth_factor=1.0, noise_threshold=0.0,
                smooth_factor2=0.25, noise_threshold2=0.01, upsample_times=U, use_cif1_cnn=cif1, upsample_type=kind)


def ragged_lens(B, T):
    """row 0 full, row 1 a single frame, the rest spread over 1..T"""
    lens = [T] + [1 + (37 * i) % T for i in range(1, B)]
    if B > 1:
        lens[1] = 1
    return lens


@functools.lru_cache(maxsize=None)
def head_case(kind, idim, U, B, T, cif1=False):
    cfg = head_cfg(idim, U, kind, cif1)
    sd = BO.predictor_v3_state_dict(cfg, seed=3)
    lens = torch.tensor(ragged_lens(B, T))
    tok = torch.clamp(U * lens // 10, min=1)                 # given, not taken from forward(): about one token per 10 frames
    for draw in range(16):
        # the first draw in which no row's weights are all below noise_threshold2 (a single-frame row is, once in eleven);
        # rows beyond len are random too: the reference's BLSTM runs over them
        hidden = torch.randn(B, T, idim, generator=_gen("head", kind, idim, U, B, T, cif1, draw))
        a64, p64 = _oracle(torch.float64, BO.upsample_timestamp, hidden.double(), lens, tok, _cast(sd, torch.float64), cfg)
        if bool(torch.isfinite(a64).all()):
            break
    a32, p32 = _oracle(torch.float32, BO.upsample_timestamp, hidden, lens, tok, sd, cfg)
    assert a64.dtype == torch.float64 and a32.dtype == torch.float32 and p32.dtype == torch.float32
    return dict(cfg=cfg, sd=sd, hidden=hidden, lens=lens, tok=tok, a64=a64, a32=a32, p32=p32, gap=_maxd(a32, a64),
                tag=f"head {kind} idim={idim} U={U} B={B} T={T} cif1={int(cif1)}")


def scan32(alphas):
    """cif_wo_hidden in float32 at float32(1 - 1e-4): the sequential loop us_scale_scan_kernel restates"""
    assert alphas.dtype == torch.float32
    return _oracle(torch.float32, BO.cif_wo_hidden, alphas, THRESHOLD)


def head_precondition(c):
    """what the GPU assertions rest on: token_num >= 1; every row's float64 total of unscaled weights is positive (a zero
    total gives 0 x inf = NaN and no row sum: the rescaled float64 row sums to token_num exactly when the total was positive
    and finite); the test's float32 scan is the oracle's; the gap is small and finite"""
    assert int(c["tok"].min()) >= 1
    a64 = c["a64"]
    assert bool(torch.isfinite(a64).all()) and bool((a64 >= 0).all()) and bool((a64.max(-1).values > 0).all())
    assert float((a64.sum(-1) - c["tok"]).abs().max()) <= 1e-9 * float(c["tok"].max())
    assert torch.equal(scan32(c["a32"]), c["p32"])
    assert math.isfinite(c["gap"]) and c["gap"] < 1e-5, (c["tag"], c["gap"])
    for b, n in enumerate(c["lens"].tolist()):
        assert bool((a64[b, c["cfg"]["upsample_times"] * n:] == 0).all())


WIDE = ("cnn_blstm", 64, 3, 66, 40)          # the second workgroup tile in the unit-major layout
WIDE_512 = ("cnn_blstm", 512, 3, 65, 4)      # the production width, 12 steps
SMALL = ("cnn_blstm", 64, 3, 3, 40)
U_CASES = [("cnn_blstm", 32, U, 3, 21) for U in (1, 2, 8)]
VARIANT_CASES = [("cnn_blstm", 32, 3, 3, 21, True), ("cnn", 32, 3, 3, 21, False), ("cnn", 32, 3, 3, 21, True)]
CNN_160 = ("cnn", 160, 3, 3, 21)
BLSTM_160 = ("cnn_blstm", 160, 3, 3, 21)     # created, `forward` works, the timestamp head refuses: never given to the oracle
# frame counts around the 4096-frame chunks of us_scale_scan_kernel, B = 3, row 0 full
SCAN_CNN = ([("cnn", 32, 1, 3, T) for T in (1, 63, 64, 65, 4095, 4096, 4097)] + [("cnn", 32, 2, 3, T) for T in (2048, 4096)] +
            [("cnn", 32, 3, 3, T) for T in (1366, 2731, 4095)])
SCAN_BLSTM = [("cnn_blstm", 32, 3, 2, 1366), ("cnn_blstm", 32, 3, 1, 4095)]


def _ids(case):
    return "-".join(str(v) for v in case)


# ------------------------------------------------------------------------------- CPU: every input meets its precondition
def test_lstm_inputs_have_small_finite_gaps():
    for c in all_lstm_cases():
        assert bool(torch.isfinite(c["want64"]).all())
        assert math.isfinite(c["gap"]) and c["gap"] < 1e-5, (c["tag"], c["gap"])
        print(f"{c['tag']}: gap {c['gap']:.3e}")


def test_lstm_saturated_inputs_really_saturate():
    assert largest_preactivation(saturated_case()) > 50
    assert largest_preactivation(alone_case()) < 10         # the ordinary scale, for contrast


def test_lstm_hotword_inputs_keep_one_row_per_length():
    rows = hotword_rows(hotword_case()["want64"])
    assert rows.shape == (HOTWORD_B, 512)
    lens = torch.arange(HOTWORD_B) % HOTWORD_T + 1
    assert sorted(set(lens.tolist())) == list(range(1, 11)) and int(lens[64:].numel()) == 66      # both workgroup tiles, every length


@pytest.mark.parametrize("case", [WIDE, WIDE_512, SMALL, CNN_160] + U_CASES + VARIANT_CASES, ids=_ids)
def test_head_inputs_meet_the_preconditions(case):
    c = head_case(*case)
    head_precondition(c)
    lens = c["lens"].tolist()
    assert lens[0] == case[4] and (len(lens) == 1 or 1 in lens)


@pytest.mark.parametrize("case", SCAN_CNN + SCAN_BLSTM, ids=_ids)
def test_scan_inputs_meet_the_preconditions(case):
    c = head_case(*case)
    head_precondition(c)
    assert int(c["lens"][0]) == case[4] and c["a64"].shape[1] == case[2] * case[4]


# -------------------------------------------------------------------------------------------------- GPU: the recurrence
def _run_lstm(cuda, c, x=None):
    from funasr_amd import ops
    y = (c["x"] if x is None else x).to(cuda)
    for k in range(c["layers"]):
        stack = lambda n: torch.stack([c["sd"][f"{n}_l{k}{s}"] for s in _sfx(c["ndir"])]).to(cuda)
        y = ops.lstm(y, stack("weight_ih"), stack("weight_hh"), stack("bias_ih"), stack("bias_hh"))
    return y.cpu()


def _check_lstm(cuda, c):
    _check(c["tag"], _run_lstm(cuda, c), c["want64"], c["gap"])


@pytest.mark.gpu
@pytest.mark.parametrize("H", HIDDEN_SIZES)
def test_lstm_every_instantiation(cuda, H):
    _check_lstm(cuda, instantiation_case(H))


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCH_TILES)
def test_lstm_batch_tiles(cuda, B):
    _check_lstm(cuda, batch_tile_case(B))


@pytest.mark.gpu
def test_lstm_production_hotword_shape(cuda):
    """B = 130 hotwords of up to 10 tokens, D = H = 512, two stacked unidirectional layers, as `_hotword_representation`
    calls it; the whole output is held to the bar, and so are the rows at len - 1 alone, with their own gap"""
    c = hotword_case()
    got = _run_lstm(cuda, c)
    _check(c["tag"], got, c["want64"], c["gap"])
    want = hotword_rows(c["want64"])
    _check(c["tag"] + " rows len-1", hotword_rows(got), want, _maxd(hotword_rows(c["want32"]), want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_lstm_step_counts(cuda, name):
    _check_lstm(cuda, lstm_case(*STEP_CASES[name]))


@pytest.mark.gpu
def test_lstm_saturated_gates(cuda):
    _check_lstm(cuda, saturated_case())


@pytest.mark.gpu
def test_lstm_twice_is_bitwise_and_alone_matches_batched(cuda):
    """bitwise equality between the batched and the single-utterance run is not promised: the input-projection GEMM picks
    its kernel by shape"""
    c = alone_case()
    a, b = _run_lstm(cuda, c), _run_lstm(cuda, c)
    assert torch.equal(a, b)
    _check(c["tag"], a, c["want64"], c["gap"])
    unit = _unit(c["want64"], c["gap"])
    for i in range(c["x"].shape[0]):
        one = _run_lstm(cuda, c, c["x"][i:i + 1])
        _check(f"{c['tag']} utterance {i} alone", one, c["want64"][i:i + 1], c["gap"])
        d = _maxd(one, a[i:i + 1])
        print(f"{c['tag']} utterance {i} alone vs batched: max |d| {d:.3e}, ratio {d / unit:.2f}")
        assert d <= FACTOR * unit


@pytest.mark.gpu
def test_lstm_refusals_and_a_valid_call_after_each(cuda):
    """argument checks of the launchers, made before any launch of the refused kernel"""
    from funasr_amd import _lib, ops
    ok = instantiation_case(32)

    def call(B, T, D, H, ndir):
        g = _gen("refused", D, H, ndir)
        return ops.lstm(torch.randn(B, T, D, generator=g).to(cuda), torch.randn(ndir, 4 * H, D, generator=g).to(cuda),
                        torch.randn(ndir, 4 * H, H, generator=g).to(cuda), torch.zeros(ndir, 4 * H).to(cuda),
                        torch.zeros(ndir, 4 * H).to(cuda))

    for args, message in (((2, 3, 32, 80, 2), "hidden size must be one of 16, 32, 48, 64, 96, 128, 256, 320, 512"),
                          ((2, 3, 48, 32, 2), "K must be a multiple of 32"),
                          ((2, 3, 32, 32, 3), "k_lstm: null/empty argument")):
        with pytest.raises(_lib.HipRuntimeError, match=message):
            call(*args)
        _check_lstm(cuda, ok)


# ------------------------------------------------------------------------------------------------ GPU: the timestamp head
def _predictor(cuda, c, cfg=None, sd=None):
    from funasr_amd.cif_predictor import CifPredictorV3
    pred = CifPredictorV3(**(c["cfg"] if cfg is None else cfg))
    pred.load_state_dict(c["sd"] if sd is None else sd, strict=True)
    return pred.to(cuda)


def _run_head(cuda, c, pred=None):
    pred = _predictor(cuda, c) if pred is None else pred
    _, _, usa, usp = pred.get_upsample_timestamp(c["hidden"].to(cuda), None, c["tok"], lengths=c["lens"])
    return usa.cpu(), usp.cpu()


def _check_head(c, usa, usp):
    _check(c["tag"], usa, c["a64"], c["gap"])
    # the scan, without a tolerance
    assert bool(torch.isfinite(usp).all())
    assert torch.equal(usp, scan32(usa)), c["tag"]
    U = c["cfg"]["upsample_times"]
    worst = 0.0
    for b, (n, tok) in enumerate(zip(c["lens"].tolist(), c["tok"].tolist())):
        assert bool((usa[b, U * n:] == 0).all())
        worst = max(worst, abs(float(usa[b].double().sum()) - tok) / (EPS * tok * math.sqrt(U * n)))
    print(f"{c['tag']}: row sums vs token_num, ratio {worst:.2f} (bar {FACTOR:g})")
    assert worst <= FACTOR, (c["tag"], worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [WIDE, WIDE_512] + U_CASES + VARIANT_CASES, ids=_ids)
def test_head_against_the_float64_oracle(cuda, case):
    c = head_case(*case)
    _check_head(c, *_run_head(cuda, c))


@pytest.mark.gpu
def test_head_one_handle_across_batch_sizes(cuda):
    """B = 66, 3, 66 on one handle: each result is bitwise that of a fresh handle with the same weights, whatever h_a, h_b,
    cell, pre and lstm_out hold from the call before"""
    wide, small = head_case(*WIDE), head_case(*SMALL)
    assert wide["cfg"] == small["cfg"] and all(torch.equal(wide["sd"][k], small["sd"][k]) for k in wide["sd"])
    pred = _predictor(cuda, wide)
    first, second, third = _run_head(cuda, wide, pred), _run_head(cuda, small, pred), _run_head(cuda, wide, pred)
    fresh_wide, fresh_small = _run_head(cuda, wide), _run_head(cuda, small)
    for got, want in ((first, fresh_wide), (second, fresh_small), (third, fresh_wide)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    _check_head(small, *second)
    _check_head(wide, *third)


@pytest.mark.gpu
def test_head_refuses_a_width_the_recurrence_does_not_have_and_goes_on(cuda):
    """idim = 160 passes pf_predictor_create_v3 (d_model % 32 == 0) but is none of launch_lstm_steps' hidden sizes: the
    handle is created and its `forward` works, the BLSTM head raises naming the sizes, `forward` still works afterwards;
    the `cnn` head has no recurrence and works at 160"""
    from funasr_amd import _lib
    cnn = head_case(*CNN_160)
    _check_head(cnn, *_run_head(cuda, cnn))
    kind, idim, U, B, T = BLSTM_160
    cfg = head_cfg(idim, U, kind, False)
    pred = _predictor(cuda, None, cfg, BO.predictor_v3_state_dict(cfg, seed=3))
    hidden, lens = cnn["hidden"].to(cuda), cnn["lens"]
    before = pred(hidden, lengths=lens)
    assert bool(torch.isfinite(before[2]).all()) and before[0].shape[0] == B
    with pytest.raises(_lib.HipRuntimeError, match="hidden size must be one of 16, 32, 48, 64, 96, 128, 256, 320, 512"):
        pred.get_upsample_timestamp(hidden, None, cnn["tok"], lengths=lens)
    after = pred(hidden, lengths=lens)
    for x, y in zip(before[:4], after[:4]):
        assert torch.equal(x, y)


# --------------------------------------------------------------------------------------- GPU: the chunked scale-and-scan
@pytest.mark.gpu
@pytest.mark.parametrize("case", SCAN_CNN, ids=_ids)
def test_scan_chunks_on_the_cnn_head(cuda, case):
    c = head_case(*case)
    _check_head(c, *_run_head(cuda, c))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCAN_BLSTM, ids=_ids)
def test_scan_chunks_behind_the_blstm(cuda, case):
    """4098 and 12285 steps of the recurrence (12285: one launch per step), then the chunked scan"""
    c = head_case(*case)
    _check_head(c, *_run_head(cuda, c))
