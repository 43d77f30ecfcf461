"""pf_decoder_create also makes decoders with heads of d_k <= 64 (the offline fp32 forward runs them through the small-head
attention kernel). Every other consumer of a decoder handle is built for d_k = 128 and must refuse such a handle with a message
instead of running its 128-wide kernels over it: the arithmetic modes, the contextual decoder, the streaming step."""
import ctypes as C

import pytest

from funasr_amd import _lib

pytestmark = pytest.mark.gpu


def _decoder(lib, heads, contextual=False):
    cfg = _lib.pf_decoder_config(31, 512, heads, 2048, 1, 11, 5, 1e-12)
    return (lib.pf_decoder_create_contextual if contextual else lib.pf_decoder_create)(C.byref(cfg))


def test_only_the_fp32_mode_of_the_plain_decoder_takes_small_heads(cuda):
    lib = _lib.load()
    d = _decoder(lib, 8)                                             # d_k = 64
    assert d, _lib.last_error()
    try:
        for mode in (1, 2, 3):
            assert lib.pf_decoder_set_precision(d, mode) != 0 and "fp32 mode only" in _lib.last_error()
        assert lib.pf_decoder_set_precision(d, 0) == 0
    finally:
        lib.pf_decoder_destroy(d)
    assert not _decoder(lib, 8, contextual=True) and "unsupported config" in _lib.last_error()
    assert not _decoder(lib, 5) and "unsupported config" in _lib.last_error()         # 512 % 5


def test_the_streaming_handle_refuses_a_small_head_decoder(cuda):
    lib = _lib.load()
    ecfg = _lib.pf_encoder_config(560, 512, 4, 2048, 1, 0, 11, 0, 1e-12)
    pcfg = _lib.pf_predictor_config(512, 1, 1, 1.0, 1.0, 0.0, 0.45, 1)
    scfg = _lib.pf_stream_config(1, 0, 10, 5, 4, 1, 10, 32, 0)
    e, p = lib.pf_encoder_create(C.byref(ecfg)), lib.pf_predictor_create(C.byref(pcfg))
    small, plain = _decoder(lib, 8), _decoder(lib, 4)
    assert e and p and small and plain, _lib.last_error()
    try:
        assert not lib.pf_stream_create(e, p, small, C.byref(scfg))
        assert "d_model / n_heads == 128" in _lib.last_error()
        st = lib.pf_stream_create(e, p, plain, C.byref(scfg))        # the same call with heads of 128 gets past that check:
        if st:                                                       # (these handles carry no weights, so it stops at the first tensor)
            lib.pf_stream_destroy(st)
        else:
            assert "tensor not set" in _lib.last_error() and "n_heads" not in _lib.last_error()
    finally:
        lib.pf_decoder_destroy(small)
        lib.pf_decoder_destroy(plain)
        lib.pf_predictor_destroy(p)
        lib.pf_encoder_destroy(e)
