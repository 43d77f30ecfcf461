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


def test_a_fresh_decoder_handle_registers_every_tensor_of_each_layer_kind_once(cuda):
    """pf_decoder_missing on handles that carry no weights counts the names the library registered. With n_blocks = 2: 18 per
    attention block (7 of the feed-forward, norm2 x 2 and fsmn_block, norm3 x 2, 6 projection tensors), 7 for decoders3.0, 2 for
    after_norm, 2 for output_layer, 9 for the contextual decoder's hotword branch, 10 per decoders2 block (an attention block less
    norm3 and the projections)."""
    lib = _lib.load()

    def make(vocab, contextual=False):
        cfg = _lib.pf_decoder_config(vocab, 256, 2, 256, 2, 11, 5, 1e-12)
        h = (lib.pf_decoder_create_contextual if contextual else lib.pf_decoder_create)(C.byref(cfg))
        assert h, _lib.last_error()
        return h

    plain, bare, ctx = make(300), make(0), make(300, contextual=True)
    try:
        assert lib.pf_decoder_missing(plain) == 2 * 18 + 7 + 2 + 2 == 47
        assert lib.pf_decoder_missing(bare) == 2 * 18 + 7 + 2 == 45
        assert lib.pf_decoder_missing(ctx) == 47 + 9 == 56
        for h, before in ((plain, 47), (ctx, 56)):
            assert lib.pf_decoder_set_decoders2(h, 1) == 0, _lib.last_error()
            assert lib.pf_decoder_missing(h) == before + 10
    finally:
        for h in (plain, bare, ctx):
            lib.pf_decoder_destroy(h)
