"""CPU: rtisi_la(..., open_end=True), the fp64 definition of what a stream (RtisiLaStream) computes.

open_end takes out of the iteration the one thing that depends on where the spectrogram ends and that a stream cannot know in time:
with perfectrec, the samples from fshift T on reading as zero.  What must hold: without perfectrec nothing changes; with it, the
frames that never saw the tail are unchanged; the rows a run on S[:T1] commits before its end are those of a run on any longer S
(which is what lets a stream commit them before the rest has arrived); and the signal is still istft of the result."""
import functools

import numpy as np
import pytest

import lws_amd
from lws_amd.lws import _perfectrec_prepad

SHAPES = [(64, 16, 12), (48, 16, 7), (256, 96, 9), (128, 32, 33)]
STEPS = [(0, 2), (1, 3), (3, 3), (5, 2)]   # (look_ahead, iterations)


@functools.lru_cache(maxsize=None)
def start(fsize, fshift, T, perfectrec):
    rng = np.random.default_rng(fsize + T)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    S = rng.standard_normal((T, fsize // 2 + 1)) + 1j * rng.standard_normal((T, fsize // 2 + 1))
    S.setflags(write=False)
    return p, S


@functools.lru_cache(maxsize=None)
def run(fsize, fshift, T, perfectrec, LA, n, open_end, rows=None):
    p, S = start(fsize, fshift, T, perfectrec)
    return lws_amd.rtisi_la(S[:rows], fsize, fshift, p.awin, p.swin, n, look_ahead=LA, perfectrec=perfectrec, return_signal=True,
                            open_end=open_end)


@pytest.mark.parametrize("fsize,fshift,T", SHAPES)
def test_without_perfectrec_open_end_changes_no_bit(fsize, fshift, T):
    for LA, n in STEPS:
        c, x = run(fsize, fshift, T, False, LA, n, False)
        co, xo = run(fsize, fshift, T, False, LA, n, True)
        assert np.array_equal(c, co) and np.array_equal(x, xo)


@pytest.mark.parametrize("fsize,fshift,T", SHAPES)
def test_with_perfectrec_the_frames_that_never_saw_the_tail_keep_their_bits(fsize, fshift, T):
    """Committing frame m reads samples up to fshift min(m + LA, T - 1) + fsize; the default zeroes from fshift T on."""
    lo = _perfectrec_prepad(fsize, fshift)
    for LA, n in STEPS:
        P = sum(1 for m in range(T) if fshift * min(m + LA, T - 1) + fsize <= fshift * T)
        c, x = run(fsize, fshift, T, True, LA, n, False)
        co, xo = run(fsize, fshift, T, True, LA, n, True)
        assert co.shape == c.shape and xo.shape == x.shape
        assert np.array_equal(c[:P], co[:P])
        k = max(fshift * P - lo, 0)
        assert np.array_equal(x[:k], xo[:k])
        print("(%d,%d) T=%d LA=%d n=%d: P=%d of %d frames, %d of %d samples" % (fsize, fshift, T, LA, n, P, T, k, len(x)))
    assert not np.array_equal(run(fsize, fshift, T, True, 1, 3, False)[0], run(fsize, fshift, T, True, 1, 3, True)[0])   # it does something


@pytest.mark.parametrize("perfectrec", [False, True])
@pytest.mark.parametrize("fsize,fshift,T", SHAPES)
def test_prefix_property_bit_for_bit(fsize, fshift, T, perfectrec):
    lo = _perfectrec_prepad(fsize, fshift) if perfectrec else 0
    for LA, n in STEPS:
        c2, x2 = run(fsize, fshift, T, perfectrec, LA, n, True)
        for T1 in sorted({T - 1, T // 2 + 1, min(LA + 1, T - 1)}):
            c1, x1 = run(fsize, fshift, T, perfectrec, LA, n, True, rows=T1)
            rows = max(T1 - LA, 0)
            assert np.array_equal(c1[:rows], c2[:rows]), (LA, n, T1)
            k = max(fshift * rows - lo, 0)
            assert k <= len(x1) and np.array_equal(x1[:k], x2[:k]), (LA, n, T1)


def test_open_end_takes_frame_counts_the_round_trip_does_not_keep():
    p, S = start(64, 16, 12, True)
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        lws_amd.rtisi_la(S[:2], 64, 16, p.awin, p.swin, 3, perfectrec=True)
    c, x = lws_amd.rtisi_la(S[:2], 64, 16, p.awin, p.swin, 3, perfectrec=True, return_signal=True, open_end=True)
    assert c.shape == (2, 33) and x.shape == (0,)            # 2 frames: istft cuts everything
    assert np.abs(np.abs(c) - np.abs(S[:2])).max() <= 1e-12 * np.abs(S).max()


@pytest.mark.parametrize("perfectrec", [False, True])
@pytest.mark.parametrize("fsize,fshift,T", SHAPES)
def test_signal_is_istft_of_the_result(fsize, fshift, T, perfectrec):
    p, S = start(fsize, fshift, T, perfectrec)
    for LA, n in STEPS:
        c, x = run(fsize, fshift, T, perfectrec, LA, n, True)
        ref = p.istft(c)
        assert x.shape == ref.shape
        assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()


def test_method_and_stack_forms():
    p, S = start(64, 16, 12, True)
    a = p.rtisi_la(S, 3, open_end=True)
    assert np.array_equal(a, run(64, 16, 12, True, 3, 3, True)[0])
    stack = np.stack([S, 2 * S])
    b = lws_amd.rtisi_la(stack, 64, 16, p.awin, p.swin, 3, perfectrec=True, open_end=True)
    assert np.array_equal(b[0], a)
    import lws
    assert lws.RtisiLaStream is lws_amd.RtisiLaStream and callable(p.rtisi_la_stream)
