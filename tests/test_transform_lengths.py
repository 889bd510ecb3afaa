"""CPU: the frame and sample counts of the device transforms (lws_stft_frames, lws_istft_length) are those of the host functions
at every edge, and the refusals / empty results decided from them come back before any device call -- on a box without a GPU a
call that went on to the device would return LWS_ERR_HIP, not the status asserted here."""
import numpy as np
import pytest

import lws_amd
from lws_amd import _capi

SHAPES = [(32, 1), (32, 16), (32, 32), (36, 12), (36, 27), (64, 16), (64, 48), (64, 64), (100, 30), (4092, 1023)]


@pytest.mark.parametrize("fsize,fshift", SHAPES)
@pytest.mark.parametrize("perfectrec", [True, False])
def test_counts_are_the_host_functions(fsize, fshift, perfectrec):
    awin = np.ones(fsize)
    F = fsize // 2 + 1
    for M in (1, 2, 3, 4, 5, 8, 33, 64):
        ref = lws_amd.istft(np.zeros((M, F), complex), fshift, awin, perfectrec=perfectrec).shape[0]
        assert _capi.istft_length(M, fsize, fshift, perfectrec) == ref, (M, ref)
    for n in sorted({0, 1, fshift - 1, fshift, fsize - fshift - 1, fsize - fshift, fsize - fshift + 1, fsize - 1, fsize, fsize + 1,
                     2 * fsize + fshift, 2 * fsize + fshift + 1} - {-1}):
        ref = lws_amd.stft(np.zeros(n), fsize, fshift, awin, perfectrec=perfectrec).shape[0]
        assert _capi.stft_frames(n, fsize, fshift, perfectrec) == ref, (n, ref)
    assert _capi.stft_frames(-1, fsize, fshift, perfectrec) == -1


# a pointer the library must never follow: every call below has to return before it would
BOGUS = 64


def test_griffin_lim_refuses_too_few_frames_for_perfectrec():
    lib = _capi.load()
    w = np.ones(64)
    for M in (1, 2):
        rc = lib.lws_griffin_lim_dev(0, BOGUS, None, 3, M, 64, 16, w.ctypes.data, w.ctypes.data, 1, 2, 0.5, None, None)
        assert rc == _capi.LWS_ERR_INVALID and b"too few frames for perfectrec" in lib.lws_last_error()
    # zero iterations ask for no round trip
    assert lib.lws_griffin_lim_dev(0, BOGUS, None, 3, 2, 64, 16, w.ctypes.data, w.ctypes.data, 1, 0, 0.5, None, None) == _capi.LWS_OK
    # hop == frame: perfectrec keeps no sample of any number of frames
    rc = lib.lws_griffin_lim_dev(0, BOGUS, None, 3, 9, 32, 32, w.ctypes.data, w.ctypes.data, 1, 2, 0.5, None, None)
    assert rc == _capi.LWS_ERR_INVALID and b"too few frames for perfectrec" in lib.lws_last_error()


def test_consistency_refuses_too_few_frames_for_perfectrec():
    lib = _capi.load()
    w = np.ones(64)
    out = np.zeros(2 * 3)
    for M in (1, 2):
        rc = lib.lws_consistency_dev(0, BOGUS, 3, M, 64, 16, w.ctypes.data, w.ctypes.data, 1, out.ctypes.data, None)
        assert rc == _capi.LWS_ERR_INVALID and b"too few frames for perfectrec" in lib.lws_last_error()


def test_misi_still_refuses_too_few_frames_for_perfectrec():
    lib = _capi.load()
    w = np.ones(64)
    for M in (1, 2, 3):                                        # (the frames the round trip does not keep are those that keep no sample)
        rc = lib.lws_misi_dev(0, BOGUS, None, BOGUS, 3, 2, M, 64, 16, w.ctypes.data, w.ctypes.data, 1, 1, None, None, None)
        assert rc == _capi.LWS_ERR_INVALID and b"leave no samples" in lib.lws_last_error()
    rc = lib.lws_misi_dev(0, BOGUS, None, BOGUS, 3, 2, 3, 32, 32, w.ctypes.data, w.ctypes.data, 1, 0, BOGUS, None, None)
    assert rc == _capi.LWS_ERR_INVALID and b"leave no samples" in lib.lws_last_error()


def test_istft_of_nothing_kept_returns_without_device_work():
    lib = _capi.load()
    w = np.ones(64)
    # frames that perfectrec cuts away entirely
    assert _capi.istft_length(1, 64, 16, True) == 0 and _capi.istft_length(3, 32, 32, True) == 0
    assert lib.lws_istft_dev(0, BOGUS, 3, 1, 64, 16, w.ctypes.data, 1, None, None) == _capi.LWS_OK
    assert lib.lws_istft_dev(0, BOGUS, 3, 3, 32, 32, w.ctypes.data, 1, None, None) == _capi.LWS_OK
    assert lib.lws_istft_dev(0, BOGUS, 3, 0, 64, 16, w.ctypes.data, 1, None, None) == _capi.LWS_ERR_INVALID      # no frames
    assert lib.lws_istft_dev(0, BOGUS, 3, -1, 64, 16, w.ctypes.data, 0, None, None) == _capi.LWS_ERR_INVALID
    assert lib.lws_istft_dev(0, BOGUS, 3, 1, 64, 65, w.ctypes.data, 1, None, None) == _capi.LWS_ERR_INVALID      # the shape is still checked


def test_stft_of_less_than_a_frame_returns_without_device_work():
    lib = _capi.load()
    w = np.ones(64)
    # shorter than one frame even after padding to the hop grid
    for n in (0, 10, 47, 48):
        assert _capi.stft_frames(n, 64, 16, False) == 0
        assert lib.lws_stft_dev(0, BOGUS, 3, n, 64, 16, w.ctypes.data, 0, None, None) == _capi.LWS_OK
        assert lib.lws_stft_zp_dev(0, BOGUS, 3, n, 64, 96, 16, w.ctypes.data, 0, None, None) == _capi.LWS_OK
    assert _capi.stft_frames(49, 64, 16, False) == 1                                  # padded up to one frame, as on the host
    assert lib.lws_stft_dev(0, BOGUS, 3, -1, 64, 16, w.ctypes.data, 0, None, None) == _capi.LWS_ERR_INVALID
    assert lib.lws_stft_dev(0, BOGUS, 3, 10, 64, 65, w.ctypes.data, 0, None, None) == _capi.LWS_ERR_INVALID      # the shape is still checked
