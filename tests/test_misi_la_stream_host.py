"""CPU: misi_la(..., open_end=True), the fp64 definition of what a stream (MisiLaStream) computes.

open_end takes out of the steps with m + look_ahead <= T - 1 everything that depends on where the input ends: the tail cut of
perfectrec, and the denominator of the entered share g, which then counts every frame that would cover a sample.  What must hold:
the default is the old function bit for bit; the rows a run on S[:, :T1] commits before its end are those of a run on any longer
input (which is what lets a stream return them early); the frames whose steps never reach the end coincide with the closed form;
the signals still sum to the mixture; a mixture of any other length is refused; and the error model of the GPU tests does not
produce, on the fp64 iteration itself, the failures those tests look for."""
import numpy as np
import pytest

import lws_amd
import misi_la_cases as mc
import misi_la_stream_cases as sc


@pytest.mark.parametrize("key", sc.HOST_KEYS, ids=sc.key_id)
def test_default_is_the_old_function_bit_for_bit(key):
    """open_end=False against the shared references of tests/misi_la_cases.py's error-free run, and against the method form."""
    p, A, c0, y = mc.case(*key)
    for LA, n in sc.STEPS:
        c, s = lws_amd.misi_la(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, perfectrec=p.perfectrec, return_signals=True,
                               open_end=False)
        (rc, rs), _ = mc.host(key, LA, n)
        assert np.array_equal(c, rc) and np.array_equal(s, rs), (LA, n)
    assert np.array_equal(p.misi_la(c0[0], y[0], 3, look_ahead=1), mc.host(key, 1, 3)[0][0][0])


@pytest.mark.parametrize("key", sc.HOST_KEYS, ids=sc.key_id)
def test_prefix_property_bit_for_bit(key):
    N, hop, _, T, K = key
    lo = sc.lead_in(key)
    for LA, n in sc.STEPS:
        c2, s2 = sc.host_open(key, LA, n)
        for T1 in sorted({t for t in (T - 1, T // 2 + 1, max(LA + 1, T - 3)) if LA < t < T}):
            c1, s1 = sc.host_open(key, LA, n, rows=T1)
            rows = T1 - LA
            assert np.array_equal(c1[:, :, :rows], c2[:, :, :rows]), (LA, n, T1)
            k = max(hop * rows - lo, 0)
            assert k <= s1.shape[-1] and np.array_equal(s1[..., :k], s2[..., :k]), (LA, n, T1)
            print("misi_la open %s LA=%d n=%d T1=%d: %d rows, %d samples" % (sc.key_id(key), LA, n, T1, rows, k))


@pytest.mark.parametrize("key", sc.HOST_KEYS, ids=sc.key_id)
def test_frames_that_never_reach_the_end_coincide_with_the_closed_form(key):
    differs = False
    for LA, n in sc.STEPS:
        P, k = sc.coincide(key, LA)
        c, s = sc.host_closed(key, LA, n)
        co, so = sc.host_open(key, LA, n)
        assert co.shape == c.shape and so.shape == s.shape
        assert np.array_equal(c[:, :, :P], co[:, :, :P]), (LA, n)
        assert np.array_equal(s[..., :k], so[..., :k]), (LA, n)
        differs = differs or not np.array_equal(c, co)
        print("misi_la open %s LA=%d n=%d: P=%d of %d frames, %d of %d samples" % (sc.key_id(key), LA, n, P, key[3], k, s.shape[-1]))
    assert differs   # it does something


@pytest.mark.parametrize("key", sc.HOST_KEYS, ids=sc.key_id)
def test_signals_sum_to_the_mixture(key):
    p, A, c0, y = sc.open_case(*key)
    for LA, n in sc.STEPS:
        c, s = sc.host_open(key, LA, n)
        assert np.abs(np.abs(c) - A).max() <= 1e-12 * A.max()
        for b in range(s.shape[0]):
            tot = s[b, 0].copy()
            for k in range(1, s.shape[1]):
                tot += s[b, k]
            yb = y[b, :s.shape[-1]].astype(np.float64)
            off = np.abs(tot - yb).max() / np.abs(yb).max()
            print("misi_la open %s LA=%d n=%d b=%d: |sum s - y| %.2e max|y|" % (sc.key_id(key), LA, n, b, off))
            assert off <= 1e-15


def test_wrong_mixture_length_raises():
    key = (64, 16, True, 12, 3)
    p, A, c0, y = sc.open_case(*key)
    closed = mc.case(*key)[3]
    assert closed.shape[1] != y.shape[1]
    for bad in (closed, y[:, :-1], np.concatenate([y, y[:, :1]], axis=1), y[0]):
        with pytest.raises(ValueError, match="mixture of shape"):
            lws_amd.misi_la(c0, bad, 64, 16, p.awin, p.swin, 2, perfectrec=True, open_end=True)
    with pytest.raises(ValueError, match="mixture of shape"):
        lws_amd.misi_la(c0, y, 64, 16, p.awin, p.swin, 2, perfectrec=True)            # the open length, closed
    # a frame count the round trip does not keep is taken
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        lws_amd.misi_la(c0[:, :, :2], closed[:, :0], 64, 16, p.awin, p.swin, 2, perfectrec=True)
    c, s = lws_amd.misi_la(c0[:, :, :2], y[:, :sc.need(key, 2)], 64, 16, p.awin, p.swin, 2, perfectrec=True, open_end=True,
                           return_signals=True)
    assert c.shape == (3, 3, 2, 33) and s.shape == (3, 3, 0)


def test_method_stack_and_exports():
    key = (64, 16, True, 12, 3)
    p, A, c0, y = sc.open_case(*key)
    a = p.misi_la(c0[0], y[0], 3, open_end=True)
    assert np.array_equal(a, sc.host_open(key, 3, 3)[0][0])
    import lws
    assert lws.MisiLaStream is lws_amd.MisiLaStream and callable(p.misi_la_stream)


@pytest.mark.parametrize("run", sc.gpu_runs(), ids=lambda r: "%s-LA%d-n%d-rows%s" % (sc.key_id(r[0]), r[1], r[2], r[3]))
def test_error_model_moves_almost_no_bin_far(run):
    """For every shape and step of the GPU file: the perturbation model alone moves at most 0.02 % of a source's bins by more than
    1e-3 max A, five times clear of the 0.1 % the GPU test allows the device (the condition tests/test_misi_la_host.py sets)."""
    key, LA, n, rows = run
    p, A, c0, y = sc.open_case(*key)
    ref, per = sc.host_open(key, LA, n, rows=rows)[0], sc.host_open_perturbed(key, LA, n, rows=rows)[0]
    far = np.mean(np.abs(per - ref) > 1e-3 * A[:, :, :rows].max(axis=(2, 3), keepdims=True), axis=(2, 3))
    print("misi_la open model %s LA=%d n=%d rows=%s: far bins at most %.4f%%" % (sc.key_id(key), LA, n, rows, 100 * far.max()))
    assert far.max() <= 2e-4
