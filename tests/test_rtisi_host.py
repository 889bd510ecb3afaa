"""CPU: the host fp64 definition of RTISI-LA (lws_amd.rtisi_la) -- its identities, its edge cases and its argument errors -- and the
argument errors of the C entry point, which must come before any device call (the pointers here are bogus)."""
import functools

import numpy as np
import pytest

import lws_amd
from lws_amd import _capi

BOGUS = 64


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, noise=0.3):
    """p, X = stft of noise with exactly T frames, c0 = X with `noise` rad of Gaussian phase noise."""
    rng = np.random.default_rng(1000 * fsize + 10 * fshift + perfectrec)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    n = lws_amd.istft(np.zeros((T, fsize // 2 + 1), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    X = p.stft(rng.standard_normal(n))
    assert X.shape == (T, fsize // 2 + 1)
    c0 = X * np.exp(1j * noise * rng.standard_normal(X.shape))
    for a in (X, c0):
        a.setflags(write=False)
    return p, X, c0


CASES = [(64, 16, True, 12), (64, 16, False, 9), (48, 16, True, 7), (256, 96, False, 5), (256, 96, True, 6)]


@pytest.mark.parametrize("key", CASES)
def test_result_magnitudes_are_the_targets(key):
    p, X, c0 = case(*key)
    out = p.rtisi_la(c0, 4, look_ahead=2)
    assert out.dtype == np.complex128 and out.shape == c0.shape
    assert np.abs(np.abs(out) - np.abs(c0)).max() <= 1e-13 * np.abs(c0).max()
    A = np.roll(np.abs(X), 1, axis=0) * 0.7 + 0.05 * np.abs(X).max()
    out = p.rtisi_la(c0, 3, magnitudes=A)
    assert np.abs(np.abs(out) - A).max() <= 1e-13 * A.max()


@pytest.mark.parametrize("key", CASES)
@pytest.mark.parametrize("LA,n", [(0, 2), (3, 3), (20, 1), (2, 0)])
def test_signal_is_istft_of_the_result(key, LA, n):
    p, X, c0 = case(*key)
    out, sig = p.rtisi_la(c0, n, look_ahead=LA, return_signal=True)
    want = p.istft(out)
    assert sig.shape == want.shape
    print("rtisi_la signal vs istft: %.2e of max |x| = %.2f" % (np.abs(sig - want).max() / np.abs(want).max(), np.abs(want).max()))
    assert np.abs(sig - want).max() <= 1e-15 * np.abs(want).max()   # the same frames added in the same order: a few roundings apart


@pytest.mark.parametrize("key", CASES)
@pytest.mark.parametrize("n", [1, 3])
def test_whole_future_look_ahead_starts_as_griffin_lim(key, n):
    """With LA >= T - 1 every frame is active at the first commit: n plain Griffin-Lim steps, whose frame 0 is final."""
    p, X, c0 = case(*key)
    T = c0.shape[0]
    want = p.griffin_lim(c0, n, alpha=0.0)
    for LA in (T - 1, T + 4):
        out = p.rtisi_la(c0, n, look_ahead=LA)
        assert np.abs(out[0] - want[0]).max() <= 1e-11 * np.abs(c0).max()


@pytest.mark.parametrize("key", [(64, 16, True, 12), (256, 96, False, 9)])
@pytest.mark.parametrize("LA", [0, 1, 3])
def test_causality_bit_for_bit(key, LA):
    """Frames 0..m of the result do not change by a bit when input frames > m + LA do (given explicit magnitudes)."""
    p, X, c0 = case(*key)
    rng = np.random.default_rng(5)
    A = np.abs(c0)
    T = c0.shape[0]
    ref = p.rtisi_la(c0, 3, look_ahead=LA, magnitudes=A)
    for m in (0, 2, T - LA - 2):
        c1 = c0.copy()
        c1[m + LA + 1:] = A[m + LA + 1:] * np.exp(2j * np.pi * rng.random(A[m + LA + 1:].shape))
        out = p.rtisi_la(c1, 3, look_ahead=LA, magnitudes=A)
        assert np.array_equal(out[:m + 1], ref[:m + 1])
        assert not np.array_equal(out[m + 1], ref[m + 1])


def test_zero_iterations_return_the_input():
    p, X, c0 = case(64, 16, True, 12)
    assert p.rtisi_la(c0, 0) is c0
    out, sig = p.rtisi_la(c0[None], 0, return_signal=True)
    assert np.array_equal(out, c0[None]) and np.allclose(sig[0], p.istft(c0), rtol=0, atol=1e-13 * np.abs(sig).max())


def test_one_frame_and_fewer_frames_than_the_look_ahead():
    p = lws_amd.lws(64, 16, perfectrec=False)
    rng = np.random.default_rng(2)
    for T in (1, 2, 3):
        c0 = rng.standard_normal((T, 33)) + 1j * rng.standard_normal((T, 33))
        out, sig = p.rtisi_la(c0, 3, look_ahead=3, return_signal=True)
        assert out.shape == c0.shape and np.isfinite(out.view(np.float64)).all()
        assert np.abs(np.abs(out) - np.abs(c0)).max() <= 1e-13
        assert np.abs(sig - p.istft(out)).max() <= 1e-14
        # every frame is active at the first commit: any larger look-ahead is the same computation
        assert np.array_equal(out, p.rtisi_la(c0, 3, look_ahead=T - 1))
        assert np.array_equal(out, p.rtisi_la(c0, 3, look_ahead=50))
    one = p.rtisi_la(c0[:1], 2, look_ahead=0)
    assert np.abs(one - p.griffin_lim(c0[:1], 2, alpha=0.0)).max() <= 1e-12


def test_stack_is_its_members_and_the_method_uses_the_plans_look_ahead():
    p, X, c0 = case(64, 16, True, 12)
    q, Y, d0 = case(64, 16, True, 12, 0.5)
    S = np.stack([c0, d0])
    out, sig = p.rtisi_la(S, 2, return_signal=True)
    assert out.shape == S.shape and sig.shape == (2, len(p.istft(c0)))
    for b in range(2):
        o, s = p.rtisi_la(S[b], 2, return_signal=True)
        assert np.array_equal(o, out[b]) and np.array_equal(s, sig[b])
    assert p.look_ahead == 3
    assert np.array_equal(out, lws_amd.rtisi_la(S, 64, 16, p.awin, p.swin, 2, look_ahead=3, perfectrec=True))
    p1 = lws_amd.lws(64, 16, perfectrec=True, look_ahead=1)
    assert np.array_equal(p1.rtisi_la(S, 2), p.rtisi_la(S, 2, look_ahead=1))
    assert not np.array_equal(p1.rtisi_la(S, 2), out)


def test_perturbation_hook_sees_every_inner_iteration():
    p, X, c0 = case(64, 16, False, 9)
    seen = []

    def hook(m, it, b, Y):
        seen.append((m, it, b, Y.shape))
        return Y
    out = lws_amd.rtisi_la(c0, 64, 16, p.awin, p.swin, 2, look_ahead=3, _perturb=hook)
    assert np.array_equal(out, p.rtisi_la(c0, 2))
    assert seen == [(m, it, 0, (min(m + 3, 8) - m + 1, 33)) for m in range(9) for it in (1, 2)]


def test_argument_errors():
    p, X, c0 = case(64, 16, True, 12)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            p.rtisi_la(c0, bad)
        with pytest.raises(ValueError):
            p.rtisi_la(c0, 2, look_ahead=bad)
    with pytest.raises(ValueError):
        p.rtisi_la(c0[0], 2)                                   # one dimension
    with pytest.raises(ValueError):
        p.rtisi_la(c0, 2, magnitudes=np.abs(c0)[:-1])
    with pytest.raises(ValueError):
        p.rtisi_la(c0[:, :-1], 2)                              # bins of another frame size
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        p.rtisi_la(c0[:2], 2)                                  # as griffin_lim: the round trip does not keep two frames
    with pytest.raises(ValueError):
        p.griffin_lim(c0[:2], 2)
    assert p.rtisi_la(c0[:2], 0) is not None                   # zero iterations ask for no round trip


def test_consistency_improves_from_noisy_true_phases():
    p, X, c0 = case(64, 16, True, 12)
    before = p.get_consistency(c0)
    after = p.get_consistency(p.rtisi_la(c0, 6, look_ahead=3))
    print("rtisi_la (64,16,perfectrec) T=12 LA=3 n=6: consistency %.2f -> %.2f dB" % (before, after))
    assert after >= before + 10.0


def test_entry_point_checks_its_arguments_before_any_device_call():
    lib = _capi.load()
    w = np.ones(64)
    wp = w.ctypes.data

    def call(C=BOGUS, x=None, B=3, M=9, N=64, hop=16, a=wp, s=wp, pr=0, iters=2, LA=3, device=0):
        return lib.lws_rtisi_la_dev(device, C, None, x, B, M, N, hop, a, s, pr, iters, LA, None)
    invalid, unsupported = _capi.LWS_ERR_INVALID, _capi.LWS_ERR_UNSUPPORTED
    assert call(iters=-1) == invalid and b"iterations" in lib.lws_last_error()
    assert call(LA=-1) == invalid and b"look-ahead" in lib.lws_last_error()
    assert call(C=None) == invalid and call(a=None) == invalid and call(s=None) == invalid
    assert call(M=0) == invalid and call(B=-1) == invalid and call(hop=0) == invalid and call(hop=65) == invalid
    assert call(device=-1) == invalid
    assert call(N=8192, hop=2048) == unsupported and call(N=30, hop=10) == unsupported and call(N=63) == unsupported
    for M in (1, 2):
        assert call(M=M, pr=1) == invalid and b"too few frames for perfectrec" in lib.lws_last_error()
    assert call(M=9, N=32, hop=32, pr=1) == invalid
    # nothing to do: no iterations and no signal asked for, or an empty batch
    assert call(iters=0) == _capi.LWS_OK and call(M=2, pr=1, iters=0) == _capi.LWS_OK and call(B=0) == _capi.LWS_OK
