"""CPU: the host fp64 definition of online MISI (lws_amd.misi_la) -- the properties it was designed for, its edge cases and its
argument errors -- the argument errors of the C entry point, which must come before any device call (the pointers here are bogus),
and what the error model of tests/test_gpu_misi_la.py does to the fp64 iteration itself."""
import numpy as np
import pytest

import lws_amd
import misi_la_cases as mc
from lws_amd import _capi

BOGUS = 64
CASES = [(64, 16, True, 12, 3), (64, 16, False, 9, 2), (48, 16, True, 7, 1), (256, 96, False, 5, 2), (256, 96, True, 6, 3)]


def prepad(N, hop):
    """The samples istft cuts in front under perfectrec (lws.pyx:55-60)."""
    return N - hop if N % hop == 0 else N - N % hop


def f64(key):
    """The case in fp64: p, c0 (B, K, T, F) complex128, y (B, len) float64."""
    p, A, c0, y = mc.case(*key)
    return p, c0.astype(np.complex128), y.astype(np.float64)


@pytest.mark.parametrize("key", CASES, ids=mc.key_id)
@pytest.mark.parametrize("n", [1, 3])
def test_whole_future_look_ahead_starts_as_misi(key, n):
    """With LA >= T - 1 every frame is active at the first commit and every g is 1: n steps of misi(), whose frame 0 is final."""
    p, c0, y = f64(key)
    T = c0.shape[2]
    want = p.misi(c0, y, n)
    for LA in (T - 1, T + 4):
        out = p.misi_la(c0, y, n, look_ahead=LA)
        for b in range(c0.shape[0]):
            d = np.abs(out[b, :, 0] - want[b, :, 0]).max() / np.abs(c0[b]).max()
            print("misi_la %s n=%d LA=%d b=%d: frame 0 against misi %.2e max A" % (key, n, LA, b, d))
            assert d <= 1e-13


@pytest.mark.parametrize("key", CASES, ids=mc.key_id)
@pytest.mark.parametrize("LA,n", [(0, 2), (3, 3), (20, 1), (2, 0)])
def test_signals_sum_to_the_mixture(key, LA, n):
    p, c0, y = f64(key)
    out, s = p.misi_la(c0, y, n, look_ahead=LA, return_signals=True)
    assert s.shape == c0.shape[:2] + y.shape[1:]
    for b in range(c0.shape[0]):
        tot = s[b, 0].copy()
        for k in range(1, s.shape[1]):
            tot += s[b, k]
        off = np.abs(tot - y[b]).max() / np.abs(y[b]).max()
        print("misi_la %s LA=%d n=%d b=%d: |sum s - y| %.2e max|y|" % (key, LA, n, b, off))
        assert off <= 1e-15


@pytest.mark.parametrize("key", [(64, 16, True, 12, 3), (256, 96, False, 9, 2)], ids=mc.key_id)
def test_causality_bit_for_bit(key):
    """With explicit magnitudes, LA = 3 and n = 3: other phases in the input frames >= 6, or another mixture from the uncut sample
    hop 5 + N on (the first one behind frame 5), leave the output frames 0..2 as they are and change frame 3."""
    p, c0, y = f64(key)
    A = np.abs(c0)
    rng = np.random.default_rng(5)
    ref = p.misi_la(c0, y, 3, look_ahead=3, magnitudes=A)
    c1 = c0.copy()
    c1[:, :, 6:] = A[:, :, 6:] * np.exp(2j * np.pi * rng.random(A[:, :, 6:].shape))
    lo = prepad(p.fsize, p.fshift) if p.perfectrec else 0
    y1 = y.copy()
    first = p.fshift * 5 + p.fsize - lo
    assert 0 < first < y.shape[1]
    y1[:, first:] += np.abs(y).max(axis=1, keepdims=True) * rng.standard_normal(y1[:, first:].shape)
    for other in (p.misi_la(c1, y, 3, look_ahead=3, magnitudes=A), p.misi_la(c0, y1, 3, look_ahead=3, magnitudes=A)):
        assert np.array_equal(other[:, :, :3], ref[:, :, :3])
        for b in range(c0.shape[0]):
            for k in range(c0.shape[1]):
                assert not np.array_equal(other[b, k, 3], ref[b, k, 3])
    # ... and one sample earlier the mixture does reach frame 2
    y2 = y.copy()
    y2[:, first - 1] += np.abs(y).max(axis=1)
    assert not np.array_equal(p.misi_la(c0, y2, 3, look_ahead=3, magnitudes=A)[:, :, 2], ref[:, :, 2])


def test_stack_is_its_members_and_the_method_uses_the_plans_look_ahead():
    key = (64, 16, True, 12, 3)
    p, c0, y = f64(key)
    out, s = p.misi_la(c0, y, 2, return_signals=True)
    assert out.shape == c0.shape and out.dtype == np.complex128 and s.shape == (3, 3, y.shape[1])
    for b in range(3):
        o, sb = p.misi_la(c0[b], y[b], 2, return_signals=True)
        assert o.shape == c0.shape[1:] and sb.shape == s.shape[1:]
        assert np.array_equal(o, out[b]) and np.array_equal(sb, s[b])
    assert p.look_ahead == 3
    assert np.array_equal(out, lws_amd.misi_la(c0, y, 64, 16, p.awin, p.swin, 2, look_ahead=3, perfectrec=True))
    p1 = lws_amd.lws(64, 16, perfectrec=True, look_ahead=1)
    assert np.array_equal(p1.misi_la(c0, y, 2), p.misi_la(c0, y, 2, look_ahead=1))
    assert not np.array_equal(p1.misi_la(c0, y, 2), out)
    assert np.array_equal(p.misi_la(c0, y, 2, look_ahead=11), p.misi_la(c0, y, 2, look_ahead=40))   # all 12 frames active either way


def test_zero_iterations_return_the_input():
    p, c0, y = f64((64, 16, True, 12, 3))
    assert np.array_equal(p.misi_la(c0[0], y[0], 0), c0[0])
    assert p.misi_la(c0, y, 0) is c0
    out, s = p.misi_la(c0, y, 0, return_signals=True)
    assert np.array_equal(out, c0)
    for b in range(3):                           # the signals of the start itself, with their residual shared out
        x = np.stack([p.istft(c) for c in c0[b]])
        want = x + (y[b] - x.sum(axis=0)) / 3
        assert np.abs(s[b] - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("key", CASES, ids=mc.key_id)
def test_result_magnitudes_are_the_targets(key):
    p, c0, y = f64(key)
    out = p.misi_la(c0, y, 4, look_ahead=2)
    assert np.abs(np.abs(out) - np.abs(c0)).max() <= 1e-13 * np.abs(c0).max()
    A = mc.magnitudes_of(np.abs(c0))
    out = p.misi_la(c0, y, 3, magnitudes=A)
    assert np.abs(np.abs(out) - A).max() <= 1e-13 * A.max()
    assert not np.array_equal(out, p.misi_la(c0, y, 3))


def test_silence_in_exact_zeros_out():
    p, c0, y = f64((64, 16, True, 12, 3))
    Z = np.zeros(c0.shape)
    out, s = p.misi_la(c0 * 0, y * 0, 4, return_signals=True)
    assert (out == 0).all() and (s == 0).all()
    out, s = p.misi_la(c0, y * 0, 4, magnitudes=Z, return_signals=True)
    assert (out == 0).all() and (s == 0).all()
    # one silent source among sounding ones stays silent in the spectrogram; its signal is its share of the mixture error
    A = np.abs(c0).copy()
    A[:, 1] = 0.0
    out = p.misi_la(c0, y, 4, magnitudes=A)
    assert (out[:, 1] == 0).all() and np.isfinite(out.view(np.float64)).all()


def test_one_frame_and_fewer_frames_than_the_look_ahead():
    p = lws_amd.lws(64, 16, perfectrec=False)
    rng = np.random.default_rng(2)
    for T in (1, 2, 3):
        c0 = rng.standard_normal((2, T, 33)) + 1j * rng.standard_normal((2, T, 33))
        y = rng.standard_normal(16 * (T - 1) + 64)
        out, s = p.misi_la(c0, y, 3, look_ahead=3, return_signals=True)
        assert out.shape == c0.shape and np.isfinite(out.view(np.float64)).all()
        assert np.abs(np.abs(out) - np.abs(c0)).max() <= 1e-13
        assert np.array_equal(out, p.misi_la(c0, y, 3, look_ahead=T - 1))
        assert np.array_equal(out, p.misi_la(c0, y, 3, look_ahead=50))


def test_perturbation_hook_sees_every_inner_iteration():
    p, c0, y = f64((64, 16, False, 9, 2))
    seen = []

    def hook(m, it, b, X):
        seen.append((m, it, b, X.shape))
        return X
    out = lws_amd.misi_la(c0[:2], y[:2], 64, 16, p.awin, p.swin, 2, look_ahead=3, _perturb=hook)
    assert np.array_equal(out, p.misi_la(c0[:2], y[:2], 2))
    assert seen == [(m, it, b, (2, min(m + 3, 8) - m + 1, 33)) for b in range(2) for m in range(9) for it in (1, 2)]


def test_argument_errors():
    p, c0, y = f64((64, 16, True, 12, 3))
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            p.misi_la(c0, y, bad)
        with pytest.raises(ValueError):
            p.misi_la(c0, y, 2, look_ahead=bad)
    with pytest.raises(ValueError):
        p.misi_la(c0[0, 0], y[0], 2)                           # a 2-D S
    with pytest.raises(ValueError):
        p.misi_la(c0[None], y[None], 2)                        # a 5-D S
    with pytest.raises(ValueError):
        p.misi_la(c0, y, 2, magnitudes=np.abs(c0)[:, :, :-1])
    with pytest.raises(ValueError):
        p.misi_la(c0, y[:, :-1], 2)                            # wrong mixture length
    with pytest.raises(ValueError):
        p.misi_la(c0, y[0], 2)                                 # one mixture for a stack
    with pytest.raises(ValueError):
        p.misi_la(c0[0], y, 2)                                 # a stack of mixtures for one set of sources
    with pytest.raises(ValueError, match="no sources"):
        p.misi_la(c0[:, :0], y, 2)
    with pytest.raises(ValueError):
        p.misi_la(c0[:, :, :, :-1], y, 2)                      # bins of another frame size
    with pytest.raises(ValueError):
        lws_amd.misi_la(np.ones((2, 5, 33), complex), np.zeros(16 * 4 + 63), 63, 16, np.ones(63), np.ones(63), 2)   # odd frame size
    short = np.zeros((3, lws_amd.istft(np.zeros((2, 33), complex), 16, p.swin, perfectrec=True).shape[0]))
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        p.misi_la(c0[:, :, :2], short, 2)                      # as misi: the round trip does not keep two frames
    with pytest.raises(ValueError):
        p.misi(c0[:, :, :2], short, 2)
    assert p.misi_la(c0[:, :, :2], short, 0) is not None       # zero iterations ask for no round trip


def restated(p, S, y, n, LA, A):
    """misi_la for one mixture, stated otherwise: no running sums -- every windowed frame is transformed back from c in every inner
    iteration, the committed ones included -- and g as one minus the share of the frames still to come."""
    K, T, F = S.shape
    N, hop = p.fsize, p.fshift
    total = hop * (T - 1) + N
    idx = hop * np.arange(T)[:, None] + np.arange(N)[None, :]
    lo, hi = 0, total
    if p.perfectrec:
        lo, hi = prepad(N, hop), total - (N - hop)
    keep = np.zeros(total)
    keep[lo:hi] = 1.0
    yfull = np.zeros(total)
    yfull[lo:hi] = y
    w = p.awin * p.swin

    def ola(frames, first=0):
        """Overlap-add of the frames first, first + 1, ... (one pass over all their samples, in index order)."""
        at = idx[first: first + len(frames)]
        return np.bincount(at.ravel(), weights=np.asarray(frames).ravel(), minlength=total)
    den = ola(np.tile(w, (T, 1)))
    c = S.astype(np.complex128)
    for m in range(T):
        last = min(m + LA, T - 1)
        later = ola(np.tile(w, (T - 1 - last, 1)), last + 1)
        g = np.where(den != 0, 1.0 - later / np.where(den != 0, den, 1.0), 1.0)
        for it in range(n):
            x = keep * np.stack([ola(p.swin * np.fft.irfft(c[k, :last + 1], N, axis=1)) for k in range(K)])
            x += keep * (g * yfull - x.sum(axis=0)) / K
            X = np.fft.rfft(p.awin * x[:, idx[m:last + 1]], axis=2)
            mag = np.abs(X)
            c[:, m:last + 1] = np.where(mag > 0, A[:, m:last + 1] * X / np.where(mag > 0, mag, 1.0), A[:, m:last + 1])
    return c


@pytest.mark.parametrize("key", CASES, ids=mc.key_id)
@pytest.mark.parametrize("LA,n", [(0, 2), (1, 3), (3, 3), (20, 2)])
def test_agrees_with_a_restatement_of_other_structure(key, LA, n):
    p, c0, y = f64(key)
    A = mc.magnitudes_of(np.abs(c0))
    out = p.misi_la(c0, y, n, look_ahead=LA, magnitudes=A)
    for b in range(c0.shape[0]):
        want = restated(p, c0[b], y[b], n, LA, A[b])
        for k in range(c0.shape[1]):
            d = mc.rel(out[b, k], want[k])
            print("misi_la %s LA=%d n=%d b=%d k=%d: rel-L2 to the restatement %.2e" % (key, LA, n, b, k, d))
            assert d <= 1e-12


def test_consistency_with_the_mixture_improves_from_noisy_true_phases():
    """What the feature is for, in the definition: at LA = 3 the sources move towards the truth and towards their mixture."""
    key = (48, 16, True, 24, 2)
    p, c0, y = f64(key)
    rng = np.random.default_rng(1000 * 48 + 10 * 16 + 1)                    # the true spectrograms of mc.case
    src = rng.standard_normal((3, 2, y.shape[1])) * mc.SOURCES[None, :2, None] * mc.SCALES[:, None, None]
    X = np.stack([p.stft(x) for x in src[0]])

    def mixture_db(c):
        e = y[0] - sum(p.istft(ck) for ck in c)
        return 10 * np.log10(np.sum(y[0] ** 2) / np.sum(e ** 2))
    out = p.misi_la(c0[0], y[0], 5, look_ahead=3)
    print("misi_la lws(48,16) K=2 LA=3 n=5: mixture consistency %.1f -> %.1f dB, distance to the truth %.3f -> %.3f"
          % (mixture_db(c0[0]), mixture_db(out), mc.rel(c0[0], X), mc.rel(out, X)))
    assert mixture_db(out) >= mixture_db(c0[0]) + 10.0 and mc.rel(out, X) < 0.5 * mc.rel(c0[0], X)


@pytest.mark.parametrize("key", mc.keys(), ids=mc.key_id)
def test_error_model_moves_almost_no_bin_far(key):
    """For every row of the GPU table, at every step count: the perturbation model alone moves at most 0.02 % of a source's bins by
    more than 1e-3 max A, five times clear of the 0.1 % the GPU test allows the device."""
    p, A, c0, y = mc.case(*key)
    worst = 0.0
    for LA, n in mc.STEPS:
        (ref, _), (per, _) = mc.host(key, LA, n)
        far = np.mean(np.abs(per - ref) > 1e-3 * A.max(axis=(2, 3), keepdims=True), axis=(2, 3))
        worst = max(worst, far.max())
        print("misi_la model %s LA=%d n=%d: far bins at most %.4f%%" % (mc.key_id(key), LA, n, 100 * far.max()))
    assert worst <= 2e-4


@pytest.mark.parametrize("key", sorted(mc.EDGE_SHAPES), ids=mc.key_id)
def test_error_model_moves_almost_no_bin_far_at_the_edge_shapes(key):
    """The same condition on every row and step of the second table of the GPU test."""
    p, A, c0, y = mc.case(*key)
    worst = 0.0
    for LA, n, _ in mc.EDGE_SHAPES[key][1]:
        (ref, _), (per, _) = mc.host(key, LA, n)
        assert np.isfinite(ref.view(np.float64)).all()
        far = np.mean(np.abs(per - ref) > 1e-3 * A.max(axis=(2, 3), keepdims=True), axis=(2, 3))
        worst = max(worst, far.max())
        print("misi_la model %s LA=%d n=%d: far bins at most %.4f%%" % (mc.key_id(key), LA, n, 100 * far.max()))
    assert worst <= 2e-4


def test_entry_point_checks_its_arguments_before_any_device_call():
    lib = _capi.load()
    w = np.ones(64)
    wp = w.ctypes.data

    def call(C=BOGUS, y=BOGUS, x=None, B=3, K=2, M=9, N=64, hop=16, a=wp, s=wp, pr=0, iters=2, LA=3, device=0):
        return lib.lws_misi_la_dev(device, C, None, y, x, B, K, M, N, hop, a, s, pr, iters, LA, None)
    invalid, unsupported = _capi.LWS_ERR_INVALID, _capi.LWS_ERR_UNSUPPORTED
    assert call(K=0) == invalid and b"sources" in lib.lws_last_error()
    assert call(iters=-1) == invalid and b"iterations" in lib.lws_last_error()
    assert call(LA=-1) == invalid and b"look-ahead" in lib.lws_last_error()
    assert call(C=None) == invalid and call(y=None) == invalid and call(a=None) == invalid and call(s=None) == invalid
    assert call(M=0) == invalid and call(B=-1) == invalid and call(hop=0) == invalid and call(hop=65) == invalid
    assert call(device=-1) == invalid
    assert call(N=8192, hop=2048) == unsupported and call(N=30, hop=10) == unsupported and call(N=63) == unsupported
    for M in (1, 2):
        assert call(M=M, pr=1) == invalid
    assert call(M=5, pr=1, iters=0) == _capi.LWS_OK and call(M=9, N=32, hop=32, pr=1) == invalid
    # nothing to do: no iterations and no signals asked for, or an empty batch
    assert call(iters=0) == _capi.LWS_OK and call(B=0) == _capi.LWS_OK
