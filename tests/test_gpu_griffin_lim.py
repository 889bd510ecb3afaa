"""GPU: Griffin-Lim refinement on the device (lws_gla.hip) against the host fp64 definition (lws_amd.griffin_lim).

The value check has no fixed tolerance: its bar is measured here, on the host side only.  The device transforms are allowed an
error of 3e-6 max|X| by tests/test_gpu_stft.py; the bar is the rel-L2 distance the host iteration moves when every projection
X_i is perturbed by seeded complex Gaussian noise of standard deviation 1e-6 max|X_i| per component, times 3 (rounding error is
structured, the model's noise is not).  Distances, caps and trace bars are taken per spectrogram, so that the small-scale
members of a stack are held as tightly as the large ones.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest

import lws_amd

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALES = np.array([1.0, 1e-3, 300.0])
STEPS = [(1, 0.0), (3, 0.0), (3, 0.99), (8, 0.99)]
# (fsize, fshift, perfectrec) -> frames: odd and even counts, 1 and 2 (with perfectrec the round trip keeps the frame count
# only from ceil(fsize / fshift) - 1 frames on); every case has more than one workgroup (one per pair of frames and spectrogram)
SHAPES = {
    (64, 16, False): 9, (64, 16, True): 12,            # power of two
    (48, 16, False): 1, (48, 16, True): 7,             # odd factor 3
    (256, 96, False): 2, (256, 96, True): 5,           # hop does not divide the frame
    (1000, 250, False): 6, (1000, 250, True): 5,       # odd factor 125
    (4096, 1024, False): 5, (4096, 1024, True): 4,     # the large-LDS path
}


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, B=3):
    """p, A = |stft(noise)| (B, T, F) at three scales, c_0 = A exp(2 pi j u) rounded to complex64 (what the device is given)."""
    rng = np.random.default_rng(1000 * fsize + 10 * fshift + perfectrec)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    A = np.abs(np.stack([p.stft(x) for x in rng.standard_normal((B, n))])) * SCALES[:B, None, None]
    assert A.shape == (B, T, F)
    c0 = (A * np.exp(2j * np.pi * rng.random(A.shape))).astype(np.complex64)
    for a in (A, c0):
        a.setflags(write=False)
    return p, A, c0


def perturbation(seed):
    rng = np.random.default_rng(seed)

    def f(i, b, X):
        sigma = 1e-6 * np.abs(X).max()
        return X + sigma * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


@functools.lru_cache(maxsize=None)
def host(key, n, alpha, explicit=False):
    """Host fp64 result and trace, and the same under the perturbation model."""
    p, A, c0 = case(*key)
    mags = magnitudes_of(A) if explicit else None
    ref = p.griffin_lim(c0, n, alpha=alpha, magnitudes=mags, return_trace=True)
    kw = dict(alpha=alpha, magnitudes=mags, perfectrec=p.perfectrec, return_trace=True, _perturb=perturbation(n + 17))
    per = lws_amd.griffin_lim(c0, p.fsize, p.fshift, p.awin, p.swin, n, **kw)
    return ref, per


def magnitudes_of(A):
    """Targets that differ from |c_0|: its magnitudes rolled along time and rescaled (a spectrogram of another signal)."""
    return np.roll(A, 1, axis=1) * 0.7 + 0.05 * A.max(axis=(1, 2), keepdims=True)


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def check_against_host(key, n, alpha, explicit=False):
    p, A, c0 = case(*key)
    (ref, ref_db), (per, per_db) = host(key, n, alpha, explicit)
    target = magnitudes_of(A) if explicit else np.abs(c0).astype(np.float64)
    out, db = p.griffin_lim_dev(c0, n, alpha=alpha, magnitudes=target if explicit else None, return_trace=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == c0.shape and db.shape == (n, c0.shape[0])
    out = out.cpu().numpy().astype(np.complex128)
    assert np.isfinite(out.view(np.float64)).all()
    for b in range(c0.shape[0]):
        top = target[b].max()
        dist, bar = rel(out[b], ref[b]), 3 * rel(per[b], ref[b])
        far = np.mean(np.abs(out[b] - ref[b]) > 1e-3 * top)
        mag = np.abs(np.abs(out[b]) - target[b]).max() / top
        ddb, bar_db = np.abs(db[:, b] - ref_db[:, b]), 0.01 + np.abs(per_db[:, b] - ref_db[:, b])
        print("gla %s n=%d alpha=%g%s b=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  trace dB off %.2e (bar %.2e)"
              % (key[:3], n, alpha, " explicit A" if explicit else "", b, dist, bar, 100 * far, mag, ddb.max(), bar_db[ddb.argmax()]))
        assert dist <= bar, (b, dist, bar)
        assert far <= 1e-3, (b, far)
        assert mag <= 2e-6, (b, mag)
        assert (ddb <= bar_db).all(), (b, ddb, bar_db)
    # the first entry is the consistency of c_0: what get_consistency says, to the bar test_consistency_matches_host uses
    for b in range(c0.shape[0]):
        assert abs(db[0, b] - p.get_consistency(c0[b].astype(np.complex128))) < 0.01


@pytest.mark.parametrize("fsize,fshift,perfectrec", sorted(SHAPES))
def test_matches_host(fsize, fshift, perfectrec):
    key = (fsize, fshift, perfectrec, SHAPES[fsize, fshift, perfectrec])
    for n, alpha in STEPS:
        check_against_host(key, n, alpha)


@pytest.mark.parametrize("key", [(64, 16, True, 12), (256, 96, False, 2)])
def test_explicit_magnitudes(key):
    check_against_host(key, 3, 0.99, explicit=True)
    check_against_host(key, 4, 0.0, explicit=True)


def test_silent_stretch_gives_exact_zeros():
    p, A, c0 = case(64, 16, True, 12)
    Z = A.copy()
    Z[:, 3:8] = 0.0
    Z[1] = 0.0                                     # a whole spectrogram of silence
    for start in (c0, (Z * np.exp(1j * np.angle(c0))).astype(np.complex64)):
        out = p.griffin_lim_dev(start, 5, magnitudes=Z).cpu().numpy()
        assert np.isfinite(out.view(np.float32)).all()
        assert (out[:, 3:8] == 0).all() and (out[1] == 0).all()
        assert np.abs(np.abs(out) - Z).max() <= 2e-6 * Z.max()
    # ... and with the default magnitudes, where the silence is in c_0 itself
    start = (Z * np.exp(1j * np.angle(c0))).astype(np.complex64)
    out = p.griffin_lim_dev(start, 5).cpu().numpy()
    assert np.isfinite(out.view(np.float32)).all() and (out[:, 3:8] == 0).all()


def test_zero_iterations_and_unmodified_input():
    p, A, c0 = case(64, 16, False, 9)
    t = torch.from_numpy(c0).cuda()
    keep = t.clone()
    out, db = p.griffin_lim_dev(t, 0, return_trace=True)
    assert torch.equal(out, keep) and db.shape == (0, 3)
    assert out.data_ptr() != t.data_ptr()
    out = p.griffin_lim_dev(t, 4)
    assert torch.equal(t, keep) and not torch.equal(out, keep)
    assert out.data_ptr() != t.data_ptr()
    single = p.griffin_lim_dev(c0[0], 0)
    assert tuple(single.shape) == c0.shape[1:] and np.array_equal(single.cpu().numpy(), c0[0])


@pytest.mark.parametrize("key", [(64, 16, False, 9), (1000, 250, True, 5)])
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A, c0 = case(*key)
    t = torch.from_numpy(c0).cuda()
    out, db = p.griffin_lim_dev(t, 5, return_trace=True)
    again, db2 = p.griffin_lim_dev(t, 5, return_trace=True)
    assert torch.equal(out, again) and np.array_equal(db, db2)
    assert torch.equal(out, p.griffin_lim_dev(t, 5))                     # with and without the trace
    for b in range(c0.shape[0]):
        one, one_db = p.griffin_lim_dev(t[b], 5, return_trace=True)
        assert tuple(one.shape) == c0.shape[1:] and one_db.shape == (5,)
        assert torch.equal(one, out[b]) and np.array_equal(one_db, db[:, b])


def test_concurrent_streams_do_not_share_windows_or_scratch():
    """Calls with different windows and shapes enqueued on two streams with no host synchronisation in between give what they
    give one at a time (the per-device context serialises its users on the device)."""
    pa, _, ca = case(256, 96, True, 5)
    pb, _, cb = case(64, 16, False, 9)
    ta, tb = torch.from_numpy(ca).cuda(), torch.from_numpy(cb).cuda()
    ref_a, ref_b = pa.griffin_lim_dev(ta, 6), pb.griffin_lim_dev(tb, 6)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for rep in range(6):
        with torch.cuda.stream(s1):
            a = pa.griffin_lim_dev(ta, 6)
        with torch.cuda.stream(s2):
            b = pb.griffin_lim_dev(tb, 6)
        outs.append((a, b))
    torch.cuda.synchronize()
    for a, b in outs:
        assert torch.equal(a, ref_a) and torch.equal(b, ref_b)


def test_unsupported_and_invalid_arguments_raise():
    p = lws_amd.lws(8192, 2048)                  # beyond the LDS-resident transform (even sizes up to 4096)
    with pytest.raises(lws_amd.LwsHipError):
        p.griffin_lim_dev(np.ones((5, 4097), complex), 2)
    p, A, c0 = case(64, 16, False, 9)
    with pytest.raises(ValueError):
        p.griffin_lim_dev(c0, 3, alpha=1.0)
    with pytest.raises(ValueError):
        p.griffin_lim_dev(c0, -1)
    with pytest.raises(ValueError):
        p.griffin_lim_dev(c0, 3, magnitudes=A[:, :-1])
    with pytest.raises(ValueError):
        p.griffin_lim_dev(c0[:, :, :-1], 3)
    # the C entry point checks for itself
    lib = lws_amd._capi.load()
    t = torch.from_numpy(c0).cuda()
    w = np.ascontiguousarray(p.awin, dtype=np.float64)
    for iters, alpha in ((-1, 0.5), (2, 1.0), (2, -0.1), (2, float("nan"))):
        rc = lib.lws_griffin_lim_dev(0, t.data_ptr(), None, 3, 9, 64, 16, w.ctypes.data, w.ctypes.data, 0, iters, alpha, None, None)
        assert rc == lws_amd._capi.LWS_ERR_INVALID
    assert np.array_equal(t.cpu().numpy(), c0)


def test_refines_what_run_lws_returns():
    """The feature's reason for existing: a few iterations started from the LWS phases end closer to a consistent spectrogram
    than LWS, whose L-bin sums leave it on a truncation floor."""
    rng = np.random.default_rng(11)
    p = lws_amd.lws(512, 128, batch_iterations=30)
    X = p.stft(rng.standard_normal(512 * 12))
    S = p.run_lws(np.abs(X))
    G = p.griffin_lim_dev(S, 10)
    before, after = p.get_consistency(S), p.get_consistency(G.cpu().numpy().astype(np.complex128))
    print("gla end to end: consistency %.2f dB after run_lws, %.2f dB after 10 more iterations" % (before, after))
    assert after > before
    assert torch.isfinite(p.istft_dev(G)).all()
