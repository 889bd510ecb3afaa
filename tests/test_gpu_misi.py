"""GPU: MISI on the device (lws_gla.hip) against the host fp64 definition (lws_amd.misi).

As in tests/test_gpu_griffin_lim.py the value check has no fixed tolerance: its bar is measured here, on the host side only.  It
is the rel-L2 distance the host iteration moves when every projection X_{i,k} is perturbed by seeded complex Gaussian noise of
standard deviation 1e-6 max|X_{i,k}| per component, times 3.  Distances, caps and bars are taken per mixture and per source, so
that the weak source of a mixture and the small-scale members of a stack are held as tightly as the loud ones.  Every figure is
printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest

import lws_amd

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALES = np.array([1.0, 1e-3, 300.0])          # of the B = 3 mixtures
SOURCES = np.array([1.0, 0.3, 3.0])            # relative levels of the sources of a mixture
STEPS = (1, 3, 8)
# (fsize, fshift, perfectrec, T, K)
SHAPES = [
    (64, 16, False, 9, 2),                     # power of two
    (64, 16, True, 12, 3),                     # power of two, perfectrec
    (48, 16, True, 7, 2),                      # odd factor 3
    (48, 16, False, 1, 1),                     # single frame and K = 1
    (256, 96, False, 2, 3),                    # hop does not divide the frame
    (256, 96, True, 5, 2),                     # same, perfectrec
    (1000, 250, True, 5, 2),                   # odd factor 125
    (4096, 1024, False, 5, 2),                 # the large-LDS path
]
EPS = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, K, B=3):
    """p, A = |stft(source)| (B, K, T, F), c_0 = A exp(2 pi j u) rounded to complex64 and the mixture y rounded to float32 (what
    the device is given, and what the host run starts from).  An iterate with a near-zero projection turns a 1e-6 error into a
    phase flip of that bin, and at these sizes one bin is more than the far-bin cap allows; the seed offset is one for which the
    host error model of this file leaves no bin beyond the cap in any shape at any step count (of offsets 0..6 times 100000 only
    this one does: a statement about the fp64 host iteration, made without a device)."""
    rng = np.random.default_rng(300000 + 1000 * fsize + 10 * fshift + perfectrec)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    src = rng.standard_normal((B, K, n)) * SOURCES[None, :K, None] * SCALES[:B, None, None]
    A = np.abs(np.stack([[p.stft(x) for x in s] for s in src]))
    assert A.shape == (B, K, T, F)
    c0 = (A * np.exp(2j * np.pi * rng.random(A.shape))).astype(np.complex64)
    y = src.sum(axis=1).astype(np.float32)
    for a in (A, c0, y):
        a.setflags(write=False)
    return p, A, c0, y


def perturbation(seed):
    rng = np.random.default_rng(seed)

    def f(i, b, k, X):
        sigma = 1e-6 * np.abs(X).max()
        return X + sigma * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


def magnitudes_of(A):
    """Targets that differ from |c_0|: its magnitudes rolled along time and rescaled (spectrograms of other signals)."""
    return np.roll(A, 1, axis=2) * 0.7 + 0.05 * A.max(axis=(2, 3), keepdims=True)


@functools.lru_cache(maxsize=None)
def host(key, n, explicit=False):
    """Host fp64 result, trace and signals, and the same under the perturbation model."""
    p, A, c0, y = case(*key)
    kw = dict(magnitudes=magnitudes_of(A) if explicit else None, perfectrec=p.perfectrec, return_trace=True, return_signals=True)
    ref = lws_amd.misi(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, **kw)
    per = lws_amd.misi(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, _perturb=perturbation(n + 17), **kw)
    return ref, per


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def mixture_bound(K, y, x):
    """Twice the worst-case fp32 rounding of K adds, one subtract, one divide and K adds on values of these sizes."""
    return 4 * (K + 1) * EPS * (np.abs(y).max() + sum(np.abs(xk).max() for xk in x))


def check_against_host(key, n, explicit=False):
    p, A, c0, y = case(*key)
    B, K = c0.shape[:2]
    (ref, ref_db, ref_s), (per, per_db, per_s) = host(key, n, explicit)
    target = magnitudes_of(A) if explicit else np.abs(c0).astype(np.float64)
    out, db, s = p.misi_dev(c0, y, n, magnitudes=target if explicit else None, return_trace=True, return_signals=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == c0.shape and db.shape == (n, B)
    assert s.dtype == torch.float32 and tuple(s.shape) == (B, K, y.shape[1])
    out, s = out.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
    tag = "misi %s n=%d%s" % (key, n, " explicit A" if explicit else "")
    for b in range(B):
        ddb, bar_db = np.abs(db[:, b] - ref_db[:, b]), 0.01 + np.abs(per_db[:, b] - ref_db[:, b])
        x_host = [p.istft(ref[b, k]) for k in range(K)]
        mix, mix_bar = np.abs(s[b].sum(axis=0) - y[b]).max(), mixture_bound(K, y[b], x_host)
        print("%s b=%d: trace dB off %.2e (bar %.2e)  |sum s - y| %.2e (bound %.2e)"
              % (tag, b, ddb.max(), bar_db[ddb.argmax()], mix, mix_bar))
        assert (ddb <= bar_db).all(), (b, ddb, bar_db)
        assert mix <= mix_bar, (b, mix, mix_bar)
        for k in range(K):
            top = target[b, k].max()
            dist, bar = rel(out[b, k], ref[b, k]), 3 * rel(per[b, k], ref[b, k])
            far = np.mean(np.abs(out[b, k] - ref[b, k]) > 1e-3 * top)
            mag = np.abs(np.abs(out[b, k]) - target[b, k]).max() / top
            ds = np.abs(s[b, k] - ref_s[b, k]).max()
            bar_s = 3 * np.abs(per_s[b, k] - ref_s[b, k]).max() + 3e-6 * np.abs(ref_s[b, k]).max()
            print("%s b=%d k=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal off %.2e (bar %.2e)"
                  % (tag, b, k, dist, bar, 100 * far, mag, ds, bar_s))
            assert dist <= bar, (b, k, dist, bar)
            assert far <= 1e-3, (b, k, far)
            assert mag <= 2e-6, (b, k, mag)
            assert ds <= bar_s, (b, k, ds, bar_s)


@pytest.mark.parametrize("key", SHAPES, ids=lambda k: "%d-%d-%s-T%d-K%d" % k)
def test_matches_host(key):
    for n in STEPS:
        check_against_host(key, n)


@pytest.mark.parametrize("key", [(64, 16, True, 12, 3), (256, 96, False, 2, 3)], ids=lambda k: "%d-%d-%s-T%d-K%d" % k)
def test_explicit_magnitudes(key):
    check_against_host(key, 3, explicit=True)


def test_zero_iterations_and_unmodified_input():
    p, A, c0, y = case(64, 16, False, 9, 2)
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    keep, keep_y = t.clone(), ty.clone()
    out, db, s = p.misi_dev(t, ty, 0, return_trace=True, return_signals=True)
    assert torch.equal(out, keep) and db.shape == (0, 3)
    assert out.data_ptr() != t.data_ptr()
    # the signals of c_0 itself sum to the mixture
    s = s.cpu().numpy().astype(np.float64)
    for b in range(3):
        x = [p.istft(c0[b, k].astype(np.complex128)) for k in range(2)]
        mix, bound = np.abs(s[b].sum(axis=0) - y[b]).max(), mixture_bound(2, y[b], x)
        print("misi zero iterations b=%d: |sum s - y| %.2e (bound %.2e)" % (b, mix, bound))
        assert mix <= bound
    out = p.misi_dev(t, ty, 4)
    assert torch.equal(t, keep) and torch.equal(ty, keep_y) and not torch.equal(out, keep)
    assert out.data_ptr() != t.data_ptr()
    single = p.misi_dev(c0[0], y[0], 0)
    assert tuple(single.shape) == c0.shape[1:] and np.array_equal(single.cpu().numpy(), c0[0])


@pytest.mark.parametrize("key", [(64, 16, False, 9, 2), (1000, 250, True, 5, 2)], ids=lambda k: "%d-%d-%s-T%d-K%d" % k)
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A, c0, y = case(*key)
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    out, db, s = p.misi_dev(t, ty, 5, return_trace=True, return_signals=True)
    again, db2, s2 = p.misi_dev(t, ty, 5, return_trace=True, return_signals=True)
    assert torch.equal(out, again) and np.array_equal(db, db2) and torch.equal(s, s2)
    assert torch.equal(out, p.misi_dev(t, ty, 5))                      # with and without the trace and the signals
    only_s = p.misi_dev(t, ty, 5, return_signals=True)
    assert torch.equal(only_s[0], out) and torch.equal(only_s[1], s)
    for b in range(c0.shape[0]):
        one, one_db, one_s = p.misi_dev(t[b], ty[b], 5, return_trace=True, return_signals=True)
        assert tuple(one.shape) == c0.shape[1:] and one_db.shape == (5,) and tuple(one_s.shape) == (c0.shape[1], y.shape[1])
        assert torch.equal(one, out[b]) and np.array_equal(one_db, db[:, b]) and torch.equal(one_s, s[b])


def test_concurrent_streams_do_not_share_windows_or_scratch():
    """Calls with different windows and shapes enqueued on two streams with no host synchronisation in between give what they
    give one at a time (the per-device context serialises its users on the device)."""
    pa, _, ca, ya = case(256, 96, True, 5, 2)
    pb, _, cb, yb = case(64, 16, False, 9, 2)
    ta, tya, tb, tyb = (torch.from_numpy(a).cuda() for a in (ca, ya, cb, yb))
    ref_a, ref_b = pa.misi_dev(ta, tya, 6, return_signals=True), pb.misi_dev(tb, tyb, 6, return_signals=True)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for rep in range(6):
        with torch.cuda.stream(s1):
            a = pa.misi_dev(ta, tya, 6, return_signals=True)
        with torch.cuda.stream(s2):
            b = pb.misi_dev(tb, tyb, 6, return_signals=True)
        outs.append((a, b))
    torch.cuda.synchronize()
    for a, b in outs:
        assert torch.equal(a[0], ref_a[0]) and torch.equal(a[1], ref_a[1])
        assert torch.equal(b[0], ref_b[0]) and torch.equal(b[1], ref_b[1])


def test_unsupported_and_invalid_arguments_raise():
    p = lws_amd.lws(8192, 2048)                  # beyond the LDS-resident transform (even sizes up to 4096)
    with pytest.raises(lws_amd.LwsHipError):
        p.misi_dev(np.ones((2, 5, 4097), complex), np.zeros(p.istft(np.ones((5, 4097), complex)).shape[0]), 2)
    p, A, c0, y = case(64, 16, False, 9, 2)
    with pytest.raises(ValueError):
        p.misi_dev(c0, y[:, :-1], 3)             # wrong mixture length
    with pytest.raises(ValueError):
        p.misi_dev(c0, y[0], 3)                  # one mixture for a stack
    with pytest.raises(ValueError):
        p.misi_dev(c0, y, -1)
    with pytest.raises(ValueError):
        p.misi_dev(c0, y, 3, magnitudes=A[:, :, :-1])
    with pytest.raises(ValueError):
        p.misi_dev(c0[0, 0], y[0], 3)            # a 2-D S
    with pytest.raises(ValueError):
        p.misi_dev(c0[:, :, :, :-1], y, 3)
    q = lws_amd.lws(64, 16, perfectrec=True)     # two frames come back from the round trip as three
    with pytest.raises(ValueError):
        q.misi_dev(c0[:, :, :2], np.zeros((3, 0), np.float32), 1)
    # the C entry point checks for itself
    lib = lws_amd._capi.load()
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    w = np.ascontiguousarray(p.awin, dtype=np.float64)
    for K, iters, yp in ((0, 2, ty.data_ptr()), (2, -1, ty.data_ptr()), (2, 2, None)):
        rc = lib.lws_misi_dev(0, t.data_ptr(), None, yp, 3, K, 9, 64, 16, w.ctypes.data, w.ctypes.data, 0, iters, None, None, None)
        assert rc == lws_amd._capi.LWS_ERR_INVALID
    rc = lib.lws_misi_dev(0, t.data_ptr(), None, ty.data_ptr(), 3, 2, 2, 64, 16, w.ctypes.data, w.ctypes.data, 1, 1, None, None, None)
    assert rc == lws_amd._capi.LWS_ERR_INVALID   # perfectrec does not keep two frames
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), c0)


def test_couples_what_run_lws_returns():
    """The feature's reason for existing: phases from LWS for each source, then MISI under the known mixture."""
    rng = np.random.default_rng(12)
    p = lws_amd.lws(512, 128, batch_iterations=30)
    src = rng.standard_normal((2, 512 * 12)) * np.array([1.0, 0.3])[:, None]
    y = src.sum(axis=0).astype(np.float32)
    S = np.stack([p.run_lws(np.abs(p.stft(x))) for x in src]).astype(np.complex64)
    out, db, s = p.misi_dev(S, y, 10, return_trace=True, return_signals=True)
    print("misi end to end: mixture consistency %.2f dB after run_lws, %.2f dB entering the 10th iteration" % (db[0], db[-1]))
    assert db[-1] > db[0]
    x_host = [p.istft(o) for o in p.misi(S, y, 10)]
    s = s.cpu().numpy().astype(np.float64)
    mix, bound = np.abs(s.sum(axis=0) - y).max(), mixture_bound(2, y, x_host)
    print("misi end to end: |sum s - y| %.2e (bound %.2e)" % (mix, bound))
    assert np.isfinite(s).all() and mix <= bound
