"""GPU: RTISI-LA on the device (k_rtisi of lws_gla.hip) against the host fp64 definition (lws_amd.rtisi_la).

The starts are true phases with 0.3 rad of Gaussian noise, not random phases: from a uniform-random start the iteration is chaotic
(under the model below the fp64 iteration itself then moves 8-23 % of the bins of lws(512,128), T = 40, at n = 8), and no device
could be held to that.  The value check is the one of tests/test_gpu_griffin_lim.py, for the reasons given there: its bar is measured
here, on the host side only, as the rel-L2 distance the host iteration moves when the stacked projections of every inner iteration
are perturbed by seeded complex Gaussian noise of standard deviation 1e-6 max|X| per component, times 3.  Distances and caps are
taken per spectrogram, so that the small-scale members of a stack are held as tightly as the large ones.  Every figure is printed
before it is asserted (pytest -s)."""
import functools
import json
import os

import numpy as np
import pytest

import lws_amd

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALES = np.array([1.0, 1e-3, 300.0])
# (look_ahead, iterations): odd and even counts of active frames, and look-aheads beyond the frames of the short cases
STEPS = [(0, 1), (0, 4), (1, 3), (2, 2), (3, 1), (3, 3), (3, 6), (5, 2)]
SHAPES = {
    (64, 16, False): 9, (64, 16, True): 12,            # power of two
    (48, 16, False): 1, (48, 16, True): 7,             # odd factor 3
    (256, 96, False): 2, (256, 96, True): 5,           # hop does not divide the frame
    (1000, 250, False): 6, (1000, 250, True): 5,       # odd factor 125
    (4096, 1024, False): 12, (4096, 1024, True): 4,    # the state does not fit in LDS: device scratch
    (512, 128, False): 40, (128, 32, True): 33,        # the rings wrap many times
}
# Placements, workgroups and overlaps SHAPES never reaches.  (fsize, fshift, perfectrec, T): (threads, [(look_ahead, iterations, state
# in LDS)]); every case asserts its placement and workgroup through lws_rtisi_la_placement before it runs.
EDGE_SHAPES = {
    (320, 80, True, 9): (512, [(2, 2, True), (3, 3, True)]),         # 512 threads over 320 samples, odd factor 5
    (600, 150, False, 7): (768, [(3, 3, True), (0, 2, True)]),       # a workgroup of 768 threads, odd factor 75
    (768, 192, True, 8): (768, [(3, 2, True)]),                      # 768 threads = N, odd factor 3
    (1536, 384, True, 8): (1024, [(3, 3, True), (1, 2, True)]),      # N > workgroup, the state in LDS behind three transform buffers
    (2048, 512, False, 8): (1024, [(3, 3, True), (5, 2, True), (6, 2, False)]),   # N = 2 workgroups; LA 5 in LDS, LA 6 in scratch
    (2048, 1228, False, 8): (1024, [(5, 2, True)]),                  # 163 824 bytes of dynamic LDS: 16 under the cap
    (2048, 1229, False, 8): (1024, [(5, 2, False)]),                 # ... and 4 over it: scratch
    (64, 64, False, 6): (256, [(3, 3, True), (0, 2, True)]),         # hop = N: every sample final after one frame
    (64, 40, False, 8): (256, [(3, 3, True)]),                       # hop > N / 2
    (64, 32, True, 8): (256, [(3, 3, True), (1, 2, True)]),          # Q = N / hop = 2
    (64, 8, True, 20): (256, [(3, 3, True), (9, 2, True)]),          # Q = 8; more active frames than overlap (LA + 1 > Q)
    (64, 4, False, 24): (256, [(3, 2, True), (17, 2, True)]),        # Q = 16; 18 active frames
}
MARGINS = {}    # (fsize, fshift, perfectrec) -> [cases, max rel-L2, max rel-L2 / bar, max far fraction, max magnitude error, max signal error]


def other_window(fsize):
    """An analysis window that is not the plan's default sqrt-Hann (the plan derives the synthesis window from it)."""
    return lws_amd.hann(fsize) ** 0.75 + 0.01


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, windows="default"):
    """p, A = |c0|, c0 = X exp(0.3j g) rounded to complex64 (what the device is given), X = stft(noise) at three scales."""
    rng = np.random.default_rng(1000 * fsize + 10 * fshift + perfectrec)
    if windows == "default":
        p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    else:
        p = lws_amd.lws(other_window(fsize), fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    X = np.stack([p.stft(x) for x in rng.standard_normal((3, n))]) * SCALES[:, None, None]
    assert X.shape == (3, T, F)
    c0 = (X * np.exp(0.3j * rng.standard_normal(X.shape))).astype(np.complex64)
    A = np.abs(c0).astype(np.float64)
    for a in (A, c0):
        a.setflags(write=False)
    return p, A, c0


def perturbation(seed):
    rng = np.random.default_rng(seed)

    def f(m, it, b, X):
        sigma = 1e-6 * np.abs(X).max()
        return X + sigma * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


def magnitudes_of(A):
    """Targets that differ from |c_0|: its magnitudes rolled along time and rescaled (a spectrogram of another signal)."""
    return np.roll(A, 1, axis=1) * 0.7 + 0.05 * A.max(axis=(1, 2), keepdims=True)


@functools.lru_cache(maxsize=None)
def host(key, LA, n, explicit=False):
    """Host fp64 result, and the same under the perturbation model."""
    p, A, c0 = case(*key)
    kw = dict(look_ahead=LA, magnitudes=magnitudes_of(A) if explicit else None, perfectrec=p.perfectrec)
    ref = lws_amd.rtisi_la(c0, p.fsize, p.fshift, p.awin, p.swin, n, **kw)
    per = lws_amd.rtisi_la(c0, p.fsize, p.fshift, p.awin, p.swin, n, _perturb=perturbation(n + 17), **kw)
    return ref, per


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def check_against_host(key, LA, n, explicit=False):
    p, A, c0 = case(*key)
    ref, per = host(key, LA, n, explicit)
    target = magnitudes_of(A) if explicit else A
    out, sig = p.rtisi_la_dev(c0, n, look_ahead=LA, magnitudes=target if explicit else None, return_signal=True)
    length = lws_amd._capi.istft_length(c0.shape[1], p.fsize, p.fshift, p.perfectrec)
    assert out.dtype == torch.complex64 and tuple(out.shape) == c0.shape
    assert sig.dtype == torch.float32 and tuple(sig.shape) == (c0.shape[0], length)
    out, sig = out.cpu().numpy().astype(np.complex128), sig.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(sig).all()
    m = MARGINS.setdefault(key[:3], [0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for b in range(c0.shape[0]):
        top = target[b].max()
        dist, bar = rel(out[b], ref[b]), 3 * rel(per[b], ref[b])
        far, far_model = np.mean(np.abs(out[b] - ref[b]) > 1e-3 * top), np.mean(np.abs(per[b] - ref[b]) > 1e-3 * top)
        mag = np.abs(np.abs(out[b]) - target[b]).max() / top
        x = p.istft(out[b])
        serr = np.abs(sig[b] - x).max() / np.abs(x).max()
        print("rtisi %s LA=%d n=%d%s b=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%% (model %.4f%%)  |mag - A| %.2e max A  signal %.2e max|x|"
              % (key[:3], LA, n, " explicit A" if explicit else "", b, dist, bar, 100 * far, 100 * far_model, mag, serr))
        m[:] = [m[0] + 1, max(m[1], dist), max(m[2], dist / bar), max(m[3], far), max(m[4], mag), max(m[5], serr)]
        assert dist <= bar, (b, dist, bar)
        assert far <= 1e-3, (b, far)
        assert mag <= 2e-6, (b, mag)
        assert serr <= 3e-6, (b, serr)


@pytest.mark.parametrize("fsize,fshift,perfectrec", sorted(SHAPES))
def test_matches_host(fsize, fshift, perfectrec):
    key = (fsize, fshift, perfectrec, SHAPES[fsize, fshift, perfectrec])
    for LA, n in STEPS:
        check_against_host(key, LA, n)


def assert_placement(key, LA, in_lds, threads, K=0):
    """The launch of this case (look-ahead clamped to its frames, as the entry points clamp it) is the one its comment claims."""
    got = lws_amd._capi.rtisi_la_placement(key[0], key[1], min(LA, key[3] - 1), K)
    print("placement %s LA=%d K=%d: state in %s, %d threads, %d bytes of dynamic LDS" % (key[:4], LA, K, "LDS" if got[0] else "scratch", got[1], got[2]))
    assert got[:2] == (in_lds, threads), (key, LA, K, got)


@pytest.mark.parametrize("key", sorted(EDGE_SHAPES))
def test_edge_shapes_match_host(key):
    threads, steps = EDGE_SHAPES[key]
    for LA, n, in_lds in steps:
        assert_placement(key, LA, in_lds, threads)
        check_against_host(key, LA, n)


@pytest.mark.parametrize("key", [(64, 16, True, 12), (256, 96, False, 2)])
def test_explicit_magnitudes(key):
    check_against_host(key, 3, 3, explicit=True)
    check_against_host(key, 1, 4, explicit=True)


@pytest.mark.parametrize("key", [(64, 16, True, 12), (512, 128, False, 40), (64, 8, True, 20)])
def test_causality_bit_for_bit(key):
    """Output frame m depends on no input frame later than m + LA: with explicit magnitudes, LA = 3 and n = 3, other phases in the
    input frames >= 6 leave the output frames 0..2 as they are, and change frame 3."""
    p, A, c0 = case(*key)
    rng = np.random.default_rng(3)
    c1 = c0.copy()
    c1[:, 6:] = (A[:, 6:] * np.exp(2j * np.pi * rng.random(A[:, 6:].shape))).astype(np.complex64)
    a = p.rtisi_la_dev(c0, 3, look_ahead=3, magnitudes=A).cpu().numpy()
    b = p.rtisi_la_dev(c1, 3, look_ahead=3, magnitudes=A).cpu().numpy()
    assert np.array_equal(a[:, :3], b[:, :3])
    for s in range(c0.shape[0]):
        assert not np.array_equal(a[s, 3], b[s, 3])


@pytest.mark.parametrize("key", [(64, 16, False, 9), (1000, 250, True, 5), (4096, 1024, True, 4), (2048, 512, False, 8)])
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A, c0 = case(*key)
    t = torch.from_numpy(c0).cuda()
    out, sig = p.rtisi_la_dev(t, 3, return_signal=True)
    again, sig2 = p.rtisi_la_dev(t, 3, return_signal=True)
    assert torch.equal(out, again) and torch.equal(sig, sig2)
    assert torch.equal(out, p.rtisi_la_dev(t, 3))                        # with and without the signal
    for b in range(c0.shape[0]):
        one, one_sig = p.rtisi_la_dev(t[b], 3, return_signal=True)
        assert tuple(one.shape) == c0.shape[1:] and tuple(one_sig.shape) == tuple(sig.shape[1:])
        assert torch.equal(one, out[b]) and torch.equal(one_sig, sig[b])


def test_zero_iterations_and_unmodified_input():
    p, A, c0 = case(64, 16, False, 9)
    t = torch.from_numpy(c0).cuda()
    keep = t.clone()
    out = p.rtisi_la_dev(t, 0)
    assert torch.equal(out, keep) and out.data_ptr() != t.data_ptr()
    out, sig = p.rtisi_la_dev(t, 0, return_signal=True)                  # the signal of the start itself
    assert torch.equal(out, keep)
    x = np.stack([p.istft(c.astype(np.complex128)) for c in c0])
    assert tuple(sig.shape) == x.shape
    assert (np.abs(sig.cpu().numpy() - x).max(axis=1) <= 3e-6 * np.abs(x).max(axis=1)).all()
    out = p.rtisi_la_dev(t, 4)
    assert torch.equal(t, keep) and not torch.equal(out, keep)
    assert out.data_ptr() != t.data_ptr()
    single = p.rtisi_la_dev(c0[0], 0)
    assert tuple(single.shape) == c0.shape[1:] and np.array_equal(single.cpu().numpy(), c0[0])
    single, x1 = p.rtisi_la_dev(c0[0], 2, return_signal=True)
    assert tuple(single.shape) == c0.shape[1:] and tuple(x1.shape) == x.shape[1:]


def test_silent_stretch_gives_exact_zeros():
    p, A, c0 = case(64, 16, True, 12)
    Z = A.copy()
    Z[:, 3:8] = 0.0
    Z[1] = 0.0                                     # a whole spectrogram of silence
    for start in (c0, (Z * np.exp(1j * np.angle(c0))).astype(np.complex64)):
        out, sig = p.rtisi_la_dev(start, 5, magnitudes=Z, return_signal=True)
        out, sig = out.cpu().numpy(), sig.cpu().numpy()
        assert np.isfinite(out.view(np.float32)).all() and np.isfinite(sig).all()
        assert (out[:, 3:8] == 0).all() and (out[1] == 0).all() and (sig[1] == 0).all()
        assert np.abs(np.abs(out) - Z).max() <= 2e-6 * Z.max()
    # ... and with the default magnitudes, where the silence is in the start itself
    start = (Z * np.exp(1j * np.angle(c0))).astype(np.complex64)
    out = p.rtisi_la_dev(start, 5).cpu().numpy()
    assert np.isfinite(out.view(np.float32)).all() and (out[:, 3:8] == 0).all() and (out[1] == 0).all()


def test_second_call_with_other_windows_is_not_served_stale_ones():
    """The windows stay on the device between calls; a call with other windows of the same length must upload its own."""
    check_against_host((64, 16, True, 12), 3, 3)
    check_against_host((64, 16, True, 12, "other"), 3, 3)
    check_against_host((64, 16, True, 12), 3, 3)
    pa, pb = case(64, 16, True, 12)[0], case(64, 16, True, 12, "other")[0]
    assert not np.array_equal(pa.awin, pb.awin) and not np.array_equal(pa.swin, pb.swin)


def test_method_uses_the_plans_look_ahead():
    p, A, c0 = case(64, 16, True, 12)
    assert p.look_ahead == 3
    p1 = lws_amd.lws(64, 16, perfectrec=True, look_ahead=1)
    t = torch.from_numpy(c0).cuda()
    assert torch.equal(p.rtisi_la_dev(t, 2), p.rtisi_la_dev(t, 2, look_ahead=3))
    assert torch.equal(p1.rtisi_la_dev(t, 2), p.rtisi_la_dev(t, 2, look_ahead=1))
    assert not torch.equal(p1.rtisi_la_dev(t, 2), p.rtisi_la_dev(t, 2))
    assert torch.equal(p.rtisi_la_dev(t, 2, look_ahead=11), p.rtisi_la_dev(t, 2, look_ahead=40))   # all 12 frames active either way


def test_concurrent_streams_do_not_share_windows_or_scratch():
    """Calls with different windows and shapes -- two whose state is in the context's scratch, which each of them grows and reuses, and
    one whose state is in LDS -- enqueued on two streams with no host synchronisation in between give what they give one at a time."""
    keys = [((4096, 1024, False, 12), 3, False), ((2048, 512, False, 8), 6, False), ((64, 16, True, 12), 3, True)]
    calls = []
    for key, LA, in_lds in keys:
        assert_placement(key, LA, in_lds, 1024 if key[0] >= 1024 else 256)
        p, A, c0 = case(*key)
        calls.append((p, torch.from_numpy(c0).cuda(), LA))
    refs = [p.rtisi_la_dev(t, 2, look_ahead=LA, return_signal=True) for p, t, LA in calls]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for rep in range(6):
        for i, (p, t, LA) in enumerate(calls):
            with torch.cuda.stream(streams[(rep + i) % 2]):
                outs.append((i, p.rtisi_la_dev(t, 2, look_ahead=LA, return_signal=True)))
    torch.cuda.synchronize()
    for i, (out, sig) in outs:
        assert torch.equal(out, refs[i][0]) and torch.equal(sig, refs[i][1]), i


def test_unsupported_and_invalid_arguments_raise():
    p = lws_amd.lws(8192, 2048)                  # beyond the LDS-resident transform (even sizes up to 4096)
    with pytest.raises(lws_amd.LwsHipError):
        p.rtisi_la_dev(np.ones((5, 4097), complex), 2)
    p, A, c0 = case(64, 16, True, 12)
    for bad in (dict(iterations=-1), dict(iterations=2, look_ahead=-1), dict(iterations=2, look_ahead=1.5),
                dict(iterations=2, magnitudes=A[:, :-1])):
        with pytest.raises(ValueError):
            p.rtisi_la_dev(c0, **bad)
    with pytest.raises(ValueError):
        p.rtisi_la_dev(c0[:, :, :-1], 3)
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        p.rtisi_la_dev(c0[:, :2], 3)
    t = torch.from_numpy(c0).cuda()
    lib = lws_amd._capi.load()
    w = np.ascontiguousarray(p.awin, dtype=np.float64)
    for iters, LA in ((-1, 3), (2, -1)):
        rc = lib.lws_rtisi_la_dev(0, t.data_ptr(), None, None, 3, 12, 64, 16, w.ctypes.data, w.ctypes.data, 1, iters, LA, None)
        assert rc == lws_amd._capi.LWS_ERR_INVALID
    assert np.array_equal(t.cpu().numpy(), c0)


def test_zz_margins_actually_achieved():
    """What the cases above reached, per shape (written to $LWS_MARGINS_DIR/rtisi_margins.json when that variable names a directory;
    profiles/rtisi_margins.json is a copy).  On an MI355X, 372 rows, 63 of them at the 12 shapes of EDGE_SHAPES: rel-L2 at most 7.5e-6 and
    at most 9.2 % of its bar (5.0 % at the edge shapes), no bin beyond 1e-3 max A, magnitudes within 2.2e-7 max A, signals within 3.6e-7
    max|x|; the whole file in 4.5 s."""
    if not MARGINS:
        check_against_host((64, 16, True, 12), 3, 3)
    report = {"%d,%d,%s" % k: {"cases": v[0], "max_rel_l2": v[1], "max_rel_l2_over_bar": v[2], "max_far_fraction": v[3],
                               "max_magnitude_error": v[4], "max_signal_error": v[5]} for k, v in sorted(MARGINS.items())}
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "rtisi_margins.json"), "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    print(report)
    assert all(v[2] <= 1.0 for v in MARGINS.values())
