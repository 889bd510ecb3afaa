"""GPU: the device transforms (fft_lds of lws_fft.h under the kernels of lws_stft.hip and lws_gla.hip) at the frame sizes, hops and
signal lengths the other transform tests never visit: N = m 2^a with a = 1 and a = 2, N = 32, the largest odd factors
(4092 = 1023 x 4, 4094 = 2047 x 2), hop = 1, hop = N, hops above N / 2 that do not divide N, signals of one sample, of exactly one
hop / one frame, and of a frame plus one sample.

References are the host fp64 functions (lws_amd.stft / istft / get_consistency / griffin_lim / misi).  The bar of the transforms is
the suite's 3e-6 of the largest value wherever three times the float32 model of the factorisation (tests/fft_model.py, same input,
window product and overlap-add included) stays below it, and three times the model elsewhere: the model measures what float32 and
m accumulated terms per output cost, the factor 3 is the allowance tests/test_gpu_griffin_lim.py makes for structured rounding
against a model.  The iterations are held as in tests/test_gpu_griffin_lim.py / test_gpu_misi.py, the perturbation's sigma being
max(1e-6, the model's error at that N) max|X|.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest

import lws_amd
from lws_amd import _capi

import fft_model as fm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCALES = np.array([1.0, 1e-3, 300.0])
# every transform: (N, hop); perfectrec keeps nothing of hop == N, so (32, 32) runs without it only
ALL = [(32, 1), (32, 16), (32, 32), (36, 12), (36, 27), (100, 20), (100, 30), (516, 129), (4092, 1023)]
# forward only (istft wants an odd bin count, i.e. N = 0 mod 4): (fsize, fftsize, hop), hop = fsize / 2 and one that does not divide
FORWARD = [(34, 34, 17), (34, 34, 12), (50, 50, 25), (50, 50, 15), (62, 62, 31), (62, 62, 20), (510, 510, 255), (510, 510, 200),
           (4094, 4094, 2047), (4094, 4094, 1500), (32, 34, 16), (32, 34, 12)]


def lengths(N, hop, perfectrec):
    return [1, hop, N, N + 1, 2 * N + hop] if perfectrec else [N, N + 1, 2 * N + hop]


def transform_cases(shapes):
    out = []
    for fsize, fftsize, hop in shapes:
        for perfectrec in (True, False):
            if perfectrec and hop == fsize:
                continue
            out += [(fsize, fftsize, hop, perfectrec, n) for n in dict.fromkeys(lengths(fsize, hop, perfectrec))]
    return out


def signals(n, seed):
    """(6, n), exactly representable in float32: noise at the three scales, a unit impulse at the first sample, one at the last,
    and the alternating +-1 signal (a mirrored index or a wrong sign moves these by O(1) at a bin where noise can hide it)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((6, n))
    x[:3] = rng.standard_normal((3, n)) * SCALES[:, None]
    x[3, 0] = 1.0
    x[4, -1] = 1.0
    x[5] = 1.0 - 2.0 * (np.arange(n) % 2)
    return x.astype(np.float32).astype(np.float64)


NAMES = ["noise", "noise 1e-3", "noise 300", "impulse first", "impulse last", "alternating"]


def hold(tag, dev, ref, mod):
    """Per signal: max |dev - ref| / max |ref| against max(3e-6, 3 x the same figure of the float32 model)."""
    assert dev.shape == ref.shape == mod.shape, (tag, dev.shape, ref.shape, mod.shape)
    worst = 0.0
    for b in range(ref.shape[0]):
        if ref[b].size == 0:
            continue
        got, model = fm.max_rel(dev[b], ref[b]), fm.max_rel(mod[b], ref[b])
        bar = max(3e-6, 3 * model)
        print("%s %-13s: dev %.2e  model %.2e  bar %.2e" % (tag, NAMES[b], got, model, bar))
        assert np.isfinite(dev[b].view(np.float32) if dev[b].dtype.kind == "c" else dev[b]).all(), (tag, b)
        assert got <= bar, (tag, NAMES[b], got, bar)
        worst = max(worst, got)
    return worst


def check_transforms(fsize, fftsize, hop, perfectrec, n, inverse):
    awin, swin = fm.windows(fsize, hop)
    x = signals(n, 7 * fsize + hop + n)
    kw = dict(fftsize=fftsize, perfectrec=perfectrec)
    tag = "stft (%d/%d, %d, %s) len %d" % (fsize, fftsize, hop, "pr" if perfectrec else "--", n)
    ref = np.stack([lws_amd.stft(xb, fsize, hop, awin, **kw) for xb in x])
    mod = fm.stft_model(x, fsize, hop, awin, **kw)
    S = lws_amd.stft_dev(x, fsize, hop, awin, **kw)
    assert S.dtype == torch.complex64 and ref.shape[1] >= 1
    hold(tag, S.cpu().numpy(), ref, mod)
    one = lws_amd.stft_dev(x[1], fsize, hop, awin, **kw)                               # the single-signal form: same bits
    assert torch.equal(one, S[1])
    if not inverse:
        return
    spec = ref.astype(np.complex64)
    back = np.stack([lws_amd.istft(sb.astype(np.complex128), hop, swin, perfectrec=perfectrec) for sb in spec])
    mod = fm.istft_model(spec, hop, swin, perfectrec=perfectrec)
    y = lws_amd.istft_dev(spec, hop, swin, perfectrec=perfectrec)
    assert y.dtype == torch.float32
    hold("i" + tag, y.cpu().numpy(), back, mod)
    assert torch.equal(lws_amd.istft_dev(spec[2], hop, swin, perfectrec=perfectrec), y[2])


@pytest.mark.parametrize("fsize,fftsize,hop,perfectrec,n", transform_cases([(N, N, h) for N, h in ALL]))
def test_stft_istft_match_host(fsize, fftsize, hop, perfectrec, n):
    check_transforms(fsize, fftsize, hop, perfectrec, n, inverse=True)


@pytest.mark.parametrize("fsize,fftsize,hop,perfectrec,n", transform_cases(FORWARD))
def test_stft_matches_host_forward_only_sizes(fsize, fftsize, hop, perfectrec, n):
    check_transforms(fsize, fftsize, hop, perfectrec, n, inverse=False)


def test_forward_error_per_size():
    """The transform alone (rectangular window, hop = N: rows of plain DFTs of unit Gaussian noise) against fp64, per N: the figure
    DESIGN.md section 6 and tests/test_fft_model.py record beside the model's."""
    print("\n    N     m   a   device     float32 model")
    for N in (32, 34, 36, 50, 62, 64, 100, 510, 516, 1000, 4092, 4094, 4096):
        x = np.random.default_rng(N).standard_normal(8 * N).astype(np.float32).astype(np.float64)
        ref = np.fft.rfft(x.reshape(8, N), axis=1)
        S = lws_amd.stft_dev(x, N, N, np.ones(N), perfectrec=False).cpu().numpy()
        mod = fm.stft_model(x, N, N, np.ones(N), perfectrec=False)
        dev, model = fm.max_rel(S, ref), fm.max_rel(mod, ref)
        print("%5d %5d %3d   %.2e   %.2e" % ((N,) + fm.factor(N) + (dev, model)))
        assert S.shape == ref.shape and dev <= max(3e-6, 3 * model), (N, dev, model)


# ---- consistency ------------------------------------------------------------------------------------------------------------
def consistency_dev(S, N, hop, awin, swin, perfectrec):
    t = torch.from_numpy(np.ascontiguousarray(S, dtype=np.complex64)).cuda()
    t = t[None] if t.dim() == 2 else t
    sums = _capi.consistency_dev(t.data_ptr(), t.shape[0], t.shape[1], N, hop, awin, swin, perfectrec,
                                 stream=torch.cuda.current_stream().cuda_stream)
    return 10 * np.log10(sums[:, 0] / sums[:, 1])


# every transform size and hop, with and without perfectrec (which keeps nothing of hop == N: refused, see the last tests)
ITER_CASES = [(N, hop, pr) for N, hop in ALL for pr in (True, False) if not (pr and hop == N)]


@pytest.mark.parametrize("N,hop,perfectrec", ITER_CASES)
def test_consistency_matches_host(N, hop, perfectrec):
    rng = np.random.default_rng(3 * N + hop)
    awin, swin = fm.windows(N, hop)
    X = lws_amd.stft(rng.standard_normal(6 * N), N, hop, awin, perfectrec=perfectrec)
    R = rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)
    # random spectrograms at two scales, zero-phase magnitudes, and a consistent spectrogram
    stack = np.stack([R, np.abs(X).astype(complex), 1e-3 * R, X]).astype(np.complex64)
    host = np.array([lws_amd.get_consistency(S.astype(np.complex128), N, hop, awin, swin, perfectrec=perfectrec) for S in stack])
    dev = consistency_dev(stack, N, hop, awin, swin, perfectrec)
    for b, name in enumerate(("random", "zero phase", "random 1e-3", "stft(noise)")):
        tag = "consistency (%d, %d, %s) %d frames, %s" % (N, hop, perfectrec, X.shape[0], name)
        if host[b] < 60:
            print("%s: dev %.4f dB  host %.4f dB" % (tag, dev[b], host[b]))
            assert abs(dev[b] - host[b]) < 0.01, (tag, dev[b], host[b])
            continue
        # consistent (stft(noise) with perfectrec; with hop == N every spectrogram whose DC and Nyquist bins are real): the host
        # value is fp64 rounding, the device reads what its own float32 round trip leaves, which the model predicts
        back = fm.stft_model(fm.istft_model(stack[b], hop, swin, perfectrec=perfectrec), N, hop, awin, perfectrec=perfectrec)
        model = 20 * np.log10(np.linalg.norm(stack[b]) / np.linalg.norm(back - stack[b]))
        print("%s: dev %.2f dB  model %.2f dB  host %.2f dB" % (tag, dev[b], model, host[b]))
        if model >= 106:
            assert dev[b] > 100.0, (tag, dev[b], model)
        else:
            assert dev[b] >= model - 6, (tag, dev[b], model)


# ---- Griffin-Lim and MISI ----------------------------------------------------------------------------------------------------
def round_trip_frames(M, N, hop, perfectrec):
    """(samples istft keeps of M frames, frames stft makes of them): lws.pyx:55-76,130-137 in integers."""
    if not perfectrec:
        return hop * (M - 1) + N, M
    pre = N - hop if N % hop == 0 else N - N % hop
    n = 0 if hop == N else max(hop * (M - 1) + N - pre - (N - hop), 0)
    return n, (pre + n + (-n) % hop) // hop


def frame_counts(N, hop, perfectrec):
    """One frame (without perfectrec) or the fewest frames the perfectrec round trip keeps with a sample left, then the next
    even and the next odd count."""
    M = 1
    while round_trip_frames(M, N, hop, perfectrec)[0] < 1 or round_trip_frames(M, N, hop, perfectrec)[1] != M:
        M += 1
    return [M, M + 1, M + 2]


def sigma_of(N):
    return max(1e-6, fm.model_error(N))


def make_case(N, hop, perfectrec, M, K, seed):
    """Windows, A = |stft(noise)| at the three scales, (3, M, F) -- for K > 0 sources at levels 1, 0.3, 3: (3, K, M, F), with their
    mixtures -- and c_0 = A exp(2 pi j u) rounded to complex64."""
    rng = np.random.default_rng([seed, N, hop, int(perfectrec), M, K])
    awin, swin = fm.windows(N, hop)
    n = round_trip_frames(M, N, hop, perfectrec)[0]
    assert lws_amd.istft(np.zeros((M, N // 2 + 1), complex), hop, swin, perfectrec=perfectrec).shape == (n,)
    src = rng.standard_normal((3, max(K, 1), n)) * np.array([1.0, 0.3, 3.0])[None, :max(K, 1), None] * SCALES[:, None, None]
    A = np.abs(np.stack([[lws_amd.stft(x, N, hop, awin, perfectrec=perfectrec) for x in s] for s in src]))
    assert A.shape == (3, max(K, 1), M, N // 2 + 1)
    c0 = (A * np.exp(2j * np.pi * rng.random(A.shape))).astype(np.complex64)
    y = src.sum(axis=1).astype(np.float32)
    if K == 0:
        A, c0 = A[:, 0], c0[:, 0]
    for a in (A, c0, y):
        a.setflags(write=False)
    return awin, swin, A, c0, y


def perturbation(seed, sigma):
    rng = np.random.default_rng(seed)

    def f(*args):
        X = args[-1]
        return X + sigma * np.abs(X).max() * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def held_db(db, ref_db, per_db):
    """The trace bar of tests/test_gpu_griffin_lim.py, 0.01 dB + what the error model moves the entry by; an entry the host puts above
    100 dB is fp64 rounding of an exact zero (the iterate is consistent / the sources add up to the mixture exactly), and there the
    float32 device must read above 100 dB too."""
    ok = np.where(ref_db > 100.0, db > 100.0, np.abs(db - ref_db) <= 0.01 + np.abs(per_db - ref_db))
    return bool(ok.all())


def quiet(ref, per, c0, y):
    """The host iteration is well conditioned and its figures can be resolved in float32: under the error model no bin moves beyond
    the far-bin threshold and no trace entry by more than 0.01 dB (entries above 100 dB apart, where the suite takes float32 to
    bottom out, tests/test_gpu_stft.py, and held_db() asks for just that); and, for MISI, the signal bar's 3e-6 of each returned
    signal's largest sample is no less than 2^-23 of the largest sample of the mixture and of all the signals, the spacing of float32
    at the terms of the sum that makes s_k -- a signal of one or two samples is +-source after one step, s_k = (y + x_0 - x_1) / 2 can
    then cancel to little or exactly nothing, and a bar below that spacing is one no float32 evaluation meets."""
    if (np.abs(per[0] - ref[0]) > 1e-3 * np.abs(c0).max(axis=(-2, -1), keepdims=True)).any():
        return False
    if not ((np.abs(per[1] - ref[1]) <= 0.01) | (ref[1] > 100.0)).all():
        return False
    if len(ref) < 3:
        return True
    big = np.maximum(np.abs(y).max(axis=-1), np.abs(ref[2]).max(axis=(-2, -1)))
    return bool((3e-6 * np.abs(ref[2]).max(axis=-1) >= 2.0 ** -23 * big[:, None]).all())


GLA_STEPS = ((1, 0.0), (3, 0.99))
MISI_STEPS = (1, 3)


@functools.lru_cache(maxsize=None)
def settled(N, hop, perfectrec, M, K=0):
    """The case and its host results (fp64, and fp64 under the perturbation model) per step setting.  At these sizes -- spectrograms
    of 17 bins -- an iterate with one projection near zero turns a 1e-6 error into a phase flip of that bin, which alone is more
    than the far-bin cap allows: the case is the first of the seeds 0, 1, 2, ... for which the HOST iteration is quiet() at every
    step setting.  A statement about the fp64 host iteration and its error model, made without a device."""
    for seed in range(256):
        awin, swin, A, c0, y = case = make_case(N, hop, perfectrec, M, K, seed)
        hosts = {}
        for step in (MISI_STEPS if K else GLA_STEPS):
            kw = dict(perfectrec=perfectrec, return_trace=True)
            if K:
                run = functools.partial(lws_amd.misi, c0, y, N, hop, awin, swin, step, return_signals=True, **kw)
            else:
                run = functools.partial(lws_amd.griffin_lim, c0, N, hop, awin, swin, step[0], alpha=step[1], **kw)
            hosts[step] = run(), run(_perturb=perturbation(17 + (step if K else step[0]), sigma_of(N)))
        if all(quiet(ref, per, c0, y) for ref, per in hosts.values()):
            return case, hosts
    raise AssertionError("no quiet seed for %r" % ((N, hop, perfectrec, M, K),))


def check_gla(N, hop, perfectrec, M, n, alpha):
    (awin, swin, A, c0, _), hosts = settled(N, hop, perfectrec, M)
    (ref, ref_db), (per, per_db) = hosts[n, alpha]
    out, db = lws_amd.griffin_lim_dev(c0, N, hop, awin, swin, n, alpha=alpha, perfectrec=perfectrec, return_trace=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == c0.shape and db.shape == (n, 3)
    out = out.cpu().numpy().astype(np.complex128)
    assert np.isfinite(out.view(np.float64)).all()
    target = np.abs(c0).astype(np.float64)
    for b in range(3):
        top = target[b].max()
        dist, bar = rel(out[b], ref[b]), 3 * rel(per[b], ref[b])
        far = np.mean(np.abs(out[b] - ref[b]) > 1e-3 * top)
        mag = np.abs(np.abs(out[b]) - target[b]).max() / top
        ddb, bar_db = np.abs(db[:, b] - ref_db[:, b]), 0.01 + np.abs(per_db[:, b] - ref_db[:, b])
        print("gla (%d, %d, %s) M=%d n=%d alpha=%g b=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  trace dB off %.2e (bar %.2e)"
              % (N, hop, perfectrec, M, n, alpha, b, dist, bar, 100 * far, mag, ddb.max(), bar_db[ddb.argmax()]))
        assert dist <= bar, (b, dist, bar)
        assert far <= 1e-3, (b, far)
        assert mag <= 2e-6, (b, mag)
        assert held_db(db[:, b], ref_db[:, b], per_db[:, b]), (b, db[:, b], ref_db[:, b], per_db[:, b])


@pytest.mark.parametrize("N,hop,perfectrec", ITER_CASES)
def test_griffin_lim_matches_host(N, hop, perfectrec):
    for M in frame_counts(N, hop, perfectrec):
        for n, alpha in GLA_STEPS:
            check_gla(N, hop, perfectrec, M, n, alpha)


EPS = 2.0 ** -24


def mixture_bound(K, y, x):
    """Twice the worst-case fp32 rounding of K adds, one subtract, one divide and K adds on values of these sizes."""
    return 4 * (K + 1) * EPS * (np.abs(y).max() + sum(np.abs(xk).max() for xk in x))


def check_misi(N, hop, perfectrec, M, K, n):
    (awin, swin, A, c0, y), hosts = settled(N, hop, perfectrec, M, K)
    (ref, ref_db, ref_s), (per, per_db, per_s) = hosts[n]
    out, db, s = lws_amd.misi_dev(c0, y, N, hop, awin, swin, n, perfectrec=perfectrec, return_trace=True, return_signals=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == c0.shape and db.shape == (n, 3)
    assert s.dtype == torch.float32 and tuple(s.shape) == (3, K, y.shape[1])
    out, s = out.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
    target = np.abs(c0).astype(np.float64)
    tag = "misi (%d, %d, %s) M=%d K=%d n=%d" % (N, hop, perfectrec, M, K, n)
    for b in range(3):
        ddb, bar_db = np.abs(db[:, b] - ref_db[:, b]), 0.01 + np.abs(per_db[:, b] - ref_db[:, b])
        x_host = [lws_amd.istft(ref[b, k], hop, swin, perfectrec=perfectrec) for k in range(K)]
        mix, mix_bar = np.abs(s[b].sum(axis=0) - y[b]).max(), mixture_bound(K, y[b], x_host)
        print("%s b=%d: trace dB off %.2e (bar %.2e)  |sum s - y| %.2e (bound %.2e)" % (tag, b, ddb.max(), bar_db[ddb.argmax()], mix, mix_bar))
        assert held_db(db[:, b], ref_db[:, b], per_db[:, b]), (b, db[:, b], ref_db[:, b], per_db[:, b])
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


@pytest.mark.parametrize("N,hop,perfectrec", ITER_CASES)
@pytest.mark.parametrize("K", [2, 3])
def test_misi_matches_host(N, hop, perfectrec, K):
    for M in frame_counts(N, hop, perfectrec):
        for n in MISI_STEPS:
            check_misi(N, hop, perfectrec, M, K, n)


# ---- batch pitch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,hop", [(36, 27), (4092, 1023)])
@pytest.mark.parametrize("perfectrec", [True, False])
def test_stack_of_three_equals_three_single_calls_bit_for_bit(N, hop, perfectrec):
    awin, swin = fm.windows(N, hop)
    M = frame_counts(N, hop, perfectrec)[1]
    x = torch.from_numpy(signals(2 * N + hop + 1, N)[:3].astype(np.float32)).cuda()
    S = lws_amd.stft_dev(x, N, hop, awin, perfectrec=perfectrec)
    y = lws_amd.istft_dev(S, hop, swin, perfectrec=perfectrec)
    db = consistency_dev(S.cpu().numpy(), N, hop, awin, swin, perfectrec)
    for b in range(3):
        assert torch.equal(lws_amd.stft_dev(x[b], N, hop, awin, perfectrec=perfectrec), S[b])
        assert torch.equal(lws_amd.istft_dev(S[b], hop, swin, perfectrec=perfectrec), y[b])
        assert consistency_dev(S[b].cpu().numpy(), N, hop, awin, swin, perfectrec)[0] == db[b]
    _, _, _, c0, _ = make_case(N, hop, perfectrec, M, 0, 0)
    t = torch.from_numpy(c0).cuda()
    out, tr = lws_amd.griffin_lim_dev(t, N, hop, awin, swin, 3, perfectrec=perfectrec, return_trace=True)
    for b in range(3):
        one, one_tr = lws_amd.griffin_lim_dev(t[b], N, hop, awin, swin, 3, perfectrec=perfectrec, return_trace=True)
        assert torch.equal(one, out[b]) and np.array_equal(one_tr, tr[:, b])
    _, _, _, c0, mix = make_case(N, hop, perfectrec, M, 2, 0)
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(mix).cuda()
    out, tr, s = lws_amd.misi_dev(t, ty, N, hop, awin, swin, 3, perfectrec=perfectrec, return_trace=True, return_signals=True)
    for b in range(3):
        one, one_tr, one_s = lws_amd.misi_dev(t[b], ty[b], N, hop, awin, swin, 3, perfectrec=perfectrec, return_trace=True,
                                              return_signals=True)
        assert torch.equal(one, out[b]) and np.array_equal(one_tr, tr[:, b]) and torch.equal(one_s, s[b])


# ---- where the device and the host definition used to part ----------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2])
def test_too_few_frames_for_perfectrec_raise(M):
    """The host griffin_lim raises when stft(istft(.)) does not give the frame count back; the device forms ran on and returned
    numbers computed from an all-zero signal."""
    rng = np.random.default_rng(M)
    awin, swin = fm.windows(64, 16)
    c0 = (rng.standard_normal((3, M, 33)) + 1j * rng.standard_normal((3, M, 33))).astype(np.complex64)
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        lws_amd.griffin_lim(c0, 64, 16, awin, swin, 2, perfectrec=True)
    t = torch.from_numpy(c0).cuda()
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        lws_amd.griffin_lim_dev(t, 64, 16, awin, swin, 2, perfectrec=True)
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        _capi.consistency_dev(t.data_ptr(), 3, M, 64, 16, awin, swin, True)
    if M > 1:                                         # (one frame broadcasts against the three that come back: a number, of nothing)
        with pytest.raises(ValueError):
            lws_amd.get_consistency(c0[0], 64, 16, awin, swin, perfectrec=True)
    lib = _capi.load()
    w = np.ascontiguousarray(awin)
    rc = lib.lws_griffin_lim_dev(0, t.data_ptr(), None, 3, M, 64, 16, w.ctypes.data, w.ctypes.data, 1, 2, 0.5, None, None)
    assert rc == _capi.LWS_ERR_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), c0)
    assert torch.equal(lws_amd.griffin_lim_dev(t, 64, 16, awin, swin, 0, perfectrec=True), t)         # zero iterations: no round trip
    lws_amd.griffin_lim_dev(t, 64, 16, awin, swin, 2, perfectrec=False)                                # ... and none without perfectrec


@pytest.mark.parametrize("N,hop,M", [(64, 16, 1), (32, 32, 3)])
def test_istft_of_frames_perfectrec_cuts_away_is_empty(N, hop, M):
    rng = np.random.default_rng(N)
    awin = np.sqrt(lws_amd.hann(N))
    swin = lws_amd.synthwin(awin, hop)
    spec = (rng.standard_normal((3, M, N // 2 + 1)) + 1j * rng.standard_normal((3, M, N // 2 + 1))).astype(np.complex64)
    assert lws_amd.istft(spec[0], hop, swin, perfectrec=True).shape == (0,)
    assert _capi.istft_length(M, N, hop, True) == 0
    y = lws_amd.istft_dev(spec, hop, swin, perfectrec=True)
    assert tuple(y.shape) == (3, 0) and y.dtype == torch.float32
    assert tuple(lws_amd.istft_dev(spec[0], hop, swin, perfectrec=True).shape) == (0,)
    with pytest.raises(ValueError):                                                  # MISI still refuses a mixture of no samples
        lws_amd.misi_dev(spec[None], np.zeros((1, 0), np.float32), N, hop, awin, swin, 0, perfectrec=True, return_signals=True)
    # without perfectrec the same frames give the whole overlap-add
    y = lws_amd.istft_dev(spec, hop, swin, perfectrec=False).cpu().numpy()
    ref = np.stack([lws_amd.istft(s.astype(np.complex128), hop, swin) for s in spec])
    assert y.shape == ref.shape and np.abs(y - ref).max() < 3e-6 * np.abs(ref).max()


@pytest.mark.parametrize("n", [1, 10, 47, 48])
def test_stft_of_less_than_a_frame_is_empty(n):
    awin = np.sqrt(lws_amd.hann(64))
    x = np.random.default_rng(n).standard_normal((3, n))
    assert lws_amd.stft(x[0], 64, 16, awin).shape == (0, 33)
    S = lws_amd.stft_dev(x, 64, 16, awin)
    assert tuple(S.shape) == (3, 0, 33) and S.dtype == torch.complex64
    assert tuple(lws_amd.stft_dev(x[0], 64, 16, awin).shape) == (0, 33)
    assert tuple(lws_amd.stft_dev(x, 64, 16, awin, fftsize=96).shape) == (3, 0, 49)
    # one more hop of samples and the host pads up to one frame: so does the device
    x = np.random.default_rng(n).standard_normal((3, 48 + n))
    ref = np.stack([lws_amd.stft(xb, 64, 16, awin) for xb in x])
    S = lws_amd.stft_dev(x, 64, 16, awin).cpu().numpy()
    assert S.shape == ref.shape and ref.shape[1] >= 1 and np.abs(S - ref).max() < 3e-6 * np.abs(ref).max()
