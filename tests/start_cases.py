"""Inputs, error model and host references of the tests of the magnitude-only starts of the look-ahead iterations
(start='overlap' of lws_amd.rtisi_la, start='mixture' of lws_amd.misi_la), shared by tests/test_start_host.py,
tests/test_gpu_rtisi_start.py and tests/test_gpu_misi_start.py so that each fp64 reference is computed once.

The inputs are magnitudes alone, rounded to float32 (what the device is given).  For a shape (fsize, fshift, perfectrec, T) the
generator is seeded as tests/test_gpu_rtisi.py seeds its own, draws the noise signal first and the noise floor of the tone signal
second, and takes the magnitudes of stft of either signal at the three scales 1, 1e-3 and 300:
  'noise' : white noise;
  'tones' : sum_i (1 + 0.3 cos(2 pi t / (3.1 fsize) + i)) cos(2 pi f_i t + 0.7 i), f = 0.031, 0.117, 0.203, 0.37 cycles per sample,
            plus 0.05 of the second noise.
The error model is that of tests/test_gpu_rtisi.py -- every projection, the entry projections included (it = 0), perturbed by seeded
complex Gaussian noise of standard deviation 1e-6 max|X| per component.

The overlap start is sensitive where the transform of a partial sum is nearly zero in a bin: the bin takes an arbitrary phase and
drags its frame along, and the fp64 definition itself then moves under the model.  So the device is held to the definition in two
ways.  (a) Teacher-forced, exact and on every shape: at iterations = 0 the device's rows are the entry estimates, and each is
recomputed in fp64 from the device's own earlier rows (entry_check below).  (b) Whole runs, by the rule of tests/test_gpu_rtisi.py,
on the inputs of WHOLE_RUNS alone: those on which the model stays at zero far bins, which tests/test_start_host.py re-asserts."""
import functools

import numpy as np

import lws_amd

SCALES = np.array([1.0, 1e-3, 300.0])
STEPS = [(0, 1), (0, 4), (1, 3), (2, 2), (3, 1), (3, 3), (3, 6), (5, 2)]     # those of tests/test_gpu_rtisi.py
TONES = (0.031, 0.117, 0.203, 0.37)
SIGMA, TAU = 1e-6, 1e-3        # the model of a device projection's error; the bins a teacher-forced check leaves out: |X| < TAU max|X|
MAX_LEFT_OUT = 0.01            # ... at most this share of the bins of the frames j >= 1 of a spectrogram
# (fsize, fshift, perfectrec, T): the signals whose whole runs are held to the host by rule (b)
WHOLE_RUNS = {
    (64, 16, False, 9): ("tones",),                    # power of two
    (64, 16, True, 12): ("noise", "tones"),
    (256, 96, True, 5): ("tones",),                    # hop does not divide the frame
    (1000, 250, True, 5): ("noise", "tones"),          # odd factor 125
    (128, 32, True, 12): ("noise",),
    (64, 8, True, 20): ("noise",),                     # Q = 8
    (64, 64, False, 6): ("noise", "tones"),            # hop = N: every frame enters as A + 0j
    (64, 32, True, 8): ("tones",),                     # Q = 2
    (4096, 1024, True, 4): ("noise", "tones"),         # the state does not fit in LDS: device scratch
}


# ... less the (input, step) cases on which the model itself moves bins with this generator (measured in fp64 over the eight seeds of
# tests/test_start_host.py: 0.01-0.8 % of the bins further than 1e-3 max A); every other step of these inputs stays
DROPPED = {
    ((256, 96, True, 5), "tones"): [(0, 4)],
    ((1000, 250, True, 5), "noise"): [(3, 1)],
    ((4096, 1024, True, 4), "noise"): [(3, 3)],
    ((128, 32, True, 12), "noise"): [(0, 4), (3, 1), (5, 2)],
}
# the streams held to rtisi_la(..., start='overlap', open_end=True), and their steps
STREAM_RUNS = [((64, 16, True, 12), "noise"), ((256, 96, True, 5), "tones"), ((64, 64, False, 6), "tones"), ((4096, 1024, True, 4), "tones")]
STREAM_STEPS = [(0, 1), (2, 2), (3, 3), (5, 2)]


def whole_runs():
    return [(key, signal) for key in sorted(WHOLE_RUNS) for signal in WHOLE_RUNS[key]]


def steps_of(run):
    return [s for s in STEPS if s not in DROPPED.get(run, [])]


def run_id(run):
    key, signal = run
    return "%d-%d-%s-T%d-%s" % (key + (signal,))


@functools.lru_cache(maxsize=None)
def signals(fsize, fshift, perfectrec, T):
    """p and the two signals, {'noise': x, 'tones': x}, of the length istft gives T frames."""
    rng = np.random.default_rng(1000 * fsize + 10 * fshift + perfectrec)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    n = lws_amd.istft(np.zeros((T, fsize // 2 + 1), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    noise, floor = rng.standard_normal(n), rng.standard_normal(n)
    t = np.arange(n)
    tones = 0.05 * floor
    for i, f in enumerate(TONES):
        tones = tones + (1 + 0.3 * np.cos(2 * np.pi * t / (3.1 * fsize) + i)) * np.cos(2 * np.pi * f * t + 0.7 * i)
    return p, {"noise": noise, "tones": tones}


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, signal="noise"):
    """p, A (3, T, F): the magnitudes of the signal's spectrogram at the three scales, rounded to float32."""
    p, x = signals(fsize, fshift, perfectrec, T)
    X = p.stft(x[signal])
    assert X.shape == (T, fsize // 2 + 1)
    A = (np.abs(X)[None] * SCALES[:, None, None]).astype(np.float32).astype(np.float64)
    A.setflags(write=False)
    return p, A


def perturbation(seed):
    rng = np.random.default_rng(seed)

    def f(m, it, b, X):
        sigma = SIGMA * np.abs(X).max()
        return X + sigma * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


@functools.lru_cache(maxsize=None)
def host(key, signal, LA, n, seed=None, open_end=False):
    """rtisi_la(A, ..., start='overlap') in fp64 with its signal; under the error model if a seed is given."""
    p, A = case(*key, signal=signal)
    out, sig = lws_amd.rtisi_la(A, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, perfectrec=p.perfectrec, return_signal=True,
                                start="overlap", open_end=open_end, _perturb=None if seed is None else perturbation(seed))
    for a in (out, sig):
        a.setflags(write=False)
    return out, sig


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def far_fraction(a, ref, top):
    return np.mean(np.abs(a - ref) > 1e-3 * top)


def entry_check(p, A, rows, open_end=False, sigma=SIGMA):
    """Teacher-forced check of entry estimates: `rows` (T, F) are the rows a run with iterations = 0 returned for the magnitudes A
    (T, F).  Every row j is recomputed in fp64 from the rows before it, y = keep sum_{i < j} swin irfft(rows[i]),
    X = rfft(awin y[window j]), and compared with A_j X / |X| on the bins with |X| >= TAU max_k |X|, where a device projection off by
    SIGMA max|X| per component turns the phase by at most sqrt(2) SIGMA / TAU: the bound is 3 sqrt(2) SIGMA / TAU A_j + 2e-6 max A
    (3: the margin the project puts on its model; 2e-6 max A: the magnitude bar of the existing tests).  Where X is exactly zero the
    row must be exactly A_j + 0j.  sigma: another model of a device projection's error where the float32 transform model says SIGMA is
    out of reach (tests/window_cases.py).  Returns (worst error / bound, share of the bins of the frames j >= 1 left out, rows that had to be
    exact)."""
    T, F = A.shape
    fsize, fshift = p.fsize, p.fshift
    total = fshift * (T - 1) + fsize
    keep = np.ones(total)
    if p.perfectrec:
        lo = fsize - fshift if fsize % fshift == 0 else fsize - fsize % fshift
        keep[:lo] = 0.0
        if not open_end:
            keep[max(total - (fsize - fshift), 0):] = 0.0
    swin = np.squeeze(np.asarray(p.swin, dtype=np.float64))
    y = np.zeros(total)
    worst, left_out, exact = 0.0, 0, 0
    for j in range(T):
        X = np.fft.rfft(p.awin * (keep * y)[fshift * j: fshift * j + fsize])
        mag = np.abs(X)
        if not mag.any():
            assert np.array_equal(rows[j], A[j] + 0j), j
            exact += 1
        else:
            use = mag >= TAU * mag.max()
            if j:
                left_out += np.count_nonzero(~use)
            err = np.abs(rows[j] - A[j] * X / np.where(mag > 0, mag, 1.0))[use]
            bound = (3 * np.sqrt(2) * sigma / TAU * A[j] + 2e-6 * A.max())[use]
            worst = max(worst, (err / bound).max())
        y[fshift * j: fshift * j + fsize] += swin * np.fft.irfft(rows[j], fsize)
    return worst, left_out / max((T - 1) * F, 1), exact


# ---- online MISI, start='mixture': K sources (tones, noise, half a second noise, 0.3 of a third, ...) and their float32 sum
MISI_LEVELS = (1.0, 1.0, 0.5, 0.3)


@functools.lru_cache(maxsize=None)
def misi_case(fsize, fshift, perfectrec, T, K):
    """p, A (3, K, T, F) rounded to float32, and the mixtures y (3, len) rounded to float32."""
    p, x = signals(fsize, fshift, perfectrec, T)
    rng = np.random.default_rng(7 + 1000 * fsize + 10 * fshift + perfectrec)
    src = [x["tones"], x["noise"]] + [rng.standard_normal(x["noise"].shape[0]) for _ in range(2)]
    src = np.stack([MISI_LEVELS[k] * src[k] for k in range(K)])
    A = np.abs(np.stack([p.stft(s) for s in src]))[None] * SCALES[:, None, None, None]
    y = (src.sum(axis=0)[None] * SCALES[:, None]).astype(np.float32)
    A = A.astype(np.float32).astype(np.float64)
    for a in (A, y):
        a.setflags(write=False)
    return p, A, y


def misi_perturbation(seed):
    rng = np.random.default_rng(seed)

    def f(m, it, b, X):
        sigma = SIGMA * np.abs(X).max(axis=(1, 2), keepdims=True)
        return X + sigma * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


def stream_mixture(p, y, T):
    """The mixture a stream of T frames is pushed: y and, with perfectrec, the fsize - fshift zeros stft pads with."""
    y = np.asarray(y)
    if not p.perfectrec:
        return y
    return np.concatenate([y, np.zeros(y.shape[:-1] + (p.fsize - p.fshift,), y.dtype)], axis=-1)


@functools.lru_cache(maxsize=None)
def misi_host(key, LA, n, seed=None, open_end=False):
    """misi_la(A, y, ..., start='mixture') in fp64 with its signals; under the error model if a seed is given."""
    p, A, y = misi_case(*key)
    mix = stream_mixture(p, y, key[3]) if open_end else y
    out, s = lws_amd.misi_la(A, mix, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, perfectrec=p.perfectrec, return_signals=True,
                             start="mixture", open_end=open_end, _perturb=None if seed is None else misi_perturbation(seed))
    for a in (out, s):
        a.setflags(write=False)
    return out, s
