"""Inputs, error model and host references of the online-MISI tests (lws_amd.misi_la / misi_la_dev), shared by
tests/test_misi_la_host.py and tests/test_gpu_misi_la.py so that each fp64 reference is computed once.

The starts are the true phases of the sources with 0.3 rad of Gaussian noise (from random phases the iteration is chaotic, see
tests/test_gpu_rtisi.py), rounded to complex64; the sources of a mixture stand at 1 : 0.3 : 3 and the three mixtures of a stack at
scales 1, 1e-3 and 300; the mixture is the float32 sum of the true signals.  The error model perturbs the projections of every inner
iteration by seeded complex Gaussian noise of standard deviation 1e-6 max|X_k| per component, per source."""
import functools

import numpy as np

import lws_amd

SCALES = np.array([1.0, 1e-3, 300.0])          # of the B = 3 mixtures
SOURCES = np.array([1.0, 0.3, 3.0, 1.0])       # relative levels of the sources of a mixture (1 : 0.3 : 3, and round again)
# (look_ahead, iterations), those of tests/test_gpu_rtisi.py: odd and even counts of active frames, look-aheads beyond the short cases
STEPS = [(0, 1), (0, 4), (1, 3), (2, 2), (3, 1), (3, 3), (3, 6), (5, 2)]
# (fsize, fshift, perfectrec): (T, K)
SHAPES = {
    (64, 16, False): (9, 2),                   # power of two
    (64, 16, True): (12, 3),                   # power of two, perfectrec
    (48, 16, False): (1, 2),                   # odd factor 3, one frame
    (48, 16, True): (7, 1),                    # K = 1
    (256, 96, False): (2, 3),                  # hop does not divide the frame
    (256, 96, True): (5, 2),                   # same, perfectrec
    (1000, 250, True): (5, 2),                 # odd factor 125
    (512, 128, False): (40, 2),                # the rings wrap many times
    (128, 32, True): (20, 3),                  # the rings wrap many times, perfectrec
    (4096, 1024, False): (6, 2),               # the state does not fit in LDS: device scratch
}
# Placements, workgroups and overlaps SHAPES never reaches, with their own steps.  (fsize, fshift, perfectrec, T, K): (threads,
# [(look_ahead, iterations, state in LDS)]); the GPU test asserts placement and workgroup through lws_rtisi_la_placement.  hop = N is
# not here: with K = 2 the error model itself moves 0.5 % of the bins (tests/test_misi_la_host.py allows it 0.02 %).
EDGE_SHAPES = {
    (64, 40, False, 8, 2): (256, [(3, 3, True)]),                    # hop > N / 2
    (64, 32, True, 8, 3): (256, [(3, 3, True)]),                     # Q = N / hop = 2
    (64, 8, True, 20, 2): (256, [(3, 3, True), (9, 2, True)]),       # Q = 8; more active frames than overlap (LA + 1 > Q)
    (600, 150, True, 7, 2): (768, [(2, 3, True)]),                   # a workgroup of 768 threads
    (2048, 512, False, 6, 1): (1024, [(3, 2, True), (4, 2, True)]),  # N > workgroup; at LA = 4 the launch asks for 163 840 bytes: the cap
    (1024, 256, False, 6, 2): (1024, [(3, 2, True)]),                # K = 2 in LDS ...
    (1024, 256, False, 6, 3): (1024, [(3, 3, False)]),               # ... K = 3 in scratch (at n = 2 the model moves 0.03 % of the bins)
    (512, 128, False, 8, 4): (512, [(5, 2, True), (6, 2, False)]),   # LA = 5 in LDS (147 968 bytes), LA = 6 in scratch
}


def keys():
    return [k + SHAPES[k] for k in sorted(SHAPES)]


def key_id(k):
    return "%d-%d-%s-T%d-K%d" % tuple(k[:5])


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, K):
    """p, A = |c0| (B, K, T, F), c0 = X exp(0.3j g) rounded to complex64 with X the sources' spectrograms, and the mixture y
    rounded to float32: what the device is given, and what the host run starts from."""
    rng = np.random.default_rng(1000 * fsize + 10 * fshift + perfectrec)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    src = rng.standard_normal((3, K, n)) * SOURCES[None, :K, None] * SCALES[:, None, None]
    X = np.stack([[p.stft(x) for x in s] for s in src])
    assert X.shape == (3, K, T, F)
    c0 = (X * np.exp(0.3j * rng.standard_normal(X.shape))).astype(np.complex64)
    A = np.abs(c0).astype(np.float64)
    y = src.sum(axis=1).astype(np.float32)
    for a in (A, c0, y):
        a.setflags(write=False)
    return p, A, c0, y


def perturbation(seed):
    rng = np.random.default_rng(seed)

    def f(m, it, b, X):
        sigma = 1e-6 * np.abs(X).max(axis=(1, 2), keepdims=True)
        return X + sigma * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


def magnitudes_of(A):
    """Targets that differ from |c_0|: its magnitudes rolled along time and rescaled (spectrograms of other signals)."""
    return np.roll(A, 1, axis=2) * 0.7 + 0.05 * A.max(axis=(2, 3), keepdims=True)


@functools.lru_cache(maxsize=None)
def host(key, LA, n, explicit=False):
    """Host fp64 result and signals, and the same under the perturbation model: ((ref, ref_s), (per, per_s))."""
    p, A, c0, y = case(*key)
    kw = dict(look_ahead=LA, magnitudes=magnitudes_of(A) if explicit else None, perfectrec=p.perfectrec, return_signals=True)
    ref = lws_amd.misi_la(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, **kw)
    per = lws_amd.misi_la(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, _perturb=perturbation(n + 17), **kw)
    return ref, per


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)
