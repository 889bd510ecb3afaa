"""Inputs, cotangents, error model and host fp64 references shared by tests/test_misi_grad_host.py (CPU) and
tests/test_gpu_misi_grad.py (GPU).  Nothing here needs torch or a device.

The error model is the one of tests/test_gpu_misi.py, extended to the backward pass: every projection argument X_{i,k} of the
forward pass, and every result of a backward transform (the gc of step 2, the gv of step 4 of lws_amd.misi_grad), is perturbed by
seeded Gaussian noise of standard deviation 1e-6 max|.| per component.  The distance the fp64 gradients move under it, times 3, is
the bar the float32 device pass is held to."""
import functools

import numpy as np

import lws_amd

SCALES = np.array([1.0, 1e-3, 300.0])          # of the B = 3 mixtures
SOURCES = np.array([1.0, 0.3, 3.0])            # relative levels of the sources of a mixture
STEPS = (1, 3, 5)
# (fsize, fshift, perfectrec, T, K)
HOST_SHAPES = [
    (64, 16, False, 9, 2),                     # power of two
    (64, 16, True, 12, 3),                     # power of two, perfectrec
    (48, 16, True, 7, 2),                      # odd factor 3
    (48, 16, False, 1, 1),                     # single frame and K = 1
    (256, 96, False, 2, 3),                    # hop does not divide the frame
    (256, 96, True, 5, 2),                     # same, perfectrec
]
GPU_SHAPES = HOST_SHAPES + [
    (1000, 250, True, 5, 2),                   # odd factor 125
    (4096, 1024, False, 5, 2),                 # the large-LDS path
]
FAR, FAR_CAP = 1e-3, 5e-3                      # entries of gA further than FAR max|gA| from the reference: at most FAR_CAP of them
SEED = 2000000


def ident(key):
    return "%d-%d-%s-T%d-K%d" % key


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, K, B=3):
    """p, the magnitudes A = |stft(source)| rounded to float32, the start c_0 = A exp(j phase) rounded to complex64 -- the true
    phase plus 0.5 rad of noise: where a separation front end starts from -- the mixture y rounded to float32, and the cotangents
    gC (complex64) and gs (float32), all as the device is given them and as the host run starts from.  A projection argument near
    zero turns a 1e-6 error into a phase flip of that bin and a large move of the entries of gA it feeds; SEED is one for which the
    host error model leaves at most FAR_CAP of the entries of gA (0.16 % at most) further than FAR max|gA| away, for every mixture
    and source of every shape at every step count: of the offsets 0, 100000 .. 2900000 only this one does
    (tests/test_misi_grad_host.py asserts it: a statement about the fp64 host pass, made without a device).  The cap is on gA alone:
    gS and gy are transforms of what a bin's gradient becomes, so one moved bin moves every entry of its frame, and a move of 1e-3
    rel-L2 -- within what the error model does to them -- already puts many of their entries beyond 1e-3 of the largest; they are
    held by their rel-L2 distance."""
    rng = np.random.default_rng(SEED + 1000 * fsize + 10 * fshift + perfectrec)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    src = rng.standard_normal((B, K, n)) * SOURCES[None, :K, None] * SCALES[:B, None, None]
    X = np.stack([[p.stft(x) for x in s] for s in src])
    assert X.shape == (B, K, T, F)
    A = np.abs(X).astype(np.float32)
    c0 = (A * np.exp(1j * (np.angle(X) + 0.5 * rng.standard_normal(X.shape)))).astype(np.complex64)
    y = src.sum(axis=1).astype(np.float32)
    gC = ((rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)) / np.sqrt(fsize)).astype(np.complex64)
    gs = rng.standard_normal(src.shape).astype(np.float32)
    for a in (A, c0, y, gC, gs):
        a.setflags(write=False)
    return p, A, c0, y, gC, gs


def sources(fsize, fshift, perfectrec, T, K, B=3):
    """The signals the magnitudes of case() were taken from (its first draw), (B, K, len): a target for a waveform loss."""
    rng = np.random.default_rng(SEED + 1000 * fsize + 10 * fshift + perfectrec)
    n = case(fsize, fshift, perfectrec, T, K, B)[3].shape[1]
    return rng.standard_normal((B, K, n)) * SOURCES[None, :K, None] * SCALES[:B, None, None]


def perturbation(seed, kinds=('X', 'gc', 'gv')):
    """The error model: Z + 1e-6 max|Z| noise (complex for the spectra, real for the signals) on the listed kinds."""
    rng = np.random.default_rng(seed)

    def f(kind, i, b, k, Z):
        if kind not in kinds:
            return Z
        sigma = 1e-6 * np.abs(Z).max()
        if np.iscomplexobj(Z):
            return Z + sigma * (rng.standard_normal(Z.shape) + 1j * rng.standard_normal(Z.shape))
        return Z + sigma * rng.standard_normal(Z.shape)
    return f


@functools.lru_cache(maxsize=None)
def host(key, n):
    """(gA, gS, gy) of lws_amd.misi_grad in fp64 from the rounded inputs, and the same under the full error model."""
    p, A, c0, y, gC, gs = case(*key)
    args = (c0, y, p.fsize, p.fshift, p.awin, p.swin, n, A.astype(np.float64))
    kw = dict(grad_out=gC, grad_signals=gs, perfectrec=p.perfectrec)
    ref = lws_amd.misi_grad(*args, **kw)
    per = lws_amd.misi_grad(*args, _perturb=perturbation(n + 17), **kw)
    return ref, per


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a - b)


def far(a, b):
    """The share of the entries of a further than FAR max|b| from b."""
    return float(np.mean(np.abs(a - b) > FAR * np.abs(b).max()))
