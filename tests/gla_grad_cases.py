"""Inputs, cotangent, error model and host fp64 references shared by tests/test_gla_grad_host.py (CPU) and
tests/test_gpu_gla_grad.py (GPU).  Nothing here needs torch or a device.

The error model is the one of tests/misi_grad_cases.py: every projection argument X_i of the forward pass, and every result of a
backward transform (the gv of step 4, the gc of step 2 of lws_amd.griffin_lim_grad), is perturbed by seeded Gaussian noise of
standard deviation 1e-6 max|.| per component.  The distance the fp64 gradients move under it, times 3, is the bar the float32
device pass is held to."""
import functools

import numpy as np

import lws_amd

SCALES = np.array([1.0, 1e-3, 300.0])          # of the B = 3 spectrograms
STEPS = (1, 3, 5)                              # 3: the first count at which momentum reaches the gradient; >= 4: both terms of step 0
ALPHAS = (0.0, 0.99)
# (fsize, fshift, perfectrec, T)
HOST_SHAPES = [
    (64, 16, False, 9),                        # power of two
    (64, 16, True, 12),                        # power of two, perfectrec
    (48, 16, True, 7),                         # odd factor 3
    (48, 16, False, 1),                        # single frame
    (256, 96, False, 2),                       # hop does not divide the frame
    (256, 96, True, 5),                        # same, perfectrec
]
GPU_SHAPES = HOST_SHAPES + [
    (1000, 250, True, 5),                      # odd factor 125
    (4096, 1024, False, 5),                    # the large-LDS path
    (512, 128, False, 5),                      # the frame of every quoted figure; 512 threads in the look-ahead kernels
    (600, 150, True, 6),                       # odd factor 75; 768 threads there
    (36, 27, False, 4),                        # hop above N/2 that does not divide N
    (36, 12, True, 5),                         # N = 4 * 9, perfectrec
    (32, 1, False, 12),                        # hop = 1, the smallest frame
    (32, 32, False, 3),                        # hop = N: frames do not overlap
]
FAR, FAR_CAP = 1e-3, 5e-3                      # entries of gA further than FAR max|gA| from the reference: at most FAR_CAP of them
START_NOISE = 0.1                              # rad: where an LWS or network start leaves a refinement
SEED = 1400000


def ident(key):
    return "%d-%d-%s-T%d" % key


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, B=3):
    """p, the magnitudes A = |stft(white noise)| rounded to float32, the start c_0 = A exp(j phase) rounded to complex64 -- the
    true phase plus START_NOISE rad of noise -- and the cotangent gC (complex64), all as the device is given them and as the host
    run starts from.  Griffin-Lim has no mixture to anchor it: a projection argument near zero turns a 1e-6 error into a phase
    flip of that bin and a large move of the entries of gA it feeds, and at the 0.5 rad start of tests/misi_grad_cases.py the model
    alone moves most of gA for some seeds.  SEED is one for which the host error model leaves at most FAR_CAP of the entries of gA
    further than FAR max|gA| away (0.039 % at most), for every spectrogram of every shape at every step count and momentum: of the
    offsets 0, 100000 .. 2900000 in this draw order ten do, and this one moves the fewest entries; 200000 leaves 39 % of a
    (256, 96, perfectrec) gA far (tests/test_gla_grad_host.py asserts the cap: a statement about the fp64 host pass, made without
    a device).  That scan was over the first eight GPU_SHAPES.  Of the six appended since, (600, 150, True, 6) reaches 0.332 % at
    n = 5 with momentum, still under the cap, and the other five move no entry far.  The cap is on gA alone,
    as in tests/misi_grad_cases.py: gS is a transform of what a bin's gradient becomes and is held by its rel-L2 distance."""
    rng = np.random.default_rng(SEED + 1000 * fsize + 10 * fshift + perfectrec)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    src = rng.standard_normal((B, n)) * SCALES[:B, None]
    X = np.stack([p.stft(x) for x in src])
    assert X.shape == (B, T, F)
    A = np.abs(X).astype(np.float32)
    c0 = (A * np.exp(1j * (np.angle(X) + START_NOISE * rng.standard_normal(X.shape)))).astype(np.complex64)
    gC = ((rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)) / np.sqrt(fsize)).astype(np.complex64)
    for a in (A, c0, gC):
        a.setflags(write=False)
    return p, A, c0, gC


def truth(fsize, fshift, perfectrec, T, B=3):
    """The spectrograms the magnitudes of case() were taken from (its first draw), (B, T, F): a target for a spectral loss."""
    rng = np.random.default_rng(SEED + 1000 * fsize + 10 * fshift + perfectrec)
    p = case(fsize, fshift, perfectrec, T, B)[0]
    n = lws_amd.istft(np.zeros((T, fsize // 2 + 1), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    return np.stack([p.stft(x) for x in rng.standard_normal((B, n)) * SCALES[:B, None]])


def perturbation(seed, kinds=('X', 'gc', 'gv')):
    """The error model: Z + 1e-6 max|Z| noise (complex for the spectra, real for the signals) on the listed kinds."""
    rng = np.random.default_rng(seed)

    def f(kind, i, b, Z):
        if kind not in kinds:
            return Z
        sigma = 1e-6 * np.abs(Z).max()
        if np.iscomplexobj(Z):
            return Z + sigma * (rng.standard_normal(Z.shape) + 1j * rng.standard_normal(Z.shape))
        return Z + sigma * rng.standard_normal(Z.shape)
    return f


@functools.lru_cache(maxsize=None)
def host(key, n, alpha):
    """(gA, gS) of lws_amd.griffin_lim_grad in fp64 from the rounded inputs, and the same under the full error model."""
    p, A, c0, gC = case(*key)
    args = (c0, p.fsize, p.fshift, p.awin, p.swin, n, A.astype(np.float64))
    kw = dict(alpha=alpha, grad_out=gC, perfectrec=p.perfectrec)
    ref = lws_amd.griffin_lim_grad(*args, **kw)
    per = lws_amd.griffin_lim_grad(*args, _perturb=perturbation(n + 17), **kw)
    return ref, per


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a - b)


def far(a, b):
    """The share of the entries of a further than FAR max|b| from b."""
    return float(np.mean(np.abs(a - b) > FAR * np.abs(b).max()))
