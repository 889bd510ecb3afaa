"""Inputs, cotangents, error model and host fp64 references shared by tests/test_rtisi_grad_host.py (CPU) and
tests/test_gpu_rtisi_grad.py (GPU).  Nothing here needs torch or a device.

The error model is the one of tests/gla_grad_cases.py: every stacked projection argument X of the forward pass, and every result
of a backward transform (the gc of inv_adj, the gv of fwd_adj of lws_amd.rtisi_la_grad), is perturbed by seeded Gaussian noise of
standard deviation 1e-6 max|.| per component.  The distance the fp64 gradients move under it, times 3, is the bar the float32
device pass is held to."""
import functools

import numpy as np

import lws_amd
import gla_grad_cases

SCALES = gla_grad_cases.SCALES                 # of the B = 3 spectrograms: 1, 1e-3, 300
# (fsize, fshift, perfectrec, T)
HOST_SHAPES = gla_grad_cases.HOST_SHAPES + [
    (64, 64, False, 4),                        # hop == N: frames do not overlap
]
GPU_SHAPES = gla_grad_cases.GPU_SHAPES + [
    (64, 64, False, 4),
    (2048, 512, False, 6),                     # 1024 threads, state in LDS
]
# (look-ahead, iterations): an even look-ahead leaves an odd last pair; 5 exceeds T - 1 on several shapes
LA_STEPS = [(0, 1), (0, 3), (1, 3), (2, 2), (3, 1), (3, 3), (3, 5), (5, 2)]
# (fsize, fshift, perfectrec, T): [(look-ahead, iterations, backward state in LDS)] -- both placements of k_rtisi_bwd, asserted on the
# device through lws_rtisi_la_bwd_placement and on the host against a restatement (tests/test_rtisi_bwd_placement.py).  At (4096, 1024)
# and LA = 3 the forward kernel's state is in scratch and the backward's in LDS.  N = 3000 is no power of two and has a third transform
# buffer: LA = 3 asks for 3 * 3000 * 8 + 12 * 7500 = 162000 bytes, 1840 under the cap, with the state at lds + 3 N; LA = 4 for 180000,
# so the state goes to scratch beside three transform buffers.
PLACEMENTS = {
    (2048, 512, False, 6): [(3, 3, True)],
    (4096, 1024, False, 6): [(3, 2, True), (5, 2, False)],
    (3000, 1500, False, 6): [(3, 2, True), (4, 2, False)],
}
FAR, FAR_CAP = gla_grad_cases.FAR, gla_grad_cases.FAR_CAP   # 1e-3 max|gA|; at most 0.5 % of a spectrogram's gA entries
START_NOISE = gla_grad_cases.START_NOISE       # 0.1 rad
SEED = 2900000


def ident(key):
    return "%d-%d-%s-T%d" % key


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, B=3):
    """p, A, c0, gC drawn as gla_grad_cases.case draws them (A = |stft(white noise)| rounded to float32, the start the true phase
    plus START_NOISE rad rounded to complex64, gC complex64) under this file's SEED, and gx, the cotangent of the signal: standard
    normal times max|gC_b|, float32.  RTISI-LA projects like Griffin-Lim, with nothing to anchor a bin whose projection argument is
    near zero: a 1e-6 error there flips its phase and moves the entries of gA it feeds far.  How many is a property of the inputs,
    so the cap (FAR_CAP of the entries of a spectrogram's gA further than FAR max|gA| away) is asserted of the fp64 error model
    alone, in tests/test_rtisi_grad_host.py, for every row of GPU_SHAPES x LA_STEPS.  With this SEED every row stays under it; the
    figures of the scan are in that test's docstring."""
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
    gx = np.stack([np.random.default_rng(SEED + 77 + b).standard_normal(n) * np.abs(gC[b]).max() for b in range(B)]).astype(np.float32)
    for a in (A, c0, gC, gx):
        a.setflags(write=False)
    return p, A, c0, gC, gx


def perturbation(seed, kinds=('X', 'gc', 'gv')):
    """The error model: Z + 1e-6 max|Z| noise (complex for the spectra, real for the signals) on the listed kinds."""
    rng = np.random.default_rng(seed)

    def f(kind, m, it, b, Z):
        if kind not in kinds:
            return Z
        sigma = 1e-6 * np.abs(Z).max()
        if np.iscomplexobj(Z):
            return Z + sigma * (rng.standard_normal(Z.shape) + 1j * rng.standard_normal(Z.shape))
        return Z + sigma * rng.standard_normal(Z.shape)
    return f


def grad(key, LA, n, **kw):
    """lws_amd.rtisi_la_grad on the case of `key` with both cotangents."""
    p, A, c0, gC, gx = case(*key)
    return lws_amd.rtisi_la_grad(c0, p.fsize, p.fshift, p.awin, p.swin, n, A.astype(np.float64), look_ahead=LA, grad_out=gC,
                                 grad_signal=gx, perfectrec=p.perfectrec, **kw)


@functools.lru_cache(maxsize=None)
def host(key, LA, n):
    """(gA, gS) of lws_amd.rtisi_la_grad in fp64 from the rounded inputs, and the same under the full error model."""
    return grad(key, LA, n), grad(key, LA, n, _perturb=perturbation(n + 17 + 100 * LA))


@functools.lru_cache(maxsize=None)
def host_tape(key, LA, n, perturbed=False):
    """The host's own tape, (B, T, n, W, F), W = min(LA, T - 1) + 1, rows beyond `last` zero; perturbed: the tape of the run under
    the error model on the projection arguments, as that run used them (the X of test_gpu_rtisi.py's model, noise included)."""
    p, A, c0, gC, gx = case(*key)
    B, T, F = c0.shape
    tape = np.zeros((B, T, n, min(LA, T - 1) + 1, F), dtype=np.complex128)
    model = perturbation(n + 17 + 100 * LA, kinds=('X',)) if perturbed else None

    def rec(m, it, b, X):
        if model is not None:
            X = model('X', m, it, b, X)
        tape[b, m, it - 1, :X.shape[0]] = X
        return X
    lws_amd.rtisi_la(c0, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=A.astype(np.float64),
                     perfectrec=p.perfectrec, _perturb=rec)
    return tape


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a - b)


def far(a, b):
    """The share of the entries of a further than FAR max|b| from b."""
    return float(np.mean(np.abs(a - b) > FAR * np.abs(b).max()))
