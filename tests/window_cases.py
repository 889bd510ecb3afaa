"""Window pairs that are not mirror-symmetric, not each other's multiple, not always dual and not free of zeros, with the inputs,
error model, host fp64 references and input gate of the tests that give them to the transform family: tests/
test_window_cases_host.py (CPU), tests/test_gpu_windows.py, tests/test_gpu_windows_la.py and tests/test_gpu_windows_grad.py (GPU).  Nothing
here needs torch or a device.

Every window the rest of the suite uses satisfies w[n] == w[N-1-n], and every synthesis window there is the normalised dual of its
analysis window; a kernel that read a window backwards, or took one window for the other, would pass all of it.  pair() gives three
pairs that tell these apart:
  'tilt'    : awin = sqrt(hann) (0.25 + 0.75 u), swin = synthwin(awin, hop, hann^1.5 (1.25 - 0.75 u)), u = (n + 0.5) / N: asymmetric,
              neither window a multiple or a mirror image of the other; a normalised dual.
  'nondual' : the same awin, swin = 0.37 hann^1.5 (1.25 - 0.75 u), NOT passed through synthwin: the round trip of a consistent
              spectrogram is not the identity, and the overlap-added product awin swin (the `den` of online MISI) varies with t.
  'padded'  : 5 zeros in front and N // 4 zeros behind a core built like 'tilt' (hann instead of hann^1.5 in swin), the whole swin
              through synthwin: awin swin is exactly zero on the pads.  Where synthwin refuses (hop = N) there is no such pair.

The inputs follow tests/misi_grad_cases.py: three mixtures at scales 1, 1e-3 and 300, sources at 1 : 0.3 : 3 (: 1), the start the
true phase plus 0.5 rad of Gaussian noise rounded to complex64, magnitudes and mixture rounded to float32, the magnitudes always
passed explicitly.  Griffin-Lim and RTISI-LA run on source 0.  The error model is the suite's: every projection argument perturbed
by seeded Gaussian noise of 1e-6 max|X| per component; three times what the fp64 definition moves under it is the device's bar.
The backward passes of Griffin-Lim and RTISI-LA have inputs of their own, grad_case(): see there.

Which inputs the GPU files run is decided here, on the host: DROPPED lists the combinations on which the fp64 model itself moves a bin
far (at most one in ten per operation), NOT_AN_OVERLAP_CASE the inputs whose overlap entries float32 cannot compute, by the float32
transform model of tests/fft_model.py.  tests/test_window_cases_host.py asserts both lists against the models."""
import functools

import numpy as np

import lws_amd
from lws_amd.lws import _perfectrec_prepad
import fft_model as fm
import gla_grad_cases

KINDS = ("tilt", "nondual", "padded")
SCALES = np.array([1.0, 1e-3, 300.0])          # of the B = 3 mixtures
SOURCES = np.array([1.0, 0.3, 3.0, 1.0])       # relative levels of the sources of a mixture
SEED = 4000000
# (fsize, fshift, perfectrec, T, K): the smallest that cover each path
SHAPES = [
    (64, 16, False, 9, 2),                     # power of two
    (64, 16, True, 12, 3),                     # power of two, perfectrec
    (48, 16, True, 7, 2),                      # odd factor 3
    (48, 16, False, 1, 1),                     # single frame and K = 1
    (256, 96, False, 2, 3),                    # hop does not divide the frame
    (256, 96, True, 5, 2),                     # same, perfectrec
    (100, 30, True, 6, 2),                     # odd factor 25, hop does not divide the frame
]
GLA_STEPS = ((1, 0.0), (3, 0.99), (8, 0.99))   # (iterations, alpha)
MISI_STEPS = (1, 3, 8)
# Iterations of the backward pass.  tests/misi_grad_cases.py also runs 5: gA does not scale with A, so a frame that barely overlaps the
# signal under a tilted or padded window (tiny X, arbitrary phase) moves whole rows of gA, and at 5 iterations the fp64 model itself
# leaves the cap at 6 more of the 21 (kind, shape) inputs -- more than the one in ten the gate may drop.  A condition on the inputs.
GRAD_STEPS = (1, 3)
TAPE_STEPS = (1, 3, 5)                         # what the gate does not condition -- the tape's bits, the teacher-forced pass -- runs at all three
LA_STEPS = ((0, 2), (1, 3), (3, 3), (5, 2))    # (look_ahead, iterations) from a given start: those of the stream tests
# ... and from magnitudes alone ('overlap' / 'mixture').  The overlap start takes an arbitrary phase wherever the transform of a partial
# sum is nearly zero (tests/start_cases.py), and more so under these windows: at (1, 3), (3, 3) and (5, 2) the fp64 model moves bins on
# 5 of the 21 inputs each, at two iterations on 0, 2 and 1.  Every shape is also held teacher-forced, at no iterations, where nothing can
# drift (tests/start_cases.entry_check).
START_STEPS = ((0, 2), (1, 2), (3, 2))
# The backward passes of Griffin-Lim and RTISI-LA (k_gla_bwd_*, k_rtisi_tape, k_rtisi_bwd), on the inputs of grad_case().  RTISI-LA runs at
# LA_STEPS with both cotangents.
GLA_GRAD_STEPS = ((1, 0.0), (3, 0.99), (5, 0.99))   # (iterations, alpha)
GRAD_SEED = 5200000
# the backward state of k_rtisi_bwd in device scratch, with two transform buffers and with three: (shape, look_ahead, iterations)
SCRATCH_RTISI_GRAD = (((4096, 1024, False, 6, 1), 5, 2), ((3000, 1500, False, 6, 1), 4, 2))
# the look-ahead kernels with their state in device scratch: (shape, look_ahead, iterations)
SCRATCH_RTISI = ((2048, 512, False, 9, 1), 7, 2)
SCRATCH_MISI = ((1000, 250, True, 5, 4), 3, 2)
# forward transform longer than the frame: (fsize, fftsize, hop)
ZERO_PADDED = [(48, 96, 16), (100, 128, 40), (32, 34, 12)]
FAR = 1e-3                                     # a bin further than FAR max A from the reference is a far bin

# Combinations the gate of tests/test_window_cases_host.py refuses -- the fp64 error model itself moves a bin beyond FAR max A there,
# so no float32 device could be held to the definition -- with the model's worst far-bin share.  Decided by the fp64 model alone;
# tests/test_window_cases_host.py asserts that every other combination is at zero and that these are not.
# operation -> {(kind, shape, step): share}
DROPPED = {
    "griffin_lim": {},                                                           # 0 of 63
    "misi": {},                                                                  # 0 of 63
    "misi_grad": {                                                               # 4 of 42 (entries of gA beyond FAR; cap FAR_CAP)
        ('tilt', (64, 16, False, 9, 2), 3): 0.00673,
        ('tilt', (100, 30, True, 6, 2), 3): 0.00980,
        ('padded', (64, 16, True, 12, 3), 3): 0.11295,
        ('padded', (256, 96, False, 2, 3), 3): 0.01163,
    },
    "rtisi_la": {                                                                # 5 of 141
        ('tilt', (2048, 512, False, 9, 1), (7, 2, 'given')): 0.00011,
        ('tilt', (64, 16, True, 12, 3), (1, 2, 'overlap')): 0.00253,
        ('tilt', (2048, 512, False, 9, 1), (7, 2, 'overlap')): 0.00152,
        ('nondual', (2048, 512, False, 9, 1), (7, 2, 'overlap')): 0.00249,
        ('padded', (2048, 512, False, 9, 1), (7, 2, 'overlap')): 0.00976,
    },
    "misi_la": {                                                                 # 4 of 153
        ('tilt', (64, 16, True, 12, 3), (1, 3, 'given')): 0.00253,
        ('tilt', (1000, 250, True, 5, 4), (3, 2, 'mixture')): 0.00080,
        ('padded', (64, 16, True, 12, 3), (5, 2, 'given')): 0.00253,
        ('padded', (1000, 250, True, 5, 4), (3, 2, 'mixture')): 0.00040,
    },
    # The two below on the inputs of grad_case(), GRAD_SEED: entries of gA beyond FAR max|gA| on the frames with A != 0, cap FAR_CAP.  Of
    # the seeds 5000000, 5100000 .. 5900000 in that draw order (dropped of 63 and of 90: 7 5, 5 10, 0 4, 2 6, 0 5, 4 5, 2 9, 2 9, 4 7, 2 10)
    # 5000000, 5100000 and 5900000 drop more than one combination in ten of an operation, and this one drops the fewest.
    "gla_grad": {},                                                              # 0 of 63; no entry far on any of them
    "rtisi_grad": {                                                              # 4 of 90; the others at 0.337 % at most
        ('tilt', (64, 16, True, 12, 3), (0, 2)): 0.03535,
        ('tilt', (256, 96, False, 2, 3), (5, 2)): 0.08915,
        ('tilt', (100, 30, True, 6, 2), (3, 3)): 0.00980,
        ('padded', (64, 16, True, 12, 3), (1, 3)): 0.00551,
    },
}
# Inputs on which start='overlap' is not compared with the fp64 run: float32 cannot compute their entry estimates to the 1e-6 max|X| that the error model and
# the teacher-forced check presume of a device.  Under 'padded' with perfectrec the first frame sees only a few samples through the
# tail of its window, enters with zero phase, and the next frame is estimated from the part of that frame's inverse transform that lies
# 1e-3 .. 1e-5 below its peak -- where a float32 transform, accurate to 1e-7 of the peak, has few digits left.  The figure is
# entry_conditioning(): the float32 transform model of tests/fft_model.py against fp64 on the fp64 entry estimates, measured on the
# host; tests/test_window_cases_host.py asserts that these inputs, and no others, exceed OVERLAP_SIGMA.  They stay on the device
# (tests/test_gpu_windows_la.py) for everything that does not hang on that phase -- finite results, the magnitudes, the signal against
# istft of the result, every chunking of a stream against the whole push, the placement -- and their entry estimates are held
# teacher-forced with the model's figure in the place of the 1e-6.  These 4 inputs x 3 steps are 12 of the 153 combinations of rtisi_la;
# with the 5 the fp64 gate drops, 17 (11 %) have no whole-run comparison with the fp64 definition.
OVERLAP_SIGMA = 1e-6
NOT_AN_OVERLAP_CASE = {
    ('padded', (64, 16, True, 12, 3)): 1.23e-05,
    ('padded', (48, 16, True, 7, 2)): 8.37e-02,
    ('padded', (256, 96, True, 5, 2)): 1.68e-06,
    ('padded', (100, 30, True, 6, 2)): 3.23e-05,
}
FAR_CAP = 5e-3                                 # of tests/misi_grad_cases.py: the share of the entries of gA that may lie beyond FAR


def ident(key):
    return "%d-%d-%s-T%d-K%d" % tuple(key[:5])


def _core(n, swin_power):
    v = (np.arange(n) + 0.5) / n
    h = lws_amd.hann(n)
    return np.sqrt(h) * (0.25 + 0.75 * v), h ** swin_power * (1.25 - 0.75 * v)


@functools.lru_cache(maxsize=None)
def pair(N, hop, kind):
    """(awin, swin) in fp64, read-only; ValueError where synthwin refuses the pair."""
    if kind == "default":
        p = lws_amd.lws(N, hop)
        awin, swin = np.array(p.awin, dtype=np.float64), np.array(p.swin, dtype=np.float64)
    elif kind == "tilt":
        awin, s = _core(N, 1.5)
        swin = lws_amd.synthwin(awin, hop, swin=s)
    elif kind == "nondual":
        awin, s = _core(N, 1.5)
        swin = 0.37 * s
    elif kind == "padded":
        front, behind = 5, N // 4
        a, s = _core(N - front - behind, 1.0)
        awin = np.concatenate([np.zeros(front), a, np.zeros(behind)])
        swin = lws_amd.synthwin(awin, hop, swin=np.concatenate([np.zeros(front), s, np.zeros(behind)]))
    else:
        raise KeyError(kind)
    for w in (awin, swin):
        w.setflags(write=False)
    return awin, swin


def has_pair(N, hop, kind):
    try:
        pair(N, hop, kind)
    except ValueError:
        return False
    return True


def mirrored(awin, swin):
    return awin[::-1].copy(), swin[::-1].copy()


def exchanged(awin, swin):
    """The windows in each other's role, each rescaled to the sum of the window it replaces."""
    return swin * (awin.sum() / swin.sum()), awin * (swin.sum() / awin.sum())


def overlap_added(awin, swin, hop, T):
    """sum over the T frames of awin swin, on the uncut timeline, and how many frames cover each sample."""
    N = len(awin)
    den, cover = np.zeros(hop * (T - 1) + N), np.zeros(hop * (T - 1) + N, dtype=int)
    for j in range(T):
        den[hop * j: hop * j + N] += awin * swin
        cover[hop * j: hop * j + N] += 1
    return den, cover


def length(fsize, fshift, perfectrec, T):
    return lws_amd.istft(np.zeros((T, fsize // 2 + 1), complex), fshift, np.ones(fsize), perfectrec=perfectrec).shape[0]


@functools.lru_cache(maxsize=None)
def case(fsize, fshift, perfectrec, T, K, kind, B=3):
    """awin, swin, the magnitudes A = |stft(source)| (B, K, T, F) rounded to float32, the start c_0 = A exp(j (true phase + 0.5 g)) rounded
    to complex64, the mixture y rounded to float32 and the cotangents gC (complex64) and gs (float32): what the device is given and
    what the host runs start from.  The draws are those of tests/misi_grad_cases.case, in its order."""
    rng = np.random.default_rng(SEED + 1000 * fsize + 10 * fshift + perfectrec)
    awin, swin = pair(fsize, fshift, kind)
    n = length(fsize, fshift, perfectrec, T)
    src = rng.standard_normal((B, K, n)) * SOURCES[None, :K, None] * SCALES[:B, None, None]
    X = np.stack([[lws_amd.stft(x, fsize, fshift, awin, perfectrec=perfectrec) for x in s] for s in src])
    assert X.shape == (B, K, T, fsize // 2 + 1)
    A = np.abs(X).astype(np.float32)
    c0 = (A * np.exp(1j * (np.angle(X) + 0.5 * rng.standard_normal(X.shape)))).astype(np.complex64)
    y = src.sum(axis=1).astype(np.float32)
    gC = ((rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)) / np.sqrt(fsize)).astype(np.complex64)
    gs = rng.standard_normal(src.shape).astype(np.float32)
    for a in (A, c0, y, gC, gs):
        a.setflags(write=False)
    return awin, swin, A, c0, y, gC, gs


@functools.lru_cache(maxsize=None)
def grad_case(fsize, fshift, perfectrec, T, kind, B=3):
    """The inputs of the backward passes of Griffin-Lim and RTISI-LA under a pair: awin, swin, A = |stft(white noise)| (B, T, F) at SCALES
    rounded to float32, the start c_0 the true phase plus gla_grad_cases.START_NOISE (0.1 rad) rounded to complex64, and the cotangents gC
    (complex64) and gx (float32, standard normal times max|gC_b|, the scale tests/rtisi_grad_cases.case gives it), drawn in this order
    from one generator under GRAD_SEED.  Not
    case() above: from its 0.5 rad an iteration that no mixture anchors moves most of gA under the error model alone (the docstring of
    tests/gla_grad_cases.case), and a draw added to case() would move every input the other GPU files are gated on."""
    rng = np.random.default_rng(GRAD_SEED + 1000 * fsize + 10 * fshift + perfectrec)
    awin, swin = pair(fsize, fshift, kind)
    n = length(fsize, fshift, perfectrec, T)
    src = rng.standard_normal((B, n)) * SCALES[:B, None]
    X = np.stack([lws_amd.stft(x, fsize, fshift, awin, perfectrec=perfectrec) for x in src])
    assert X.shape == (B, T, fsize // 2 + 1)
    A = np.abs(X).astype(np.float32)
    c0 = (A * np.exp(1j * (np.angle(X) + gla_grad_cases.START_NOISE * rng.standard_normal(X.shape)))).astype(np.complex64)
    gC = ((rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)) / np.sqrt(fsize)).astype(np.complex64)
    gx = (rng.standard_normal((B, n)) * np.abs(gC).max(axis=(1, 2))[:, None]).astype(np.float32)
    for a in (A, c0, gC, gx):
        a.setflags(write=False)
    return awin, swin, A, c0, gC, gx


def open_mixture(key, y):
    """The mixture an open end reads: y and, with perfectrec, the fsize - fshift zeros stft pads behind the signal."""
    if not key[2]:
        return y
    out = np.zeros(y.shape[:-1] + (y.shape[-1] + key[0] - key[1],), y.dtype)
    out[..., :y.shape[-1]] = y
    return out


def need(key, M):
    """Mixture samples under the first M frames of an open end."""
    return 0 if M <= 0 else key[1] * (M - 1) + key[0] - (_perfectrec_prepad(key[0], key[1]) if key[2] else 0)


def _seen(X):
    """0 for the rows of X that are exactly zero, 1 for the others.  A frame that lies under the zeros of a 'padded' window and the
    samples perfectrec reads as zero has A == 0 and, in the definition, X == 0 at every step: its projection is 0 whatever the phase,
    and its row of gA is the |X| == 0 convention, not a derivative.  The model leaves such rows alone, and the GPU test compares gA on
    the other frames (tests/test_gpu_windows.py says what the device does there).  Under the symmetric default no window has zeros and
    no such row exists: there this is the model of the existing tests unchanged."""
    return (np.asarray(X) != 0).any(axis=-1, keepdims=True)


def perturbation(seed, per_source=False):
    """X + 1e-6 max|X| (g + j g'), X the last argument of the hook of any of the host definitions; per_source: the maximum taken per
    source of a (K, frames, F) stack, as tests/misi_la_cases.py takes it."""
    rng = np.random.default_rng(seed)

    def f(*args):
        X = args[-1]
        top = np.abs(X).max(axis=(1, 2), keepdims=True) if per_source else np.abs(X).max()
        return X + 1e-6 * top * _seen(X) * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return f


def grad_perturbation(seed, kinds=("X", "gc", "gv")):
    """The error model of tests/misi_grad_cases.py, and with the hooks' other signatures -- (kind, i, b, Z) and (kind, m, it, b, Z) -- of
    tests/gla_grad_cases.py and tests/rtisi_grad_cases.py: the array is the last argument of all three."""
    rng = np.random.default_rng(seed)

    def f(kind, *where):
        Z = where[-1]
        if kind not in kinds:
            return Z
        sigma = 1e-6 * np.abs(Z).max() * _seen(Z)
        if np.iscomplexobj(Z):
            return Z + sigma * (rng.standard_normal(Z.shape) + 1j * rng.standard_normal(Z.shape))
        return Z + sigma * rng.standard_normal(Z.shape)
    return f


# ---- host fp64 references: (reference, the same under the error model) ---------------------------------------------------------
def _frozen(res):
    for a in res:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def host_gla(key, kind, n, alpha):
    """((out, dB), (out, dB)) of griffin_lim on source 0."""
    awin, swin, A, c0, y, gC, gs = case(*key, kind)
    run = functools.partial(lws_amd.griffin_lim, c0[:, 0], key[0], key[1], awin, swin, n, alpha=alpha, magnitudes=A[:, 0].astype(np.float64),
                            perfectrec=key[2], return_trace=True)
    return _frozen(run()), _frozen(run(_perturb=perturbation(n + 17)))


@functools.lru_cache(maxsize=None)
def host_misi(key, kind, n):
    """((out, dB, signals), (out, dB, signals)) of misi."""
    awin, swin, A, c0, y, gC, gs = case(*key, kind)
    run = functools.partial(lws_amd.misi, c0, y, key[0], key[1], awin, swin, n, magnitudes=A.astype(np.float64), perfectrec=key[2],
                            return_trace=True, return_signals=True)
    return _frozen(run()), _frozen(run(_perturb=perturbation(n + 17)))


@functools.lru_cache(maxsize=None)
def host_grad(key, kind, n):
    """((gA, gS, gy), (gA, gS, gy)) of misi_grad."""
    awin, swin, A, c0, y, gC, gs = case(*key, kind)
    run = functools.partial(lws_amd.misi_grad, c0, y, key[0], key[1], awin, swin, n, A.astype(np.float64), grad_out=gC, grad_signals=gs,
                            perfectrec=key[2])
    return _frozen(run()), _frozen(run(_perturb=grad_perturbation(n + 17)))


def gla_grad(key, kind, n, alpha, **kw):
    """lws_amd.griffin_lim_grad on grad_case() of `key` under `kind`; windows=(awin, swin) puts another pair in their place."""
    awin, swin, A, c0, gC, gx = grad_case(*key[:4], kind)
    awin, swin = kw.pop("windows", (awin, swin))
    return lws_amd.griffin_lim_grad(c0, key[0], key[1], awin, swin, n, A.astype(np.float64), alpha=alpha, grad_out=gC, perfectrec=key[2], **kw)


def rtisi_grad(key, kind, LA, n, **kw):
    """lws_amd.rtisi_la_grad on grad_case() of `key` under `kind`, both cotangents; windows=(awin, swin) as above."""
    awin, swin, A, c0, gC, gx = grad_case(*key[:4], kind)
    awin, swin = kw.pop("windows", (awin, swin))
    return lws_amd.rtisi_la_grad(c0, key[0], key[1], awin, swin, n, A.astype(np.float64), look_ahead=LA, grad_out=gC, grad_signal=gx,
                                 perfectrec=key[2], **kw)


@functools.lru_cache(maxsize=None)
def host_gla_grad(key, kind, n, alpha):
    """((gA, gS), (gA, gS)) of griffin_lim_grad."""
    return _frozen(gla_grad(key, kind, n, alpha)), _frozen(gla_grad(key, kind, n, alpha, _perturb=grad_perturbation(n + 17)))


@functools.lru_cache(maxsize=None)
def host_rtisi_grad(key, kind, LA, n):
    """((gA, gS), (gA, gS)) of rtisi_la_grad."""
    return _frozen(rtisi_grad(key, kind, LA, n)), _frozen(rtisi_grad(key, kind, LA, n, _perturb=grad_perturbation(n + 17 + 100 * LA)))


@functools.lru_cache(maxsize=None)
def host_gla_tape(key, kind, n, alpha, perturbed=False):
    """The projection arguments of the host's griffin_lim on grad_case(), (n, B, T, F); perturbed: of the run under the error model on
    them, as that run used them."""
    awin, swin, A, c0, gC, gx = grad_case(*key[:4], kind)
    tape = np.zeros((n,) + c0.shape, dtype=np.complex128)
    model = grad_perturbation(n + 17, kinds=("X",)) if perturbed else None

    def rec(i, b, X):
        if model is not None:
            X = model("X", i, b, X)
        tape[i - 1, b] = X
        return X
    lws_amd.griffin_lim(c0, key[0], key[1], awin, swin, n, alpha=alpha, magnitudes=A.astype(np.float64), perfectrec=key[2], _perturb=rec)
    tape.setflags(write=False)
    return tape


@functools.lru_cache(maxsize=None)
def host_rtisi_tape(key, kind, LA, n, perturbed=False):
    """The same of rtisi_la, (B, T, n, W, F) as tests/rtisi_grad_cases.host_tape lays it out."""
    awin, swin, A, c0, gC, gx = grad_case(*key[:4], kind)
    B, T, F = c0.shape
    tape = np.zeros((B, T, n, min(LA, T - 1) + 1, F), dtype=np.complex128)
    model = grad_perturbation(n + 17 + 100 * LA, kinds=("X",)) if perturbed else None

    def rec(m, it, b, X):
        if model is not None:
            X = model("X", m, it, b, X)
        tape[b, m, it - 1, :X.shape[0]] = X
        return X
    lws_amd.rtisi_la(c0, key[0], key[1], awin, swin, n, look_ahead=LA, magnitudes=A.astype(np.float64), perfectrec=key[2], _perturb=rec)
    tape.setflags(write=False)
    return tape


def seen_far(per, ref, A):
    """The largest share, over the spectrograms of a stack, of the entries of gA the model moves further than FAR max|gA|, on the frames
    with A != 0 (_seen())."""
    worst = 0.0
    for p, r, a in zip(per, ref, A):
        seen = a.any(axis=-1)
        worst = max(worst, float(np.mean(np.abs(p[seen] - r[seen]) > FAR * np.abs(r[seen]).max())))
    return worst


def rtisi_input(key, kind, start):
    """(rows, magnitudes) of source 0 as rtisi_la takes them under `start`."""
    A, c0 = case(*key, kind)[2:4]
    A0 = A[:, 0].astype(np.float64)
    return (c0[:, 0], A0) if start == "given" else (A0, None)


@functools.lru_cache(maxsize=None)
def host_rtisi(key, kind, LA, n, start="given", open_end=False):
    """((out, signal), (out, signal)) of rtisi_la on source 0."""
    awin, swin = pair(key[0], key[1], kind)
    rows, mags = rtisi_input(key, kind, start)
    run = functools.partial(lws_amd.rtisi_la, rows, key[0], key[1], awin, swin, n, look_ahead=LA, magnitudes=mags, perfectrec=key[2],
                            return_signal=True, start=start, open_end=open_end)
    return _frozen(run()), _frozen(run(_perturb=perturbation(n + 17)))


def misi_la_input(key, kind, start, open_end=False):
    """(rows, magnitudes, mixture) as misi_la takes them under `start`."""
    A, c0, y = case(*key, kind)[2:5]
    A = A.astype(np.float64)
    y = open_mixture(key, y) if open_end else y
    return (c0, A, y) if start == "given" else (A, None, y)


@functools.lru_cache(maxsize=None)
def host_misi_la(key, kind, LA, n, start="given", open_end=False):
    """((out, signals), (out, signals)) of misi_la."""
    awin, swin = pair(key[0], key[1], kind)
    rows, mags, y = misi_la_input(key, kind, start, open_end)
    run = functools.partial(lws_amd.misi_la, rows, y, key[0], key[1], awin, swin, n, look_ahead=LA, magnitudes=mags, perfectrec=key[2],
                            return_signals=True, start=start, open_end=open_end)
    return _frozen(run()), _frozen(run(_perturb=perturbation(n + 17, per_source=True)))


# ---- what the GPU files run, and the gate on it ----------------------------------------------------------------------------------
def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a - b)


def far_share(per, ref, A):
    """The largest share, over the spectrograms of a stack, of bins the model moves further than FAR max A."""
    per, ref, A = (np.asarray(a).reshape((-1,) + np.shape(a)[-2:]) for a in (per, ref, A))
    return max(float(np.mean(np.abs(p - r) > FAR * a.max())) for p, r, a in zip(per, ref, A))


def shapes_of(kind, K_min=1):
    return [s for s in SHAPES if has_pair(s[0], s[1], kind) and s[4] >= K_min]


def entry_conditioning(key, kind, open_end=False):
    """The largest error, relative to max|X|, that the float32 transform model makes in the argument X of an entry projection of
    rtisi_la(..., start='overlap') when every frame before it is transformed back and overlap-added in float32 too: fp64 entry rows in,
    teacher-forced, so that nothing but the two transforms of one step is measured."""
    N, hop, perfectrec, T = key[:4]
    awin, swin = pair(N, hop, kind)
    A0 = rtisi_input(key, kind, "overlap")[0]
    E = lws_amd.rtisi_la(A0, N, hop, awin, swin, 0, look_ahead=0, perfectrec=perfectrec, start="overlap", open_end=open_end)
    total = hop * (T - 1) + N
    keep = np.ones(total)
    if perfectrec:
        keep[:_perfectrec_prepad(N, hop)] = 0.0
        if not open_end:
            keep[total - (N - hop):] = 0.0
    a32, s32, k32 = awin.astype(np.float32), swin.astype(np.float32), keep.astype(np.float32)
    worst = 0.0
    for b in range(E.shape[0]):
        y64, y32 = np.zeros(total), np.zeros(total, np.float32)
        for j in range(T):
            X64 = np.fft.rfft(awin * (keep * y64)[hop * j: hop * j + N])
            X32 = fm.fft_model((a32 * (k32 * y32)[hop * j: hop * j + N])[None], -1)[0][:N // 2 + 1]
            if np.abs(X64).max() > 0:
                worst = max(worst, float(np.abs(X32 - X64).max() / np.abs(X64).max()))
            y64[hop * j: hop * j + N] += swin * np.fft.irfft(E[b, j], N)
            full = np.concatenate([E[b, j], np.conj(E[b, j, -2:0:-1])]).astype(np.complex64)
            y32[hop * j: hop * j + N] += (np.real(fm.fft_model(full[None], +1)[0]).astype(np.float32) * np.float32(1.0 / N)) * s32
    return worst


def has_overlap_case(kind, key):
    return (kind, tuple(key)) not in NOT_AN_OVERLAP_CASE


def overlap_sigma(kind, key):
    """The error of an entry projection's argument that the teacher-forced check allows a device: 1e-6 max|X|, or what the float32
    transform model itself makes of this input where that is more (measured on the host, for the closed and the open end)."""
    if has_overlap_case(kind, key):
        return OVERLAP_SIGMA
    return max(OVERLAP_SIGMA, max(entry_conditioning(key, kind, open_end) for open_end in (False, True)))


def overlap_property_runs():
    """(kind, shape, look_ahead, iterations) of start='overlap' on the inputs of NOT_AN_OVERLAP_CASE: run for their properties alone."""
    return [(kind, key, LA, n) for kind, key in sorted(NOT_AN_OVERLAP_CASE) for LA, n in START_STEPS]


def la_runs(op, start="given"):
    """(shape, look_ahead, iterations) of the look-ahead calls: every shape at its steps, and the scratch placement."""
    runs = [(s, LA, n) for s in SHAPES for LA, n in (LA_STEPS if start == "given" else START_STEPS)]
    return runs + [SCRATCH_RTISI if op == "rtisi_la" else SCRATCH_MISI]


def combinations(op):
    """Every (kind, shape, step) of an operation before the gate."""
    out = []
    for kind in KINDS:
        for s in shapes_of(kind):
            if op == "griffin_lim":
                out += [(kind, s, step) for step in GLA_STEPS]
            elif op == "misi":
                out += [(kind, s, n) for n in MISI_STEPS]
            elif op == "misi_grad":
                out += [(kind, s, n) for n in GRAD_STEPS]
            elif op == "gla_grad":
                out += [(kind, s, step) for step in GLA_GRAD_STEPS]
            elif op == "rtisi_grad":
                out += [(kind, s, step) for step in LA_STEPS]
        if op == "rtisi_grad":
            out += [(kind, s, (LA, n)) for s, LA, n in SCRATCH_RTISI_GRAD if has_pair(s[0], s[1], kind)]
        if op in ("rtisi_la", "misi_la"):
            out += [(kind, s, (LA, n, start)) for start in ("given", "overlap" if op == "rtisi_la" else "mixture")
                    for s, LA, n in la_runs(op, start) if has_pair(s[0], s[1], kind) and (start != "overlap" or has_overlap_case(kind, s))]
    return out


def runs(op, kind=None):
    """The combinations the GPU files run: those the gate lets through."""
    return [c for c in combinations(op) if c not in DROPPED[op] and (kind is None or c[0] == kind)]


def model_share(op, combo):
    """The gate's figure of one combination: the far-bin share of the fp64 error model (for misi_grad: of the entries of gA)."""
    kind, key, step = combo
    if op == "gla_grad":
        ref, per = host_gla_grad(key, kind, *step)
        return seen_far(per[0], ref[0], grad_case(*key[:4], kind)[2])
    if op == "rtisi_grad":
        ref, per = host_rtisi_grad(key, kind, *step)
        return seen_far(per[0], ref[0], grad_case(*key[:4], kind)[2])
    A = case(*key, kind)[2]
    if op == "griffin_lim":
        (ref, _), (per, _) = host_gla(key, kind, *step)
        return far_share(per, ref, A[:, 0])
    if op == "misi":
        ref, per = host_misi(key, kind, step)
        return far_share(per[0], ref[0], A)
    if op == "misi_grad":
        ref, per = host_grad(key, kind, step)
        seen = A.any(axis=-1)                   # gA on a frame with A == 0 and X == 0 is a convention: see _seen()
        return max(float(np.mean(np.abs(per[0][b, k][seen[b, k]] - ref[0][b, k][seen[b, k]]) > FAR * np.abs(ref[0][b, k][seen[b, k]]).max()))
                   for b in range(A.shape[0]) for k in range(A.shape[1]))
    LA, n, start = step
    worst = 0.0
    for open_end in (False, True):          # the one-shot call and the stream
        if op == "rtisi_la":
            ref, per = host_rtisi(key, kind, LA, n, start, open_end)
            worst = max(worst, far_share(per[0], ref[0], A[:, 0]))
        else:
            ref, per = host_misi_la(key, kind, LA, n, start, open_end)
            worst = max(worst, far_share(per[0], ref[0], A))
    return worst


# ---- the record of a GPU run --------------------------------------------------------------------------------------------------------
def note(margins, op, kind, key, **figures):
    """Keep the largest of each figure per operation, kind and shape: margins[op]["kind,fsize,fshift,perfectrec"][name]."""
    row = margins.setdefault(op, {}).setdefault("%s,%d,%d,%s" % ((kind,) + tuple(key[:3])), {"cases": 0})
    row["cases"] += 1
    for name, v in figures.items():
        row[name] = max(row.get(name, 0.0), float(v))


def write_margins(margins):
    """Merge the operations of `margins` into $LWS_MARGINS_DIR/window_margins.json when that variable names a directory
    (profiles/window_margins.json is a copy of what an MI355X gave); returns the worst figure-over-bar per operation."""
    import json
    import os
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        path = os.path.join(out, "window_margins.json")
        report = {}
        if os.path.exists(path):
            with open(path) as f:
                report = json.load(f)
        report.update(margins)
        with open(path, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")
    return {op: max([v for row in rows.values() for name, v in row.items() if name.endswith("_over_bar")] or [0.0])
            for op, rows in margins.items()}
