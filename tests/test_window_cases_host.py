"""CPU: the window pairs of tests/window_cases.py -- that they are what they claim to be; the host fp64 definitions of the transform
family under them against independent restatements (those definitions are what the device is held to, and the rest of the suite only
ever gives them the mirror-symmetric default); how far each operation moves when a window is read backwards or the two windows change
roles, which is the reason the pairs exist; and the gate on the inputs of tests/test_gpu_windows.py, tests/test_gpu_windows_la.py and
tests/test_gpu_windows_grad.py.
Every figure is printed before it is asserted (pytest -s)."""
import functools
import types

import numpy as np
import pytest

import lws_amd
from lws_amd import _capi
import window_cases as wc

PAIRS = [(kind, s) for kind in wc.KINDS for s in wc.SHAPES if wc.has_pair(s[0], s[1], kind)]
PAIR_IDS = ["%s-%s" % (kind, wc.ident(s)) for kind, s in PAIRS]
MULTI = [(kind, s) for kind, s in PAIRS if s[3] > 1]


def plan(key, kind):
    """What the restatements of the other host files read of an lws object."""
    awin, swin = wc.pair(key[0], key[1], kind)
    return types.SimpleNamespace(fsize=key[0], fshift=key[1], perfectrec=key[2], awin=awin.copy(), swin=swin.copy())   # (writable: torch.from_numpy)


def one(key, kind):
    """Mixture 0 of the case in fp64: A, c0, y, gC, gs."""
    return tuple(np.asarray(a[0], dtype=np.complex128 if np.iscomplexobj(a) else np.float64) for a in wc.case(*key, kind)[2:])


# ---- the windows -----------------------------------------------------------------------------------------------------------------
def not_a_multiple(a, b):
    """The angle between a and b as vectors: sin, 0 for multiples."""
    cos = abs(np.dot(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return np.sqrt(max(0.0, 1.0 - cos * cos))


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("N,hop", sorted({s[:2] for s in wc.SHAPES} | {wc.SCRATCH_RTISI[0][:2], wc.SCRATCH_MISI[0][:2]}))
def test_window_properties(N, hop, kind):
    awin, swin = wc.pair(N, hop, kind)
    assert awin.dtype == swin.dtype == np.float64 and awin.shape == swin.shape == (N,)
    for name, w in (("awin", awin), ("swin", swin)):
        asym = np.abs(w - w[::-1]).max() / np.abs(w).max()
        print("%s (%d, %d) %s: max|w - w[::-1]| = %.3f max|w|" % (kind, N, hop, name, asym))
        assert asym >= 0.1
    s1, s2 = not_a_multiple(swin, awin), not_a_multiple(swin, awin[::-1])
    print("%s (%d, %d): sin of the angle between swin and awin %.3f, and awin mirrored %.3f" % (kind, N, hop, s1, s2))
    assert s1 >= 0.05 and s2 >= 0.05
    T = 3 * (-(-N // hop))
    den, cover = wc.overlap_added(awin, swin, hop, T)
    inner = slice(N, len(den) - N)                          # where every frame that could cover a sample does
    dev = np.abs(den[inner] - 1.0).max()
    print("%s (%d, %d): overlap-added awin swin deviates from 1 by %.2e in the interior" % (kind, N, hop, dev))
    if kind == "nondual":
        assert dev > 0.1
    else:
        assert dev <= 1e-12
    if kind == "padded":
        w = awin * swin
        assert (w[:5] == 0).all() and (w[N - N // 4:] == 0).all() and (w[5:N - N // 4] > 0).all()
        assert (awin[:5] == 0).all() and (swin[:5] == 0).all() and (awin[N - N // 4:] == 0).all() and (swin[N - N // 4:] == 0).all()
        one_frame, _ = wc.overlap_added(awin, swin, hop, 1)
        assert (one_frame == 0).sum() == 5 + N // 4         # den == 0 under a covering frame: the 1.0f branch of the mixture weighting


def test_padded_has_no_pair_where_synthwin_refuses():
    assert not wc.has_pair(64, 64, "padded") and wc.has_pair(64, 64, "tilt") and wc.has_pair(64, 64, "nondual")
    assert all(wc.has_pair(s[0], s[1], kind) for kind in wc.KINDS for s in wc.SHAPES + [wc.SCRATCH_RTISI[0], wc.SCRATCH_MISI[0]])
    assert all(wc.has_pair(N, hop, kind) for kind in wc.KINDS for N, _, hop in wc.ZERO_PADDED)


def test_default_pair_is_mirror_symmetric_to_rounding():
    """What the old suite could not see: under its windows a mirrored index reads the same numbers -- to the last bits of fp64 (the
    cosine at (2 n + 1) / 2 N and at its mirror image are rounded apart, 1.3e-15 at most here), eight orders below float32."""
    for N, hop in sorted({s[:2] for s in wc.SHAPES}):
        awin, swin = wc.pair(N, hop, "default")
        off = max(np.abs(w - w[::-1]).max() / np.abs(w).max() for w in (awin, swin))
        print("default (%d, %d): max|w - w[::-1]| = %.2e max|w|" % (N, hop, off))
        assert off <= 2.0 ** -48


def test_scratch_placements():
    for (key, LA, n), K in ((wc.SCRATCH_RTISI, 0), (wc.SCRATCH_MISI, wc.SCRATCH_MISI[0][4])):
        got = _capi.rtisi_la_placement(key[0], key[1], min(LA, key[3] - 1), K)
        print("placement %s LA=%d K=%d: state in %s, %d threads, %d bytes" % (wc.ident(key), LA, K, "LDS" if got[0] else "scratch", got[1], got[2]))
        assert got[0] is False
    assert all(_capi.rtisi_la_placement(s[0], s[1], min(LA, s[3] - 1), K)[0] for s in wc.SHAPES for LA, _ in wc.LA_STEPS for K in (0, s[4]))


# ---- stft / istft against an explicit DFT matrix and a loop overlap-add -----------------------------------------------------------
def stft_restated(x, N, nfft, hop, awin, perfectrec):
    x = np.asarray(x, dtype=np.float64)
    if perfectrec:
        lead = N - hop if N % hop == 0 else N - N % hop
        x = np.concatenate([np.zeros(lead), x])
        x = np.concatenate([x, np.zeros((-len(x) + lead) % hop)])          # the signal itself padded to whole hops
        M = len(x) // hop
    else:
        while (len(x) - N) % hop:
            x = np.append(x, 0.0)
        M = (len(x) - N) // hop + 1
    x = np.concatenate([x, np.zeros(max(0, hop * (M - 1) + N - len(x)))])
    W = np.exp(-2j * np.pi * np.outer(np.arange(nfft // 2 + 1), np.arange(N)) / nfft)       # (bins, samples of the frame)
    return np.stack([W @ (awin * x[hop * m: hop * m + N]) for m in range(M)])


def istft_restated(S, N, hop, swin, perfectrec):
    M, F = S.shape
    k, n = np.arange(F), np.arange(N)
    weight = np.where((k == 0) | (k == N // 2), 1.0, 2.0)                                 # the conjugate half, folded in
    E = np.exp(2j * np.pi * np.outer(n, k) / N)
    out = np.zeros(hop * (M - 1) + N)
    for m in range(M):
        S_m = S[m].copy()
        S_m[[0, -1]] = S_m[[0, -1]].real                                                  # irfft reads no imaginary part there
        frame = np.real(E @ (weight * S_m)) / N
        for i in range(N):
            out[hop * m + i] += swin[i] * frame[i]
    if perfectrec:
        lead = N - hop if N % hop == 0 else N - N % hop
        out = out[lead: len(out) - (N - hop)]
    return out


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_stft_and_istft_match_explicit_restatements(kind, key):
    N, hop, perfectrec, T, K = key
    awin, swin = wc.pair(N, hop, kind)
    rng = np.random.default_rng(N + hop)
    for n in sorted({wc.length(N, hop, perfectrec, T), N + 1, 2 * N + hop}):
        x = rng.standard_normal(n)
        got, want = lws_amd.stft(x, N, hop, awin, perfectrec=perfectrec), stft_restated(x, N, N, hop, awin, perfectrec)
        assert got.shape == want.shape
        err = np.abs(got - want).max() / np.abs(want).max()
        S = got * np.exp(1j * rng.standard_normal(got.shape))                             # not a consistent spectrogram
        back, want_back = lws_amd.istft(S, hop, swin, perfectrec=perfectrec), istft_restated(S, N, hop, swin, perfectrec)
        assert back.shape == want_back.shape
        ierr = np.abs(back - want_back).max() / max(np.abs(want_back).max(), 1e-300) if back.size else 0.0
        print("%s %s len %d: stft off %.2e, istft off %.2e of the largest value" % (kind, wc.ident(key), n, err, ierr))
        assert err <= 1e-12 and ierr <= 1e-12


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("N,nfft,hop", wc.ZERO_PADDED)
def test_zero_padded_forward_transform_matches_its_restatement(N, nfft, hop, kind):
    awin, _ = wc.pair(N, hop, kind)
    rng = np.random.default_rng(N + nfft)
    for perfectrec in (True, False):
        x = rng.standard_normal(2 * N + hop + 1)
        got, want = lws_amd.stft(x, N, hop, awin, fftsize=nfft, perfectrec=perfectrec), stft_restated(x, N, nfft, hop, awin, perfectrec)
        assert got.shape == want.shape and got.shape[1] == nfft // 2 + 1
        err = np.abs(got - want).max() / np.abs(want).max()
        print("%s (%d/%d, %d, %s): stft off %.2e" % (kind, N, nfft, hop, perfectrec, err))
        assert err <= 1e-12


# ---- misi and misi_grad against torch fp64 and its autograd, and against central differences ------------------------------------
STEPS = (0, 1, 3)


@functools.lru_cache(maxsize=None)
def autograd(key, kind, n):
    torch = pytest.importorskip("torch")
    from test_misi_grad_host import torch_misi
    A, c0, y, gC, gs = one(key, kind)
    tA, tS, ty = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (A, c0, y))
    C, s = torch_misi(torch, plan(key, kind), tA, tS, ty, n)
    ((torch.from_numpy(gC).conj() * C).real.sum() + (torch.from_numpy(gs) * s).sum()).backward()
    grads = tuple(np.zeros(a.shape, a.dtype) if t.grad is None else t.grad.numpy() for a, t in ((A, tA), (c0, tS), (y, ty)))
    return C.detach().numpy(), s.detach().numpy(), grads


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_misi_and_its_gradient_match_torch(kind, key):
    A, c0, y, gC, gs = one(key, kind)
    awin, swin = wc.pair(key[0], key[1], kind)
    for n in STEPS:
        C, s, want = autograd(key, kind, n)
        ref, ref_s = lws_amd.misi(c0, y, key[0], key[1], awin, swin, n, magnitudes=A, perfectrec=key[2], return_signals=True)
        dC, ds = np.abs(C - ref).max() / np.abs(A).max(), np.abs(s - ref_s).max() / np.abs(y).max()
        got = lws_amd.misi_grad(c0, y, key[0], key[1], awin, swin, n, A, grad_out=gC, grad_signals=gs, perfectrec=key[2])
        d = [wc.rel(g, w) for g, w in zip(got, want)]
        print("%s %s n=%d: misi off the torch restatement by %.2e max A, %.2e max|y|; misi_grad rel-L2 to autograd gA %.2e gS %.2e gy %.2e"
              % ((kind, wc.ident(key), n, dC, ds) + tuple(d)))
        assert dC <= 1e-12 and ds <= 1e-12
        assert max(d) <= 1e-10


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_misi_grad_matches_central_differences_of_misi(kind, key):
    A, c0, y, gC, gs = one(key, kind)
    awin, swin = wc.pair(key[0], key[1], kind)
    rng = np.random.default_rng(5)
    dA = rng.standard_normal(A.shape) * np.abs(A).mean()
    dS = (rng.standard_normal(c0.shape) + 1j * rng.standard_normal(c0.shape)) * np.abs(A).mean()
    h = 1e-6

    def loss(A_, S_, n):
        C, s = lws_amd.misi(S_, y, key[0], key[1], awin, swin, n, magnitudes=A_, perfectrec=key[2], return_signals=True)
        return np.sum(np.real(np.conj(gC) * C)) + np.sum(gs * s)

    for n in (1, 3):
        gA, gS, gy = lws_amd.misi_grad(c0, y, key[0], key[1], awin, swin, n, A, grad_out=gC, grad_signals=gs, perfectrec=key[2])
        rows = (("A", (loss(A + h * dA, c0, n) - loss(A - h * dA, c0, n)) / (2 * h), np.sum(gA * dA)),
                ("S", (loss(A, c0 + h * dS, n) - loss(A, c0 - h * dS, n)) / (2 * h), np.sum(np.real(np.conj(gS) * dS))))
        for name, fd, an in rows:
            print("%s %s n=%d along d%s: central difference %.10e, <g, d> %.10e" % (kind, wc.ident(key), n, name, fd, an))
            assert abs(fd - an) <= 1e-5 * abs(an)


# ---- griffin_lim_grad and rtisi_la_grad against torch fp64 autograd -----------------------------------------------------------------------
GRAD_AUTOGRAD_SHAPES = [(64, 16, True, 12, 3), (256, 96, False, 2, 3)]


def grad_one(key, kind):
    """Spectrogram 0 of grad_case in fp64: A, c0, gC, gx."""
    return tuple(np.asarray(a[0], dtype=np.complex128 if np.iscomplexobj(a) else np.float64) for a in wc.grad_case(*key[:4], kind)[2:])


@pytest.mark.parametrize("key", GRAD_AUTOGRAD_SHAPES, ids=wc.ident)
@pytest.mark.parametrize("kind", wc.KINDS)
def test_gla_and_rtisi_gradients_match_torch(kind, key):
    """The restatements of tests/test_gla_grad_host.py and tests/test_rtisi_grad_host.py -- frames gathered by an index or placed by
    padding, torch.fft, the projection -- under the pair: there the two windows are multiples of each other and the adjoint transforms
    of the definitions, where they change roles, have only ever been held up to that."""
    torch = pytest.importorskip("torch")
    from test_gla_grad_host import torch_griffin_lim
    from test_rtisi_grad_host import torch_rtisi_la
    A, c0, gC, gx = grad_one(key, kind)
    p = plan(key, kind)
    leaves = lambda: tuple(torch.from_numpy(a.copy()).requires_grad_(True) for a in (A, c0))
    grads = lambda tA, tS: tuple(np.zeros(a.shape, a.dtype) if t.grad is None else t.grad.numpy() for a, t in ((A, tA), (c0, tS)))
    for n, alpha in ((0, 0.99),) + wc.GLA_GRAD_STEPS:
        tA, tS = leaves()
        C = torch_griffin_lim(torch, p, tA, tS, n, alpha)
        (torch.from_numpy(gC).conj() * C).real.sum().backward()
        ref = lws_amd.griffin_lim(c0, p.fsize, p.fshift, p.awin, p.swin, n, alpha=alpha, magnitudes=A, perfectrec=p.perfectrec)
        dC = np.abs(C.detach().numpy() - ref).max() / np.abs(A).max()
        got = lws_amd.griffin_lim_grad(c0, p.fsize, p.fshift, p.awin, p.swin, n, A, alpha=alpha, grad_out=gC, perfectrec=p.perfectrec)
        d = [wc.rel(g, w) for g, w in zip(got, grads(tA, tS))]
        print("%s %s n=%d alpha=%g: griffin_lim off the torch restatement by %.2e max A; griffin_lim_grad rel-L2 to autograd gA %.2e gS %.2e"
              % ((kind, wc.ident(key), n, alpha, dC) + tuple(d)))
        assert dC <= 1e-12 and max(d) <= 1e-10
    for LA, n in ((3, 0),) + wc.LA_STEPS:
        tA, tS = leaves()
        C, x = torch_rtisi_la(torch, p, tA, tS, n, LA)
        ((torch.from_numpy(gC).conj() * C).real.sum() + (torch.from_numpy(gx) * x).sum()).backward()
        ref, sig = lws_amd.rtisi_la(c0, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=A, perfectrec=p.perfectrec, return_signal=True)
        dC = max(np.abs(C.detach().numpy() - ref).max(), np.abs(x.detach().numpy() - sig).max()) / np.abs(A).max()
        got = lws_amd.rtisi_la_grad(c0, p.fsize, p.fshift, p.awin, p.swin, n, A, look_ahead=LA, grad_out=gC, grad_signal=gx, perfectrec=p.perfectrec)
        d = [wc.rel(g, w) for g, w in zip(got, grads(tA, tS))]
        print("%s %s LA=%d n=%d: rtisi_la off the torch restatement by %.2e max A; rtisi_la_grad rel-L2 to autograd gA %.2e gS %.2e"
              % ((kind, wc.ident(key), LA, n, dC) + tuple(d)))
        assert dC <= 1e-12 and max(d) <= 1e-10


# ---- the look-ahead definitions ----------------------------------------------------------------------------------------------------
def rtisi_restated(p, S, n, LA, A):
    """rtisi_la for one spectrogram, stated otherwise: no running sum and no stored frames -- in every inner iteration every frame
    that has entered, the committed ones included, is transformed back from c and overlap-added in one pass."""
    T = S.shape[0]
    N, hop = p.fsize, p.fshift
    total = hop * (T - 1) + N
    idx = hop * np.arange(T)[:, None] + np.arange(N)[None, :]
    keep = np.ones(total)
    if p.perfectrec:
        keep[:N - hop if N % hop == 0 else N - N % hop] = 0.0
        keep[total - (N - hop):] = 0.0
    c = S.astype(np.complex128)
    for m in range(T):
        last = min(m + LA, T - 1)
        for it in range(n):
            frames = p.swin * np.fft.irfft(c[:last + 1], N, axis=1)
            x = keep * np.bincount(idx[:last + 1].ravel(), weights=frames.ravel(), minlength=total)
            X = np.fft.rfft(p.awin * x[idx[m:last + 1]], axis=1)
            mag = np.abs(X)
            c[m:last + 1] = np.where(mag > 0, A[m:last + 1] * X / np.where(mag > 0, mag, 1.0), A[m:last + 1])
    return c


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_look_ahead_definitions_match_restatements_of_other_structure(kind, key):
    from test_misi_la_host import restated as misi_la_restated
    A, c0, y, gC, gs = one(key, kind)
    p = plan(key, kind)
    for LA, n in ((0, 2), (1, 3), (3, 3), (20, 2)):
        out = lws_amd.rtisi_la(c0[0], p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=A[0], perfectrec=p.perfectrec)
        d = wc.rel(out, rtisi_restated(p, c0[0], n, LA, A[0]))
        out = lws_amd.misi_la(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=A, perfectrec=p.perfectrec)
        want = misi_la_restated(p, c0, y, n, LA, A)
        dm = max(wc.rel(out[k], want[k]) for k in range(key[4]))
        print("%s %s LA=%d n=%d: rel-L2 to the restatement, rtisi_la %.2e, misi_la %.2e" % (kind, wc.ident(key), LA, n, d, dm))
        assert d <= 1e-12 and dm <= 1e-12


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_look_ahead_results_are_finite_and_signals_add_up(kind, key):
    with np.errstate(all="raise"):
        for start in ("given", "mixture"):
            for LA, n in wc.LA_STEPS:
                for open_end in (False, True):
                    (out, s), _ = wc.host_misi_la(key, kind, LA, n, start, open_end)
                    y = wc.misi_la_input(key, kind, start, open_end)[2].astype(np.float64)[:, :s.shape[-1]]
                    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
                    tot = s[:, 0].copy()
                    for k in range(1, s.shape[1]):
                        tot += s[:, k]
                    off = (np.abs(tot - y).max(axis=1) / np.abs(y).max(axis=1)).max()
                    assert off <= 2e-15, (start, LA, n, open_end, off)
        for start in ("given", "overlap"):
            for LA, n in wc.LA_STEPS:
                (out, x), _ = wc.host_rtisi(key, kind, LA, n, start)
                assert np.isfinite(out.view(np.float64)).all() and np.isfinite(x).all()
                awin, swin = wc.pair(key[0], key[1], kind)
                want = np.stack([lws_amd.istft(o, key[1], swin, perfectrec=key[2]) for o in out])
                assert np.abs(x - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("kind,key", MULTI, ids=["%s-%s" % (k, wc.ident(s)) for k, s in MULTI])
def test_open_end_prefix_property_bit_for_bit(kind, key):
    """What the streams rest on: the rows [:T1 - LA] of an open-end run on the first T1 frames are those of the run on all of them."""
    N, hop, perfectrec, T, K = key
    awin, swin = wc.pair(N, hop, kind)
    lo = (N - hop if N % hop == 0 else N - N % hop) if perfectrec else 0
    checked = 0
    for LA, n in wc.LA_STEPS:
        for T1 in sorted({t for t in (T - 1, T // 2 + 1) if LA < t < T}):
            rows, samples = T1 - LA, max(hop * (T1 - LA) - lo, 0)
            for start in ("given", "overlap"):
                S, mags = wc.rtisi_input(key, kind, start)
                kw = dict(look_ahead=LA, perfectrec=perfectrec, return_signal=True, start=start, open_end=True)
                c2, x2 = lws_amd.rtisi_la(S, N, hop, awin, swin, n, magnitudes=mags, **kw)
                c1, x1 = lws_amd.rtisi_la(S[:, :T1], N, hop, awin, swin, n, magnitudes=None if mags is None else mags[:, :T1], **kw)
                assert np.array_equal(c1[:, :rows], c2[:, :rows]) and np.array_equal(x1[:, :samples], x2[:, :samples]), (start, LA, n, T1)
            for start in ("given", "mixture"):
                S, mags, y = wc.misi_la_input(key, kind, start, open_end=True)
                kw = dict(look_ahead=LA, perfectrec=perfectrec, return_signals=True, start=start, open_end=True)
                c2, s2 = lws_amd.misi_la(S, y, N, hop, awin, swin, n, magnitudes=mags, **kw)
                c1, s1 = lws_amd.misi_la(S[:, :, :T1], y[:, :wc.need(key, T1)], N, hop, awin, swin, n,
                                         magnitudes=None if mags is None else mags[:, :, :T1], **kw)
                assert np.array_equal(c1[:, :, :rows], c2[:, :, :rows]) and np.array_equal(s1[..., :samples], s2[..., :samples]), (start, LA, n, T1)
            checked += 1
    assert checked or T <= 2


@pytest.mark.parametrize("kind,key", MULTI, ids=["%s-%s" % (k, wc.ident(s)) for k, s in MULTI])
def test_magnitude_only_starts_are_given_started_from_their_entry_estimates(kind, key):
    """The identities of tests/test_start_host.py: 'overlap' at a look-ahead that lets every frame enter before the first iteration is
    'given' started from its own entry estimates; 'mixture' is 'given' started from the mixture's phase, at any look-ahead."""
    N, hop, perfectrec, T, K = key
    awin, swin = wc.pair(N, hop, kind)
    A0, _ = wc.rtisi_input(key, kind, "overlap")
    kw = dict(look_ahead=T - 1, perfectrec=perfectrec)
    E = lws_amd.rtisi_la(A0, N, hop, awin, swin, 0, start="overlap", **kw)
    for n in (1, 3):
        a = lws_amd.rtisi_la(A0, N, hop, awin, swin, n, start="overlap", **kw)
        b = lws_amd.rtisi_la(E, N, hop, awin, swin, n, magnitudes=A0, **kw)
        err = np.abs(a - b).max() / A0.max()
        print("%s %s n=%d: overlap = given(E) to %.2e max A" % (kind, wc.ident(key), n, err))
        assert err <= 1e-12
    A, _, y = wc.misi_la_input(key, kind, "mixture")
    y = y.astype(np.float64)
    total = hop * (T - 1) + N
    lo = (N - hop if N % hop == 0 else N - N % hop) if perfectrec else 0
    full = np.zeros((y.shape[0], total))
    full[:, lo: lo + y.shape[1]] = y
    X = np.stack([[np.fft.rfft(awin * v[hop * j: hop * j + N]) for j in range(T)] for v in full])
    S0 = A * np.exp(1j * np.angle(X))[:, None]
    for LA, n in ((3, 0), (3, 3), (0, 2)):
        kw = dict(look_ahead=LA, perfectrec=perfectrec, return_signals=True)
        a, sa = lws_amd.misi_la(A, y, N, hop, awin, swin, n, start="mixture", **kw)
        b, sb = lws_amd.misi_la(S0, y, N, hop, awin, swin, n, magnitudes=A, **kw)
        err, serr = np.abs(a - b).max() / A.max(), np.abs(sa - sb).max() / np.abs(y).max()
        print("%s %s LA=%d n=%d: mixture = given(S0) to %.2e max A, signals %.2e max|y|" % (kind, wc.ident(key), LA, n, err, serr))
        assert err <= 1e-12 and serr <= 1e-12


# ---- sensitivity: what a mirrored index or exchanged roles would do ----------------------------------------------------------------
SENSITIVITY_SHAPES = [(64, 16, True, 12, 3), (256, 96, False, 2, 3), (48, 16, True, 7, 2)]


def operations(key, kind):
    """name -> (function of (awin, swin) giving the fp64 result, the bar the GPU files hold the operation to on this input).  The
    iterations at 3 steps, the gradient at 1: at 3 the gate drops two of these inputs for it (wc.DROPPED)."""
    N, hop, perfectrec, T, K = key
    _, _, A, c0, y, gC, gs = wc.case(*key, kind)
    A = A.astype(np.float64)
    x = np.random.default_rng(N).standard_normal(wc.length(N, hop, perfectrec, T))
    S = c0[0, 0].astype(np.complex128)

    def bar_of(ref, per):
        ref, per = (np.asarray(a).reshape((-1,) + np.shape(a)[-2:]) for a in (ref, per))
        return max(3 * wc.rel(p, r) for p, r in zip(per, ref))

    gl, ms, gr = wc.host_gla(key, kind, 3, 0.99), wc.host_misi(key, kind, 3), wc.host_grad(key, kind, 1)
    rt, ml = wc.host_rtisi(key, kind, 3, 3), wc.host_misi_la(key, kind, 3, 3)
    kw = dict(perfectrec=perfectrec)
    return {
        # the transforms: 3e-6 of the largest value (tests/test_gpu_transform_edges.py), a max-norm bar on a max-norm distance
        "stft": (lambda a, s: lws_amd.stft(x, N, hop, a, **kw), 3e-6),
        "istft": (lambda a, s: lws_amd.istft(S, hop, s, **kw), 3e-6),
        "griffin_lim": (lambda a, s: lws_amd.griffin_lim(c0[:, 0], N, hop, a, s, 3, alpha=0.99, magnitudes=A[:, 0], **kw), bar_of(gl[0][0], gl[1][0])),
        "misi": (lambda a, s: lws_amd.misi(c0, y, N, hop, a, s, 3, magnitudes=A, **kw), bar_of(ms[0][0], ms[1][0])),
        "misi_grad": (lambda a, s: lws_amd.misi_grad(c0, y, N, hop, a, s, 1, A, grad_out=gC, grad_signals=gs, **kw)[0], bar_of(gr[0][0], gr[1][0])),
        "rtisi_la": (lambda a, s: lws_amd.rtisi_la(c0[:, 0], N, hop, a, s, 3, look_ahead=3, magnitudes=A[:, 0], **kw), bar_of(rt[0][0], rt[1][0])),
        "misi_la": (lambda a, s: lws_amd.misi_la(c0, y, N, hop, a, s, 3, look_ahead=3, magnitudes=A, **kw), bar_of(ml[0][0], ml[1][0])),
    }


def distance(name, a, b):
    """Of the smallest member of a stack: max-norm for the transforms, rel-L2 for the rest -- the metric of the operation's bar."""
    if name in ("stft", "istft"):
        return float(np.abs(a - b).max() / np.abs(b).max())
    a, b = (np.asarray(v).reshape((-1,) + np.shape(v)[-2:]) for v in (a, b))
    return min(wc.rel(p, r) for p, r in zip(a, b))


@pytest.mark.parametrize("key", SENSITIVITY_SHAPES, ids=wc.ident)
@pytest.mark.parametrize("kind", wc.KINDS)
def test_mirrored_or_exchanged_windows_move_every_operation_by_100_bars(kind, key):
    awin, swin = wc.pair(key[0], key[1], kind)
    for name, (f, bar) in operations(key, kind).items():
        ref = f(awin, swin)
        mirrored, exchanged = distance(name, f(*wc.mirrored(awin, swin)), ref), distance(name, f(*wc.exchanged(awin, swin)), ref)
        print("%s %s %-11s: mirrored windows move it by %.3e, exchanged roles by %.3e; the device's bar is %.3e"
              % (kind, wc.ident(key), name, mirrored, exchanged, bar))
        assert mirrored >= 100 * bar and exchanged >= 100 * bar, (name, mirrored, exchanged, bar)


@pytest.mark.parametrize("key", SENSITIVITY_SHAPES, ids=wc.ident)
def test_under_the_default_pair_mirrored_windows_move_nothing_a_device_could_see(key):
    """The statement of what the old suite could not see.  The default windows equal their mirror images to fp64 rounding, not to
    the bit (test_default_pair_is_mirror_symmetric_to_rounding), so neither are the results: they move by the fp64 rounding of the
    definition itself, held here to a millionth of the bar the device is held to -- against at least 100 bars under the new pairs."""
    awin, swin = wc.pair(key[0], key[1], "default")
    for name, (f, bar) in operations(key, "default").items():
        ref, got = f(awin, swin), f(*wc.mirrored(awin, swin))
        a, b = (np.asarray(v).reshape((-1,) + np.shape(v)[-2:]) for v in (got, ref))
        moved = float(np.abs(got - ref).max() / np.abs(ref).max()) if name in ("stft", "istft") else max(wc.rel(p, r) for p, r in zip(a, b))
        print("default %s %-11s: mirrored windows move it by %.3e; the device's bar is %.3e" % (wc.ident(key), name, moved, bar))
        assert moved <= 1e-6 * bar, (name, moved, bar)


def grad_call(op, kind, key, step):
    """(function of keywords giving (gA, gS) of the fp64 definition, (reference, the same under the error model))."""
    if op == "gla_grad":
        return functools.partial(wc.gla_grad, key, kind, *step), wc.host_gla_grad(key, kind, *step)
    return functools.partial(wc.rtisi_grad, key, kind, *step), wc.host_rtisi_grad(key, kind, *step)


def bars_moved(got, ref, per, A):
    """Per spectrogram, on the frames with A != 0: rel-L2 of got from ref over the bar tests/test_gpu_windows_grad.py holds gA to."""
    seen = A.any(axis=-1)
    return [wc.rel(got[b][seen[b]], ref[b][seen[b]]) / (3 * wc.rel(per[b][seen[b]], ref[b][seen[b]])) for b in range(A.shape[0])]


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("op", ("gla_grad", "rtisi_grad"))
def test_mirrored_or_exchanged_windows_move_every_gradient_by_10_bars(op, kind):
    """On every combination the GPU file runs and every spectrogram of it: the fp64 gA under the mirrored pair, and under the
    exchanged one, lies at least 10 of that spectrogram's bars from the fp64 gA under the pair itself.  One frame of Griffin-Lim
    reads only the product awin swin, in the round trip and in its adjoint, so an exchange moves nothing there: those rows are exempt
    from it.  Measured: at least 1359 (mirrored) and 1003 (exchanged) bars for Griffin-Lim, 28 and 25 for RTISI-LA."""
    low = {"mirrored": np.inf, "exchanged": np.inf}
    for _, key, step in wc.runs(op, kind):
        awin, swin, A = wc.grad_case(*key[:4], kind)[:3]
        f, (ref, per) = grad_call(op, kind, key, step)
        for name, windows in (("mirrored", wc.mirrored(awin, swin)), ("exchanged", wc.exchanged(awin, swin))):
            if name == "exchanged" and op == "gla_grad" and key[3] == 1:
                continue
            moved = min(bars_moved(f(windows=windows)[0], ref[0], per[0], A))
            low[name] = min(low[name], moved)
            assert moved >= 10, (op, kind, key, step, name, moved)
    print("%s %s: mirrored windows move gA by at least %.0f bars, exchanged roles by at least %.0f" % (op, kind, low["mirrored"], low["exchanged"]))


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("op", ("gla_grad", "rtisi_grad"))
def test_a_backward_pass_that_confuses_the_windows_misses_the_device_bar(op, kind):
    """What a kernel bug of this kind would look like: the forward pass right (the definition's own tape, teacher-forced) and only the
    backward transforms given awin and swin in each other's place -- the forward kernels' roles carried over -- or read backwards.
    Under the pair the gA or the gS of such a pass is outside the bar the device's is held to (dist <= 1 bar), on every combination the GPU
    file runs and every spectrogram.  The single-frame rows are exempt from the exchange: one frame reads only the product."""
    low = {"mirrored": np.inf, "exchanged": np.inf}
    for _, key, step in wc.runs(op, kind):
        awin, swin, A = wc.grad_case(*key[:4], kind)[:3]
        f, (ref, per) = grad_call(op, kind, key, step)
        tape = wc.host_gla_tape(key, kind, *step) if op == "gla_grad" else wc.host_rtisi_tape(key, kind, *step)
        assert all(np.array_equal(a, b) for a, b in zip(f(_tape=tape), ref))          # the teacher-forced definition is the definition
        for name, windows in (("mirrored", wc.mirrored(awin, swin)), ("exchanged", (swin, awin))):
            if name == "exchanged" and key[3] == 1:
                continue
            got = f(windows=windows, _tape=tape)
            # one step of Griffin-Lim feeds gA from no transform: there the windows are in gS alone, held on every frame
            out = zip(bars_moved(got[0], ref[0], per[0], A), bars_moved(got[1], ref[1], per[1], np.ones_like(A)))
            moved = min(max(a, s) for a, s in out)
            low[name] = min(low[name], moved)
            assert moved > 1, (op, kind, key, step, name, moved)
    print("%s %s: a backward pass with mirrored windows is at least %.0f bars out, one with the windows exchanged at least %.0f"
          % (op, kind, low["mirrored"], low["exchanged"]))


def test_overlap_entries_are_within_what_float32_can_compute_except_where_recorded():
    """start='overlap' estimates a frame from the inverse transforms of the frames before it.  The float32 transform model makes at most
    OVERLAP_SIGMA max|X| of that on every input but 'padded' under perfectrec, where the second frame reads the far tail of a zero-phase
    first frame: there the whole run is not compared with the fp64 one (the device still runs them for everything else, and their
    entries teacher-forced to three times this model), by name and with the model's figure."""
    for kind in wc.KINDS:
        for key in wc.SHAPES + [wc.SCRATCH_RTISI[0]]:
            worst = max(wc.entry_conditioning(key, kind, open_end) for open_end in (False, True))
            print("%s %s: the float32 model moves an entry projection's argument by %.2e max|X|%s"
                  % (kind, wc.ident(key), worst, "" if wc.has_overlap_case(kind, key) else "  (start='overlap': no whole-run comparison)"))
            assert (worst <= wc.OVERLAP_SIGMA) == wc.has_overlap_case(kind, key)
            if not wc.has_overlap_case(kind, key):
                assert abs(worst / wc.NOT_AN_OVERLAP_CASE[kind, key] - 1) <= 0.01 and wc.overlap_sigma(kind, key) == worst
            else:
                assert wc.overlap_sigma(kind, key) == wc.OVERLAP_SIGMA
    for kind in wc.KINDS:
        assert sum(wc.has_overlap_case(kind, s) for s in wc.SHAPES) >= 3


# ---- the gate on the inputs of the GPU files ------------------------------------------------------------------------------------------
OPS = ("griffin_lim", "misi", "misi_grad", "rtisi_la", "misi_la", "gla_grad", "rtisi_grad")
GRAD_OPS = ("misi_grad", "gla_grad", "rtisi_grad")       # gated on the share of the entries of gA, up to FAR_CAP


@pytest.mark.parametrize("op", OPS)
def test_gate_lets_through_what_the_model_keeps_and_nothing_else(op):
    cap = wc.FAR_CAP if op in GRAD_OPS else 0.0
    combos = wc.combinations(op)
    dropped = wc.DROPPED[op]
    assert set(dropped) <= set(combos)
    worst = 0.0
    for c in combos:
        share = wc.model_share(op, c)
        if c in dropped:
            print("%s dropped %r: the model moves %.3f%% (recorded %.3f%%)" % (op, c, 100 * share, 100 * dropped[c]))
            assert share > cap and abs(share - dropped[c]) <= 1e-5
        else:
            worst = max(worst, share)
            assert share <= cap, (op, c, share)
    print("%s: %d of %d combinations dropped; the others at %.3f%% at most (cap %.3f%%)" % (op, len(dropped), len(combos), 100 * worst, 100 * cap))
    if op == "rtisi_la":
        beyond = len(wc.overlap_property_runs())
        print("rtisi_la: %d more, start='overlap' beyond float32 (wc.NOT_AN_OVERLAP_CASE), run on the device for their properties and "
              "teacher-forced, not compared with the fp64 run: %d of %d without that comparison" % (beyond, beyond + len(dropped), beyond + len(combos)))
        assert beyond == 12 and len(combos) == 141
    if op in ("gla_grad", "rtisi_grad"):
        assert (len(combos), len(dropped)) == ((63, 0) if op == "gla_grad" else (90, 4))
    if op == "rtisi_grad":                               # the gate keeps every scratch row
        assert all((kind, s, (LA, n)) in wc.runs(op) for kind in wc.KINDS for s, LA, n in wc.SCRATCH_RTISI_GRAD)
    assert 10 * len(dropped) <= len(combos)
    for kind in wc.KINDS:
        assert {c[1] for c in wc.runs(op, kind)} == {c[1] for c in combos if c[0] == kind} or op in ("rtisi_la", "misi_la")
        assert wc.runs(op, kind)
    assert len(wc.runs(op)) == len(combos) - len(dropped)
