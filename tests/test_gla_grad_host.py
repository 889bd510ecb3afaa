"""CPU: lws_amd.griffin_lim_grad, the fp64 definition of the gradient through (Fast) Griffin-Lim, against torch fp64 autograd of a
restatement of lws_amd.griffin_lim written here, against central differences of lws_amd.griffin_lim itself, at its |X| = 0
convention, against the same recurrence without its momentum terms, and -- for the GPU file that is held to it
(tests/test_gpu_gla_grad.py) -- the share of gradient entries the error model of tests/gla_grad_cases.py moves far.  Every figure
is printed before it is asserted (pytest -s)."""
import functools
import sys

import numpy as np
import pytest

import lws_amd
import gla_grad_cases as gc

host = sys.modules["lws_amd.lws"]            # the module: lws_amd.lws is the class of that name

STEPS = (0, 1, 2, 3, 5)
ALPHAS = (0.0, 0.5, 0.99)


def one(key):
    """Spectrogram 0 of the case of `key` in fp64: p, A, c0, gC."""
    p, A, c0, gC = gc.case(*key)
    return (p,) + tuple(np.asarray(a[0], dtype=np.complex128 if np.iscomplexobj(a) else np.float64) for a in (A, c0, gC))


def torch_griffin_lim(torch, p, A, S, n, alpha):
    """lws_amd.griffin_lim(..., alpha=alpha, magnitudes=A) for one spectrogram, restated on torch fp64 tensors: the frames of the
    uncut timeline gathered with an index, transformed with torch.fft, overlap-added with index_add."""
    T, F = S.shape
    N, hop = p.fsize, p.fshift
    full = hop * (T - 1) + N
    lo, hi = (N - (N % hop or hop), full - (N - hop)) if p.perfectrec else (0, full)     # the cuts of lws.pyx:130-137
    idx = torch.from_numpy(hop * np.arange(T)[:, None] + np.arange(N)[None, :])
    awin, swin = torch.from_numpy(np.asarray(p.awin, dtype=np.float64)), torch.from_numpy(np.asarray(p.swin, dtype=np.float64))
    c, t_prev = S, None
    for i in range(1, n + 1):
        frames = torch.fft.irfft(c, n=N, dim=-1) * swin                    # (T, N)
        x = torch.zeros(full, dtype=torch.float64).index_add(0, idx.reshape(-1), frames.reshape(-1))[lo:hi]
        v = torch.nn.functional.pad(x, (lo, full - hi))
        X = torch.fft.rfft(v[idx] * awin, dim=-1)
        mag = X.abs()
        safe = torch.where(mag > 0, mag, torch.ones_like(mag))
        t = torch.where(mag > 0, A * X / safe, A + 0j)
        c = t if i == 1 else t + alpha * (t - t_prev)
        t_prev = t
    return S if n == 0 else t_prev


@functools.lru_cache(maxsize=None)
def autograd(key, n, alpha):
    torch = pytest.importorskip("torch")
    p, A, c0, gC = one(key)
    tA, tS = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (A, c0))
    C = torch_griffin_lim(torch, p, tA, tS, n, alpha)
    (torch.from_numpy(gC).conj() * C).real.sum().backward()
    grads = tuple(np.zeros(a.shape, a.dtype) if t.grad is None else t.grad.numpy() for a, t in ((A, tA), (c0, tS)))
    return C.detach().numpy(), grads


@pytest.mark.parametrize("key", gc.HOST_SHAPES, ids=gc.ident)
def test_restatement_is_griffin_lim(key):
    p, A, c0, gC = one(key)
    for n in STEPS:
        for alpha in ALPHAS:
            C, _ = autograd(key, n, alpha)
            ref = p.griffin_lim(c0, n, alpha=alpha, magnitudes=A)
            d = np.abs(C - ref).max() / np.abs(A).max()
            print("gla_grad %s n=%d alpha=%g: restatement off %.2e max A" % (gc.ident(key), n, alpha, d))
            assert d <= 1e-12


@pytest.mark.parametrize("key", gc.HOST_SHAPES, ids=gc.ident)
def test_matches_autograd(key):
    p, A, c0, gC = one(key)
    for n in STEPS:
        for alpha in ALPHAS:
            want = autograd(key, n, alpha)[1]
            got = lws_amd.griffin_lim_grad(c0, p.fsize, p.fshift, p.awin, p.swin, n, A, alpha=alpha, grad_out=gC,
                                           perfectrec=p.perfectrec)
            d = [gc.rel(g, w) for g, w in zip(got, want)]
            print("gla_grad %s n=%d alpha=%g: rel-L2 to autograd gA %.2e gS %.2e" % ((gc.ident(key), n, alpha) + tuple(d)))
            assert got[0].dtype == np.float64 and got[1].dtype == np.complex128
            assert [g.shape for g in got] == [A.shape, c0.shape]
            assert max(d) <= 1e-10
            if n == 0:
                assert not got[0].any() and np.array_equal(got[1], gC)
    pm = p.griffin_lim_grad(c0, 5, A, alpha=0.5, grad_out=gC)                # the method, and a stack of one
    st = lws_amd.griffin_lim_grad(c0[None], p.fsize, p.fshift, p.awin, p.swin, 5, A[None], alpha=0.5, grad_out=gC[None],
                                  perfectrec=p.perfectrec)
    ref = lws_amd.griffin_lim_grad(c0, p.fsize, p.fshift, p.awin, p.swin, 5, A, alpha=0.5, grad_out=gC, perfectrec=p.perfectrec)
    assert all(np.array_equal(a, b) and np.array_equal(a, c[0]) for a, b, c in zip(ref, pm, st))
    none = p.griffin_lim_grad(c0, 3, A)                                      # no cotangent: zeros
    assert not none[0].any() and not none[1].any()


@pytest.mark.parametrize("key", gc.HOST_SHAPES, ids=gc.ident)
def test_matches_central_differences_of_griffin_lim(key):
    """No torch: L = Re <gC, C> of lws_amd.griffin_lim itself, differentiated along a random direction in A and one in S."""
    p, A, c0, gC = one(key)
    rng = np.random.default_rng(5)
    dA = rng.standard_normal(A.shape) * np.abs(A).mean()
    dS = (rng.standard_normal(c0.shape) + 1j * rng.standard_normal(c0.shape)) * np.abs(A).mean()
    h = 1e-6
    for n in STEPS:
        for alpha in ALPHAS:
            def loss(A_, S_):
                return np.sum(np.real(np.conj(gC) * p.griffin_lim(S_, n, alpha=alpha, magnitudes=A_)))

            gA, gS = p.griffin_lim_grad(c0, n, A, alpha=alpha, grad_out=gC)
            rows = (("A", (loss(A + h * dA, c0) - loss(A - h * dA, c0)) / (2 * h), np.sum(gA * dA)),
                    ("S", (loss(A, c0 + h * dS) - loss(A, c0 - h * dS)) / (2 * h), np.sum(np.real(np.conj(gS) * dS))))
            for name, fd, an in rows:
                print("gla_grad %s n=%d alpha=%g along d%s: central difference %.10e, <g, d> %.10e"
                      % (gc.ident(key), n, alpha, name, fd, an))
                if name == "A" and n == 0:
                    assert fd == 0 and an == 0                              # nothing reads A without a projection
                else:
                    assert abs(fd - an) <= 1e-5 * abs(an)


def zero_case():
    """S = 0: the X of step 1 is 0, so t_1 = A + 0j."""
    p = lws_amd.lws(64, 16, perfectrec=False)
    rng = np.random.default_rng(3)
    A = rng.random((9, 33)) + 0.5
    gC = rng.standard_normal(A.shape) + 1j * rng.standard_normal(A.shape)
    return p, A, np.zeros(A.shape, complex), gC


def test_zero_projection_convention():
    p, A, S, gC = zero_case()
    assert np.array_equal(p.griffin_lim(S, 1, magnitudes=A), A + 0j)
    gA, gS = p.griffin_lim_grad(S, 1, A, grad_out=gC)
    print("gla_grad zero |X| n=1: |gA - Re gt| %.2e, |gS| %.2e" % (np.abs(gA - gC.real).max(), np.abs(gS).max()))
    assert np.array_equal(gA, gC.real) and not gS.any()                      # u = 1: gA = Re gt; gX = 0: nothing goes further back
    # more steps: only step 1 has a zero argument; its share of gA is Re gt_1 and the start still gets nothing
    for n, alpha in ((3, 0.0), (3, 0.99), (5, 0.99)):
        gA, gS = p.griffin_lim_grad(S, n, A, alpha=alpha, grad_out=gC)
        assert np.isfinite(gA).all() and not gS.any()


def plain_backward(p, tape, A, gC):
    """The recurrence of griffin_lim_grad with the momentum terms deleted: gt_i = gc_i."""
    T = A.shape[0]
    gA, g = np.zeros(A.shape), gC
    for i in range(tape.shape[0], 0, -1):
        X = tape[i - 1]
        mag = np.abs(X)
        u = np.where(mag > 0, X / np.where(mag > 0, mag, 1.0), 1.0 + 0j)
        q = np.conj(u) * g
        gA += q.real
        gX = np.where(mag > 0, 1j * u * (A / np.where(mag > 0, mag, 1.0)) * q.imag, 0j)
        gv = host._misi_stft_adjoint(gX, p.fsize, p.fshift, p.awin, p.perfectrec)
        g = host._misi_istft_adjoint(gv, T, p.fsize, p.fshift, p.swin, p.perfectrec)
    return gA, g


@pytest.mark.parametrize("key", gc.HOST_SHAPES, ids=gc.ident)
def test_no_momentum_is_the_plain_recurrence(key):
    p, A, c0, gC = one(key)
    for n in (1, 2, 3, 5):
        tape = []
        p_ = lambda i, b, X: (tape.append(X), X)[1]
        lws_amd.griffin_lim(c0, p.fsize, p.fshift, p.awin, p.swin, n, alpha=0.0, magnitudes=A, perfectrec=p.perfectrec, _perturb=p_)
        want = plain_backward(p, np.stack(tape), A, gC)
        got = p.griffin_lim_grad(c0, n, A, alpha=0.0, grad_out=gC)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if n <= 2:                                                          # the first step has no momentum, the last leaves t_n
            with_m = p.griffin_lim_grad(c0, n, A, alpha=0.99, grad_out=gC)
            assert np.array_equal(with_m[0], want[0]) and np.array_equal(with_m[1], want[1])
        else:
            with_m = p.griffin_lim_grad(c0, n, A, alpha=0.99, grad_out=gC)
            assert gc.rel(with_m[0], want[0]) > 1e-3                        # ... and from three steps on it reaches the gradient


def test_teacher_forced_tape_is_used():
    p, A, c0, gC = one((64, 16, True, 12))
    tape = np.empty((3,) + c0.shape, dtype=np.complex128)

    def rec(i, b, X):
        tape[i - 1] = X
        return X
    lws_amd.griffin_lim(c0, p.fsize, p.fshift, p.awin, p.swin, 3, alpha=0.99, magnitudes=A, perfectrec=p.perfectrec, _perturb=rec)
    args = (c0, p.fsize, p.fshift, p.awin, p.swin, 3, A)
    ref = lws_amd.griffin_lim_grad(*args, alpha=0.99, grad_out=gC, perfectrec=p.perfectrec)
    forced = lws_amd.griffin_lim_grad(np.zeros_like(c0), *args[1:], alpha=0.99, grad_out=gC, perfectrec=p.perfectrec, _tape=tape)
    assert all(np.array_equal(a, b) for a, b in zip(ref, forced))            # the start is not read when a tape is given
    seen = []
    lws_amd.griffin_lim_grad(*args, alpha=0.99, grad_out=gC, perfectrec=p.perfectrec,
                             _perturb=lambda kind, i, b, Z: (seen.append((kind, i, b)), Z)[1])
    assert seen == [('X', 1, 0), ('X', 2, 0), ('X', 3, 0), ('gv', 3, 0), ('gc', 2, 0), ('gv', 2, 0), ('gc', 1, 0), ('gv', 1, 0),
                    ('gc', 0, 0)]


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_far_entry_cap_is_honest_for_the_chosen_seed(key):
    p, A, c0, gC = gc.case(*key)
    B = c0.shape[0]
    for n in gc.STEPS:
        for alpha in gc.ALPHAS:
            ref, per = gc.host(key, n, alpha)
            worst = max(gc.far(per[0][b], ref[0][b]) for b in range(B))
            move = [max(gc.rel(per[j][b], ref[j][b]) for b in range(B)) for j in (0, 1)]
            print("gla_grad %s n=%d alpha=%g: the error model moves gA by at most %.2e and gS by at most %.2e rel-L2; far entries "
                  "of gA %.3f%%" % (gc.ident(key), n, alpha, move[0], move[1], 100 * worst))
            assert worst <= gc.FAR_CAP, worst                               # (gS: see gla_grad_cases.case)


def test_invalid_arguments():
    p, A, c0, gC = one((64, 16, False, 9))
    with pytest.raises(ValueError):
        p.griffin_lim_grad(c0, 2, None)
    with pytest.raises(ValueError):
        p.griffin_lim_grad(c0, 2, A[:-1])
    with pytest.raises(ValueError):
        p.griffin_lim_grad(c0, 2, A, grad_out=gC[:, :-1])
    with pytest.raises(ValueError):
        p.griffin_lim_grad(c0, -1, A)
    with pytest.raises(ValueError):
        p.griffin_lim_grad(c0, 2, A, alpha=1.0)
    with pytest.raises(ValueError):
        p.griffin_lim_grad(c0[0], 2, A[0])                                   # a 1-D S
    q = lws_amd.lws(64, 16, perfectrec=True)
    with pytest.raises(ValueError):
        q.griffin_lim_grad(c0[:2], 1, A[:2])                                 # perfectrec does not keep two frames
