"""CPU: lws_amd.misi_grad, the fp64 definition of the gradient through MISI, against torch fp64 autograd of a restatement of
lws_amd.misi written here, against central differences of lws_amd.misi itself, at its |X| = 0 convention, and -- for the GPU file
that is held to it (tests/test_gpu_misi_grad.py) -- the share of gradient entries the error model of tests/misi_grad_cases.py
moves far.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest

import lws_amd
import misi_grad_cases as gc

STEPS = (0, 1, 3)


def one(key):
    """Mixture 0 of the case of `key` in fp64: p, A, c0, y, gC, gs."""
    p, A, c0, y, gC, gs = gc.case(*key)
    return (p,) + tuple(np.asarray(a[0], dtype=np.complex128 if np.iscomplexobj(a) else np.float64) for a in (A, c0, y, gC, gs))


def torch_misi(torch, p, A, S, y, n):
    """lws_amd.misi(..., magnitudes=A, return_signals=True) for one mixture, restated on torch fp64 tensors: the frames of the
    uncut timeline gathered with an index, transformed with torch.fft, overlap-added with index_add."""
    K, T, F = S.shape
    N, hop = p.fsize, p.fshift
    full = hop * (T - 1) + N
    lo, hi = (N - (N % hop or hop), full - (N - hop)) if p.perfectrec else (0, full)     # the cuts of lws.pyx:130-137
    idx = torch.from_numpy(hop * np.arange(T)[:, None] + np.arange(N)[None, :])
    awin, swin = torch.from_numpy(np.asarray(p.awin, dtype=np.float64)), torch.from_numpy(np.asarray(p.swin, dtype=np.float64))

    def signals(c):
        frames = torch.fft.irfft(c, n=N, dim=-1) * swin                    # (K, T, N)
        x = torch.zeros((K, full), dtype=torch.float64).index_add(1, idx.reshape(-1), frames.reshape(K, -1))[:, lo:hi]
        tot = x[0]
        for k in range(1, K):
            tot = tot + x[k]
        return x + (y - tot) / K

    c = S
    for _ in range(n):
        v = torch.nn.functional.pad(signals(c), (lo, full - hi))
        X = torch.fft.rfft(v[:, idx] * awin, dim=-1)
        mag = X.abs()
        safe = torch.where(mag > 0, mag, torch.ones_like(mag))
        c = torch.where(mag > 0, A * X / safe, A + 0j)
    return c, signals(c)


@functools.lru_cache(maxsize=None)
def autograd(key, n, which):
    torch = pytest.importorskip("torch")
    p, A, c0, y, gC, gs = one(key)
    tA, tS, ty = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (A, c0, y))
    C, s = torch_misi(torch, p, tA, tS, ty, n)
    loss = 0.0
    if which in ("both", "C"):
        loss = loss + (torch.from_numpy(gC).conj() * C).real.sum()
    if which in ("both", "s"):
        loss = loss + (torch.from_numpy(gs) * s).sum()
    loss.backward()
    grads = tuple(np.zeros(a.shape, a.dtype) if t.grad is None else t.grad.numpy() for a, t in ((A, tA), (c0, tS), (y, ty)))
    return C.detach().numpy(), s.detach().numpy(), grads


@pytest.mark.parametrize("key", gc.HOST_SHAPES, ids=gc.ident)
def test_restatement_is_misi(key):
    p, A, c0, y, gC, gs = one(key)
    for n in STEPS:
        C, s, _ = autograd(key, n, "both")
        ref, ref_s = p.misi(c0, y, n, magnitudes=A, return_signals=True)
        dC, ds = np.abs(C - ref).max() / np.abs(A).max(), np.abs(s - ref_s).max() / np.abs(y).max()
        print("misi_grad %s n=%d: restatement off %.2e max A (spectrograms), %.2e max|y| (signals)" % (gc.ident(key), n, dC, ds))
        assert dC <= 1e-12 and ds <= 1e-12


@pytest.mark.parametrize("which", ["both", "C", "s"])
@pytest.mark.parametrize("key", gc.HOST_SHAPES, ids=gc.ident)
def test_matches_autograd(key, which):
    p, A, c0, y, gC, gs = one(key)
    for n in STEPS:
        want = autograd(key, n, which)[2]
        got = lws_amd.misi_grad(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, A, grad_out=gC if which != "s" else None,
                                grad_signals=gs if which != "C" else None, perfectrec=p.perfectrec)
        d = [gc.rel(g, w) for g, w in zip(got, want)]
        print("misi_grad %s n=%d cotangents %s: rel-L2 to autograd gA %.2e gS %.2e gy %.2e" % ((gc.ident(key), n, which) + tuple(d)))
        assert got[0].dtype == np.float64 and got[1].dtype == np.complex128 and got[2].dtype == np.float64
        assert [g.shape for g in got] == [A.shape, c0.shape, y.shape]
        assert max(d) <= 1e-10
        if n == 0:
            assert not got[0].any()
    pm = p.misi_grad(c0, y, 3, A, grad_out=gC, grad_signals=gs)          # the method, and a stack of one
    st = lws_amd.misi_grad(c0[None], y[None], p.fsize, p.fshift, p.awin, p.swin, 3, A[None], grad_out=gC[None], grad_signals=gs[None],
                           perfectrec=p.perfectrec)
    ref = lws_amd.misi_grad(c0, y, p.fsize, p.fshift, p.awin, p.swin, 3, A, grad_out=gC, grad_signals=gs, perfectrec=p.perfectrec)
    assert all(np.array_equal(a, b) and np.array_equal(a, c[0]) for a, b, c in zip(ref, pm, st))


@pytest.mark.parametrize("key", gc.HOST_SHAPES, ids=gc.ident)
def test_matches_central_differences_of_misi(key):
    """No torch: L = Re <gC, C> + <gs, s> of lws_amd.misi itself, differentiated along a random direction in A and one in S."""
    p, A, c0, y, gC, gs = one(key)
    rng = np.random.default_rng(5)
    dA = rng.standard_normal(A.shape) * np.abs(A).mean()
    dS = (rng.standard_normal(c0.shape) + 1j * rng.standard_normal(c0.shape)) * np.abs(A).mean()
    h = 1e-6

    def loss(A_, S_, n):
        C, s = p.misi(S_, y, n, magnitudes=A_, return_signals=True)
        return np.sum(np.real(np.conj(gC) * C)) + np.sum(gs * s)

    for n in STEPS:
        gA, gS, gy = p.misi_grad(c0, y, n, A, grad_out=gC, grad_signals=gs)
        rows = (("A", (loss(A + h * dA, c0, n) - loss(A - h * dA, c0, n)) / (2 * h), np.sum(gA * dA)),
                ("S", (loss(A, c0 + h * dS, n) - loss(A, c0 - h * dS, n)) / (2 * h), np.sum(np.real(np.conj(gS) * dS))))
        for name, fd, an in rows:
            print("misi_grad %s n=%d along d%s: central difference %.10e, <g, d> %.10e" % (gc.ident(key), n, name, fd, an))
            if name == "A" and n == 0:
                assert fd == 0 and an == 0                                  # nothing reads A without a projection
            else:
                assert abs(fd - an) <= 1e-5 * abs(an)


def zero_case(K):
    """y = 0 and S = 0: the X of step 1 are 0, so c_1 = A + 0j; with K = 1 the one source gets all of the mixture back, v = y = 0,
    so the X of every later step are 0 too (with K > 1 the sources of c_1 differ from their mean)."""
    p = lws_amd.lws(64, 16, perfectrec=False)
    rng = np.random.default_rng(3)
    T = 9
    A = rng.random((K, T, 33)) + 0.5
    n = p.istft(np.zeros((T, 33), complex)).shape[0]
    gC = rng.standard_normal(A.shape) + 1j * rng.standard_normal(A.shape)
    gs = rng.standard_normal((K, n))
    return p, A, np.zeros(A.shape, complex), np.zeros(n), gC, gs


@pytest.mark.parametrize("K,n", [(2, 1), (1, 1), (1, 3)])
def test_zero_projection_convention(K, n):
    p, A, S, y, gC, gs = zero_case(K)
    out = p.misi(S, y, n, magnitudes=A)
    assert np.array_equal(out, A + 0j)
    gA, gS, gy = p.misi_grad(S, y, n, A, grad_out=gC, grad_signals=gs)
    assert all(np.isfinite(g.view(np.float64)).all() for g in (gA, gS, gy))
    # step 3 with u = 1: gA = Re gc at the last step, gc = gC + the entry pass of gs; gX = 0 there, so nothing goes further back
    entry = lws_amd.misi_grad(S, y, p.fsize, p.fshift, p.awin, p.swin, 0, A, grad_out=gC, grad_signals=gs)
    print("misi_grad zero |X| K=%d n=%d: |gA - Re gc| %.2e, |gS| %.2e, |gy - entry| %.2e"
          % (K, n, np.abs(gA - entry[1].real).max(), np.abs(gS).max(), np.abs(gy - entry[2]).max()))
    assert np.array_equal(gA, entry[1].real)
    assert not gS.any() and np.array_equal(gy, entry[2])


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_far_entry_cap_is_honest_for_the_chosen_seed(key):
    p, A, c0, y, gC, gs = gc.case(*key)
    B, K = c0.shape[:2]
    for n in gc.STEPS:
        ref, per = gc.host(key, n)
        worst = {"gA": max(gc.far(per[0][b, k], ref[0][b, k]) for b in range(B) for k in range(K)),
                 "gS": max(gc.far(per[1][b, k], ref[1][b, k]) for b in range(B) for k in range(K)),
                 "gy": max(gc.far(per[2][b], ref[2][b]) for b in range(B))}
        move = max(gc.rel(per[0][b, k], ref[0][b, k]) for b in range(B) for k in range(K))
        print("misi_grad %s n=%d: the error model moves gA by at most %.2e rel-L2; far entries gA %.3f%% gS %.3f%% gy %.3f%%"
              % (gc.ident(key), n, move, 100 * worst["gA"], 100 * worst["gS"], 100 * worst["gy"]))
        assert worst["gA"] <= gc.FAR_CAP, worst                             # (gS and gy: see misi_grad_cases.case)
