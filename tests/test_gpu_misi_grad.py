"""GPU: the backward pass of MISI on the device (k_misi_bwd_* of lws_gla.hip, lws_amd.misi_layer) against the host fp64 definition
(lws_amd.misi_grad), and against the forward kernels themselves.

Inputs, cotangents, error model and host references are those of tests/misi_grad_cases.py.  As in tests/test_gpu_misi.py the value
checks have no fixed tolerance: a bar is the rel-L2 distance the host fp64 pass moves under the error model, times 3, measured
here on the host side only; tests/test_misi_grad_host.py holds the model itself to the far-entry cap.  Distances, caps and bars are
taken per mixture and per source (per mixture for gy), so that the weak source of a mixture and the small-scale members of a stack
are held as tightly as the loud ones.  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import lws_amd
import misi_grad_cases as gc
from gpu_grad_helpers import Margins, dev, f64, ptr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

capi = lws_amd._capi
# per (fsize, fshift, perfectrec): [rows, max rel-L2 of gA, max rel-L2 / bar of the whole run (gA, gS, gy), max far fraction of gA,
# max rel-L2 / bar of the teacher-forced pass]
FIGURES = ("rows", "max_rel_l2_gA", "max_rel_l2_over_bar", "max_far_fraction_gA", "max_teacher_forced_rel_l2_over_bar")
MARGINS = Margins(FIGURES)


def run(p, A, S, y, n, gC, gs, want_S=True, want_y=True):
    """lws_misi_tape_dev then lws_misi_backward_dev on device tensors (stacked): C, s, tape, gA, gS, gy."""
    B, K, T, F = S.shape
    C, tape = S.clone(), torch.empty((n, B, K, T, F), dtype=torch.complex64, device=S.device)
    s = torch.empty((B, K, y.shape[1]), dtype=torch.float32, device=S.device)
    capi.misi_tape_dev(C.data_ptr(), A.data_ptr(), y.data_ptr(), B, K, T, p.fsize, p.fshift, p.awin, p.swin, p.perfectrec, n,
                       s.data_ptr(), ptr(tape) if n else None)
    gA = torch.full(A.shape, float("nan"), dtype=torch.float32, device=S.device)
    gS = torch.full(S.shape, float("nan"), dtype=torch.complex64, device=S.device) if want_S else None
    gy = torch.full(y.shape, float("nan"), dtype=torch.float32, device=S.device) if want_y else None
    capi.misi_backward_dev(ptr(gC), ptr(gs), A.data_ptr(), ptr(tape) if n else None, B, K, T, p.fsize, p.fshift, p.awin, p.swin,
                           p.perfectrec, n, gA.data_ptr(), ptr(gS), ptr(gy))
    return C, s, tape, gA, gS, gy


def on_device(key):
    p, A, c0, y, gC, gs = gc.case(*key)
    return (p,) + tuple(dev(a) for a in (A, c0, y, gC, gs))


def ratio(dist, bar):
    """dist / bar, with 0 / 0 = 0: with one source the start has no gradient, exactly, on both sides."""
    return dist / bar if bar > 0 else (0.0 if dist == 0 else float("inf"))


def rows_of(name, got, ref, per):
    """(label, distance, bar) per mixture and source (per mixture for gy)."""
    if name == "gy":
        return [("%s b=%d" % (name, b), gc.rel(got[b], ref[b]), 3 * gc.rel(per[b], ref[b])) for b in range(ref.shape[0])]
    return [("%s b=%d k=%d" % (name, b, k), gc.rel(got[b, k], ref[b, k]), 3 * gc.rel(per[b, k], ref[b, k]))
            for b in range(ref.shape[0]) for k in range(ref.shape[1])]


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_same_bits_as_misi_dev(key):
    p, A, S, y, gC, gs = on_device(key)
    top = f64(A).max(axis=(2, 3))
    for n in gc.STEPS:
        want_C, want_s = p.misi_dev(S, y, n, magnitudes=A, return_signals=True)
        C, s = p.misi_layer(A, S, y, n)
        C2, s2, tape = run(p, A, S, y, n, None, None)[:3]
        assert C.dtype == torch.complex64 and s.dtype == torch.float32
        assert torch.equal(C, want_C) and torch.equal(s, want_s) and torch.equal(C2, want_C) and torch.equal(s2, want_s)
        X, a = f64(tape[n - 1]), f64(A)
        mag = np.abs(X)
        proj = np.where(mag > 0, a * X / np.where(mag > 0, mag, 1.0), a + 0j)
        off = (np.abs(proj - f64(C)).max(axis=(2, 3)) / top).max()
        print("misi_grad %s n=%d: same bits as misi_dev; the last tape entry projected in fp64 is within %.2e max A of C"
              % (gc.ident(key), n, off))
        assert off <= 2e-6


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_adjoint_of_the_forward_kernels(key):
    """n = 0: the signals are affine in S and in y, so <s(S + d) - s(S), gs> = Re <d, gS> and <s(y + d) - s(y), gs> = <d, gy> with
    the differences taken from the forward kernels' own float32 outputs (d about 0.1 of its argument, so that their rounding,
    1e-7 of s, stays 1e-6 of the difference) and the inner products in fp64 on the host."""
    p, A, c0, y, gC, gs = gc.case(*key)
    rng = np.random.default_rng(11)
    B = c0.shape[0]
    rms = np.sqrt(np.mean(np.abs(c0) ** 2, axis=(1, 2, 3), keepdims=True))
    S2 = (c0 + 0.1 * rms * (rng.standard_normal(c0.shape) + 1j * rng.standard_normal(c0.shape)) / np.sqrt(2)).astype(np.complex64)
    y2 = (y + 0.1 * np.sqrt(np.mean(y.astype(np.float64) ** 2, axis=1, keepdims=True)) * rng.standard_normal(y.shape)).astype(np.float32)
    dS, dy = S2.astype(np.complex128) - c0, y2.astype(np.float64) - y
    s0 = f64(p.misi_dev(c0, y, 0, return_signals=True)[1])
    s_S = f64(p.misi_dev(S2, y, 0, return_signals=True)[1])
    s_y = f64(p.misi_dev(c0, y2, 0, return_signals=True)[1])
    _, _, _, gA, gS, gy = run(p, dev(A), dev(c0), dev(y), 0, None, dev(gs))
    assert not gA.any()
    gS, gy, g = f64(gS), f64(gy), gs.astype(np.float64)
    for b in range(B):
        if c0.shape[1] == 1:
            # one source gets the whole mixture back, s = x + (y - x): nothing depends on S, the difference is the rounding of that
            # sum alone and no scale for a relative bar; the gradient is zero exactly and the signals stay within their rounding
            x = [np.abs(p.istft(c[b, 0].astype(np.complex128))).max() for c in (c0, S2)]
            bound = 4 * 2.0 ** -24 * (2 * np.abs(y[b]).max() + x[0] + x[1])
            print("misi_grad %s b=%d adjoint in S, one source: |gS| %.2e, |ds| %.2e (rounding bound %.2e)"
                  % (gc.ident(key), b, np.abs(gS[b]).max(), np.abs(s_S[b] - s0[b]).max(), bound))
            assert not gS[b].any() and np.abs(s_S[b] - s0[b]).max() <= bound
        for name, lhs, rhs, ds in (("S", np.sum((s_S[b] - s0[b]) * g[b]), np.sum(np.real(np.conj(gS[b]) * dS[b])), s_S[b] - s0[b]),
                                   ("y", np.sum((s_y[b] - s0[b]) * g[b]), np.sum(gy[b] * dy[b]), s_y[b] - s0[b])):
            if name == "S" and c0.shape[1] == 1:
                continue
            scale = np.linalg.norm(ds) * np.linalg.norm(g[b])
            print("misi_grad %s b=%d adjoint in %s: <ds, gs> %.8e, <d, g> %.8e, apart %.2e of |ds||gs|"
                  % (gc.ident(key), b, name, lhs, rhs, abs(lhs - rhs) / scale))
            assert abs(lhs - rhs) <= 1e-4 * scale


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_teacher_forced_backward(key):
    """The device backward pass against the host one fed the device's own tape: the projections' arguments are the same numbers
    on both sides, so the bar is what the host pass moves when only its transforms are perturbed (three times that)."""
    p, A, c0, y, gC, gs = gc.case(*key)
    dA, dS, dY, dgC, dgs = (dev(a) for a in (A, c0, y, gC, gs))
    m = MARGINS.setdefault(key[:3], [0, 0.0, 0.0, 0.0, 0.0])
    for n in gc.STEPS:
        _, _, tape, gA, gS, gy = run(p, dA, dS, dY, n, dgC, dgs)
        args = (c0, y, p.fsize, p.fshift, p.awin, p.swin, n, A.astype(np.float64))
        kw = dict(grad_out=gC, grad_signals=gs, perfectrec=p.perfectrec, _tape=f64(tape))
        ref = lws_amd.misi_grad(*args, **kw)
        per = lws_amd.misi_grad(*args, _perturb=gc.perturbation(n + 29, kinds=("gc", "gv")), **kw)
        for name, got, r, q in zip(("gA", "gS", "gy"), (f64(gA), f64(gS), f64(gy)), ref, per):
            assert np.isfinite(got.view(np.float64)).all()
            for label, dist, bar in rows_of(name, got, r, q):
                if bar == 0 and name == "gA":
                    # one source: the share leaves nothing of gs or of an earlier step (gv - mean gv = 0 exactly), so gA is
                    # Re(conj(u) gC) per bin of the last step and no transform feeds it: nothing was perturbed and the bar above is
                    # no bar.  What is left is that product in float32: |X| by two multiplies, an add and a square root, u by a
                    # division, q by two multiplies and an add -- six roundings of 2^-24 of |gC| per entry at most, taken as eight
                    bar = 8 * 2.0 ** -24
                print("misi_grad %s n=%d teacher-forced %s: rel-L2 %.3e (bar %.3e)" % (gc.ident(key), n, label, dist, bar))
                m[4] = max(m[4], ratio(dist, bar))
                assert dist <= bar, (label, dist, bar)


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_matches_host(key):
    p, A, S, y, gC, gs = on_device(key)
    m = MARGINS.setdefault(key[:3], [0, 0.0, 0.0, 0.0, 0.0])
    for n in gc.STEPS:
        ref, per = gc.host(key, n)
        got = [f64(t) for t in run(p, A, S, y, n, gC, gs)[3:]]
        for name, g, r, q in zip(("gA", "gS", "gy"), got, ref, per):
            assert g.shape == r.shape and np.isfinite(g.view(np.float64)).all()
            for i, (label, dist, bar) in enumerate(rows_of(name, g, r, q)):
                far = gc.far(g.reshape((-1,) + g.shape[-2:])[i], r.reshape((-1,) + r.shape[-2:])[i]) if name == "gA" else 0.0
                print("misi_grad %s n=%d %s: rel-L2 %.3e (bar %.3e)%s"
                      % (gc.ident(key), n, label, dist, bar, "  far entries %.4f%%" % (100 * far) if name == "gA" else ""))
                m[0] += 1
                m[2], m[3] = max(m[2], ratio(dist, bar)), max(m[3], far)
                if name == "gA":
                    m[1] = max(m[1], dist)
                assert dist <= bar, (label, dist, bar)
                assert far <= gc.FAR_CAP, (label, far)


@pytest.mark.parametrize("K,n", [(2, 1), (1, 1), (1, 3)])
def test_zero_projection_convention(K, n):
    """The input of tests/test_misi_grad_host.py: y = 0 and S = 0 make every X of these runs exactly zero on the device too (the
    one source of K = 1 gets x + (0 - x) back), where the forward gives A + 0j: u = 1, gA = Re gc, gX = 0."""
    from test_misi_grad_host import zero_case
    p, A, S, y, gC, gs = zero_case(K)
    A, S, y, gC, gs = (dev(a[None].astype(np.complex64 if np.iscomplexobj(a) else np.float32)) for a in (A, S, y, gC, gs))
    C, s, tape, gA, gS, gy = run(p, A, S, y, n, gC, gs)
    entry = run(p, A, S, y, 0, gC, gs)
    assert not tape.abs().any() and torch.equal(C, A + 0j)
    print("misi_grad zero |X| K=%d n=%d: |gA - Re gc| %.2e, |gS| %.2e, |gy - entry| %.2e"
          % (K, n, (gA - entry[4].real).abs().max(), gS.abs().max(), (gy - entry[5]).abs().max()))
    assert all(torch.isfinite(torch.view_as_real(g) if g.is_complex() else g).all() for g in (gA, gS, gy))
    assert torch.equal(gA, entry[4].real) and not gS.abs().any() and torch.equal(gy, entry[5])


@pytest.mark.parametrize("key", [(64, 16, True, 12, 3), (1000, 250, True, 5, 2)], ids=gc.ident)
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A, S, y, gC, gs = on_device(key)
    n = 5
    first = run(p, A, S, y, n, gC, gs)
    again = run(p, A, S, y, n, gC, gs)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for want_S, want_y in ((False, False), (True, False), (False, True)):      # computing gS or gy, or not, does not change the rest
        part = run(p, A, S, y, n, gC, gs, want_S=want_S, want_y=want_y)
        assert torch.equal(part[3], first[3])
        assert part[4] is None if not want_S else torch.equal(part[4], first[4])
        assert part[5] is None if not want_y else torch.equal(part[5], first[5])
    for b in range(S.shape[0]):
        one = run(p, A[b:b + 1], S[b:b + 1], y[b:b + 1], n, gC[b:b + 1], gs[b:b + 1])
        assert all(torch.equal(a[0] if i != 2 else a[:, 0], f[b] if i != 2 else f[:, b]) for i, (a, f) in enumerate(zip(one, first)))
    only_C, only_s = run(p, A, S, y, n, gC, None), run(p, A, S, y, n, None, gs)  # a null cotangent is zeros
    zero_C, zero_s = run(p, A, S, y, n, torch.zeros_like(gC), gs), run(p, A, S, y, n, gC, torch.zeros_like(gs))
    assert all(torch.equal(a, b) for a, b in zip(only_C[3:], zero_s[3:])) and all(torch.equal(a, b) for a, b in zip(only_s[3:], zero_C[3:]))
    none = run(p, A, S, y, n, None, None)
    assert not any(g.abs().any() for g in none[3:])


def test_autograd_plumbing():
    key = (64, 16, True, 12, 3)
    p, A, S, y, gC, gs = on_device(key)
    keep = [t.clone() for t in (A, S, y)]
    for n in (3, 0):
        direct = run(p, A, S, y, n, gC, gs)
        for needs in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)):
            leaves = [t.clone().requires_grad_(r) for t, r in zip((A, S, y), needs)]
            C, s = p.misi_layer(*leaves, n)
            assert torch.equal(C, direct[0]) and torch.equal(s, direct[1]) and C.data_ptr() != leaves[1].data_ptr()
            loss = (gC.conj() * C).real.sum() + (gs * s).sum()
            loss.backward()
            for leaf, r, want, kept in zip(leaves, needs, direct[3:], keep):
                assert (leaf.grad is not None) == r and torch.equal(leaf.detach(), kept)
                if r:
                    assert leaf.grad.dtype == leaf.dtype and torch.equal(leaf.grad, want)
            with pytest.raises(RuntimeError, match="second time|already been freed"):
                loss.backward()
        if n == 0:
            assert torch.equal(direct[0], S) and not direct[3].any()
    # a loss on one of the results only, and spectrograms that are no stack
    a = A[1].clone().requires_grad_(True)
    C, s = p.misi_layer(a, S[1], y[1], 3)
    assert tuple(C.shape) == tuple(S.shape[1:]) and tuple(s.shape) == (S.shape[1], y.shape[1])
    (gs[1] * s).sum().backward()
    assert torch.equal(a.grad, run(p, A[1:2], S[1:2], y[1:2], 3, None, gs[1:2])[3][0])
    assert all(torch.equal(t, k) for t, k in zip((A, S, y), keep))
    # retain_graph keeps the tape: the same gradient twice
    a = A.clone().requires_grad_(True)
    C, s = p.misi_layer(a, S, y, 3)
    loss = (gs * s).sum()
    loss.backward(retain_graph=True)
    g1 = a.grad.clone()
    a.grad = None
    loss.backward()
    assert torch.equal(a.grad, g1)


def test_one_gradient_step_descends():
    """L = |s - s_true|^2 of one mixture after 3 iterations; A - eta gA with eta such that the first-order decrease is 1 % of L."""
    key = (64, 16, False, 9, 2)
    p, A, S, y, gC, gs = on_device(key)
    target = dev(gc.sources(*key)[0].astype(np.float32))
    a = A[0].clone().requires_grad_(True)
    C, s = p.misi_layer(a, S[0], y[0], 3)
    loss = ((s - target) ** 2).sum()
    loss.backward()
    eta = 0.01 * loss.item() / (a.grad.double() ** 2).sum().item()
    stepped = (a.detach() - eta * a.grad).contiguous()
    s2 = p.misi_dev(S[0], y[0], 3, magnitudes=stepped, return_signals=True)[1]
    after = ((s2 - target) ** 2).sum().item()
    print("misi_grad descent: L %.6e -> %.6e (%.3f%% down; first order predicts 1%%)" % (loss.item(), after, 100 * (1 - after / loss.item())))
    assert after < loss.item()


def test_invalid_arguments():
    p, A, S, y, gC, gs = on_device((64, 16, False, 9, 2))
    lib = capi.load()
    w = np.ascontiguousarray(p.awin, dtype=np.float64)
    B, K, T, F = S.shape
    C, tape = S.clone(), torch.zeros((2, B, K, T, F), dtype=torch.complex64, device=S.device)
    gA = torch.zeros_like(A)
    win = (w.ctypes.data, w.ctypes.data)
    # (tape, K, iterations, A) of the forward call; then the backward one
    for tp, k, iters, a in ((None, K, 2, A.data_ptr()), (tape.data_ptr(), 0, 2, A.data_ptr()), (tape.data_ptr(), K, -1, A.data_ptr()),
                            (tape.data_ptr(), K, 2, None)):
        rc = lib.lws_misi_tape_dev(0, C.data_ptr(), a, y.data_ptr(), B, k, T, 64, 16, *win, 0, iters, None, tp, None)
        assert rc == capi.LWS_ERR_INVALID, (tp, k, iters, a)
        rc = lib.lws_misi_backward_dev(0, gC.data_ptr(), gs.data_ptr(), a, tp, B, k, T, 64, 16, *win, 0, iters, gA.data_ptr(), None, None, None)
        assert rc == capi.LWS_ERR_INVALID, (tp, k, iters, a)
    rc = lib.lws_misi_backward_dev(0, gC.data_ptr(), gs.data_ptr(), A.data_ptr(), tape.data_ptr(), B, K, T, 64, 16, *win, 0, 2, None, None, None, None)
    assert rc == capi.LWS_ERR_INVALID                    # nowhere to put gA
    for fn_args in ((lib.lws_misi_tape_dev, (0, C.data_ptr(), A.data_ptr(), y.data_ptr(), B, K, 2, 64, 16) + win + (1, 1, None, tape.data_ptr(), None)),
                    (lib.lws_misi_backward_dev, (0, None, None, A.data_ptr(), tape.data_ptr(), B, K, 2, 64, 16) + win + (1, 1, gA.data_ptr(), None, None, None))):
        assert fn_args[0](*fn_args[1]) == capi.LWS_ERR_INVALID     # perfectrec does not keep two frames
    torch.cuda.synchronize()
    assert torch.equal(C, S) and not gA.any()
    q = lws_amd.lws(64, 16, perfectrec=True)
    with pytest.raises(ValueError):
        q.misi_layer(A[:, :, :2].contiguous(), S[:, :, :2].contiguous(), torch.zeros((3, 0), device=S.device), 1)
    with pytest.raises(ValueError):
        p.misi_layer(A, S, y, -1)
    with pytest.raises(ValueError):
        p.misi_layer(A[:, :, :-1], S, y, 2)
    with pytest.raises(ValueError):
        p.misi_layer(A, S, y[:, :-1], 2)
    with pytest.raises(ValueError):
        p.misi_layer(A, S, y[0], 2)                      # one mixture for a stack
    with pytest.raises(ValueError):
        p.misi_layer(A.double(), S, y, 2)
    with pytest.raises(ValueError):
        p.misi_layer(A.cpu(), S.cpu(), y.cpu(), 2)
    with pytest.raises(ValueError):
        p.misi_layer(A[0, 0], S[0, 0], y[0], 2)          # a 2-D S
    _, A_, c0, y_, gC_, gs_ = gc.case(64, 16, False, 9, 2)
    with pytest.raises(ValueError):                      # cotangents of the wrong shapes
        p.misi_grad(c0, y_, 2, A_, grad_out=gC_[:, :, :-1])
    with pytest.raises(ValueError):
        p.misi_grad(c0, y_, 2, A_, grad_signals=gs_[:, :, :-1])
    with pytest.raises(ValueError):
        p.misi_grad(c0, y_, 2, None)


def test_zz_margins_actually_achieved():
    """What the cases above reached, per shape (written to $LWS_MARGINS_DIR/misi_grad_margins.json when that variable names a
    directory; profiles/misi_grad_margins.json is a copy).  On an MI355X, 378 whole-run rows (gA, gS and gy per mixture and source at
    8 shapes and 3 step counts): rel-L2 of gA 7.0e-8 ... 1.9e-4, every row at most 9.2 % of its bar, no entry of gA beyond 1e-3 max|gA|;
    378 teacher-forced rows at most 2.7 % of their bar, the one-source rows of gA at most 11 % of their rounding bound; the adjoint
    identities within 3.1e-7 of |ds||gs|; the whole file in 3.3 s."""
    if not MARGINS:
        test_matches_host((64, 16, True, 12, 3))
        test_teacher_forced_backward((64, 16, True, 12, 3))
    MARGINS.report("misi_grad_margins.json")
    assert all(v[2] <= 1.0 and v[3] <= gc.FAR_CAP and v[4] <= 1.0 for v in MARGINS.values())
