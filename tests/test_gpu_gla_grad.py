"""GPU: the backward pass of (Fast) Griffin-Lim on the device (k_gla_bwd_* of lws_gla.hip, lws_amd.griffin_lim_layer) against the
host fp64 definition (lws_amd.griffin_lim_grad), and against the forward kernels themselves.

Inputs, cotangent, error model and host references are those of tests/gla_grad_cases.py.  As in tests/test_gpu_misi_grad.py the
value checks have no fixed tolerance: a bar is the rel-L2 distance the host fp64 pass moves under the error model, times 3,
measured here on the host side only; tests/test_gla_grad_host.py holds the model itself to the far-entry cap.  Distances, caps and
bars are taken per spectrogram, so that the small-scale members of a stack are held as tightly as the loud ones.  Every figure is
printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import lws_amd
import gla_grad_cases as gc
from gpu_grad_helpers import Margins, dev, f64, ptr, rows_of

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

capi = lws_amd._capi
# per (fsize, fshift, perfectrec): [rows, max rel-L2 of gA, max rel-L2 / bar of the whole run (gA, gS), max far fraction of gA,
# max rel-L2 / bar of the teacher-forced pass, max |lhs - rhs| / bar of the adjoint identity]
FIGURES = ("rows", "max_rel_l2_gA", "max_rel_l2_over_bar", "max_far_fraction_gA", "max_teacher_forced_rel_l2_over_bar",
           "max_adjoint_gap_over_bar")
MARGINS = Margins(FIGURES)
margins = MARGINS.row
RUNS = [(n, alpha) for n in gc.STEPS for alpha in gc.ALPHAS]


def run(p, A, S, n, alpha, gC, want_S=True):
    """lws_griffin_lim_tape_dev then lws_griffin_lim_backward_dev on device tensors (stacked): C, tape, gA, gS."""
    B, T, F = S.shape
    C, tape = S.clone(), torch.empty((n, B, T, F), dtype=torch.complex64, device=S.device)
    capi.griffin_lim_tape_dev(C.data_ptr(), A.data_ptr(), B, T, p.fsize, p.fshift, p.awin, p.swin, p.perfectrec, n, alpha,
                              ptr(tape) if n else None)
    gA = torch.full(A.shape, float("nan"), dtype=torch.float32, device=S.device)
    gS = torch.full(S.shape, float("nan"), dtype=torch.complex64, device=S.device) if want_S else None
    capi.griffin_lim_backward_dev(ptr(gC), A.data_ptr(), ptr(tape) if n else None, B, T, p.fsize, p.fshift, p.awin, p.swin,
                                  p.perfectrec, n, alpha, gA.data_ptr(), ptr(gS))
    return C, tape, gA, gS


class Cases:
    """Where the checks below take their inputs, host references, error model, forward calls and record from: tests/gla_grad_cases.py,
    the plan's default windows, the methods of the plan.  tests/test_gpu_windows_grad.py runs the same checks from the window pairs of
    tests/window_cases.py through the module-level calls."""
    tag = "gla_grad"
    ident = staticmethod(gc.ident)
    host = staticmethod(gc.host)                          # (key, n, alpha) -> ((gA, gS), the same under the error model)

    @staticmethod
    def case(key):
        return gc.case(*key)                              # p, A, c0, gC

    @staticmethod
    def grad(key, n, alpha, **kw):
        p, A, c0, gC = gc.case(*key)
        return lws_amd.griffin_lim_grad(c0, p.fsize, p.fshift, p.awin, p.swin, n, A.astype(np.float64), alpha=alpha, grad_out=gC,
                                        perfectrec=p.perfectrec, **kw)

    @staticmethod
    def transform_model(seed):
        return gc.perturbation(seed, kinds=("gc", "gv"))

    @staticmethod
    def forward(p, A, S, n, alpha):
        return p.griffin_lim_dev(S, n, alpha=alpha, magnitudes=A), p.griffin_lim_layer(A, S, n, alpha=alpha)

    @staticmethod
    def seen(A):
        """(B, T) bool, the frames gA is compared on, or None for all of them: every frame of these cases sounds."""
        assert A.any(axis=-1).all()
        return None

    note = staticmethod(MARGINS.note)             # (key, rows=0, **figures): count rows, keep the largest of each figure


def on_device(key, src=Cases):
    p, A, c0, gC = src.case(key)
    return (p,) + tuple(dev(a) for a in (A, c0, gC))


def check_bits(key, n, alpha, src=Cases):
    """The tape call and the layer give the bits of griffin_lim_dev, and the last tape entry projected in fp64 is C."""
    p, A, S, gC = on_device(key, src)
    top = f64(A).max(axis=(1, 2))
    want, C = src.forward(p, A, S, n, alpha)
    C2, tape = run(p, A, S, n, alpha, None)[:2]
    assert C.dtype == torch.complex64 and torch.equal(C, want) and torch.equal(C2, want)
    X, a = f64(tape[n - 1]), f64(A)
    mag = np.abs(X)
    proj = np.where(mag > 0, a * X / np.where(mag > 0, mag, 1.0), a + 0j)
    off = (np.abs(proj - f64(C)).max(axis=(1, 2)) / top).max()
    print("%s %s n=%d alpha=%g: same bits as griffin_lim_dev; the last tape entry projected in fp64 is within %.2e max A "
          "of C" % (src.tag, src.ident(key), n, alpha, off))
    assert off <= 2e-6
    return tape


def check_teacher_forced(key, n, alpha, src=Cases):
    """The device backward pass against the host one fed the device's own tape: the projections' arguments are the same numbers
    on both sides, so the bar is what the host pass moves when only its transforms are perturbed (three times that)."""
    p, A, c0, gC = src.case(key)
    seen = src.seen(A.astype(np.float64))
    _, tape, gA, gS = run(p, dev(A), dev(c0), n, alpha, dev(gC))
    kw = dict(_tape=f64(tape))
    ref = src.grad(key, n, alpha, **kw)
    per = src.grad(key, n, alpha, _perturb=src.transform_model(n + 29), **kw)
    for name, got, r, q in zip(("gA", "gS"), (f64(gA), f64(gS)), ref, per):
        assert np.isfinite(got.view(np.float64)).all()
        for b, (label, dist, bar) in enumerate(rows_of(name, got, r, q, seen if name == "gA" else None)):
            if bar == 0 and name == "gA":
                # one step: gA is Re(conj(u) gOut) per bin and no transform feeds it: nothing was perturbed and the bar above is
                # no bar.  What is left is that product in float32: |X| by two multiplies, an add and a square root, u by a
                # division, q by two multiplies and an add -- six roundings of 2^-24 of |gOut| per entry at most, taken as
                # eight, relative to |gA| of the spectrogram (both norms over the frames compared)
                assert n == 1
                on = slice(None) if seen is None else seen[b]
                bar = 8 * 2.0 ** -24 * np.linalg.norm(gC[b][on].astype(np.complex128)) / np.linalg.norm(r[b][on])
            print("%s %s n=%d alpha=%g teacher-forced %s: rel-L2 %.3e (bar %.3e)" % (src.tag, src.ident(key), n, alpha, label, dist, bar))
            src.note(key, max_teacher_forced_rel_l2_over_bar=dist / bar)
            assert dist <= bar, (label, dist, bar)


def check_whole_run(key, n, alpha, src=Cases):
    p, A, S, gC = on_device(key, src)
    ref, per = src.host(key, n, alpha)
    seen = src.seen(f64(A))
    got = [f64(t) for t in run(p, A, S, n, alpha, gC)[2:]]
    for name, g, r, q in zip(("gA", "gS"), got, ref, per):
        assert g.shape == r.shape and np.isfinite(g.view(np.float64)).all()
        on = seen if name == "gA" else None
        for b, (label, dist, bar) in enumerate(rows_of(name, g, r, q, on)):
            far = (gc.far(g[b], r[b]) if on is None else gc.far(g[b][on[b]], r[b][on[b]])) if name == "gA" else 0.0
            print("%s %s n=%d alpha=%g %s: rel-L2 %.3e (bar %.3e)%s"
                  % (src.tag, src.ident(key), n, alpha, label, dist, bar, "  far entries %.4f%%" % (100 * far) if name == "gA" else ""))
            src.note(key, rows=1, max_rel_l2_over_bar=dist / bar, max_far_fraction_gA=far, **({"max_rel_l2_gA": dist} if name == "gA" else {}))
            assert dist <= bar, (label, dist, bar)
            assert far <= gc.FAR_CAP, (label, far)


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_same_bits_as_griffin_lim_dev(key):
    for n, alpha in RUNS:
        check_bits(key, n, alpha)


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_adjoint_of_the_forward_kernels(key):
    """n = 1, alpha = 0: Re <C(S + d/2) - C(S - d/2), gOut> against Re <d, gS>, the difference taken from the forward kernels' own
    float32 outputs and the inner products in fp64 on the host.  One step is not affine in S, so the bar, relative to |dC| |gOut|,
    is worked out on the host for the same d and has three parts: what the centred difference of the fp64 host forward itself
    leaves (its truncation), what the error model of tests/gla_grad_cases.py moves the two host forward results by (three times
    that, times |gOut|: Cauchy-Schwarz), and what it moves the host gS by (three times that, times |d|).  d is 0.02 of the rms of
    S: the rounding of C, 1e-7 of C, stays 1e-5 of the difference."""
    p, A, c0, gC = gc.case(*key)
    rng = np.random.default_rng(11)
    B = c0.shape[0]
    rms = np.sqrt(np.mean(np.abs(c0) ** 2, axis=(1, 2), keepdims=True))
    half = 0.01 * rms * (rng.standard_normal(c0.shape) + 1j * rng.standard_normal(c0.shape)) / np.sqrt(2)
    Sp, Sm = (c0 + half).astype(np.complex64), (c0 - half).astype(np.complex64)
    d = Sp.astype(np.complex128) - Sm
    a64, g = A.astype(np.float64), gC.astype(np.complex128)
    Cp, Cm = (f64(p.griffin_lim_dev(s, 1, alpha=0.0, magnitudes=dev(A))) for s in (Sp, Sm))
    gS = f64(run(p, dev(A), dev(c0), 1, 0.0, dev(gC))[3])
    hp, hm = (p.griffin_lim(s, 1, alpha=0.0, magnitudes=a64) for s in (Sp, Sm))
    model = lambda seed: (lambda i, b, X: gc.perturbation(seed + b, kinds=('X',))('X', i, b, X))
    pp, pm = (lws_amd.griffin_lim(s, p.fsize, p.fshift, p.awin, p.swin, 1, alpha=0.0, magnitudes=a64, perfectrec=p.perfectrec,
                                  _perturb=model(seed)) for s, seed in ((Sp, 41), (Sm, 47)))
    ref, per = gc.host(key, 1, 0.0)
    m = margins(key)
    for b in range(B):
        inner = lambda x, y: np.sum(np.real(np.conj(y) * x))
        lhs, rhs = inner(Cp[b] - Cm[b], g[b]), inner(d[b], gS[b])
        scale = np.linalg.norm(hp[b] - hm[b]) * np.linalg.norm(g[b])
        trunc = abs(inner(hp[b] - hm[b], g[b]) - inner(d[b], ref[1][b]))
        fwd = 3 * (np.linalg.norm(pp[b] - hp[b]) + np.linalg.norm(pm[b] - hm[b])) * np.linalg.norm(g[b])
        bwd = 3 * np.linalg.norm(per[1][b] - ref[1][b]) * np.linalg.norm(d[b])
        bar = (trunc + fwd + bwd) / scale
        print("gla_grad %s b=%d adjoint in S: <dC, gOut> %.8e, <d, gS> %.8e, apart %.2e of |dC||gOut| (bar %.2e: truncation %.2e, "
              "forward %.2e, backward %.2e)" % (gc.ident(key), b, lhs, rhs, abs(lhs - rhs) / scale, bar, trunc / scale, fwd / scale,
                                                bwd / scale))
        m[5] = max(m[5], abs(lhs - rhs) / scale / bar)
        assert abs(lhs - rhs) <= bar * scale


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_teacher_forced_backward(key):
    for n, alpha in RUNS:
        check_teacher_forced(key, n, alpha)


@pytest.mark.parametrize("key", gc.GPU_SHAPES, ids=gc.ident)
def test_matches_host(key):
    for n, alpha in RUNS:
        check_whole_run(key, n, alpha)


def test_zero_projection_convention():
    """The input of tests/test_gla_grad_host.py: S = 0 makes every X of step 1 exactly zero on the device too, where the forward
    gives A + 0j: u = 1, gA = Re gt, gX = 0."""
    from test_gla_grad_host import zero_case
    p, A, S, gC = zero_case()
    A, S, gC = (dev(a[None].astype(np.complex64 if np.iscomplexobj(a) else np.float32)) for a in (A, S, gC))
    C, tape, gA, gS = run(p, A, S, 1, 0.99, gC)
    assert not tape.abs().any() and torch.equal(C, A + 0j)
    print("gla_grad zero |X| n=1: |gA - Re gt| %.2e, |gS| %.2e" % ((gA - gC.real).abs().max(), gS.abs().max()))
    assert torch.equal(gA, gC.real) and not gS.abs().any()
    for n in (3, 5):                                     # later steps have arguments of their own; the start still gets nothing
        C, tape, gA, gS = run(p, A, S, n, 0.99, gC)
        assert not tape[0].abs().any() and torch.isfinite(gA).all() and not gS.abs().any()


@pytest.mark.parametrize("key", [(64, 16, True, 12), (1000, 250, True, 5)], ids=gc.ident)
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A, S, gC = on_device(key)
    n, alpha = 5, 0.99
    first = run(p, A, S, n, alpha, gC)
    again = run(p, A, S, n, alpha, gC)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    part = run(p, A, S, n, alpha, gC, want_S=False)       # leaving gS out does not change gA
    assert part[3] is None and torch.equal(part[2], first[2])
    for b in range(S.shape[0]):
        one = run(p, A[b:b + 1], S[b:b + 1], n, alpha, gC[b:b + 1])
        assert all(torch.equal(a[0] if i != 1 else a[:, 0], f[b] if i != 1 else f[:, b]) for i, (a, f) in enumerate(zip(one, first)))
    none, zero = run(p, A, S, n, alpha, None), run(p, A, S, n, alpha, torch.zeros_like(gC))   # a null cotangent is zeros
    assert all(torch.equal(a, b) for a, b in zip(none[2:], zero[2:])) and not any(g.abs().any() for g in none[2:])
    plain = run(p, A, S, n, 0.0, gC)                      # the momentum is in the gradient
    assert not torch.equal(plain[2], first[2])


def test_autograd_plumbing():
    key = (64, 16, True, 12)
    p, A, S, gC = on_device(key)
    keep = [t.clone() for t in (A, S)]
    for n in (5, 0):
        direct = run(p, A, S, n, 0.99, gC)
        for needs in ((True, True), (True, False), (False, True)):
            leaves = [t.clone().requires_grad_(r) for t, r in zip((A, S), needs)]
            C = p.griffin_lim_layer(*leaves, n)
            assert torch.equal(C, direct[0]) and C.data_ptr() != leaves[1].data_ptr()
            loss = (gC.conj() * C).real.sum()
            loss.backward()
            for leaf, r, want, kept in zip(leaves, needs, direct[2:], keep):
                assert (leaf.grad is not None) == r and torch.equal(leaf.detach(), kept)
                if r:
                    assert leaf.grad.dtype == leaf.dtype and torch.equal(leaf.grad, want)
            with pytest.raises(RuntimeError, match="second time|already been freed"):
                loss.backward()
        if n == 0:
            assert torch.equal(direct[0], S) and not direct[2].any() and torch.equal(direct[3], gC)
    # a spectrogram that is no stack, the module's function, and alpha = 0
    a = A[1].clone().requires_grad_(True)
    C = lws_amd.griffin_lim_layer(a, S[1], p.fsize, p.fshift, p.awin, p.swin, 3, alpha=0.0, perfectrec=p.perfectrec)
    assert tuple(C.shape) == tuple(S.shape[1:])
    (gC[1].conj() * C).real.sum().backward()
    assert torch.equal(a.grad, run(p, A[1:2], S[1:2], 3, 0.0, gC[1:2])[2][0])
    assert all(torch.equal(t, k) for t, k in zip((A, S), keep))
    # retain_graph keeps the tape: the same gradient twice
    a = A.clone().requires_grad_(True)
    loss = (gC.conj() * p.griffin_lim_layer(a, S, 3)).real.sum()
    loss.backward(retain_graph=True)
    g1 = a.grad.clone()
    a.grad = None
    loss.backward()
    assert torch.equal(a.grad, g1)


def test_one_gradient_step_descends():
    """L = |C - C_true|^2 of one spectrogram after 5 steps with momentum; A - eta gA with eta such that the first-order decrease is
    1 % of L.  The loss is quadratic in C and the step moves A by a fraction of a per cent, so the second-order share is a small
    part of the first: the decrease is held to between half and one and a half times the prediction."""
    key = (64, 16, False, 9)
    p, A, S, gC = on_device(key)
    target = dev(gc.truth(*key)[0].astype(np.complex64))
    a = A[0].clone().requires_grad_(True)
    C = p.griffin_lim_layer(a, S[0], 5)
    loss = ((C - target).abs() ** 2).sum()
    loss.backward()
    eta = 0.01 * loss.item() / (a.grad.double() ** 2).sum().item()
    stepped = (a.detach() - eta * a.grad).contiguous()
    C2 = p.griffin_lim_dev(S[0], 5, magnitudes=stepped)
    after = ((C2 - target).abs() ** 2).sum().item()
    down = 100 * (1 - after / loss.item())
    print("gla_grad descent: L %.6e -> %.6e (%.3f%% down; first order predicts 1%%)" % (loss.item(), after, down))
    assert 0.5 <= down <= 1.5


def test_invalid_arguments():
    p, A, S, gC = on_device((64, 16, False, 9))
    lib = capi.load()
    w = np.ascontiguousarray(p.awin, dtype=np.float64)
    B, T, F = S.shape
    C, tape = S.clone(), torch.zeros((2, B, T, F), dtype=torch.complex64, device=S.device)
    gA = torch.zeros_like(A)
    win = (w.ctypes.data, w.ctypes.data)
    # (tape, iterations, alpha, A) of the forward call; then the backward one
    for tp, iters, alpha, a in ((None, 2, 0.5, A.data_ptr()), (tape.data_ptr(), -1, 0.5, A.data_ptr()), (tape.data_ptr(), 2, 1.0, A.data_ptr()),
                                (tape.data_ptr(), 2, -0.1, A.data_ptr()), (tape.data_ptr(), 2, 0.5, None)):
        rc = lib.lws_griffin_lim_tape_dev(0, C.data_ptr(), a, B, T, 64, 16, *win, 0, iters, alpha, tp, None)
        assert rc == capi.LWS_ERR_INVALID, (tp, iters, alpha, a)
        rc = lib.lws_griffin_lim_backward_dev(0, gC.data_ptr(), a, tp, B, T, 64, 16, *win, 0, iters, alpha, gA.data_ptr(), None, None)
        assert rc == capi.LWS_ERR_INVALID, (tp, iters, alpha, a)
    rc = lib.lws_griffin_lim_backward_dev(0, gC.data_ptr(), A.data_ptr(), tape.data_ptr(), B, T, 64, 16, *win, 0, 2, 0.5, None, None, None)
    assert rc == capi.LWS_ERR_INVALID                    # nowhere to put gA
    for fn_args in ((lib.lws_griffin_lim_tape_dev, (0, C.data_ptr(), A.data_ptr(), B, 2, 64, 16) + win + (1, 1, 0.5, tape.data_ptr(), None)),
                    (lib.lws_griffin_lim_backward_dev, (0, None, A.data_ptr(), tape.data_ptr(), B, 2, 64, 16) + win + (1, 1, 0.5, gA.data_ptr(), None, None))):
        assert fn_args[0](*fn_args[1]) == capi.LWS_ERR_INVALID     # perfectrec does not keep two frames
    torch.cuda.synchronize()
    assert torch.equal(C, S) and not gA.any()
    q = lws_amd.lws(64, 16, perfectrec=True)
    with pytest.raises(ValueError, match="round trip"):
        q.griffin_lim_layer(A[:, :2].contiguous(), S[:, :2].contiguous(), 1)
    with pytest.raises(ValueError):
        p.griffin_lim_layer(A, S, -1)
    with pytest.raises(ValueError):
        p.griffin_lim_layer(A, S, 2, alpha=1.0)
    with pytest.raises(ValueError):
        p.griffin_lim_layer(A[:, :-1], S, 2)
    with pytest.raises(ValueError):
        p.griffin_lim_layer(A[:, :, :-1].contiguous(), S[:, :, :-1].contiguous(), 2)
    with pytest.raises(ValueError):
        p.griffin_lim_layer(A.double(), S, 2)
    with pytest.raises(ValueError):
        p.griffin_lim_layer(A.cpu(), S.cpu(), 2)
    with pytest.raises(ValueError):
        p.griffin_lim_layer(A[0, 0], S[0, 0], 2)          # a 1-D S


def test_zz_margins_actually_achieved():
    """What the cases above reached, per shape (written to $LWS_MARGINS_DIR/gla_grad_margins.json when that variable names a
    directory; profiles/gla_grad_margins.json is a copy).  On an MI355X, 504 whole-run rows (gA and gS per spectrogram at 14 shapes,
    3 step counts and 2 momenta): rel-L2 of gA 7.2e-8 ... 1.5e-5, every row at most 9.6 % of its bar, no entry of gA beyond 1e-3 max|gA|;
    504 teacher-forced rows at most 9.7 % of their bar (the n = 1 rows of gA, of their rounding bound); the adjoint identity at most
    19 % of its bar (at hop = N; 11 % on the shapes before it); the six shapes added last -- (512, 128), (600, 150), N = 36, hop = 1,
    hop = N -- at most 3.2 % whole-run and 8.3 % teacher-forced; the whole file in 3.7 s."""
    if not MARGINS:
        test_matches_host((64, 16, True, 12))
        test_teacher_forced_backward((64, 16, True, 12))
        test_adjoint_of_the_forward_kernels((64, 16, True, 12))
    MARGINS.report("gla_grad_margins.json")
    assert all(v[2] <= 1.0 and v[3] <= gc.FAR_CAP and v[4] <= 1.0 and v[5] <= 1.0 for v in MARGINS.values())
