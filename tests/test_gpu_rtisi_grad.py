"""GPU: the backward pass of RTISI-LA on the device (k_rtisi_tape, k_rtisi_bwd of lws_gla.hip, lws_amd.rtisi_la_layer) against the
host fp64 definition (lws_amd.rtisi_la_grad), and against the forward kernel itself.

Inputs, cotangents, error model and host references are those of tests/rtisi_grad_cases.py.  As in tests/test_gpu_gla_grad.py the
value checks have no fixed tolerance: a bar is the rel-L2 distance the host fp64 pass moves under the error model, times 3,
measured here on the host side only; tests/test_rtisi_grad_host.py holds the model itself to the far-entry cap.  Distances, caps
and bars are taken per spectrogram, so that the small-scale members of a stack are held as tightly as the loud ones.  Every case
has at most 12 frames.  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import lws_amd
import rtisi_grad_cases as rc
from gpu_grad_helpers import Margins, dev, f64, ptr, rows_of

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

capi = lws_amd._capi
# per (fsize, fshift, perfectrec): [rows, max rel-L2 of gA, max rel-L2 / bar of the whole run (gA, gS), max far fraction of gA,
# max rel-L2 / bar of the teacher-forced pass, max rel-L2 / bar of the tape]
FIGURES = ("rows", "max_rel_l2_gA", "max_rel_l2_over_bar", "max_far_fraction_gA", "max_teacher_forced_rel_l2_over_bar",
           "max_tape_rel_l2_over_bar")
MARGINS = Margins(FIGURES)
# (fsize, fshift, perfectrec, T): [(look-ahead, iterations, backward state in LDS)] -- both placements of k_rtisi_bwd, asserted
# through lws_rtisi_la_bwd_placement; the table is with the cases, where the host tests read it too
PLACEMENTS = rc.PLACEMENTS


def run(p, A, S, LA, n, gC, gx, want_S=True):
    """lws_rtisi_la_tape_dev then lws_rtisi_la_backward_dev on device tensors (stacked): C, x, tape, gA, gS.  The tape starts as
    zeros: the rows no frame has stay zero."""
    B, T, F = S.shape
    length = capi.istft_length(T, p.fsize, p.fshift, p.perfectrec)
    C, x = S.clone(), torch.empty((B, length), dtype=torch.float32, device=S.device)
    tape = torch.zeros((B, T, n, min(LA, T - 1) + 1, F), dtype=torch.complex64, device=S.device)
    capi.rtisi_la_tape_dev(C.data_ptr(), A.data_ptr(), x.data_ptr(), B, T, p.fsize, p.fshift, p.awin, p.swin, p.perfectrec, n, LA,
                           ptr(tape) if n else None)
    gA = torch.full(A.shape, float("nan"), dtype=torch.float32, device=S.device)
    gS = torch.full(S.shape, float("nan"), dtype=torch.complex64, device=S.device) if want_S else None
    capi.rtisi_la_backward_dev(ptr(gC), ptr(gx), A.data_ptr(), ptr(tape) if n else None, B, T, p.fsize, p.fshift, p.awin, p.swin,
                               p.perfectrec, n, LA, gA.data_ptr(), ptr(gS))
    return C, x, tape, gA, gS


class Cases:
    """Where the checks below take their inputs, host references, error model and record from: tests/rtisi_grad_cases.py, the plan's
    default windows.  tests/test_gpu_windows_grad.py runs the same checks from the window pairs of tests/window_cases.py."""
    tag = "rtisi_grad"
    ident = staticmethod(rc.ident)
    host = staticmethod(rc.host)                          # (key, LA, n) -> ((gA, gS), the same under the error model)
    grad = staticmethod(rc.grad)                          # (key, LA, n, **kw) -> (gA, gS) of lws_amd.rtisi_la_grad
    host_tape = staticmethod(rc.host_tape)                # (key, LA, n, perturbed=False)

    note = staticmethod(MARGINS.note)             # (key, rows=0, **figures): count rows, keep the largest of each figure

    @staticmethod
    def case(key):
        return rc.case(*key)                              # p, A, c0, gC, gx

    @staticmethod
    def transform_model(seed):
        return rc.perturbation(seed, kinds=("gc", "gv"))

    @staticmethod
    def seen(A):
        """(B, T) bool, the frames gA is compared on, or None for all of them: every frame of these cases sounds."""
        assert A.any(axis=-1).all()
        return None


def on_device(key, src=Cases):
    p, A, c0, gC, gx = src.case(key)
    return (p,) + tuple(dev(a) for a in (A, c0, gC, gx))


def check_whole_run(key, LA, n, src=Cases):
    p, A, S, gC, gx = on_device(key, src)
    ref, per = src.host(key, LA, n)
    seen = src.seen(f64(A))
    got = [f64(t) for t in run(p, A, S, LA, n, gC, gx)[3:]]
    for name, g, r, q in zip(("gA", "gS"), got, ref, per):
        assert g.shape == r.shape and np.isfinite(g.view(np.float64)).all()
        on = seen if name == "gA" else None
        for b, (label, dist, bar) in enumerate(rows_of(name, g, r, q, on)):
            far = (rc.far(g[b], r[b]) if on is None else rc.far(g[b][on[b]], r[b][on[b]])) if name == "gA" else 0.0
            print("%s %s LA=%d n=%d %s: rel-L2 %.3e (bar %.3e)%s"
                  % (src.tag, src.ident(key), LA, n, label, dist, bar, "  far entries %.4f%%" % (100 * far) if name == "gA" else ""))
            src.note(key, rows=1, max_rel_l2_over_bar=dist / bar, max_far_fraction_gA=far, **({"max_rel_l2_gA": dist} if name == "gA" else {}))
            assert dist <= bar, (label, dist, bar)
            assert far <= rc.FAR_CAP, (label, far)


def check_teacher_forced(key, LA, n, src=Cases):
    """The device backward pass against the host one fed the device's own tape: the projections' arguments are the same numbers
    on both sides, so the bar is what the host pass moves when only its transforms are perturbed (three times that)."""
    p, A, c0, gC, gx = src.case(key)
    seen = src.seen(A.astype(np.float64))
    _, _, tape, gA, gS = run(p, dev(A), dev(c0), LA, n, dev(gC), dev(gx))
    kw = dict(_tape=f64(tape))
    ref = src.grad(key, LA, n, **kw)
    per = src.grad(key, LA, n, _perturb=src.transform_model(n + 29 + 100 * LA), **kw)
    for name, got, r, q in zip(("gA", "gS"), (f64(gA), f64(gS)), ref, per):
        assert np.isfinite(got.view(np.float64)).all()
        for label, dist, bar in rows_of(name, got, r, q, seen if name == "gA" else None):
            print("%s %s LA=%d n=%d teacher-forced %s: rel-L2 %.3e (bar %.3e)" % (src.tag, src.ident(key), LA, n, label, dist, bar))
            src.note(key, max_teacher_forced_rel_l2_over_bar=dist / bar)
            assert dist <= bar, (label, dist, bar)


def check_tape(key, LA, n, src=Cases):
    """The device tape against the host's X, per spectrogram, held to the bar of tests/test_gpu_rtisi.py: three times what the host's
    own projection arguments move under the error model.  The rows of no frame are as the caller left them."""
    p, A, S, gC, gx = on_device(key, src)
    tape = f64(run(p, A, S, LA, n, None, None, want_S=False)[2])
    ref, per = src.host_tape(key, LA, n), src.host_tape(key, LA, n, perturbed=True)
    T = S.shape[1]
    for mm in range(T):
        assert not tape[:, mm, :, min(mm + LA, T - 1) - mm + 1:].any()
    for label, dist, bar in rows_of("tape", tape, ref, per):
        print("%s %s LA=%d n=%d %s: rel-L2 %.3e (bar %.3e)" % (src.tag, src.ident(key), LA, n, label, dist, bar))
        src.note(key, max_tape_rel_l2_over_bar=dist / bar)
        assert dist <= bar, (label, dist, bar)


@pytest.mark.parametrize("key", rc.GPU_SHAPES, ids=rc.ident)
def test_same_bits_as_rtisi_la_dev(key):
    p, A, S, gC, gx = on_device(key)
    keep = [t.clone() for t in (A, S)]
    for LA, n in rc.LA_STEPS + [(3, 0)]:
        want, want_x = p.rtisi_la_dev(S, n, look_ahead=LA, magnitudes=A, return_signal=True)
        C, x = p.rtisi_la_layer(A, S, n, look_ahead=LA, return_signal=True)
        only = p.rtisi_la_layer(A, S, n, look_ahead=LA)
        C2, x2 = run(p, A, S, LA, n, None, None, want_S=False)[:2]
        assert C.dtype == torch.complex64 and x.dtype == torch.float32 and tuple(x.shape) == tuple(want_x.shape)
        assert torch.equal(C, want) and torch.equal(x, want_x) and torch.equal(only, want)
        assert torch.equal(C2, want) and torch.equal(x2, want_x)
        assert C.data_ptr() != S.data_ptr() and all(torch.equal(t, k) for t, k in zip((A, S), keep))


@pytest.mark.parametrize("key", rc.GPU_SHAPES, ids=rc.ident)
def test_tape_matches_host(key):
    for LA, n in rc.LA_STEPS:
        check_tape(key, LA, n)


@pytest.mark.parametrize("key", rc.GPU_SHAPES, ids=rc.ident)
def test_matches_host(key):
    for LA, n in rc.LA_STEPS:
        check_whole_run(key, LA, n)


@pytest.mark.parametrize("key", rc.GPU_SHAPES, ids=rc.ident)
def test_teacher_forced_backward(key):
    for LA, n in rc.LA_STEPS:
        check_teacher_forced(key, LA, n)


@pytest.mark.parametrize("key", sorted(PLACEMENTS), ids=rc.ident)
def test_both_placements(key):
    for LA, n, in_lds in PLACEMENTS[key]:
        got = capi.rtisi_la_bwd_placement(key[0], key[1], min(LA, key[3] - 1))
        print("rtisi_grad placement %s LA=%d: backward state in %s, %d threads, %d bytes of dynamic LDS"
              % (rc.ident(key), LA, "LDS" if got[0] else "scratch", got[1], got[2]))
        assert got[:2] == (in_lds, 1024), (key, LA, got)
        assert got[2] <= 160 * 1024
        check_tape(key, LA, n)
        check_whole_run(key, LA, n)
        check_teacher_forced(key, LA, n)


def test_zero_iterations():
    key = (64, 16, True, 12)
    p, A, S, gC, gx = on_device(key)
    C, x, _, gA, gS = run(p, A, S, 3, 0, gC, gx)
    ref = rc.grad(key, 3, 0)
    d = max(rc.rel(f64(gS)[b], ref[1][b]) for b in range(S.shape[0]))
    print("rtisi_grad n=0: gS off gC + adjoint of istft by %.2e" % d)
    assert torch.equal(C, S) and not gA.any() and d <= 1e-6
    assert torch.equal(run(p, A, S, 3, 0, gC, None)[4], gC)                 # the start is the result


@pytest.mark.parametrize("key", [(64, 16, True, 12), (1000, 250, True, 5), (4096, 1024, False, 6)], ids=rc.ident)
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A, S, gC, gx = on_device(key)
    LA, n = (5, 2) if key[0] == 4096 else (3, 3)
    first = run(p, A, S, LA, n, gC, gx)
    again = run(p, A, S, LA, n, gC, gx)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    part = run(p, A, S, LA, n, gC, gx, want_S=False)      # leaving gS out does not change gA
    assert part[4] is None and torch.equal(part[3], first[3])
    for b in range(S.shape[0]):
        one = run(p, A[b:b + 1], S[b:b + 1], LA, n, gC[b:b + 1], gx[b:b + 1])
        assert all(torch.equal(a[0], f[b]) for a, f in zip(one, first))
    none, zero = run(p, A, S, LA, n, None, None), run(p, A, S, LA, n, torch.zeros_like(gC), torch.zeros_like(gx))
    assert all(torch.equal(a, b) for a, b in zip(none[3:], zero[3:])) and not any(g.abs().any() for g in none[3:])   # zeros give zeros
    only_c, only_x = run(p, A, S, LA, n, gC, None), run(p, A, S, LA, n, None, gx)
    assert not torch.equal(only_c[3], first[3]) and not torch.equal(only_x[3], first[3])     # both cotangents reach the gradient


def test_autograd_plumbing():
    key = (64, 16, True, 12)
    p, A, S, gC, gx = on_device(key)
    keep = [t.clone() for t in (A, S)]
    for n in (3, 0):
        for with_c, with_x in ((True, True), (True, False), (False, True)):
            direct = run(p, A, S, 3, n, gC if with_c else None, gx if with_x else None)
            for needs in ((True, True), (True, False), (False, True)):
                leaves = [t.clone().requires_grad_(r) for t, r in zip((A, S), needs)]
                C, x = p.rtisi_la_layer(*leaves, n, look_ahead=3, return_signal=True)
                assert torch.equal(C, direct[0]) and torch.equal(x, direct[1])
                loss = 0
                if with_c:
                    loss = loss + (gC.conj() * C).real.sum()
                if with_x:
                    loss = loss + (gx * x).sum()
                loss.backward()
                for leaf, r, want, kept in zip(leaves, needs, direct[3:], keep):
                    assert (leaf.grad is not None) == r and torch.equal(leaf.detach(), kept)
                    if r:
                        assert leaf.grad.dtype == leaf.dtype and torch.equal(leaf.grad, want)
                with pytest.raises(RuntimeError, match="second time|already been freed"):
                    loss.backward()
    # a spectrogram that is no stack, the module's function, a loss on C alone through the single return
    a = A[1].clone().requires_grad_(True)
    C = lws_amd.rtisi_la_layer(a, S[1], p.fsize, p.fshift, p.awin, p.swin, 2, look_ahead=2, perfectrec=p.perfectrec)
    assert tuple(C.shape) == tuple(S.shape[1:])
    (gC[1].conj() * C).real.sum().backward()
    assert torch.equal(a.grad, run(p, A[1:2], S[1:2], 2, 2, gC[1:2], None)[3][0])
    assert all(torch.equal(t, k) for t, k in zip((A, S), keep))
    # the plan's look-ahead is the default
    assert torch.equal(p.rtisi_la_layer(A, S, 2), p.rtisi_la_layer(A, S, 2, look_ahead=p.look_ahead))


def test_causality_is_exact():
    """The host test's case: LA = 3, n = 3, T = 9, cotangents on the frames 0..2 and the samples they finalise only."""
    p, A, S, gC, gx = on_device((64, 16, False, 9))
    gC, gx = gC.clone(), gx.clone()
    gC[:, 3:] = 0
    gx[:, 3 * 16:] = 0
    for c, x in ((gC, None), (None, gx), (gC, gx)):
        gA, gS = run(p, A, S, 3, 3, c, x)[3:]
        assert not gA[:, 6:].any() and not gS[:, 6:].abs().any()
        assert all(gA[b, m].any() and gS[b, m].abs().any() for b in range(S.shape[0]) for m in range(6))


def test_invalid_arguments():
    p, A, S, gC, gx = on_device((64, 16, False, 9))
    lib = capi.load()
    w = np.ascontiguousarray(p.awin, dtype=np.float64)
    B, T, F = S.shape
    C, tape = S.clone(), torch.zeros((B, T, 2, 4, F), dtype=torch.complex64, device=S.device)
    gA = torch.zeros_like(A)
    win = (w.ctypes.data, w.ctypes.data)
    # (tape, iterations, look-ahead, A, frames) of the forward call; then the backward one
    for tp, iters, LA, a, frames in ((None, 2, 3, A.data_ptr(), T), (tape.data_ptr(), -1, 3, A.data_ptr(), T),
                                     (tape.data_ptr(), 2, -1, A.data_ptr(), T), (tape.data_ptr(), 2, 3, None, T),
                                     (tape.data_ptr(), 2, 3, A.data_ptr(), 0)):
        rc_ = lib.lws_rtisi_la_tape_dev(0, C.data_ptr(), a, None, B, frames, 64, 16, *win, 0, iters, LA, tp, None)
        assert rc_ == capi.LWS_ERR_INVALID, (tp, iters, LA, a, frames)
        rc_ = lib.lws_rtisi_la_backward_dev(0, gC.data_ptr(), None, a, tp, B, frames, 64, 16, *win, 0, iters, LA, gA.data_ptr(), None, None)
        assert rc_ == capi.LWS_ERR_INVALID, (tp, iters, LA, a, frames)
    rc_ = lib.lws_rtisi_la_backward_dev(0, gC.data_ptr(), None, A.data_ptr(), tape.data_ptr(), B, T, 64, 16, *win, 0, 2, 3, None, None, None)
    assert rc_ == capi.LWS_ERR_INVALID                   # nowhere to put gA
    assert lib.lws_rtisi_la_tape_dev(0, C.data_ptr(), A.data_ptr(), None, -1, T, 64, 16, *win, 0, 2, 3, tape.data_ptr(), None) == capi.LWS_ERR_INVALID
    for fn_args in ((lib.lws_rtisi_la_tape_dev, (0, C.data_ptr(), A.data_ptr(), None, B, 2, 64, 16) + win + (1, 1, 3, tape.data_ptr(), None)),
                    (lib.lws_rtisi_la_backward_dev, (0, None, None, A.data_ptr(), tape.data_ptr(), B, 2, 64, 16) + win + (1, 1, 3, gA.data_ptr(), None, None))):
        assert fn_args[0](*fn_args[1]) == capi.LWS_ERR_INVALID     # perfectrec does not keep two frames
    assert lib.lws_rtisi_la_bwd_placement(64, 16, -1, None, None, None) == capi.LWS_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(C, S) and not gA.any()
    q = lws_amd.lws(64, 16, perfectrec=True)
    with pytest.raises(ValueError, match="round trip"):
        q.rtisi_la_layer(A[:, :2].contiguous(), S[:, :2].contiguous(), 1)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A, S, -1)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A, S, 2, look_ahead=-1)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A[:, :-1], S, 2)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A[:, :, :-1].contiguous(), S[:, :, :-1].contiguous(), 2)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A.double(), S, 2)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A, S.real.contiguous(), 2)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A.cpu(), S.cpu(), 2)
    with pytest.raises(ValueError):
        p.rtisi_la_layer(A[0, 0], S[0, 0], 2)             # a 1-D S


def test_zz_margins_actually_achieved():
    """What the cases above reached, per shape (written to $LWS_MARGINS_DIR/rtisi_grad_margins.json when that variable names a
    directory; profiles/rtisi_grad_margins.json is a copy).  On an MI355X, 798 whole-run rows (gA and gS per spectrogram at 16 shapes
    and 8 pairs of look-ahead and iterations, and the five placement cases): rel-L2 of gA 9.7e-8 ... 1.0e-3, every row at most 26 % of its
    bar, at most 0.1 % of a spectrogram's gA beyond 1e-3 max|gA| (at (3000, 1500), LA = 4, state in scratch; none anywhere else); 798
    teacher-forced rows at most 6.8 % of their bar; the tape at most 5.4 % of its bar; (512, 128) at 512 threads at most 3.8 %, (600, 150)
    at 768 threads 6.5 %, (3000, 1500) 19 % with the state 1840 bytes under the LDS cap and beside three transform buffers in scratch; the
    whole file in 6.7 s."""
    if not MARGINS:
        check_whole_run((64, 16, True, 12), 3, 3)
        check_teacher_forced((64, 16, True, 12), 3, 3)
        check_tape((64, 16, True, 12), 3, 3)
    MARGINS.report("rtisi_grad_margins.json")
    assert all(v[2] <= 1.0 and v[3] <= rc.FAR_CAP and v[4] <= 1.0 and v[5] <= 1.0 for v in MARGINS.values())
