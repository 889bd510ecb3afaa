"""GPU: the backward passes of Griffin-Lim and RTISI-LA (k_gla_forward<..., TAPE>, k_gla_bwd_project, k_gla_bwd_frames, k_rtisi_tape,
k_rtisi_bwd of lws_gla.hip; lws_amd.griffin_lim_layer, lws_amd.rtisi_la_layer) under the window pairs of tests/window_cases.py, each
against the host fp64 definition of the same call under the same pair.  The backward kernels use the windows in the roles opposite
to the forward kernels': swin before a forward transform, awin after a raw inverse one.  tests/test_gpu_gla_grad.py and tests/
test_gpu_rtisi_grad.py give them windows with w[n] == w[N-1-n] and a swin that is a multiple of awin, under which an exchanged pair, a
mirrored index or the forward's roles give the same bits; tests/test_window_cases_host.py shows that under these pairs each of them
misses the bars below by a factor of 25 at the least.

The checks are those of the two files named, run from other inputs (tests/window_cases.grad_case), with the same bars: 3 x what the
fp64 pass moves under the error model, measured on the host only, per spectrogram; gA also the far-entry cap.  gA is compared on
the frames with A != 0 and is finite on the others (the docstring of tests/test_gpu_windows.test_backward_matches_host says why).  gA
and gS against the fp64 run are held on the combinations the gate of tests/test_window_cases_host.py lets through: the gate is on
gA.  The bits of the forward calls, the tape against the host's projection arguments and the teacher-forced pass do not depend on
it and run at every step of every shape.  Every figure is printed before it is asserted (pytest -s)."""
import types

import numpy as np
import pytest

import lws_amd
import window_cases as wc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_gla_grad as gg  # noqa: E402
import test_gpu_rtisi_grad as rg  # noqa: E402
from gpu_grad_helpers import dev, f64, rows_of  # noqa: E402

capi = lws_amd._capi
MARGINS = {}
PAIRS = [(kind, s) for kind in wc.KINDS for s in wc.shapes_of(kind)]
PAIR_IDS = ["%s-%s" % (kind, wc.ident(s)) for kind, s in PAIRS]
PLACED = [(kind, s, LA, n) for kind in wc.KINDS for s, LA, n in wc.SCRATCH_RTISI_GRAD]
PLACED_IDS = ["%s-%s-LA%d" % (kind, wc.ident(s), LA) for kind, s, LA, n in PLACED]


def plan(key, kind):
    awin, swin = wc.pair(key[0], key[1], kind)
    return types.SimpleNamespace(fsize=key[0], fshift=key[1], perfectrec=key[2], awin=awin, swin=swin)


def on_device(kind, key):
    """p, A, S, gC, gx"""
    return (plan(key, kind),) + tuple(dev(a) for a in wc.grad_case(*key[:4], kind)[2:])


def kept(op, kind, key):
    return [c[2] for c in wc.runs(op, kind) if c[1] == key]


class PairCases:
    """What test_gpu_rtisi_grad.Cases is for the default windows, for the pair `kind`: inputs from wc.grad_case, the fp64 references
    of tests/window_cases.py, gA compared on the frames with A != 0, every row noted in MARGINS."""
    op = "rtisi_grad"
    ident = staticmethod(wc.ident)

    def __init__(self, kind):
        self.kind, self.tag = kind, "%s %s" % (kind, self.op)

    def case(self, key):
        return (plan(key, self.kind),) + wc.grad_case(*key[:4], self.kind)[2:]               # p, A, c0, gC, gx

    def host(self, key, LA, n):
        return wc.host_rtisi_grad(key, self.kind, LA, n)

    def grad(self, key, LA, n, **kw):
        return wc.rtisi_grad(key, self.kind, LA, n, **kw)

    def host_tape(self, key, LA, n, perturbed=False):
        return wc.host_rtisi_tape(key, self.kind, LA, n, perturbed)

    @staticmethod
    def transform_model(seed):
        return wc.grad_perturbation(seed, kinds=("gc", "gv"))

    @staticmethod
    def seen(A):
        return A.any(axis=-1)

    def note(self, key, rows=0, **figures):
        wc.note(MARGINS, self.op, self.kind, key, **figures)


class GlaPairCases(PairCases):
    """The same for test_gpu_gla_grad.Cases; the forward calls are the module-level ones, which take the pair."""
    op = "gla_grad"

    def case(self, key):
        return (plan(key, self.kind),) + wc.grad_case(*key[:4], self.kind)[2:5]              # p, A, c0, gC

    def host(self, key, n, alpha):
        return wc.host_gla_grad(key, self.kind, n, alpha)

    def grad(self, key, n, alpha, **kw):
        return wc.gla_grad(key, self.kind, n, alpha, **kw)

    def host_tape(self, key, n, alpha, perturbed=False):
        return wc.host_gla_tape(key, self.kind, n, alpha, perturbed)

    @staticmethod
    def forward(p, A, S, n, alpha):
        kw = dict(alpha=alpha, perfectrec=p.perfectrec)
        return (lws_amd.griffin_lim_dev(S, p.fsize, p.fshift, p.awin, p.swin, n, magnitudes=A, **kw),
                lws_amd.griffin_lim_layer(A, S, p.fsize, p.fshift, p.awin, p.swin, n, **kw))


# ---- Griffin-Lim ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_gla_tape_and_layer_give_the_bits_of_griffin_lim_dev(kind, key):
    """... and the device tape is the host's projection arguments to 3 x what the error model moves those, at every step."""
    src = GlaPairCases(kind)
    for n, alpha in wc.GLA_GRAD_STEPS:
        tape = f64(gg.check_bits(key, n, alpha, src))
        stack = lambda t: np.moveaxis(t, 1, 0)                          # (B, n, T, F)
        ref, per = src.host_tape(key, n, alpha), src.host_tape(key, n, alpha, perturbed=True)
        for label, dist, bar in rows_of("tape", stack(tape), stack(ref), stack(per)):
            print("%s %s n=%d alpha=%g %s: rel-L2 %.3e (bar %.3e)" % (src.tag, wc.ident(key), n, alpha, label, dist, bar))
            src.note(key, max_tape_rel_l2_over_bar=dist / bar)
            assert dist <= bar, (label, dist, bar)


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_gla_teacher_forced_backward(kind, key):
    seen = wc.grad_case(*key[:4], kind)[2].any(axis=-1)
    assert seen.all() or (kind == "padded" and key[2])
    for n, alpha in wc.GLA_GRAD_STEPS:
        gg.check_teacher_forced(key, n, alpha, GlaPairCases(kind))


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_gla_backward_matches_host(kind, key):
    steps = kept("gla_grad", kind, key)
    assert steps
    for n, alpha in steps:
        gg.check_whole_run(key, n, alpha, GlaPairCases(kind))


# ---- RTISI-LA ---------------------------------------------------------------------------------------------------------------------------
def rtisi_bits(kind, key, LA, n):
    p, A, S, gC, gx = on_device(kind, key)
    kw = dict(look_ahead=LA, perfectrec=p.perfectrec, return_signal=True)
    want, want_x = lws_amd.rtisi_la_dev(S, p.fsize, p.fshift, p.awin, p.swin, n, magnitudes=A, **kw)
    C, x = lws_amd.rtisi_la_layer(A, S, p.fsize, p.fshift, p.awin, p.swin, n, **kw)
    C2, x2 = rg.run(p, A, S, LA, n, None, None, want_S=False)[:2]
    assert C.dtype == torch.complex64 and x.dtype == torch.float32 and tuple(x.shape) == tuple(want_x.shape)
    assert torch.equal(C, want) and torch.equal(x, want_x) and torch.equal(C2, want) and torch.equal(x2, want_x)


def placed(key, LA):
    return capi.rtisi_la_bwd_placement(key[0], key[1], min(LA, key[3] - 1))


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_rtisi_tape_and_layer_give_the_bits_of_rtisi_la_dev(kind, key):
    """... and the device tape is the host's projection arguments to 3 x what the error model moves those, at every step: the bar
    moves with the model's tape, so the gate on gA does not condition it."""
    for LA, n in wc.LA_STEPS:
        assert placed(key, LA)[0]
        rtisi_bits(kind, key, LA, n)
        rg.check_tape(key, LA, n, PairCases(kind))


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_rtisi_teacher_forced_backward(kind, key):
    for LA, n in wc.LA_STEPS:
        rg.check_teacher_forced(key, LA, n, PairCases(kind))


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_rtisi_backward_matches_host(kind, key):
    steps = kept("rtisi_grad", kind, key)
    assert steps
    for LA, n in steps:
        rg.check_whole_run(key, LA, n, PairCases(kind))


@pytest.mark.parametrize("kind,key,LA,n", PLACED, ids=PLACED_IDS)
def test_rtisi_backward_state_in_scratch(kind, key, LA, n):
    """k_rtisi_bwd<false> beside two transform buffers (N = 4096) and beside three (N = 3000, where x is bufA or bufC)."""
    got = placed(key, LA)
    print("%s rtisi_grad placement %s LA=%d: backward state in %s, %d threads, %d bytes of dynamic LDS"
          % (kind, wc.ident(key), LA, "LDS" if got[0] else "scratch", got[1], got[2]))
    assert got == (False, 1024, (2 if key[0] & (key[0] - 1) == 0 else 3) * key[0] * 8)
    assert (LA, n) in kept("rtisi_grad", kind, key)
    rtisi_bits(kind, key, LA, n)
    rg.check_tape(key, LA, n, PairCases(kind))
    rg.check_whole_run(key, LA, n, PairCases(kind))
    rg.check_teacher_forced(key, LA, n, PairCases(kind))


# ---- through autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", wc.KINDS)
def test_one_autograd_step_hands_the_leaves_the_bits_of_the_direct_calls(kind):
    key = (64, 16, False, 9, 2)
    p, A, S, gC, gx = on_device(kind, key)
    kw = dict(perfectrec=p.perfectrec)
    direct = gg.run(p, A, S, 3, 0.99, gC)
    leaves = [t.clone().requires_grad_(True) for t in (A, S)]
    C = lws_amd.griffin_lim_layer(*leaves, p.fsize, p.fshift, p.awin, p.swin, 3, alpha=0.99, **kw)
    assert torch.equal(C, direct[0])
    (gC.conj() * C).real.sum().backward()
    for leaf, want in zip(leaves, direct[2:]):
        assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype and torch.equal(leaf.grad, want)
    direct = rg.run(p, A, S, 3, 3, gC, gx)
    leaves = [t.clone().requires_grad_(True) for t in (A, S)]
    C, x = lws_amd.rtisi_la_layer(*leaves, p.fsize, p.fshift, p.awin, p.swin, 3, look_ahead=3, return_signal=True, **kw)
    assert torch.equal(C, direct[0]) and torch.equal(x, direct[1])
    ((gC.conj() * C).real.sum() + (gx * x).sum()).backward()
    for leaf, want in zip(leaves, direct[3:]):
        assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype and torch.equal(leaf.grad, want)


# ---- the window cache between the tape and the backward call -------------------------------------------------------------------------------
def split_run(op, p, A, S, gC, gx, between):
    """The two calls of gg.run / rg.run (n = 3, alpha = 0.99 / LA = 3) with between() after the first and no synchronisation by the caller."""
    B, T, F = S.shape
    C = S.clone()
    gA, gS = torch.full(A.shape, float("nan"), dtype=torch.float32, device=S.device), torch.full(S.shape, float("nan"), dtype=torch.complex64, device=S.device)
    win = (p.fsize, p.fshift, p.awin, p.swin, p.perfectrec)
    if op == "gla":
        tape = torch.empty((3, B, T, F), dtype=torch.complex64, device=S.device)
        capi.griffin_lim_tape_dev(C.data_ptr(), A.data_ptr(), B, T, *win, 3, 0.99, tape.data_ptr())
        between()
        capi.griffin_lim_backward_dev(gC.data_ptr(), A.data_ptr(), tape.data_ptr(), B, T, *win, 3, 0.99, gA.data_ptr(), gS.data_ptr())
    else:
        x = torch.empty((B, capi.istft_length(T, p.fsize, p.fshift, p.perfectrec)), dtype=torch.float32, device=S.device)
        tape = torch.zeros((B, T, 3, 4, F), dtype=torch.complex64, device=S.device)
        capi.rtisi_la_tape_dev(C.data_ptr(), A.data_ptr(), x.data_ptr(), B, T, *win, 3, 3, tape.data_ptr())
        between()
        capi.rtisi_la_backward_dev(gC.data_ptr(), gx.data_ptr(), A.data_ptr(), tape.data_ptr(), B, T, *win, 3, 3, gA.data_ptr(), gS.data_ptr())
    return C, tape, gA, gS


@pytest.mark.parametrize("P,Q", [("tilt", "nondual"), ("padded", "default")])
@pytest.mark.parametrize("op", ["gla", "rtisi"])
def test_window_cache_between_tape_and_backward(op, P, Q):
    """The device windows persist between calls and a call with the windows of the previous one uploads nothing (GlaCtx).  A forward
    call under another pair of the same length between the tape call and the backward call: the backward call must upload P again,
    and gives the bits of an uninterrupted pair of calls.  The caller does not synchronise between the three calls; the library does
    when it uploads a changed pair, so this is the cache's bookkeeping, not an upload overlapping a running kernel."""
    key = (64, 16, True, 12, 3)
    p, A, S, gC, gx = on_device(P, key)
    q = plan(key, Q)
    assert not np.array_equal(p.awin, q.awin) or not np.array_equal(p.swin, q.swin)
    other = []

    def forward_under_Q():
        kw = dict(magnitudes=A, perfectrec=q.perfectrec)
        if op == "gla":
            other.append(lws_amd.griffin_lim_dev(S, q.fsize, q.fshift, q.awin, q.swin, 2, **kw))
        else:
            other.append(lws_amd.rtisi_la_dev(S, q.fsize, q.fshift, q.awin, q.swin, 2, look_ahead=3, **kw))

    plain = split_run(op, p, A, S, gC, gx, lambda: None)
    torch.cuda.synchronize()
    mixed = split_run(op, p, A, S, gC, gx, forward_under_Q)
    torch.cuda.synchronize()
    assert len(other) == 1 and all(torch.equal(a, b) for a, b in zip(plain, mixed)), (op, P, Q)
    under_Q = split_run(op, q, A, S, gC, gx, lambda: None)                # ... and the pair is in the gradient
    assert not torch.equal(under_Q[2], plain[2]) and not torch.equal(under_Q[3], plain[3])
    whole = (gg.run(p, A, S, 3, 0.99, gC) if op == "gla" else rg.run(p, A, S, 3, 3, gC, gx))[-2:]
    assert torch.equal(whole[0], plain[2]) and torch.equal(whole[1], plain[3])


def test_zz_margins_actually_achieved():
    """What the cases above reached per operation, kind and shape (merged into $LWS_MARGINS_DIR/window_margins.json when that variable
    names a directory; profiles/window_margins.json is a copy).  On an MI355X, worst figure over its bar: Griffin-Lim 9.6 % whole-run
    (tilt 8.5 %, nondual 9.6 %, padded 8.2 %, the teacher-forced pass and the tape included: 8.5 % and 6.5 %), no entry of gA beyond
    1e-3 max|gA|; RTISI-LA 22.9 % whole-run (tilt 22.9 %, nondual 8.3 %, padded 10.1 %), 5.4 % teacher-forced, the tape 4.9 % (both
    at every step, the four combinations the gate drops included), at most 0.022 % of a spectrogram's gA far; rel-L2 of gA
    5.6e-8 ... 5.9e-4 over 447 whole-run rows; the whole file, 140 tests, in 6 s."""
    if "gla_grad" not in MARGINS:
        test_gla_backward_matches_host("tilt", (64, 16, True, 12, 3))
    if "rtisi_grad" not in MARGINS:
        rg.check_whole_run((64, 16, True, 12, 3), 3, 3, PairCases("nondual"))
    worst = wc.write_margins(MARGINS)
    print(worst)
    assert all(v <= 1.0 for v in worst.values())
    assert all(row.get("max_far_fraction_gA", 0.0) <= wc.FAR_CAP for rows in MARGINS.values() for row in rows.values())
