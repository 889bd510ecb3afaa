"""GPU: the transforms, the consistency pair, Griffin-Lim, MISI and its backward pass (lws_stft.hip, lws_gla.hip) under window pairs
that are not mirror-symmetric, not multiples of each other, not always dual and not free of zeros (tests/window_cases.py), each
against the host fp64 definition of the same call under the same pair.  Every other test gives these kernels windows with
w[n] == w[N-1-n] and a synthesis window that is the normalised dual of the analysis window: a kernel that read a window backwards or
took one for the other would pass them all, and tests/test_window_cases_host.py shows it would miss the bars below a hundredfold.

The bars are the ones the suite already uses, with their figures measured on the host for these inputs: the transforms as tests/
test_gpu_transform_edges.py holds them (max(3e-6, 3 x the float32 model of tests/fft_model.py) of the largest value, consistency within
0.01 dB), Griffin-Lim and MISI as tests/test_gpu_griffin_lim.py and test_gpu_misi.py (rel-L2 within 3 x what the fp64 definition moves
under the error model, no more than 0.1 % of the bins beyond 1e-3 max A, magnitudes within 2e-6 max A, the trace within 0.01 dB + the
model's move, the signals and their sum), the backward pass as tests/test_gpu_misi_grad.py.  The inputs are those the gate of tests/
test_window_cases_host.py lets through.  Every figure is printed before it is asserted (pytest -s)."""
import contextlib
import io
import types

import numpy as np
import pytest

import lws_amd
import fft_model as fm
import window_cases as wc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_misi import mixture_bound  # noqa: E402
from test_gpu_misi_grad import dev, f64, ratio, rows_of, run  # noqa: E402
from test_gpu_transform_edges import NAMES, consistency_dev, held_db, signals  # noqa: E402

MARGINS = {}
PAIRS = [(kind, s) for kind in wc.KINDS for s in wc.SHAPES]
PAIR_IDS = ["%s-%s" % (kind, wc.ident(s)) for kind, s in PAIRS]


def plan(key, kind):
    awin, swin = wc.pair(key[0], key[1], kind)
    return types.SimpleNamespace(fsize=key[0], fshift=key[1], perfectrec=key[2], awin=awin, swin=swin)


# ---- stft_dev, istft_dev, consistency_dev -------------------------------------------------------------------------------------------
SIZES = sorted({(s[0], s[0], s[1]) for s in wc.SHAPES})          # (fsize, fftsize, hop)


def hold(tag, got, ref, mod, op, kind, key):
    """tests/test_gpu_transform_edges.hold, with the margin kept."""
    assert got.shape == ref.shape == mod.shape, (tag, got.shape, ref.shape, mod.shape)
    for b in range(ref.shape[0]):
        if not ref[b].any():
            # an impulse under the zeros of a 'padded' window: every product is an exact zero in any format, and so is its transform
            print("%s %-13s: the reference is exactly zero" % (tag, NAMES[b]))
            assert not got[b].any() and not mod[b].any(), (tag, NAMES[b])
            continue
        err, model = fm.max_rel(got[b], ref[b]), fm.max_rel(mod[b], ref[b])
        bar = max(3e-6, 3 * model)
        print("%s %-13s: dev %.2e  model %.2e  bar %.2e" % (tag, NAMES[b], err, model, bar))
        wc.note(MARGINS, op, kind, key, max_error=err, max_error_over_bar=err / bar)
        assert np.isfinite(got[b].view(np.float32) if got[b].dtype.kind == "c" else got[b]).all(), (tag, b)
        assert err <= bar, (tag, NAMES[b], err, bar)


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("fsize,fftsize,hop", SIZES + wc.ZERO_PADDED)
def test_stft_and_istft_match_host(fsize, fftsize, hop, kind):
    awin, swin = wc.pair(fsize, hop, kind)
    for perfectrec in (True, False):
        key = (fsize, hop, perfectrec)
        for n in ([1, hop] if perfectrec else []) + [fsize + 1, 2 * fsize + hop]:
            x = signals(n, 7 * fsize + hop + n)
            kw = dict(fftsize=fftsize, perfectrec=perfectrec)
            tag = "%s stft (%d/%d, %d, %s) len %d" % (kind, fsize, fftsize, hop, "pr" if perfectrec else "--", n)
            ref = np.stack([lws_amd.stft(xb, fsize, hop, awin, **kw) for xb in x])
            S = lws_amd.stft_dev(x, fsize, hop, awin, **kw)
            assert S.dtype == torch.complex64 and ref.shape[1] >= 1
            hold(tag, S.cpu().numpy(), ref, fm.stft_model(x, fsize, hop, awin, **kw), "stft", kind, key)
            assert torch.equal(lws_amd.stft_dev(x[1], fsize, hop, awin, **kw), S[1])
            if fftsize != fsize:
                continue
            spec = ref.astype(np.complex64)
            back = np.stack([lws_amd.istft(sb.astype(np.complex128), hop, swin, perfectrec=perfectrec) for sb in spec])
            y = lws_amd.istft_dev(spec, hop, swin, perfectrec=perfectrec)
            assert y.dtype == torch.float32
            hold("%s i%s" % (kind, tag[len(kind) + 1:]), y.cpu().numpy(), back, fm.istft_model(spec, hop, swin, perfectrec=perfectrec), "istft", kind, key)
            assert torch.equal(lws_amd.istft_dev(spec[2], hop, swin, perfectrec=perfectrec), y[2])


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("N,_,hop", SIZES)
def test_consistency_matches_host(N, _, hop, kind):
    awin, swin = wc.pair(N, hop, kind)
    for perfectrec in (True, False):
        rng = np.random.default_rng(3 * N + hop)
        X = lws_amd.stft(rng.standard_normal(6 * N), N, hop, awin, perfectrec=perfectrec)
        R = rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)
        stack = np.stack([R, np.abs(X).astype(complex), 1e-3 * R, X]).astype(np.complex64)
        host = np.array([lws_amd.get_consistency(S.astype(np.complex128), N, hop, awin, swin, perfectrec=perfectrec) for S in stack])
        got = consistency_dev(stack, N, hop, awin, swin, perfectrec)
        for b, name in enumerate(("random", "zero phase", "random 1e-3", "stft(noise)")):
            tag = "%s consistency (%d, %d, %s) %d frames, %s" % (kind, N, hop, perfectrec, X.shape[0], name)
            if host[b] < 60:
                print("%s: dev %.4f dB  host %.4f dB" % (tag, got[b], host[b]))
                wc.note(MARGINS, "consistency", kind, (N, hop, perfectrec), max_db_off=abs(got[b] - host[b]), max_db_off_over_bar=abs(got[b] - host[b]) / 0.01)
                assert abs(got[b] - host[b]) < 0.01, (tag, got[b], host[b])
                continue
            # consistent (a dual pair under perfectrec): the host value is fp64 rounding, the device reads what its own float32
            # round trip leaves, which the model predicts -- as tests/test_gpu_transform_edges.py holds it
            back = fm.stft_model(fm.istft_model(stack[b], hop, swin, perfectrec=perfectrec), N, hop, awin, perfectrec=perfectrec)
            model = 20 * np.log10(np.linalg.norm(stack[b]) / np.linalg.norm(back - stack[b]))
            print("%s: dev %.2f dB  model %.2f dB  host %.2f dB" % (tag, got[b], model, host[b]))
            assert kind != "nondual"
            if model >= 106:
                assert got[b] > 100.0, (tag, got[b], model)
            else:
                assert got[b] >= model - 6, (tag, got[b], model)


# ---- Griffin-Lim and MISI ---------------------------------------------------------------------------------------------------------------
def steps_of(op, kind, key):
    return [c[2] for c in wc.runs(op, kind) if c[1] == key]


def check_gla(kind, key, n, alpha):
    N, hop, perfectrec = key[:3]
    awin, swin, A, c0 = wc.case(*key, kind)[:4]
    (ref, ref_db), (per, per_db) = wc.host_gla(key, kind, n, alpha)
    target = A[:, 0].astype(np.float64)
    out, db = lws_amd.griffin_lim_dev(c0[:, 0], N, hop, awin, swin, n, alpha=alpha, magnitudes=target, perfectrec=perfectrec, return_trace=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == ref.shape and db.shape == (n, 3)
    out = out.cpu().numpy().astype(np.complex128)
    assert np.isfinite(out.view(np.float64)).all()
    for b in range(3):
        top = target[b].max()
        dist, bar = wc.rel(out[b], ref[b]), 3 * wc.rel(per[b], ref[b])
        far = np.mean(np.abs(out[b] - ref[b]) > 1e-3 * top)
        mag = np.abs(np.abs(out[b]) - target[b]).max() / top
        ddb, bar_db = np.abs(db[:, b] - ref_db[:, b]), 0.01 + np.abs(per_db[:, b] - ref_db[:, b])
        print("%s gla %s n=%d alpha=%g b=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  trace dB off %.2e (bar %.2e)"
              % (kind, wc.ident(key), n, alpha, b, dist, bar, 100 * far, mag, ddb.max(), bar_db[ddb.argmax()]))
        wc.note(MARGINS, "griffin_lim", kind, key, max_rel_l2=dist, max_rel_l2_over_bar=dist / bar, max_far_fraction=far,
                max_magnitude_error=mag, max_trace_off_over_bar=(ddb / bar_db).max())
        assert dist <= bar, (b, dist, bar)
        assert far <= 1e-3, (b, far)
        assert mag <= 2e-6, (b, mag)
        assert held_db(db[:, b], ref_db[:, b], per_db[:, b]), (b, db[:, b], ref_db[:, b], per_db[:, b])


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_griffin_lim_matches_host(kind, key):
    steps = steps_of("griffin_lim", kind, key)
    assert steps
    for n, alpha in steps:
        check_gla(kind, key, n, alpha)


def check_misi(kind, key, n):
    N, hop, perfectrec, T, K = key
    awin, swin, A, c0, y = wc.case(*key, kind)[:5]
    (ref, ref_db, ref_s), (per, per_db, per_s) = wc.host_misi(key, kind, n)
    target = A.astype(np.float64)
    out, db, s = lws_amd.misi_dev(c0, y, N, hop, awin, swin, n, magnitudes=target, perfectrec=perfectrec, return_trace=True, return_signals=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == c0.shape and db.shape == (n, 3)
    assert s.dtype == torch.float32 and tuple(s.shape) == (3, K, y.shape[1])
    out, s = out.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
    tag = "%s misi %s n=%d" % (kind, wc.ident(key), n)
    for b in range(3):
        ddb, bar_db = np.abs(db[:, b] - ref_db[:, b]), 0.01 + np.abs(per_db[:, b] - ref_db[:, b])
        x_host = [lws_amd.istft(ref[b, k], hop, swin, perfectrec=perfectrec) for k in range(K)]
        mix, mix_bar = np.abs(s[b].sum(axis=0) - y[b]).max(), mixture_bound(K, y[b], x_host)
        print("%s b=%d: trace dB off %.2e (bar %.2e)  |sum s - y| %.2e (bound %.2e)" % (tag, b, ddb.max(), bar_db[ddb.argmax()], mix, mix_bar))
        wc.note(MARGINS, "misi", kind, key, max_mixture_error_over_bar=mix / mix_bar)
        assert held_db(db[:, b], ref_db[:, b], per_db[:, b]), (b, db[:, b], ref_db[:, b], per_db[:, b])
        assert mix <= mix_bar, (b, mix, mix_bar)
        for k in range(K):
            top = target[b, k].max()
            dist, bar = wc.rel(out[b, k], ref[b, k]), 3 * wc.rel(per[b, k], ref[b, k])
            far = np.mean(np.abs(out[b, k] - ref[b, k]) > 1e-3 * top)
            mag = np.abs(np.abs(out[b, k]) - target[b, k]).max() / top
            ds = np.abs(s[b, k] - ref_s[b, k]).max()
            bar_s = 3 * np.abs(per_s[b, k] - ref_s[b, k]).max() + 3e-6 * np.abs(ref_s[b, k]).max()
            print("%s b=%d k=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal off %.2e (bar %.2e)"
                  % (tag, b, k, dist, bar, 100 * far, mag, ds, bar_s))
            wc.note(MARGINS, "misi", kind, key, max_rel_l2=dist, max_rel_l2_over_bar=dist / bar, max_far_fraction=far,
                    max_magnitude_error=mag, max_signal_error_over_bar=ds / bar_s)
            assert dist <= bar, (b, k, dist, bar)
            assert far <= 1e-3, (b, k, far)
            assert mag <= 2e-6, (b, k, mag)
            assert ds <= bar_s, (b, k, ds, bar_s)


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_misi_matches_host(kind, key):
    steps = steps_of("misi", kind, key)
    assert steps
    for n in steps:
        check_misi(kind, key, n)


# ---- the tape and the backward pass -----------------------------------------------------------------------------------------------
def on_device(kind, key):
    return (plan(key, kind),) + tuple(dev(a) for a in wc.case(*key, kind)[2:])


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_tape_and_layer_give_the_bits_of_misi_dev(kind, key):
    p, A, S, y, gC, gs = on_device(kind, key)
    top = f64(A).max(axis=(2, 3))
    for n in wc.TAPE_STEPS:
        want_C, want_s = lws_amd.misi_dev(S, y, p.fsize, p.fshift, p.awin, p.swin, n, magnitudes=A, perfectrec=p.perfectrec, return_signals=True)
        C, s = lws_amd.misi_layer(A, S, y, p.fsize, p.fshift, p.awin, p.swin, n, perfectrec=p.perfectrec)
        C2, s2, tape = run(p, A, S, y, n, None, None)[:3]
        assert torch.equal(C, want_C) and torch.equal(s, want_s) and torch.equal(C2, want_C) and torch.equal(s2, want_s)
        X, a = f64(tape[n - 1]), f64(A)
        mag = np.abs(X)
        proj = np.where(mag > 0, a * X / np.where(mag > 0, mag, 1.0), a + 0j)
        off = (np.abs(proj - f64(C)).max(axis=(2, 3)) / np.where(top > 0, top, 1.0)).max()
        print("%s misi_grad %s n=%d: same bits as misi_dev; the last tape entry projected in fp64 is within %.2e max A of C" % (kind, wc.ident(key), n, off))
        assert off <= 2e-6


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_teacher_forced_backward(kind, key):
    """The device backward pass against the host one fed the device's own tape, as tests/test_gpu_misi_grad.py holds it: the bar is what
    the host pass moves when only its transforms are perturbed, times 3.  The windows change roles here (the inverse transform is
    multiplied by awin, the frames by swin): under a pair whose windows are multiples of each other that is a rescale."""
    p, A, S, y, gC, gs = on_device(kind, key)
    _, _, hA, c0, hy, hgC, hgs = wc.case(*key, kind)
    for n in wc.TAPE_STEPS:
        _, _, tape, gA, gS, gy = run(p, A, S, y, n, gC, gs)
        args = (c0, hy, p.fsize, p.fshift, p.awin, p.swin, n, hA.astype(np.float64))
        kw = dict(grad_out=hgC, grad_signals=hgs, perfectrec=p.perfectrec, _tape=f64(tape))
        ref = lws_amd.misi_grad(*args, **kw)
        per = lws_amd.misi_grad(*args, _perturb=wc.grad_perturbation(n + 29, kinds=("gc", "gv")), **kw)
        for name, got, r, q in zip(("gA", "gS", "gy"), (f64(gA), f64(gS), f64(gy)), ref, per):
            assert np.isfinite(got.view(np.float64)).all()
            for label, dist, bar in rows_of(name, got, r, q):
                if bar == 0 and name == "gA":
                    bar = 8 * 2.0 ** -24           # one source: no transform feeds gA (tests/test_gpu_misi_grad.py)
                print("%s misi_grad %s n=%d teacher-forced %s: rel-L2 %.3e (bar %.3e)" % (kind, wc.ident(key), n, label, dist, bar))
                wc.note(MARGINS, "misi_backward_teacher_forced", kind, key, max_rel_l2_over_bar=ratio(dist, bar))
                assert dist <= bar, (label, dist, bar)


@pytest.mark.parametrize("kind,key", PAIRS, ids=PAIR_IDS)
def test_backward_matches_host(kind, key):
    """Held as tests/test_gpu_misi_grad.py holds it, gA on the frames the analysis window can see.  Under 'padded' with perfectrec the
    first frame lies under the zeros of the window and the samples read as zero: A is exactly 0 there and so is X in the definition,
    where gA is then a convention (u = 1), not a derivative.  The device transforms two frames at a time as one complex transform, so
    next to a sounding frame such a frame comes out as rounding noise of its partner, not as exact zeros, and takes that noise's
    phase for u.  Nothing else reads it: A / |X| is 0 there, so gS, gy and every other row of gA are held as they stand.  On those
    frames the tape is held to the transforms' bar, 3e-6 of the largest value, and gA to being finite."""
    p, A, S, y, gC, gs = on_device(kind, key)
    steps = steps_of("misi_grad", kind, key)
    assert steps
    seen = f64(A).any(axis=-1)                                                  # (B, K, T)
    assert seen.all() or (kind == "padded" and key[2])
    for n in steps:
        ref, per = wc.host_grad(key, kind, n)
        res = run(p, A, S, y, n, gC, gs)
        tape, got = f64(res[2]), [f64(t) for t in res[3:]]
        blind = max([np.abs(tape[:, b, k][:, ~seen[b, k]]).max() / np.abs(tape[:, b, k]).max()
                     for b in range(seen.shape[0]) for k in range(seen.shape[1]) if not seen[b, k].all()] or [0.0])
        print("%s misi_grad %s n=%d: %d frames under the zeros of the window, the tape there within %.2e of its spectrogram's largest value"
              % (kind, wc.ident(key), n, (~seen).sum(), blind))
        assert blind <= 3e-6
        for name, g, r, q in zip(("gA", "gS", "gy"), got, ref, per):
            assert g.shape == r.shape and np.isfinite(g.view(np.float64)).all()
            if name == "gA":
                rows = [("gA b=%d k=%d" % (b, k), g[b, k][seen[b, k]], r[b, k][seen[b, k]], q[b, k][seen[b, k]])
                        for b in range(g.shape[0]) for k in range(g.shape[1])]
                rows = [(label, wc.rel(gi, ri), 3 * wc.rel(qi, ri), float(np.mean(np.abs(gi - ri) > wc.FAR * np.abs(ri).max())))
                        for label, gi, ri, qi in rows]
            else:
                rows = [row + (0.0,) for row in rows_of(name, g, r, q)]
            for label, dist, bar, far in rows:
                print("%s misi_grad %s n=%d %s: rel-L2 %.3e (bar %.3e)%s"
                      % (kind, wc.ident(key), n, label, dist, bar, "  far entries %.4f%%" % (100 * far) if name == "gA" else ""))
                wc.note(MARGINS, "misi_backward", kind, key, max_rel_l2_over_bar=ratio(dist, bar), max_far_fraction_gA=far)
                assert dist <= bar, (label, dist, bar)
                assert far <= wc.FAR_CAP, (label, far)


@pytest.mark.parametrize("kind", wc.KINDS)
def test_one_training_step_through_misi_layer(kind):
    """loss.backward() through lws_amd.misi_layer hands the leaves the bits of the direct calls, and A - eta gA descends."""
    key = (64, 16, False, 9, 2)
    p, A, S, y, gC, gs = on_device(kind, key)
    direct = run(p, A, S, y, 3, gC, gs)
    leaves = [t.clone().requires_grad_(True) for t in (A, S, y)]
    C, s = lws_amd.misi_layer(*leaves, p.fsize, p.fshift, p.awin, p.swin, 3, perfectrec=p.perfectrec)
    assert torch.equal(C, direct[0]) and torch.equal(s, direct[1])
    ((gC.conj() * C).real.sum() + (gs * s).sum()).backward()
    for leaf, want in zip(leaves, direct[3:]):
        assert leaf.grad is not None and torch.equal(leaf.grad, want)
    rng = np.random.default_rng(wc.SEED + 1000 * key[0] + 10 * key[1] + key[2])
    src = rng.standard_normal((3, key[4], y.shape[1])) * wc.SOURCES[None, :key[4], None] * wc.SCALES[:, None, None]   # the first draw of case()
    target = dev(src[0].astype(np.float32))
    a = A[0].clone().requires_grad_(True)
    C, s = lws_amd.misi_layer(a, S[0], y[0], p.fsize, p.fshift, p.awin, p.swin, 3, perfectrec=p.perfectrec)
    loss = ((s - target) ** 2).sum()
    loss.backward()
    eta = 0.01 * loss.item() / (a.grad.double() ** 2).sum().item()
    stepped = (a.detach() - eta * a.grad).contiguous()
    s2 = lws_amd.misi_dev(S[0], y[0], p.fsize, p.fshift, p.awin, p.swin, 3, magnitudes=stepped, perfectrec=p.perfectrec, return_signals=True)[1]
    after = ((s2 - target) ** 2).sum().item()
    print("%s misi_layer descent: L %.6e -> %.6e (%.3f%% down; first order predicts 1%%)" % (kind, loss.item(), after, 100 * (1 - after / loss.item())))
    assert after < loss.item()


# ---- through the class ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", wc.KINDS)
def test_class_methods_give_the_bits_of_the_module_calls(kind):
    """lws(awin, hop, swin=...) renormalises the synthesis window it is given (so a non-dual pair cannot be held by the class) and
    warns about the asymmetry; its *_dev methods are the module-level calls with p.awin and p.swin."""
    key = (64, 16, True, 12, 3)
    awin, swin, A, c0, y = wc.case(*key, kind)[:5]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        p = lws_amd.lws(awin, 16, swin=swin, perfectrec=True)
    assert "analysis window that is not symmetric" in text.getvalue() and "renormalized" in text.getvalue()
    assert np.array_equal(p.awin, awin)
    assert np.allclose(p.swin, wc.pair(64, 16, "tilt" if kind == "nondual" else kind)[1], rtol=1e-12, atol=0)
    kw = dict(perfectrec=True)
    t, ty, tA = dev(c0), dev(y), dev(A)
    x, g = ty, t[:, 0].contiguous()
    assert torch.equal(p.stft_dev(x), lws_amd.stft_dev(x, 64, 16, p.awin, **kw))
    assert torch.equal(p.istft_dev(g), lws_amd.istft_dev(g, 16, p.swin, **kw))
    assert np.array_equal(p.get_consistency_dev(g), 10 * np.log10(np.divide(*consistency_sums(g, p))))
    assert torch.equal(p.griffin_lim_dev(t[:, 0], 3), lws_amd.griffin_lim_dev(t[:, 0], 64, 16, p.awin, p.swin, 3, **kw))
    a, b = p.misi_dev(t, ty, 3, return_signals=True), lws_amd.misi_dev(t, ty, 64, 16, p.awin, p.swin, 3, return_signals=True, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = p.misi_layer(tA, t, ty, 2), lws_amd.misi_layer(tA, t, ty, 64, 16, p.awin, p.swin, 2, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = p.rtisi_la_dev(t[:, 0], 2, return_signal=True), lws_amd.rtisi_la_dev(t[:, 0], 64, 16, p.awin, p.swin, 2, look_ahead=3, return_signal=True, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = p.misi_la_dev(t, ty, 2, return_signals=True), lws_amd.misi_la_dev(t, ty, 64, 16, p.awin, p.swin, 2, look_ahead=3, return_signals=True, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and the methods are held to the host definition under the renormalised pair as the module calls are above
    ref = p.misi(c0, y, 3)
    per = lws_amd.misi(c0, y, 64, 16, p.awin, p.swin, 3, perfectrec=True, _perturb=wc.perturbation(20))
    out = p.misi_dev(t, ty, 3).cpu().numpy().astype(np.complex128)
    for b in range(3):
        for k in range(3):
            dist, bar = wc.rel(out[b, k], ref[b, k]), 3 * wc.rel(per[b, k], ref[b, k])
            print("%s class misi_dev b=%d k=%d: rel-L2 %.3e (bar %.3e)" % (kind, b, k, dist, bar))
            assert dist <= bar


def consistency_sums(t, p):
    sums = lws_amd._capi.consistency_dev(t.data_ptr(), t.shape[0], t.shape[1], p.fsize, p.fshift, p.awin, p.swin, p.perfectrec,
                                         stream=torch.cuda.current_stream().cuda_stream)
    return sums[:, 0], sums[:, 1]


# ---- the window caches -----------------------------------------------------------------------------------------------------------------
def cached_calls(key, windows):
    """Functions of nothing that call griffin_lim_dev, misi_dev and rtisi_la_dev on the inputs of the 'tilt' case under `windows`."""
    N, hop, perfectrec = key[:3]
    _, _, A, c0, y = wc.case(*key, "tilt")[:5]
    t, ty = dev(c0), dev(y)
    awin, swin = windows
    kw = dict(perfectrec=perfectrec)
    return [lambda: (lws_amd.griffin_lim_dev(t[:, 0], N, hop, awin, swin, 3, **kw),),
            lambda: lws_amd.misi_dev(t, ty, N, hop, awin, swin, 3, return_signals=True, **kw),
            lambda: lws_amd.rtisi_la_dev(t[:, 0], N, hop, awin, swin, 2, return_signal=True, **kw)]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


CACHE_KEY = (64, 16, True, 12, 3)
# pairs of the same length: both windows other, only swin other, only awin other
ALTERNATIVES = {"both": lambda P, Q: Q, "swin only": lambda P, Q: (P[0], Q[1]), "awin only": lambda P, Q: (Q[0], P[1])}


@pytest.mark.parametrize("which", sorted(ALTERNATIVES))
def test_window_cache_is_not_served_stale_at_one_frame_size(which):
    """The per-device context keeps the last uploaded windows and skips the upload when the caller's compare equal; every other test
    that changes windows between calls changes the frame size too.  P, then Q, then P again: the third call gives the bits of the
    first and Q's differ -- with both windows changed, with only swin, with only awin."""
    P, Q0 = wc.pair(64, 16, "tilt"), wc.pair(64, 16, "padded")
    Q = ALTERNATIVES[which](P, Q0)
    for i, (call_P, call_Q) in enumerate(zip(cached_calls(CACHE_KEY, P), cached_calls(CACHE_KEY, Q))):
        first, other, third = call_P(), call_Q(), call_P()
        assert same(first, third), (which, i)
        assert not any(torch.equal(x, y) for x, y in zip(first, other)), (which, i)
        assert same(other, call_Q())


@pytest.mark.parametrize("which", sorted(ALTERNATIVES))
def test_window_cache_on_two_streams_without_host_synchronisation(which):
    """The same alternation -- both windows other, only swin, only awin -- with P on one torch stream and Q on the other, the streams
    changing sides, and no host synchronisation between the calls."""
    P = wc.pair(64, 16, "tilt")
    Q = ALTERNATIVES[which](P, wc.pair(64, 16, "padded"))
    calls_P, calls_Q = cached_calls(CACHE_KEY, P), cached_calls(CACHE_KEY, Q)
    refs_P, refs_Q = [c() for c in calls_P], [c() for c in calls_Q]
    assert not any(torch.equal(x, y) for a, b in zip(refs_P, refs_Q) for x, y in zip(a, b))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for rep in range(4):
        for i in range(3):
            with torch.cuda.stream(s1 if rep % 2 else s2):
                a = calls_P[i]()
            with torch.cuda.stream(s2 if rep % 2 else s1):
                b = calls_Q[i]()
            outs.append((i, a, b))
    torch.cuda.synchronize()
    for i, a, b in outs:
        assert same(a, refs_P[i]) and same(b, refs_Q[i]), (which, i)


def test_zz_margins_actually_achieved():
    """What the cases above reached per operation, kind and shape (written to $LWS_MARGINS_DIR/window_margins.json when that variable
    names a directory; profiles/window_margins.json is a copy).  On an MI355X, worst figure over its bar: stft 11 %, istft 58 % (an impulse
    under the edge of a tilted window: the float32 model is off by 1.2e-3 of the largest value there, the device by 2.0e-3),
    consistency within 8e-7 dB, Griffin-Lim 7.8 % (rel-L2 at most 2.4e-6), MISI 6.2 % (4.6e-6; the signal sum 9.9 % of its bound), the
    backward pass 12.7 % and 12.7 % teacher-forced; no bin or entry beyond 1e-3 of the largest; the whole file, 151 tests, in 3.5 s."""
    if not MARGINS:
        check_misi("tilt", (64, 16, True, 12, 3), 3)
    worst = wc.write_margins(MARGINS)
    print(worst)
    assert all(v <= 1.0 for v in worst.values())
