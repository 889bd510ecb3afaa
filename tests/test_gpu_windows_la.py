"""GPU: the look-ahead kernels (k_rtisi, k_misi_la and their stream forms, lws_gla.hip) under the window pairs of tests/
window_cases.py -- asymmetric, not multiples of each other, one of them not dual, one with exact zeros -- each against the host fp64
definition of the same call under the same pair, with the state in LDS and in device scratch.

rtisi_la_dev and RtisiLaStream are held as tests/test_gpu_rtisi.py and test_gpu_rtisi_stream.py hold them (rel-L2 within 3 x what the
fp64 definition moves under the error model, at most 0.1 % of the bins beyond 1e-3 max A, magnitudes within 2e-6 max A, the signal
within 3e-6 max|x| of istft of the result), misi_la_dev and MisiLaStream as tests/test_gpu_misi_la.py and test_gpu_misi_la_stream.py
(the same per source, the signals within 3 x the model's move + 3e-6 max|s_k|, their sum within mixture_bound of the mixture); the
magnitude-only starts also teacher-forced at no iterations, as tests/test_gpu_rtisi_start.py holds them.  A stream is pushed frame by
frame and in uneven chunks with an empty one, and every chunking gives the bits of the whole input pushed at once.

Both online-MISI kernels weight the mixture by num / den, den the overlap-added awin swin, 1 where den is 0.  Under a dual pair den is 1
away from the ends, which is all the other tests run; under 'nondual' it varies everywhere and under 'padded' it is 0 under the pads at
both ends of the timeline.  So under those two the first and the last fsize samples of the timeline are also held on their own, to
bars taken over those samples alone, and their worst figure is printed separately.  The inputs are those the gate of tests/
test_window_cases_host.py lets through.  Every figure is printed before it is asserted (pytest -s)."""
import types

import numpy as np
import pytest

import lws_amd
from lws_amd.lws import _perfectrec_prepad
import start_cases as sc
import window_cases as wc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_misi import mixture_bound  # noqa: E402

MARGINS = {}
LA_SHAPES = {"rtisi_la": wc.SHAPES + [wc.SCRATCH_RTISI[0]], "misi_la": wc.SHAPES + [wc.SCRATCH_MISI[0]]}
# (the gate leaves no whole run of RTISI-LA at the scratch shape under 'tilt': there the placement is held teacher-forced, below)
CASES = {op: [(kind, s) for kind in wc.KINDS for s in shapes if any(c[1] == s for c in wc.runs(op, kind))] for op, shapes in LA_SHAPES.items()}
ENTRY_CASES = [(kind, s) for kind in wc.KINDS for s in LA_SHAPES["rtisi_la"]]


def case_id(c):
    return "%s-%s" % (c[0], wc.ident(c[1]))


def steps_of(op, kind, key):
    return [c[2] for c in wc.runs(op, kind) if c[1] == key]


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()              # (a copy: the cases are read-only)
    return t if dtype is None else t.to(dtype)


def assert_placement(op, key, LA):
    """The scratch rows are in scratch and every other row in LDS: what the launch of this case is, by lws_rtisi_la_placement."""
    scratch = (key, LA) in (wc.SCRATCH_RTISI[:2], wc.SCRATCH_MISI[:2])
    got = lws_amd._capi.rtisi_la_placement(key[0], key[1], min(LA, key[3] - 1), 0 if op == "rtisi_la" else key[4])
    print("placement %s %s LA=%d: state in %s, %d threads, %d bytes of dynamic LDS" % (op, wc.ident(key), LA, "LDS" if got[0] else "scratch", got[1], got[2]))
    if scratch or key in wc.SHAPES:
        assert got[0] == (not scratch), (op, key, LA, got)


def edges(key, n_samples):
    """Index arrays into a returned signal of n_samples: the first and the last fsize samples of the uncut timeline that it keeps."""
    N, hop, perfectrec, T = key[:4]
    lo = _perfectrec_prepad(N, hop) if perfectrec else 0
    total = hop * (T - 1) + N
    at = np.arange(n_samples) + lo                          # timeline position of each returned sample
    return np.nonzero(at < N)[0], np.nonzero(at >= total - N)[0]


# ---- RTISI-LA -------------------------------------------------------------------------------------------------------------------------
def hold_rtisi(tag, op, kind, key, out, sig, ref, per, target):
    awin, swin = wc.pair(key[0], key[1], kind)
    assert out.dtype == torch.complex64 and tuple(out.shape) == ref.shape and sig.dtype == torch.float32
    out, sig = out.cpu().numpy().astype(np.complex128), sig.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(sig).all()
    for b in range(3):
        top = target[b].max()
        dist, bar = wc.rel(out[b], ref[b]), 3 * wc.rel(per[b], ref[b])
        far = np.mean(np.abs(out[b] - ref[b]) > 1e-3 * top)
        mag = np.abs(np.abs(out[b]) - target[b]).max() / top
        x = lws_amd.istft(out[b], key[1], swin, perfectrec=key[2])
        assert sig[b].shape == x.shape
        serr = np.abs(sig[b] - x).max() / np.abs(x).max() if x.size else 0.0
        print("%s b=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal %.2e max|x|" % (tag, b, dist, bar, 100 * far, mag, serr))
        wc.note(MARGINS, op, kind, key, max_rel_l2=dist, max_rel_l2_over_bar=dist / bar, max_far_fraction=far, max_magnitude_error=mag,
                max_signal_error=serr, max_signal_error_over_bar=serr / 3e-6)
        assert dist <= bar, (b, dist, bar)
        assert far <= 1e-3, (b, far)
        assert mag <= 2e-6, (b, mag)
        assert serr <= 3e-6, (b, serr)
        if kind != "tilt" and x.size:
            for name, idx in zip(("first", "last"), edges(key, x.size)):
                e = np.abs(sig[b, idx] - x[idx]).max() / np.abs(x[idx]).max()
                print("%s b=%d: the %s %d samples of the timeline on their own: signal %.2e of their max|x|" % (tag, b, name, key[0], e))
                wc.note(MARGINS, op, kind, key, max_edge_signal_error_over_bar=e / 3e-6)
                assert e <= 3e-6, (b, name, e)


def check_rtisi(kind, key, LA, n, start):
    awin, swin = wc.pair(key[0], key[1], kind)
    rows, mags = wc.rtisi_input(key, kind, start)
    (ref, _), (per, _) = wc.host_rtisi(key, kind, LA, n, start)
    out, sig = lws_amd.rtisi_la_dev(rows, key[0], key[1], awin, swin, n, look_ahead=LA, magnitudes=mags, perfectrec=key[2],
                                    return_signal=True, start=start)
    target = wc.case(*key, kind)[2][:, 0].astype(np.float64)
    hold_rtisi("%s rtisi_la %s LA=%d n=%d %s" % (kind, wc.ident(key), LA, n, start), "rtisi_la", kind, key, out, sig, ref, per, target)


@pytest.mark.parametrize("case", CASES["rtisi_la"], ids=case_id)
def test_rtisi_la_matches_host(case):
    kind, key = case
    steps = steps_of("rtisi_la", kind, key)
    assert steps
    for LA, n, start in steps:
        assert_placement("rtisi_la", key, LA)
        check_rtisi(kind, key, LA, n, start)


def entry_plan(key, kind):
    awin, swin = wc.pair(key[0], key[1], kind)
    return types.SimpleNamespace(fsize=key[0], fshift=key[1], perfectrec=key[2], awin=awin, swin=swin)


@pytest.mark.parametrize("case", ENTRY_CASES, ids=case_id)
def test_overlap_entry_estimates_teacher_forced(case):
    """start='overlap' without iterations returns the entry estimates; each row is recomputed in fp64 from the device's own earlier
    rows (tests/start_cases.entry_check): nothing can drift, so this holds every input, the scratch placement included, also where
    the gate drops the whole runs.  The check presumes a projection argument good to 1e-6 max|X|; on the four inputs of
    wc.NOT_AN_OVERLAP_CASE, where the float32 transform model itself makes more of it, the model's figure (measured on the host,
    wc.overlap_sigma) takes the place of the 1e-6 and the bound is three times the model, as everywhere.  The stream's rows pass the
    same check under the open end."""
    kind, key = case
    awin, swin = wc.pair(key[0], key[1], kind)
    A0, _ = wc.rtisi_input(key, kind, "overlap")
    p = entry_plan(key, kind)
    sigma = wc.overlap_sigma(kind, key)
    print("%s entry %s: a projection argument is taken to be good to %.2e max|X|" % (kind, wc.ident(key), sigma))
    for LA in sorted({0, 3, wc.SCRATCH_RTISI[1] if key == wc.SCRATCH_RTISI[0] else 1}):
        assert_placement("rtisi_la", key, LA)
        out, sig = lws_amd.rtisi_la_dev(A0, key[0], key[1], awin, swin, 0, look_ahead=LA, perfectrec=key[2], return_signal=True, start="overlap")
        streamed, _ = run_rtisi_stream(kind, key, LA, 0, "overlap", [key[3]])
        for name, rows, open_end in (("one shot", out, False), ("stream", streamed, True)):
            rows = rows.cpu().numpy().astype(np.complex128)
            for b in range(3):
                worst, left_out, exact = sc.entry_check(p, A0[b], rows[b], open_end=open_end, sigma=sigma)
                print("%s entry %s LA=%d %s b=%d: error %.3f of its bound, %.3f%% of the bins left out, %d exact rows"
                      % (kind, wc.ident(key), LA, name, b, worst, 100 * left_out, exact))
                wc.note(MARGINS, "rtisi_la_entry", kind, key, max_error_over_bar=worst, max_left_out=left_out)
                assert exact >= 1 and worst <= 1.0 and left_out <= sc.MAX_LEFT_OUT, (name, b, worst, left_out, exact)


def properties(tag, kind, key, out, sig, target):
    """What does not hang on an ill-conditioned phase: finite, the magnitudes are the targets, the signal is istft of the result."""
    swin = wc.pair(key[0], key[1], kind)[1]
    assert out.dtype == torch.complex64 and tuple(out.shape) == target.shape and sig.dtype == torch.float32
    out, sig = out.cpu().numpy().astype(np.complex128), sig.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(sig).all()
    for b in range(3):
        mag = np.abs(np.abs(out[b]) - target[b]).max() / target[b].max()
        x = lws_amd.istft(out[b], key[1], swin, perfectrec=key[2])
        serr = np.abs(sig[b] - x).max() / np.abs(x).max()
        print("%s b=%d: |mag - A| %.2e max A  signal %.2e max|x|" % (tag, b, mag, serr))
        wc.note(MARGINS, "rtisi_la_overlap_properties", kind, key, max_magnitude_error=mag, max_signal_error_over_bar=serr / 3e-6)
        assert mag <= 2e-6, (b, mag)
        assert serr <= 3e-6, (b, serr)


@pytest.mark.parametrize("run", wc.overlap_property_runs(), ids=lambda r: "%s-%s-LA%d-n%d" % (r[0], wc.ident(r[1]), r[2], r[3]))
def test_overlap_start_beyond_float32_keeps_its_properties(run):
    """start='overlap' under 'padded' with perfectrec: the phase of the second frame is more than float32 can compute
    (wc.NOT_AN_OVERLAP_CASE), so the whole run is not compared with the fp64 one.  Everything else is held as on every other input,
    for rtisi_la_dev and for the stream in every chunking."""
    kind, key, LA, n = run
    awin, swin = wc.pair(key[0], key[1], kind)
    A0, _ = wc.rtisi_input(key, kind, "overlap")
    assert_placement("rtisi_la", key, LA)
    out, sig = lws_amd.rtisi_la_dev(A0, key[0], key[1], awin, swin, n, look_ahead=LA, perfectrec=key[2], return_signal=True, start="overlap")
    tag = "%s rtisi_la %s LA=%d n=%d overlap" % (kind, wc.ident(key), LA, n)
    properties(tag, kind, key, out, sig, A0)
    again = lws_amd.rtisi_la_dev(A0, key[0], key[1], awin, swin, n, look_ahead=LA, perfectrec=key[2], return_signal=True, start="overlap")
    assert torch.equal(out, again[0]) and torch.equal(sig, again[1])
    whole, whole_x = run_rtisi_stream(kind, key, LA, n, "overlap", [key[3]])
    for chunks in chunkings(key[3])[1:]:
        o, x = run_rtisi_stream(kind, key, LA, n, "overlap", chunks)
        assert torch.equal(o, whole) and torch.equal(x, whole_x), chunks
    properties(tag + " stream", kind, key, whole, whole_x, A0)


# ---- online MISI ------------------------------------------------------------------------------------------------------------------------
def hold_misi(tag, op, kind, key, out, s, y, ref, ref_s, per, per_s, target):
    awin, swin = wc.pair(key[0], key[1], kind)
    K = key[4]
    assert out.dtype == torch.complex64 and tuple(out.shape) == ref.shape
    assert s.dtype == torch.float32 and tuple(s.shape) == ref_s.shape
    out, s = out.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
    for b in range(3):
        first, last = edges(key, s.shape[-1])
        if s.shape[-1]:
            x_host = [lws_amd.istft(ref[b, k], key[1], swin, perfectrec=key[2]) for k in range(K)]
            yb = y[b, :s.shape[-1]].astype(np.float64)
            mix, mix_bar = np.abs(s[b].sum(axis=0) - yb).max(), mixture_bound(K, yb, x_host)
            print("%s b=%d: |sum s - y| %.2e (bound %.2e)" % (tag, b, mix, mix_bar))
            wc.note(MARGINS, op, kind, key, max_mixture_error_over_bar=mix / mix_bar)
            assert mix <= mix_bar, (b, mix, mix_bar)
        for k in range(K):
            top = target[b, k].max()
            dist, bar = wc.rel(out[b, k], ref[b, k]), 3 * wc.rel(per[b, k], ref[b, k])
            far = np.mean(np.abs(out[b, k] - ref[b, k]) > 1e-3 * top)
            mag = np.abs(np.abs(out[b, k]) - target[b, k]).max() / top
            ds = bar_s = 0.0
            if s.shape[-1]:
                ds = np.abs(s[b, k] - ref_s[b, k]).max()
                bar_s = 3 * np.abs(per_s[b, k] - ref_s[b, k]).max() + 3e-6 * np.abs(ref_s[b, k]).max()
            print("%s b=%d k=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal off %.2e (bar %.2e)"
                  % (tag, b, k, dist, bar, 100 * far, mag, ds, bar_s))
            wc.note(MARGINS, op, kind, key, max_rel_l2=dist, max_rel_l2_over_bar=dist / bar, max_far_fraction=far, max_magnitude_error=mag,
                    max_signal_error_over_bar=ds / bar_s if bar_s else 0.0)
            assert dist <= bar, (b, k, dist, bar)
            assert far <= 1e-3, (b, k, far)
            assert mag <= 2e-6, (b, k, mag)
            assert ds <= bar_s, (b, k, ds, bar_s)
            if kind != "tilt" and s.shape[-1]:
                for name, idx in (("first", first), ("last", last)):
                    e = np.abs(s[b, k, idx] - ref_s[b, k, idx]).max()
                    e_bar = 3 * np.abs(per_s[b, k, idx] - ref_s[b, k, idx]).max() + 3e-6 * np.abs(ref_s[b, k, idx]).max()
                    print("%s b=%d k=%d: the %s %d samples of the timeline on their own: signal off %.2e (bar %.2e)" % (tag, b, k, name, key[0], e, e_bar))
                    wc.note(MARGINS, op, kind, key, max_edge_signal_error_over_bar=e / e_bar)
                    assert e <= e_bar, (b, k, name, e, e_bar)


def check_misi_la(kind, key, LA, n, start):
    awin, swin = wc.pair(key[0], key[1], kind)
    rows, mags, y = wc.misi_la_input(key, kind, start)
    (ref, ref_s), (per, per_s) = wc.host_misi_la(key, kind, LA, n, start)
    out, s = lws_amd.misi_la_dev(rows, y, key[0], key[1], awin, swin, n, look_ahead=LA, magnitudes=mags, perfectrec=key[2],
                                 return_signals=True, start=start)
    target = wc.case(*key, kind)[2].astype(np.float64)
    hold_misi("%s misi_la %s LA=%d n=%d %s" % (kind, wc.ident(key), LA, n, start), "misi_la", kind, key, out, s, y, ref, ref_s, per, per_s, target)


@pytest.mark.parametrize("case", CASES["misi_la"], ids=case_id)
def test_misi_la_matches_host(case):
    kind, key = case
    steps = steps_of("misi_la", kind, key)
    assert steps
    for LA, n, start in steps:
        assert_placement("misi_la", key, LA)
        check_misi_la(kind, key, LA, n, start)


# ---- the streams --------------------------------------------------------------------------------------------------------------------------
def chunkings(T):
    """The whole input at once; frame by frame; uneven chunks with an empty one."""
    return [[T], [1] * T, [2, 0, 1, T - 3] if T >= 4 else [0, 1, T - 1] if T >= 2 else [0, 1]]


def run_rtisi_stream(kind, key, LA, n, start, chunks):
    N, hop, perfectrec, T = key[:4]
    awin, swin = wc.pair(N, hop, kind)
    rows, mags = wc.rtisi_input(key, kind, start)
    t = dev(rows) if start == "given" else dev(rows, torch.float32)
    A = None if mags is None else dev(mags, torch.float32)
    s = lws_amd.RtisiLaStream(N, hop, awin, swin, n, look_ahead=LA, perfectrec=perfectrec, batch=3, return_signal=True, start=start)
    frames, sig, at = [], [], 0
    for k in chunks:
        out, x = s.push(t[:, at:at + k], None if A is None else A[:, at:at + k])
        at += k
        frames.append(out)
        sig.append(x)
    assert at == T
    out, x = s.finish()
    s.close()
    frames, sig = torch.cat(frames + [out], dim=-2), torch.cat(sig + [x], dim=-1)
    assert frames.shape[-2] == T and sig.shape[-1] == max(lws_amd._capi.istft_length(T, N, hop, perfectrec), 0)
    return frames, sig


def run_misi_stream(kind, key, LA, n, start, chunks):
    N, hop, perfectrec, T, K = key
    awin, swin = wc.pair(N, hop, kind)
    rows, mags, y = wc.misi_la_input(key, kind, start, open_end=True)
    t = dev(rows) if start == "given" else dev(rows, torch.float32)
    A, ty = None if mags is None else dev(mags, torch.float32), dev(y)
    assert ty.shape[-1] == wc.need(key, T)
    s = lws_amd.MisiLaStream(K, N, hop, awin, swin, n, look_ahead=LA, perfectrec=perfectrec, batch=3, return_signals=True, start=start)
    frames, sig, at, yat = [], [], 0, 0
    for k in chunks:
        ns = s.samples_needed(k)
        out, x = s.push(t[:, :, at:at + k], ty[:, yat:yat + ns], None if A is None else A[:, :, at:at + k])
        at, yat = at + k, yat + ns
        frames.append(out)
        sig.append(x)
    assert at == T and yat == ty.shape[-1]
    out, x = s.finish()
    s.close()
    frames, sig = torch.cat(frames + [out], dim=-2), torch.cat(sig + [x], dim=-1)
    assert frames.shape[-2] == T and sig.shape[-1] == max(lws_amd._capi.istft_length(T, N, hop, perfectrec), 0)
    return frames, sig


@pytest.mark.parametrize("case", CASES["rtisi_la"], ids=case_id)
def test_rtisi_stream_matches_host_open_end_in_every_chunking(case):
    kind, key = case
    steps = steps_of("rtisi_la", kind, key)
    assert steps
    target = wc.case(*key, kind)[2][:, 0].astype(np.float64)
    for LA, n, start in steps:
        whole, whole_x = run_rtisi_stream(kind, key, LA, n, start, [key[3]])
        for chunks in chunkings(key[3])[1:]:
            out, x = run_rtisi_stream(kind, key, LA, n, start, chunks)
            assert torch.equal(out, whole) and torch.equal(x, whole_x), (LA, n, start, chunks)
        (ref, _), (per, _) = wc.host_rtisi(key, kind, LA, n, start, True)
        hold_rtisi("%s rtisi stream %s LA=%d n=%d %s" % (kind, wc.ident(key), LA, n, start), "rtisi_la_stream", kind, key, whole, whole_x, ref, per, target)


@pytest.mark.parametrize("case", CASES["misi_la"], ids=case_id)
def test_misi_stream_matches_host_open_end_in_every_chunking(case):
    kind, key = case
    steps = steps_of("misi_la", kind, key)
    assert steps
    target = wc.case(*key, kind)[2].astype(np.float64)
    for LA, n, start in steps:
        whole, whole_x = run_misi_stream(kind, key, LA, n, start, [key[3]])
        for chunks in chunkings(key[3])[1:]:
            out, x = run_misi_stream(kind, key, LA, n, start, chunks)
            assert torch.equal(out, whole) and torch.equal(x, whole_x), (LA, n, start, chunks)
        (ref, ref_s), (per, per_s) = wc.host_misi_la(key, kind, LA, n, start, True)
        y = wc.misi_la_input(key, kind, start, open_end=True)[2]
        hold_misi("%s misi stream %s LA=%d n=%d %s" % (kind, wc.ident(key), LA, n, start), "misi_la_stream", kind, key, whole, whole_x, y,
                  ref, ref_s, per, per_s, target)


# ---- the handles keep windows of their own --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(64, 16, True, 12, 3), wc.SCRATCH_MISI[0]], ids=wc.ident)
def test_a_stream_is_not_disturbed_by_other_windows_of_its_frame_size(key):
    """Handles under pair P pushed frame by frame; between their pushes, one-shot calls and second handles under pair Q of the same
    frame size (another swin, the same awin; then both other) run to their end.  The first handles return the bits of an undisturbed
    run, and so do the disturbing calls."""
    N, hop, perfectrec, T, K = key
    LA, n = 3, 2
    quiet_r, quiet_m = run_rtisi_stream("tilt", key, LA, n, "given", [1] * T), run_misi_stream("tilt", key, LA, n, "given", [1] * T)
    others = {}
    for q in ("nondual", "padded"):
        aq, sq = wc.pair(N, hop, q)
        rows, mags, y = wc.misi_la_input(key, q, "given")
        others[q] = (lws_amd.rtisi_la_dev(rows[:, 0], N, hop, aq, sq, n, look_ahead=LA, magnitudes=mags[:, 0], perfectrec=perfectrec),
                     lws_amd.misi_la_dev(rows, y, N, hop, aq, sq, n, look_ahead=LA, magnitudes=mags, perfectrec=perfectrec),
                     run_rtisi_stream(q, key, LA, n, "given", [T])[0], run_misi_stream(q, key, LA, n, "given", [T])[0])
    awin, swin = wc.pair(N, hop, "tilt")
    rows, mags, y = wc.misi_la_input(key, "tilt", "given", open_end=True)
    t, A, ty = dev(rows), dev(mags, torch.float32), dev(y)
    sr = lws_amd.RtisiLaStream(N, hop, awin, swin, n, look_ahead=LA, perfectrec=perfectrec, batch=3, return_signal=True)
    sm = lws_amd.MisiLaStream(K, N, hop, awin, swin, n, look_ahead=LA, perfectrec=perfectrec, batch=3, return_signals=True)
    got_r, got_m, yat = [], [], 0
    for j in range(T):
        got_r.append(sr.push(t[:, 0, j:j + 1].contiguous(), A[:, 0, j:j + 1].contiguous()))
        ns = sm.samples_needed(1)
        got_m.append(sm.push(t[:, :, j:j + 1], ty[:, yat:yat + ns], A[:, :, j:j + 1]))
        yat += ns
        q = ("nondual", "padded")[j % 2]
        aq, sq = wc.pair(N, hop, q)
        rq, mq, yq = wc.misi_la_input(key, q, "given")
        assert torch.equal(lws_amd.rtisi_la_dev(rq[:, 0], N, hop, aq, sq, n, look_ahead=LA, magnitudes=mq[:, 0], perfectrec=perfectrec), others[q][0])
        assert torch.equal(lws_amd.misi_la_dev(rq, yq, N, hop, aq, sq, n, look_ahead=LA, magnitudes=mq, perfectrec=perfectrec), others[q][1])
        assert torch.equal(run_rtisi_stream(q, key, LA, n, "given", [T])[0], others[q][2])
        assert torch.equal(run_misi_stream(q, key, LA, n, "given", [T])[0], others[q][3])
    got_r.append(sr.finish())
    got_m.append(sm.finish())
    sr.close()
    sm.close()
    for got, quiet in ((got_r, quiet_r), (got_m, quiet_m)):
        assert torch.equal(torch.cat([g[0] for g in got], dim=-2), quiet[0]) and torch.equal(torch.cat([g[1] for g in got], dim=-1), quiet[1])
    assert not torch.equal(others["nondual"][0], others["padded"][0])


def test_window_cache_of_rtisi_la_dev_and_misi_la_dev_at_one_frame_size():
    """P, then Q, then P again with the frame size fixed: the third call gives the bits of the first and Q's differ -- with both windows
    changed, with only swin, with only awin."""
    key = (64, 16, True, 12, 3)
    N, hop, perfectrec = key[:3]
    rows, mags, y = wc.misi_la_input(key, "tilt", "given")
    t, A, ty = dev(rows), dev(mags, torch.float32), dev(y)
    P, Q = wc.pair(N, hop, "tilt"), wc.pair(N, hop, "padded")

    def call(w):
        return (lws_amd.rtisi_la_dev(t[:, 0], N, hop, w[0], w[1], 2, magnitudes=A[:, 0], perfectrec=perfectrec),
                lws_amd.misi_la_dev(t, ty, N, hop, w[0], w[1], 2, magnitudes=A, perfectrec=perfectrec))
    for other in (Q, (P[0], Q[1]), (Q[0], P[1])):
        first, second, third = call(P), call(other), call(P)
        assert all(torch.equal(a, b) for a, b in zip(first, third))
        assert not any(torch.equal(a, b) for a, b in zip(first, second))


def test_zz_margins_actually_achieved():
    """What the cases above reached per operation, kind and shape (merged into $LWS_MARGINS_DIR/window_margins.json when that variable
    names a directory; profiles/window_margins.json is a copy).  On an MI355X, worst figure over its bar: rtisi_la_dev 44 % (rel-L2
    5.4e-5 at 'nondual' (64, 16, perfectrec)), its stream 33 %, misi_la_dev 19 %, its stream 6.6 %, the overlap entries 3.8 % of their
    bound (those of wc.NOT_AN_OVERLAP_CASE included, under the float32 model's sigma), the signal sums 9.9 % of theirs; the first and
    last fsize samples on their own 7.8 % at most; no bin beyond 1e-3 max A; the whole file, 134 tests, in 6.0 s."""
    if not MARGINS:
        check_misi_la("nondual", (64, 16, True, 12, 3), 3, 3, "given")
    worst = wc.write_margins(MARGINS)
    print(worst)
    assert all(v <= 1.0 for v in worst.values())
