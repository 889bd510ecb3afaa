"""CPU: the magnitude-only starts of the look-ahead iterations in their fp64 definitions (start='overlap' of lws_amd.rtisi_la,
start='mixture' of lws_amd.misi_la), and the gate of the GPU tests: every whole run tests/test_gpu_rtisi_start.py holds the device
to is one on which the error model leaves the fp64 definition at zero far bins, and every teacher-forced check it makes leaves out at
most 1 % of the bins (tests/start_cases.py says why both are needed).  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import lws_amd
import start_cases as sc
from test_gpu_rtisi import EDGE_SHAPES, SHAPES

ENTRY_KEYS = [k + (SHAPES[k],) for k in sorted(SHAPES)] + sorted(EDGE_SHAPES)      # (fsize, fshift, perfectrec, T) of check (a)
T40 = [(512, 128, False, 40), (256, 64, True, 40), (64, 16, True, 40)]             # the shapes of the consistency figures


def run(p, S, n, **kw):
    return lws_amd.rtisi_la(S, p.fsize, p.fshift, p.awin, p.swin, n, perfectrec=p.perfectrec, **kw)


@pytest.mark.parametrize("run_", sc.whole_runs(), ids=sc.run_id)
def test_model_keeps_the_whole_runs_at_zero_far_bins(run_):
    """Eight seeds of the error model on every (input, step) of check (b): no bin of the perturbed fp64 run is further than 1e-3
    max A from the unperturbed one."""
    check_model(run_, sc.steps_of(run_), False)


@pytest.mark.parametrize("run_", sc.STREAM_RUNS, ids=sc.run_id)
def test_model_keeps_the_streamed_runs_at_zero_far_bins(run_):
    """... and on every (input, step) a stream is held to, under the open end a stream computes."""
    check_model(run_, sc.STREAM_STEPS, True)


def check_model(run_, steps, open_end):
    key, signal = run_
    p, A = sc.case(*key, signal=signal)
    assert len(steps) >= 4
    for LA, n in steps:
        ref, _ = sc.host(key, signal, LA, n, open_end=open_end)
        worst_far, worst_rel = 0.0, 0.0
        for seed in [n + 17] + list(range(100, 107)):
            per, _ = sc.host(key, signal, LA, n, seed=seed, open_end=open_end)
            for b in range(A.shape[0]):
                worst_far = max(worst_far, sc.far_fraction(per[b], ref[b], A[b].max()))
                worst_rel = max(worst_rel, sc.rel(per[b], ref[b]))
        print("model %s LA=%d n=%d: far bins %.4f%%, rel-L2 %.3e" % (sc.run_id(run_), LA, n, 100 * worst_far, worst_rel))
        assert worst_far == 0.0, (LA, n, worst_far)


@pytest.mark.parametrize("key", ENTRY_KEYS)
def test_teacher_forced_check_leaves_out_at_most_one_percent(key):
    """The fp64 entry estimates pass their own teacher-forced check exactly, and the bins that check leaves out are at most 1 % of
    the bins of the frames j >= 1 of every spectrogram, at both look-aheads the GPU test uses."""
    p, A = sc.case(*key)
    for LA in (0, 3):
        E, _ = sc.host(key, "noise", LA, 0)
        for b in range(A.shape[0]):
            worst, left_out, exact = sc.entry_check(p, A[b], E[b])
            print("entry %s LA=%d b=%d: error %.2e of its bound, %.3f%% of the bins left out, %d exact rows" %
                  (key, LA, b, worst, 100 * left_out, exact))
            assert worst <= 1e-6 and left_out <= sc.MAX_LEFT_OUT and exact >= 1


def test_given_is_the_default_and_what_it_was():
    p, A = sc.case(64, 16, True, 12)
    rng = np.random.default_rng(0)
    S = A * np.exp(2j * np.pi * rng.random(A.shape))
    for n in (0, 3):
        a, xa = run(p, S, n, return_signal=True)
        b, xb = run(p, S, n, return_signal=True, start="given")
        c, xc = p.rtisi_la(S, n, return_signal=True, start="given")
        assert np.array_equal(a, b) and np.array_equal(xa, xb) and np.array_equal(a, c) and np.array_equal(xa, xc)
    assert run(p, S, 0) is not None and np.array_equal(run(p, S, 0), S)


@pytest.mark.parametrize("key", [(64, 16, True, 12), (256, 96, False, 5), (48, 16, False, 7)])
def test_overlap_reads_magnitudes_alone(key):
    p, A = sc.case(*key)
    rng = np.random.default_rng(1)
    phased = A * np.exp(2j * np.pi * rng.random(A.shape))
    quarter = A * np.array([1, 1j, -1, -1j])[rng.integers(0, 4, A.shape)]       # phases under which |S| is A to the bit
    assert np.array_equal(np.abs(quarter), A)
    for LA, n in ((3, 0), (3, 3), (0, 2)):
        ref, xr = run(p, A, n, look_ahead=LA, start="overlap", return_signal=True)       # a real array
        assert ref.dtype == np.complex128 and ref.shape == A.shape
        for S, mags in ((quarter, None), (A + 0j, None), (phased, A), (np.zeros_like(phased), A), (phased[:, ::-1], A)):
            out, x = run(p, S, n, look_ahead=LA, start="overlap", magnitudes=mags, return_signal=True)
            assert np.array_equal(out, ref) and np.array_equal(x, xr)
        assert np.allclose(np.abs(ref), A, rtol=0, atol=1e-12 * A.max())
        assert np.array_equal(p.rtisi_la(A, n, look_ahead=LA, start="overlap"), ref)
        assert np.array_equal(run(p, A[1], n, look_ahead=LA, start="overlap"), ref[1])     # a stack equals its members


def test_first_frame_and_silent_sums_enter_with_zero_phase():
    p, A = sc.case(64, 16, False, 9)
    for LA, n in ((3, 0), (0, 0), (2, 2)):
        out = run(p, A, n, look_ahead=LA, start="overlap")
        if n == 0:
            assert np.array_equal(out[:, 0], A[:, 0] + 0j)
    Z = A.copy()
    Z[:, 2:7] = 0.0                                    # silence longer than a frame: the sum under frame 7 is silent
    out = run(p, Z, 0, start="overlap")
    assert np.array_equal(out[:, 7], Z[:, 7] + 0j) and (out[:, 2:7] == 0).all()
    assert not np.array_equal(out[:, 8], Z[:, 8] + 0j)
    p, A = sc.case(64, 64, False, 6)                   # fshift == fsize: no frame overlaps another
    for LA in (0, 3):
        assert np.array_equal(run(p, A, 0, look_ahead=LA, start="overlap"), A + 0j)


@pytest.mark.parametrize("key,signal", [((64, 16, True, 12), "noise"), ((256, 96, True, 5), "tones"), ((64, 8, True, 20), "noise")])
def test_overlap_is_given_started_from_its_own_entry_estimates(key, signal):
    """rtisi_la(A, n, start='overlap') takes the steps of rtisi_la(E, n, magnitudes=A), E its own result without iterations, to
    1e-12 -- where E is what the iterated run enters with: at look_ahead >= T - 1, where every frame enters before the first
    iteration.  Under a shorter look-ahead a frame that enters after step 0 is estimated from frames the iterations have already
    moved, so its entry row is not the row of E and the two runs differ from there on (by more than max A at LA = 0 and 3 on the
    first case below): there the identity is none, and nothing is asserted."""
    p, A = sc.case(*key, signal=signal)
    T = key[3]
    for n in (1, 3):
        E = run(p, A, 0, look_ahead=T - 1, start="overlap")
        a = run(p, A, n, look_ahead=T - 1, start="overlap")
        b = run(p, E, n, look_ahead=T - 1, magnitudes=A)
        err = np.abs(a - b).max() / A.max()
        print("overlap = given(E) %s n=%d: %.2e max A" % (key, n, err))
        assert err <= 1e-12


def test_open_end_rows_do_not_depend_on_what_follows():
    p, A = sc.case(64, 16, True, 12)
    LA, T1 = 3, 8
    for n in (0, 2):
        long_ = run(p, A, n, look_ahead=LA, start="overlap", open_end=True)
        short = run(p, A[:, :T1], n, look_ahead=LA, start="overlap", open_end=True)
        assert np.array_equal(short[:, :T1 - LA], long_[:, :T1 - LA])
        assert not np.array_equal(short[:, T1 - LA:], long_[:, T1 - LA:T1]) or n == 0


def consistency_db(p, S):
    return float(np.mean([p.get_consistency(s) for s in S])) if S.ndim == 3 else float(p.get_consistency(S))


@pytest.mark.parametrize("key", T40)
def test_overlap_start_is_more_consistent_than_zero_phase(key):
    """Without iterations, on T = 40 frames of either signal: the overlap start is at least 2 dB more consistent than A + 0j (the
    gaps measured in fp64 are 3.6-4.5 dB; 2 dB leaves room for another seed)."""
    for signal in ("noise", "tones"):
        p, A = sc.case(*key, signal=signal)
        E = run(p, A[0], 0, start="overlap")
        over, zero = consistency_db(p, E), consistency_db(p, A[0] + 0j)
        print("consistency %s %s: overlap %.2f dB, zero phase %.2f dB" % (key, signal, over, zero))
        assert over >= zero + 2.0


@pytest.mark.parametrize("key", [(64, 16, False, 9, 2), (64, 16, True, 12, 3), (256, 96, True, 5, 1), (48, 16, True, 7, 4)])
def test_mixture_start_is_given_started_from_the_mixture_phase(key):
    p, A, y = sc.misi_case(*key)
    y = y.astype(np.float64)
    kw = dict(perfectrec=p.perfectrec, return_signals=True)
    if not p.perfectrec:
        S0 = A * np.exp(1j * np.angle(np.stack([p.stft(v) for v in y])))[:, None]
    else:   # the same construction on the timeline: the frames of the mixture where misi_la places and cuts it
        total = p.fshift * (key[3] - 1) + p.fsize
        lo = p.fsize - p.fshift if p.fsize % p.fshift == 0 else p.fsize - p.fsize % p.fshift
        full = np.zeros((y.shape[0], total))
        full[:, lo: lo + y.shape[1]] = y
        X = np.stack([[np.fft.rfft(p.awin * v[p.fshift * j: p.fshift * j + p.fsize]) for j in range(key[3])] for v in full])
        S0 = A * np.exp(1j * np.angle(X))[:, None]
    for LA, n in ((3, 0), (3, 3), (0, 2)):
        a, sa = lws_amd.misi_la(A, y, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, start="mixture", **kw)
        b, sb = lws_amd.misi_la(S0, y, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=A, **kw)
        err, serr = np.abs(a - b).max() / A.max(), np.abs(sa - sb).max() / np.abs(y).max()
        print("mixture = given(S0) %s LA=%d n=%d: %.2e max A, signals %.2e max|y|" % (key, LA, n, err, serr))
        assert err <= 1e-12 and serr <= 1e-12
        assert np.allclose(sa.sum(axis=1), y, rtol=0, atol=1e-9 * np.abs(y).max())
        rng = np.random.default_rng(2)
        for S, mags in ((A * np.exp(2j * np.pi * rng.random(A.shape)), A), (-A + 0j, None), (1j * A, None)):
            c, _ = lws_amd.misi_la(S, y, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=mags, start="mixture", **kw)
            assert np.array_equal(a, c)                # the phases of S are not read
        assert np.array_equal(p.misi_la(A, y, n, look_ahead=LA, start="mixture"), a)


def test_mixture_given_is_the_default_and_what_it_was():
    p, A, y = sc.misi_case(64, 16, True, 12, 2)
    rng = np.random.default_rng(0)
    S = A * np.exp(2j * np.pi * rng.random(A.shape))
    for n in (0, 2):
        a = lws_amd.misi_la(S, y, p.fsize, p.fshift, p.awin, p.swin, n, perfectrec=True)
        b = lws_amd.misi_la(S, y, p.fsize, p.fshift, p.awin, p.swin, n, perfectrec=True, start="given")
        assert np.array_equal(a, b)


def test_invalid_starts_raise():
    p, A = sc.case(64, 16, True, 12)
    for bad in ("mixture", "zero", None, 1, "Overlap"):
        with pytest.raises(ValueError, match="start"):
            run(p, A, 2, start=bad)
        with pytest.raises(ValueError, match="start"):
            p.rtisi_la(A, 2, start=bad)
    p, A, y = sc.misi_case(64, 16, True, 12, 2)
    for bad in ("overlap", "zero", None, 2):
        with pytest.raises(ValueError, match="start"):
            lws_amd.misi_la(A, y, p.fsize, p.fshift, p.awin, p.swin, 2, perfectrec=True, start=bad)
        with pytest.raises(ValueError, match="start"):
            p.misi_la(A, y, 2, start=bad)
    with pytest.raises(ValueError, match="start"):
        lws_amd._capi.start_code("mixture", ("given", "overlap"))
    assert lws_amd._capi.start_code("overlap", ("given", "overlap")) == lws_amd._capi.LWS_START_OVERLAP == 1
    assert (lws_amd._capi.LWS_START_GIVEN, lws_amd._capi.LWS_START_MIXTURE) == (0, 2)
