"""GPU: RTISI-LA from magnitudes alone -- start='overlap' of rtisi_la_dev and RtisiLaStream (the OVERLAP instances of k_rtisi and
k_rtisi_stream of lws_gla.hip) against the host fp64 definition lws_amd.rtisi_la(..., start='overlap').

tests/start_cases.py says why the device is held in two ways: (a) teacher-forced at iterations = 0, exact, on every shape of
tests/test_gpu_rtisi.py; (b) whole runs by the rule of that file -- rel-L2 at most 3 x the distance the fp64 run moves under the error
model, at most 0.1 % of the bins further than 1e-3 max A, magnitudes within 2e-6 max A, the signal within 3e-6 max|x| of istft of the
result -- on the inputs tests/test_start_host.py keeps at zero far bins under that model.  Every figure is printed before it is
asserted (pytest -s)."""
import json
import os

import numpy as np
import pytest

import lws_amd
import start_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_rtisi import EDGE_SHAPES, SHAPES, assert_placement   # noqa: E402
from test_gpu_rtisi import case as phased_case   # noqa: E402

MARGINS = {"entry": {}, "whole": {}, "stream": {}}


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def entry_rows(key, LA, **kw):
    p, A = sc.case(*key)
    out = p.rtisi_la_dev(dev(A, np.float32), 0, look_ahead=LA, start="overlap", **kw)
    return out


def check_entries(key, LA):
    """Check (a): the rows of a run without iterations, each against fp64 from the rows before it."""
    p, A = sc.case(*key)
    out, sig = entry_rows(key, LA, return_signal=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == A.shape
    out, sig = out.cpu().numpy().astype(np.complex128), sig.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(sig).all()
    m = MARGINS["entry"].setdefault("%d,%d,%s" % key[:3], {"cases": 0, "max_error_over_bound": 0.0, "max_left_out": 0.0,
                                                           "max_signal_error": 0.0})
    for b in range(A.shape[0]):
        worst, left_out, exact = sc.entry_check(p, A[b], out[b])
        x = p.istft(out[b])
        serr = np.abs(sig[b] - x).max() / np.abs(x).max() if x.size and np.abs(x).max() > 0 else 0.0
        print("entry %s LA=%d b=%d: error %.3f of its bound, %.3f%% of the bins left out, %d exact rows, signal %.2e max|x|"
              % (key, LA, b, worst, 100 * left_out, exact, serr))
        m["cases"] += 1
        m["max_error_over_bound"] = max(m["max_error_over_bound"], float(worst))
        m["max_left_out"] = max(m["max_left_out"], float(left_out))
        m["max_signal_error"] = max(m["max_signal_error"], float(serr))
        assert exact >= 1                                  # frame 0 at least
        assert worst <= 1.0, (b, worst)
        assert left_out <= sc.MAX_LEFT_OUT, (b, left_out)
        assert serr <= 3e-6, (b, serr)


@pytest.mark.parametrize("fsize,fshift,perfectrec", sorted(SHAPES))
def test_entry_estimates_teacher_forced(fsize, fshift, perfectrec):
    key = (fsize, fshift, perfectrec, SHAPES[fsize, fshift, perfectrec])
    for LA in (0, 3):
        check_entries(key, LA)


@pytest.mark.parametrize("key", sorted(EDGE_SHAPES))
def test_entry_estimates_teacher_forced_edge_shapes(key):
    threads, steps = EDGE_SHAPES[key]
    in_lds = {LA: lds for LA, n, lds in steps}
    for LA in (0, 3):
        got = lws_amd._capi.rtisi_la_placement(key[0], key[1], min(LA, key[3] - 1), 0)
        if LA in in_lds:
            assert_placement(key, LA, in_lds[LA], threads)
        else:
            assert got[1] == threads, (key, LA, got)
        check_entries(key, LA)
    for LA, n, lds in steps:                               # ... and at the look-aheads that put these shapes where their comments say
        if LA not in (0, 3):
            assert_placement(key, LA, lds, threads)
            check_entries(key, LA)


def compare_whole(tag, group, key, p, A, out, sig, ref, per):
    out, sig = out.cpu().numpy().astype(np.complex128), sig.cpu().numpy().astype(np.float64)
    assert out.shape == A.shape and np.isfinite(out.view(np.float64)).all() and np.isfinite(sig).all()
    m = MARGINS[group].setdefault("%d,%d,%s" % key[:3], {"cases": 0, "max_rel_l2": 0.0, "max_rel_l2_over_bar": 0.0, "max_far_fraction": 0.0,
                                                         "max_magnitude_error": 0.0, "max_signal_error": 0.0})
    for b in range(A.shape[0]):
        top = A[b].max()
        dist, bar = sc.rel(out[b], ref[b]), 3 * sc.rel(per[b], ref[b])
        far, far_model = sc.far_fraction(out[b], ref[b], top), sc.far_fraction(per[b], ref[b], top)
        mag = np.abs(np.abs(out[b]) - A[b]).max() / top
        x = p.istft(out[b])
        serr = np.abs(sig[b] - x).max() / np.abs(x).max()
        print("%s b=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%% (model %.4f%%)  |mag - A| %.2e max A  signal %.2e max|x|"
              % (tag, b, dist, bar, 100 * far, 100 * far_model, mag, serr))
        m["cases"] += 1
        for name, v in (("max_rel_l2", dist), ("max_rel_l2_over_bar", dist / bar if bar else float(dist > 0)), ("max_far_fraction", far),
                        ("max_magnitude_error", mag), ("max_signal_error", serr)):
            m[name] = max(m[name], float(v))
        assert dist <= bar, (b, dist, bar)
        assert far <= 1e-3, (b, far)
        assert mag <= 2e-6, (b, mag)
        assert serr <= 3e-6, (b, serr)


@pytest.mark.parametrize("run", sc.whole_runs(), ids=sc.run_id)
def test_whole_runs_match_host(run):
    """Check (b) on the listed inputs, every step of tests/test_gpu_rtisi.py."""
    key, signal = run
    p, A = sc.case(*key, signal=signal)
    t = dev(A, np.float32)
    if key == (4096, 1024, True, 4):
        assert_placement(key, 3, False, 1024)
    for LA, n in sc.steps_of(run):
        ref, _ = sc.host(key, signal, LA, n)
        per, _ = sc.host(key, signal, LA, n, seed=n + 17)
        out, sig = p.rtisi_la_dev(t, n, look_ahead=LA, return_signal=True, start="overlap")
        length = lws_amd._capi.istft_length(A.shape[1], p.fsize, p.fshift, p.perfectrec)
        assert out.dtype == torch.complex64 and sig.dtype == torch.float32 and tuple(sig.shape) == (A.shape[0], length)
        compare_whole("overlap %s LA=%d n=%d" % (sc.run_id(run), LA, n), "whole", key, p, A, out, sig, ref, per)


@pytest.mark.parametrize("key", [(64, 16, True, 12), (1000, 250, True, 5), (2048, 512, False, 8), (4096, 1024, True, 4)])
def test_phases_are_ignored_bit_for_bit(key):
    """A real S, A + 0j, A turned by quarter turns (whose float32 magnitudes are A exactly, so that |S| is), and any S at all
    beside explicit magnitudes: the same bits."""
    p, A = sc.case(*key)
    rng = np.random.default_rng(5)
    real = dev(A, np.float32)
    phased = dev(A * np.exp(2j * np.pi * rng.random(A.shape)), np.complex64)
    quarter = dev(A * np.array([1, 1j, -1, -1j])[rng.integers(0, 4, A.shape)], np.complex64)
    assert torch.equal(quarter.real.abs() + quarter.imag.abs(), real)
    for n in (0, 3):
        ref, x = p.rtisi_la_dev(real, n, start="overlap", return_signal=True)
        for S, given in ((real + 0j, None), (quarter, None), (phased, real), (quarter.flip(1), real), (torch.zeros_like(phased), real)):
            out, y = p.rtisi_la_dev(S, n, start="overlap", magnitudes=given, return_signal=True)
            assert torch.equal(out, ref) and torch.equal(x, y)
    out = p.rtisi_la_dev(A, 2, start="overlap")                 # numpy, real, float64
    assert torch.equal(out, p.rtisi_la_dev(real, 2, start="overlap"))


@pytest.mark.parametrize("key", [(64, 16, True, 12), (512, 128, False, 40), (64, 8, True, 20)])
def test_causality_bit_for_bit(key):
    """Output frame m depends on no input frame later than m + LA: at LA = 3 other magnitudes in the frames >= 6 leave the output
    frames 0..2 as they are, and change frame 3 -- with iterations, and without (then frame 5 is the last unchanged: an entry estimate
    depends on the frames before it alone)."""
    p, A = sc.case(*key)
    B = A.copy()
    B[:, 6:] = np.roll(A[:, 6:], 1, axis=2) * 1.3
    a, b = p.rtisi_la_dev(A, 3, look_ahead=3, start="overlap").cpu().numpy(), p.rtisi_la_dev(B, 3, look_ahead=3, start="overlap").cpu().numpy()
    assert np.array_equal(a[:, :3], b[:, :3])
    for s in range(A.shape[0]):
        assert not np.array_equal(a[s, 3], b[s, 3])
    a, b = p.rtisi_la_dev(A, 0, look_ahead=3, start="overlap").cpu().numpy(), p.rtisi_la_dev(B, 0, look_ahead=3, start="overlap").cpu().numpy()
    assert np.array_equal(a[:, :6], b[:, :6]) and not np.array_equal(a[:, 6], b[:, 6])


@pytest.mark.parametrize("key", [(64, 16, False, 9), (1000, 250, True, 5), (4096, 1024, True, 4), (2048, 512, False, 8)])
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A = sc.case(*key)
    t = dev(A, np.float32)
    for n in (0, 3):
        out, sig = p.rtisi_la_dev(t, n, return_signal=True, start="overlap")
        again, sig2 = p.rtisi_la_dev(t, n, return_signal=True, start="overlap")
        assert torch.equal(out, again) and torch.equal(sig, sig2)
        assert torch.equal(out, p.rtisi_la_dev(t, n, start="overlap"))               # with and without the signal
        for b in range(A.shape[0]):
            one, one_sig = p.rtisi_la_dev(t[b], n, return_signal=True, start="overlap")
            assert tuple(one.shape) == A.shape[1:] and torch.equal(one, out[b]) and torch.equal(one_sig, sig[b])


def test_silent_stretch_gives_exact_rows():
    """Silence longer than a frame: exact zeros inside it, and the frame behind it enters as A + 0j, as frame 0 does."""
    p, A = sc.case(64, 16, True, 12)
    Z = A.copy()
    Z[:, 3:8] = 0.0
    Z[1] = 0.0                                     # a whole spectrogram of silence
    Zf = Z.astype(np.float32)
    out, sig = p.rtisi_la_dev(Z, 0, start="overlap", return_signal=True)
    out, sig = out.cpu().numpy(), sig.cpu().numpy()
    assert np.isfinite(out.view(np.float32)).all() and np.isfinite(sig).all()
    assert (out[:, 3:8] == 0).all() and (out[1] == 0).all() and (sig[1] == 0).all()
    assert np.array_equal(out[:, 8], Zf[:, 8] + 0j) and np.array_equal(out[:, 0], Zf[:, 0] + 0j)
    assert not np.array_equal(out[0, 9], Zf[0, 9] + 0j)
    out, sig = p.rtisi_la_dev(Z, 5, start="overlap", return_signal=True)
    out, sig = out.cpu().numpy(), sig.cpu().numpy()
    assert np.isfinite(out.view(np.float32)).all() and np.isfinite(sig).all()
    assert (out[:, 3:8] == 0).all() and (out[1] == 0).all() and (sig[1] == 0).all()
    assert np.abs(np.abs(out) - Z).max() <= 2e-6 * Z.max()
    p, A = sc.case(64, 64, False, 6)               # hop = N: every frame enters as A + 0j
    assert np.array_equal(p.rtisi_la_dev(A, 0, start="overlap").cpu().numpy(), A.astype(np.float32) + 0j)


@pytest.mark.parametrize("key", [(64, 16, True, 12), (4096, 1024, False, 12)])
def test_given_is_the_default_bit_for_bit(key):
    p, A, c0 = phased_case(*key)
    t = torch.from_numpy(c0).cuda()
    for n in (0, 3):
        a, xa = p.rtisi_la_dev(t, n, return_signal=True)
        b, xb = p.rtisi_la_dev(t, n, return_signal=True, start="given")
        assert torch.equal(a, b) and torch.equal(xa, xb)
        s1, s2 = p.rtisi_la_stream(n, batch=3, return_signal=True), p.rtisi_la_stream(n, batch=3, return_signal=True, start="given")
        for s in (s1, s2):
            s.rows = [s.push(t[:, :5]), s.push(t[:, 5:]), s.finish()]
            s.close()
        for (f1, x1), (f2, x2) in zip(s1.rows, s2.rows):
            assert torch.equal(f1, f2) and torch.equal(x1, x2)
    lib, w = lws_amd._capi.load(), np.ascontiguousarray(p.awin, dtype=np.float64)
    u, v = t.clone(), t.clone()
    rc1 = lib.lws_rtisi_la_dev(0, u.data_ptr(), None, None, 3, c0.shape[1], key[0], key[1], w.ctypes.data, w.ctypes.data, int(key[2]), 2, 3, None)
    rc2 = lib.lws_rtisi_la_dev_ex(0, v.data_ptr(), None, None, 3, c0.shape[1], key[0], key[1], w.ctypes.data, w.ctypes.data, int(key[2]), 2, 3,
                                  lws_amd._capi.LWS_START_GIVEN, None)
    assert rc1 == rc2 == lws_amd._capi.LWS_OK and torch.equal(u, v) and not torch.equal(u, t)


# ---- the stream
def chunkings(T):
    return [[T], [1] * T, [2, 0, 1, T - 3]]


def run_stream(p, rows, LA, n, chunks, batch="stack", magnitudes=None):
    """Push `rows` (B, T, F), a real or complex device tensor, in `chunks`, then finish: the concatenated frames and signal."""
    T = rows.shape[-2]
    assert sum(chunks) == T
    s = p.rtisi_la_stream(n, look_ahead=LA, batch=None if batch is None else rows.shape[0], return_signal=True, start="overlap")
    frames, sig, at = [], [], 0
    for k in chunks:
        out, x = s.push(rows[..., at:at + k, :], None if magnitudes is None else magnitudes[..., at:at + k, :])
        assert out.dtype == torch.complex64 and x.dtype == torch.float32
        at += k
        frames.append(out)
        sig.append(x)
    out, x = s.finish()
    frames.append(out)
    sig.append(x)
    s.close()
    frames, sig = torch.cat(frames, dim=-2), torch.cat(sig, dim=-1)
    assert frames.shape[-2] == T and sig.shape[-1] == max(lws_amd._capi.istft_length(T, p.fsize, p.fshift, p.perfectrec), 0)
    return frames, sig


@pytest.mark.parametrize("key", [(64, 16, True, 12), (48, 16, False, 7), (256, 96, True, 5), (512, 128, False, 40), (4096, 1024, False, 12),
                                 (2048, 512, False, 8), (64, 64, False, 6)])
def test_stream_chunking_changes_no_bit(key):
    """Pushed whole, a row at a time, and with a chunk shorter than LA + 1 and an empty one: the same frames and signals, with
    iterations and without (where the rows returned are entry estimates held over from the launch they entered in)."""
    p, A = sc.case(*key)
    t = dev(A, np.float32)
    steps = [(0, 0), (3, 0), (0, 2), (1, 3), (3, 3), (5, 2)] + ([(6, 2)] if key[0] == 2048 else [])
    for LA, n in steps:
        ref = None
        for chunks in chunkings(key[3]):
            got = run_stream(p, t, LA, n, chunks)
            if ref is None:
                ref = got
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (LA, n, chunks)
        one = run_stream(p, t[1], LA, n, [1] * key[3], batch=None)                   # a stream of its own equals the member
        assert torch.equal(one[0], ref[0][1]) and torch.equal(one[1], ref[1][1])
        if n == 0:                                                                   # the entry estimates, teacher-forced
            out = ref[0].cpu().numpy().astype(np.complex128)
            for b in range(A.shape[0]):
                worst, left_out, exact = sc.entry_check(p, A[b], out[b], open_end=True)
                print("stream entry %s LA=%d b=%d: error %.3f of its bound, %.3f%% left out" % (key, LA, b, worst, 100 * left_out))
                assert worst <= 1.0 and left_out <= sc.MAX_LEFT_OUT and exact >= 1


@pytest.mark.parametrize("run", sc.STREAM_RUNS, ids=sc.run_id)
def test_stream_matches_host_open_end(run):
    key, signal = run
    p, A = sc.case(*key, signal=signal)
    t = dev(A, np.float32)
    same = {}
    for LA, n in sc.STREAM_STEPS:
        ref, _ = sc.host(key, signal, LA, n, open_end=True)
        per, _ = sc.host(key, signal, LA, n, seed=n + 17, open_end=True)
        out, sig = run_stream(p, t, LA, n, [2, 0, 1, key[3] - 3])
        compare_whole("overlap stream %s LA=%d n=%d" % (sc.run_id(run), LA, n), "stream", key, p, A, out, sig, ref, per)
        one = p.rtisi_la_dev(t, n, look_ahead=LA, start="overlap")
        same["LA=%d n=%d" % (LA, n)] = bool(torch.equal(one, out))
    print("stream %s has the bits of rtisi_la_dev(..., start='overlap'): %s" % (sc.run_id(run), same))
    MARGINS["stream"].setdefault("same_bits_as_rtisi_la_dev", {})[sc.run_id(run)] = same


def test_push_takes_real_and_complex_rows():
    p, A = sc.case(64, 16, True, 12)
    real = dev(A, np.float32)
    rng = np.random.default_rng(9)
    phased = dev(A * np.exp(2j * np.pi * rng.random(A.shape)), np.complex64)
    quarter = dev(A * np.array([1, 1j, -1, -1j])[rng.integers(0, 4, A.shape)], np.complex64)      # |S| is A exactly
    ref = run_stream(p, real, 3, 3, [5, 7])
    for rows, given in ((quarter, None), (real + 0j, None), (phased, real), (torch.zeros_like(phased), real)):
        got = run_stream(p, rows, 3, 3, [5, 7], magnitudes=given)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    s = p.rtisi_la_stream(2, start="overlap")                                        # numpy rows, one stream
    out = torch.cat([s.push(A[0, :6]), s.push(A[0, 6:]), s.finish()])
    assert torch.equal(out, run_stream(p, real[0], 3, 2, [12], batch=None)[0])


def test_invalid_arguments_raise_with_nothing_enqueued():
    p, A = sc.case(64, 16, True, 12)
    for bad in ("mixture", "zero", None, 1):
        with pytest.raises(ValueError, match="start"):
            p.rtisi_la_dev(A, 2, start=bad)
        with pytest.raises(ValueError, match="start"):
            p.rtisi_la_stream(2, start=bad)
        with pytest.raises(ValueError, match="start"):
            lws_amd.RtisiLaStream(64, 16, p.awin, p.swin, 2, start=bad)
    for bad in (dict(iterations=-1), dict(iterations=2, look_ahead=-1), dict(iterations=2, magnitudes=A[:, :-1])):
        with pytest.raises(ValueError):
            p.rtisi_la_dev(A, start="overlap", **bad)
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        p.rtisi_la_dev(A[:, :2], 3, start="overlap")
    import ctypes
    lib, w = lws_amd._capi.load(), np.ascontiguousarray(p.awin, dtype=np.float64)
    t = dev(A + 0j, np.complex64)
    keep = t.clone()
    for start in (lws_amd._capi.LWS_START_MIXTURE, 3, -1):
        rc = lib.lws_rtisi_la_dev_ex(0, t.data_ptr(), None, None, 3, 12, 64, 16, w.ctypes.data, w.ctypes.data, 1, 2, 3, start, None)
        assert rc == lws_amd._capi.LWS_ERR_INVALID
        h = ctypes.c_void_p()
        rc = lib.lws_rtisi_stream_create_ex(0, 3, 64, 16, w.ctypes.data, w.ctypes.data, 1, 2, 3, start, ctypes.byref(h))
        assert rc == lws_amd._capi.LWS_ERR_INVALID and not h.value
    for iters, LA in ((-1, 3), (2, -1)):
        rc = lib.lws_rtisi_la_dev_ex(0, t.data_ptr(), None, None, 3, 12, 64, 16, w.ctypes.data, w.ctypes.data, 1, iters, LA, 1, None)
        assert rc == lws_amd._capi.LWS_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(t, keep)
    s = p.rtisi_la_stream(2, batch=3, start="overlap")
    with pytest.raises(ValueError):
        s.push(A[:, :4, :-1])
    with pytest.raises(ValueError):
        s.push(A[:, :4], magnitudes=A[:, :3])
    nf, ns = ctypes.c_int(7), ctypes.c_int(7)                                       # neither rows nor magnitudes
    rc = lib.lws_rtisi_stream_push(s._h, None, None, 4, None, None, ctypes.byref(nf), ctypes.byref(ns), None)
    assert rc == lws_amd._capi.LWS_ERR_INVALID and (nf.value, ns.value) == (0, 0)
    assert s.push(A[:, :3]).shape[1] == 0 and s.push(A[:, 3:]).shape[1] == 9 and s.finish().shape[1] == 3
    s.close()


def test_zz_margins_actually_achieved():
    """What the cases above reached (written to $LWS_MARGINS_DIR/start_margins.json when that variable names a directory;
    profiles/start_margins.json is a copy, with the figures of tests/test_gpu_misi_start.py under "misi").  On an MI355X: 171 entry
    rows at most 3.5 % of their bound, at most 0.43 % of a spectrogram's bins left out; 294 whole-run rows at most 18 % of their bar and 48
    streamed ones at most 3.7 %, no bin beyond 1e-3 max A, magnitudes within 1.3e-7 max A, signals within 3.3e-7 max|x|; the whole file in
    3.9 s."""
    if not MARGINS["entry"]:
        check_entries((64, 16, True, 12), 3)
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "start_margins.json"), "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)
            f.write("\n")
    print(MARGINS)
    assert all(v["max_error_over_bound"] <= 1.0 and v["max_left_out"] <= sc.MAX_LEFT_OUT for v in MARGINS["entry"].values())
    assert all(v["max_rel_l2_over_bar"] <= 1.0 for g in ("whole", "stream") for k, v in MARGINS[g].items() if k != "same_bits_as_rtisi_la_dev")
