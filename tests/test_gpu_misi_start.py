"""GPU: online MISI from magnitudes alone -- start='mixture' of misi_la_dev and MisiLaStream (the MIXTURE instances of k_misi_la and
k_misi_la_stream of lws_gla.hip) against the host fp64 definition lws_amd.misi_la(..., start='mixture').

Inputs are those of tests/start_cases.py: K sources (tones, noise, quieter noises) at three scales and their float32 sum as mixture.
An entry depends on the mixture alone, so nothing here is as sensitive as the overlap start of RTISI-LA; the device is held (a) at
iterations = 0, exactly, to A_kj X / |X| with X the fp64 transform of the float32 mixture under frame j, by the bound of
start_cases.entry_check, and (b) on whole runs by the rule of tests/test_gpu_misi_la.py as it stands.  Every figure is printed
before it is asserted (pytest -s)."""
import ctypes
import json
import os

import numpy as np
import pytest

import lws_amd
import start_cases as sc
from lws_amd.lws import _perfectrec_prepad

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_misi import mixture_bound  # noqa: E402
from test_gpu_rtisi import assert_placement  # noqa: E402

# (fsize, fshift, perfectrec, T, K): (threads, state in LDS at LA = 3)
KEYS = {
    (64, 16, False, 9, 2): (256, True),            # power of two
    (64, 16, True, 12, 4): (256, True),            # four sources
    (48, 16, True, 7, 1): (256, True),             # odd factor 3, K = 1
    (256, 96, True, 5, 2): (256, True),            # hop does not divide the frame
    (1000, 250, True, 5, 2): (1024, True),         # odd factor 125
    (64, 8, True, 20, 2): (256, True),             # Q = 8
    (512, 128, False, 40, 2): (512, True),         # the rings wrap many times
    (2048, 512, False, 6, 2): (1024, False),       # N > workgroup: two bins of a frame per thread (K = 2, so that the mixture is not
                                                   # the tones alone: 16 % of the bins of their 2048-point frames lie under TAU max|X|)
    (1024, 256, False, 6, 4): (1024, False),       # four sources whose state goes to scratch
    (4096, 1024, False, 6, 2): (1024, False),      # three bins per thread, scratch
}
STEPS = [(0, 1), (0, 4), (1, 3), (3, 3), (3, 6), (5, 2)]
STREAM_KEYS = [(64, 16, True, 12, 4), (48, 16, True, 7, 1), (256, 96, True, 5, 2), (512, 128, False, 40, 2), (1024, 256, False, 6, 4),
               (4096, 1024, False, 6, 2)]
MARGINS = {"entry": {}, "whole": {}, "stream": {}}


def key_id(k):
    return "%d-%d-%s-T%d-K%d" % tuple(k)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def mixture_rows(p, y, T, open_end=False):
    """X (T, F): the fp64 transforms of the mixture under every frame, on the timeline as misi_la places and cuts it."""
    total = p.fshift * (T - 1) + p.fsize
    lo = _perfectrec_prepad(p.fsize, p.fshift) if p.perfectrec else 0
    full = np.zeros(total)
    y = sc.stream_mixture(p, y, T) if open_end else y
    full[lo: lo + y.shape[0]] = y
    if p.perfectrec and not open_end:
        full[max(total - (p.fsize - p.fshift), 0):] = 0.0
    return np.stack([np.fft.rfft(p.awin * full[p.fshift * j: p.fshift * j + p.fsize]) for j in range(T)])


def check_entries(key, out, open_end=False):
    """(a): rows without iterations against A X / |X| on the bins with |X| >= TAU max|X|; exact A + 0j where X == 0."""
    p, A, y = sc.misi_case(*key)
    out = out.cpu().numpy().astype(np.complex128)
    assert out.shape == A.shape and np.isfinite(out.view(np.float64)).all()
    m = MARGINS["entry"].setdefault(key_id(key), {"cases": 0, "max_error_over_bound": 0.0, "max_left_out": 0.0})
    for b in range(A.shape[0]):
        X = mixture_rows(p, y[b].astype(np.float64), key[3], open_end)
        mag = np.abs(X)
        use = mag >= sc.TAU * mag.max(axis=1, keepdims=True)
        left_out = np.mean(~use)
        unit = X / np.where(mag > 0, mag, 1.0)
        worst = 0.0
        for k in range(key[4]):
            err = np.abs(out[b, k] - A[b, k] * unit)
            bound = 3 * np.sqrt(2) * sc.SIGMA / sc.TAU * A[b, k] + 2e-6 * A[b, k].max()
            worst = max(worst, (err / bound)[use].max())
            silent = ~mag.any(axis=1)
            assert np.array_equal(out[b, k][silent], (A[b, k] + 0j)[silent])
        print("mixture entry %s b=%d: error %.3f of its bound, %.3f%% of the bins left out" % (key_id(key), b, worst, 100 * left_out))
        m["cases"] += 1
        m["max_error_over_bound"] = max(m["max_error_over_bound"], float(worst))
        m["max_left_out"] = max(m["max_left_out"], float(left_out))
        assert worst <= 1.0 and left_out <= sc.MAX_LEFT_OUT, (b, worst, left_out)


def compare_whole(tag, group, key, out, s, ref, ref_s, per, per_s):
    """The rule of tests/test_gpu_misi_la.py."""
    p, A, y = sc.misi_case(*key)
    B, K = A.shape[:2]
    out, s = out.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.float64)
    assert out.shape == A.shape and s.shape == (B, K, y.shape[1])
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
    m = MARGINS[group].setdefault(key_id(key), {"cases": 0, "max_rel_l2": 0.0, "max_rel_l2_over_bar": 0.0, "max_far_fraction": 0.0,
                                                "max_magnitude_error": 0.0, "max_mixture_error_over_bound": 0.0,
                                                "max_signal_error_over_bar": 0.0})
    for b in range(B):
        x_host = [p.istft(ref[b, k]) for k in range(K)]
        mix, mix_bar = np.abs(s[b].sum(axis=0) - y[b]).max(), mixture_bound(K, y[b], x_host)
        print("%s b=%d: |sum s - y| %.2e (bound %.2e)" % (tag, b, mix, mix_bar))
        m["max_mixture_error_over_bound"] = max(m["max_mixture_error_over_bound"], float(mix / mix_bar))
        assert mix <= mix_bar, (b, mix, mix_bar)
        for k in range(K):
            top = A[b, k].max()
            dist, bar = sc.rel(out[b, k], ref[b, k]), 3 * sc.rel(per[b, k], ref[b, k])
            far = sc.far_fraction(out[b, k], ref[b, k], top)
            mag = np.abs(np.abs(out[b, k]) - A[b, k]).max() / top
            ds = np.abs(s[b, k] - ref_s[b, k]).max()
            bar_s = 3 * np.abs(per_s[b, k] - ref_s[b, k]).max() + 3e-6 * np.abs(ref_s[b, k]).max()
            print("%s b=%d k=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal off %.2e (bar %.2e)"
                  % (tag, b, k, dist, bar, 100 * far, mag, ds, bar_s))
            m["cases"] += 1
            for name, v in (("max_rel_l2", dist), ("max_rel_l2_over_bar", dist / bar), ("max_far_fraction", far),
                            ("max_magnitude_error", mag), ("max_signal_error_over_bar", ds / bar_s)):
                m[name] = max(m[name], float(v))
            assert dist <= bar, (b, k, dist, bar)
            assert far <= 1e-3, (b, k, far)
            assert mag <= 2e-6, (b, k, mag)
            assert ds <= bar_s, (b, k, ds, bar_s)


@pytest.mark.parametrize("key", sorted(KEYS), ids=key_id)
def test_entries_and_whole_runs_match_host(key):
    p, A, y = sc.misi_case(*key)
    threads, in_lds = KEYS[key]
    assert_placement(key, 3, in_lds, threads, K=key[4])
    tA, ty = dev(A, np.float32), dev(y, np.float32)
    for LA in (0, 3):
        out, s = p.misi_la_dev(tA, ty, 0, look_ahead=LA, start="mixture", return_signals=True)
        check_entries(key, out)
        assert (np.abs(s.cpu().numpy().astype(np.float64).sum(axis=1) - y).max(axis=1)
                <= [mixture_bound(key[4], y[b], [p.istft(c) for c in out[b].cpu().numpy().astype(np.complex128)]) for b in range(3)]).all()
    steps = STEPS if key[0] <= 1024 else [(0, 1), (3, 3), (5, 2)]
    for LA, n in steps:
        ref, ref_s = sc.misi_host(key, LA, n)
        per, per_s = sc.misi_host(key, LA, n, seed=n + 17)
        out, s = p.misi_la_dev(tA, ty, n, look_ahead=LA, start="mixture", return_signals=True)
        assert out.dtype == torch.complex64 and s.dtype == torch.float32
        compare_whole("mixture %s LA=%d n=%d" % (key_id(key), LA, n), "whole", key, out, s, ref, ref_s, per, per_s)


@pytest.mark.parametrize("key", [(64, 16, True, 12, 4), (1000, 250, True, 5, 2), (2048, 512, False, 6, 2), (4096, 1024, False, 6, 2)], ids=key_id)
def test_phases_are_ignored_and_stack_equals_members_bit_for_bit(key):
    p, A, y = sc.misi_case(*key)
    rng = np.random.default_rng(5)
    real, ty = dev(A, np.float32), dev(y, np.float32)
    phased = dev(A * np.exp(2j * np.pi * rng.random(A.shape)), np.complex64)
    quarter = dev(A * np.array([1, 1j, -1, -1j])[rng.integers(0, 4, A.shape)], np.complex64)       # |S| is A exactly
    for n in (0, 3):
        ref, x = p.misi_la_dev(real, ty, n, start="mixture", return_signals=True)
        for S, given in ((real + 0j, None), (quarter, None), (phased, real), (torch.zeros_like(phased), real)):
            out, s = p.misi_la_dev(S, ty, n, start="mixture", magnitudes=given, return_signals=True)
            assert torch.equal(out, ref) and torch.equal(s, x)
        assert torch.equal(ref, p.misi_la_dev(real, ty, n, start="mixture"))             # with and without the signals, and again
        for b in range(A.shape[0]):
            one, one_s = p.misi_la_dev(real[b], ty[b], n, start="mixture", return_signals=True)
            assert torch.equal(one, ref[b]) and torch.equal(one_s, x[b])
    assert torch.equal(p.misi_la_dev(A, y, 2, start="mixture"), p.misi_la_dev(real, ty, 2, start="mixture"))   # numpy, float64


def test_device_identity_with_the_given_start():
    """The entry rows a run without iterations returns, given back as the start of a 'given' run, give the mixture-start run up to
    the pairing of the entry transforms (one frame per transform there, two here): held by the rule of the whole runs."""
    key = (64, 16, True, 12, 4)
    p, A, y = sc.misi_case(*key)
    tA, ty = dev(A, np.float32), dev(y, np.float32)
    S0 = p.misi_la_dev(tA, ty, 0, start="mixture")
    assert torch.equal(S0, p.misi_la_dev(S0, ty, 0, magnitudes=tA))
    out, s = p.misi_la_dev(S0, ty, 3, magnitudes=tA, return_signals=True)
    ref, ref_s = sc.misi_host(key, 3, 3)
    per, per_s = sc.misi_host(key, 3, 3, seed=20)
    compare_whole("given from mixture rows %s" % key_id(key), "whole", key, out, s, ref, ref_s, per, per_s)


@pytest.mark.parametrize("key", [(64, 16, True, 12, 4), (512, 128, False, 40, 2)], ids=key_id)
def test_causality_bit_for_bit(key):
    """At LA = 3 other magnitudes in the frames >= 6, or another mixture from the uncut sample hop 5 + N on, leave the output frames
    0..2 as they are and change frame 3."""
    p, A, y = sc.misi_case(*key)
    rng = np.random.default_rng(3)
    B_ = A.copy()
    B_[:, :, 6:] = np.roll(A[:, :, 6:], 1, axis=3) * 1.3
    lo = _perfectrec_prepad(p.fsize, p.fshift) if p.perfectrec else 0
    first = p.fshift * 5 + p.fsize - lo
    assert 0 < first < y.shape[1]
    y1 = y.copy()
    y1[:, first:] += (np.abs(y).max(axis=1, keepdims=True) * rng.standard_normal(y1[:, first:].shape)).astype(np.float32)
    a = p.misi_la_dev(A, y, 3, look_ahead=3, start="mixture").cpu().numpy()
    for other in (p.misi_la_dev(B_, y, 3, look_ahead=3, start="mixture").cpu().numpy(),
                  p.misi_la_dev(A, y1, 3, look_ahead=3, start="mixture").cpu().numpy()):
        assert np.array_equal(a[:, :, :3], other[:, :, :3])
        for b in range(A.shape[0]):
            for k in range(A.shape[1]):
                assert not np.array_equal(a[b, k, 3], other[b, k, 3])


def test_silent_mixture_gives_exact_rows():
    key = (64, 16, True, 12, 2)
    p, A, y = sc.misi_case(*key)
    y0 = y.copy()
    y0[:, :p.fshift * 7] = 0.0                    # the frames that lie wholly in the silence enter as A + 0j
    y0[1] = 0.0                                   # a whole mixture of silence
    Z = A.copy()
    Z[2] = 0.0                                    # ... and silent sources under a mixture that is not
    out = p.misi_la_dev(Z, y0, 0, start="mixture").cpu().numpy()
    Zf = Z.astype(np.float32)
    X = np.stack([mixture_rows(p, v.astype(np.float64), key[3]) for v in y0])
    silent = ~np.abs(X).any(axis=2)
    assert silent[1].all() and silent[0].sum() >= 3 and not silent[0].all()
    for b in range(3):
        assert np.array_equal(out[b][:, silent[b]], (Zf[b] + 0j)[:, silent[b]])
    assert (out[2] == 0).all()
    out, s = p.misi_la_dev(Z, y0, 4, start="mixture", return_signals=True)
    out, s = out.cpu().numpy(), s.cpu().numpy()
    assert np.isfinite(out.view(np.float32)).all() and np.isfinite(s).all() and (out[2] == 0).all()
    assert np.abs(np.abs(out) - Z).max() <= 2e-6 * Z.max()


def test_given_is_the_default_bit_for_bit():
    import misi_la_cases as mc
    key = (64, 16, True, 12, 3)
    p, A, c0, y = mc.case(*key)
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    for n in (0, 3):
        a, xa = p.misi_la_dev(t, ty, n, return_signals=True)
        b, xb = p.misi_la_dev(t, ty, n, return_signals=True, start="given")
        assert torch.equal(a, b) and torch.equal(xa, xb)
        s1, s2 = p.misi_la_stream(3, n, batch=3, return_signals=True), p.misi_la_stream(3, n, batch=3, return_signals=True, start="given")
        ypad = torch.from_numpy(sc.stream_mixture(p, y, key[3])).cuda()
        for s in (s1, s2):
            n5 = s.samples_needed(5)
            first = s.push(t[:, :, :5], ypad[:, :n5])
            s.rows = [first, s.push(t[:, :, 5:], ypad[:, n5:n5 + s.samples_needed(7)]), s.finish()]
            s.close()
        for (f1, x1), (f2, x2) in zip(s1.rows, s2.rows):
            assert torch.equal(f1, f2) and torch.equal(x1, x2)


# ---- the stream
def run_stream(p, K, rows, ypad, LA, n, chunks, batch="stack", magnitudes=None):
    """Push `rows` (B, K, T, F), real or complex, and the mixture by samples_needed, in `chunks`; finish."""
    T = rows.shape[-2]
    assert sum(chunks) == T
    s = p.misi_la_stream(K, n, look_ahead=LA, batch=None if batch is None else rows.shape[0], return_signals=True, start="mixture")
    frames, sig, at, yat = [], [], 0, 0
    for k in chunks:
        ns = s.samples_needed(k)
        out, x = s.push(rows[..., at:at + k, :], ypad[..., yat:yat + ns], None if magnitudes is None else magnitudes[..., at:at + k, :])
        assert out.dtype == torch.complex64 and x.dtype == torch.float32
        at, yat = at + k, yat + ns
        frames.append(out)
        sig.append(x)
    assert yat == ypad.shape[-1]
    out, x = s.finish()
    frames.append(out)
    sig.append(x)
    s.close()
    return torch.cat(frames, dim=-2), torch.cat(sig, dim=-1)


@pytest.mark.parametrize("key", STREAM_KEYS, ids=key_id)
def test_stream_chunking_changes_no_bit_and_matches_host(key):
    p, A, y = sc.misi_case(*key)
    T, K = key[3], key[4]
    tA, ypad = dev(A, np.float32), dev(sc.stream_mixture(p, y, T), np.float32)
    same = {}
    for LA, n in [(3, 0), (0, 0), (0, 2), (3, 3), (5, 2)]:
        ref = None
        for chunks in ([T], [1] * T, [2, 0, 1, T - 3]):
            got = run_stream(p, K, tA, ypad, LA, n, chunks)
            if ref is None:
                ref = got
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (LA, n, chunks)
        assert ref[1].shape[-1] == y.shape[1]
        one = run_stream(p, K, tA[1], ypad[1], LA, n, [1] * T, batch=None)
        assert torch.equal(one[0], ref[0][1]) and torch.equal(one[1], ref[1][1])
        if n == 0:
            check_entries(key, ref[0], open_end=True)
        else:
            hr, hs = sc.misi_host(key, LA, n, open_end=True)
            pr, ps = sc.misi_host(key, LA, n, seed=n + 17, open_end=True)
            compare_whole("mixture stream %s LA=%d n=%d" % (key_id(key), LA, n), "stream", key, ref[0], ref[1], hr, hs, pr, ps)
            same["LA=%d n=%d" % (LA, n)] = bool(torch.equal(ref[0], p.misi_la_dev(tA, dev(y, np.float32), n, look_ahead=LA, start="mixture")))
    print("stream %s has the bits of misi_la_dev(..., start='mixture'): %s" % (key_id(key), same))
    MARGINS["stream"].setdefault("same_bits_as_misi_la_dev", {})[key_id(key)] = same


def test_push_takes_real_and_complex_rows():
    key = (64, 16, True, 12, 4)
    p, A, y = sc.misi_case(*key)
    rng = np.random.default_rng(9)
    real, ypad = dev(A, np.float32), dev(sc.stream_mixture(p, y, 12), np.float32)
    phased = dev(A * np.exp(2j * np.pi * rng.random(A.shape)), np.complex64)
    quarter = dev(A * np.array([1, 1j, -1, -1j])[rng.integers(0, 4, A.shape)], np.complex64)
    ref = run_stream(p, 4, real, ypad, 3, 3, [5, 7])
    for rows, given in ((quarter, None), (real + 0j, None), (phased, real), (torch.zeros_like(phased), real)):
        got = run_stream(p, 4, rows, ypad, 3, 3, [5, 7], magnitudes=given)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_invalid_arguments_raise_with_nothing_enqueued():
    key = (64, 16, True, 12, 2)
    p, A, y = sc.misi_case(*key)
    for bad in ("overlap", "zero", None, 2):
        with pytest.raises(ValueError, match="start"):
            p.misi_la_dev(A, y, 2, start=bad)
        with pytest.raises(ValueError, match="start"):
            p.misi_la_stream(2, 2, start=bad)
        with pytest.raises(ValueError, match="start"):
            lws_amd.MisiLaStream(2, 64, 16, p.awin, p.swin, 2, start=bad)
    for bad in (dict(iterations=-1), dict(iterations=2, look_ahead=-1), dict(iterations=2, magnitudes=A[:, :, :-1])):
        with pytest.raises(ValueError):
            p.misi_la_dev(A, y, start="mixture", **bad)
    with pytest.raises(ValueError):
        p.misi_la_dev(A, y[:, :-1], 2, start="mixture")
    lib, w = lws_amd._capi.load(), np.ascontiguousarray(p.awin, dtype=np.float64)
    t, ty = dev(A + 0j, np.complex64), dev(y, np.float32)
    keep = t.clone()
    for start in (lws_amd._capi.LWS_START_OVERLAP, 3, -1):
        rc = lib.lws_misi_la_dev_ex(0, t.data_ptr(), None, ty.data_ptr(), None, 3, 2, 12, 64, 16, w.ctypes.data, w.ctypes.data, 1, 2, 3, start,
                                    None)
        assert rc == lws_amd._capi.LWS_ERR_INVALID
        h = ctypes.c_void_p()
        rc = lib.lws_misi_stream_create_ex(0, 3, 2, 64, 16, w.ctypes.data, w.ctypes.data, 1, 2, 3, start, ctypes.byref(h))
        assert rc == lws_amd._capi.LWS_ERR_INVALID and not h.value
    torch.cuda.synchronize()
    assert torch.equal(t, keep)
    s = p.misi_la_stream(2, 2, batch=3, start="mixture")
    n4 = s.samples_needed(4)
    with pytest.raises(ValueError):
        s.push(A[:, :, :4], y[:, :n4 - 1])
    nf, ns = ctypes.c_int(7), ctypes.c_int(7)                                       # neither rows nor magnitudes
    rc = lib.lws_misi_stream_push(s._h, None, None, ty.data_ptr(), 4, n4, None, None, ctypes.byref(nf), ctypes.byref(ns), None)
    assert rc == lws_amd._capi.LWS_ERR_INVALID and (nf.value, ns.value) == (0, 0)
    assert s.push(A[:, :, :4], y[:, :n4]).shape[2] == 1
    s.close()


def test_zz_margins_actually_achieved():
    """What the cases above reached (written to $LWS_MARGINS_DIR/start_margins_misi.json when that variable names a directory;
    profiles/start_margins.json holds a copy under "misi").  On an MI355X: entry rows at most 0.4 % of their bound, at most 0.1 % of the
    bins left out; 390 whole-run rows and 135 streamed ones at most 8.1 % of their bar, no bin beyond 1e-3 max A, magnitudes within 1.4e-7
    max A, |sum s - y| at most 5.1 % of its bound, signals at most 6.9 % of their bar; the whole file in 5.1 s."""
    if not MARGINS["entry"]:
        key = (64, 16, True, 12, 4)
        p, A, y = sc.misi_case(*key)
        check_entries(key, p.misi_la_dev(A, y, 0, start="mixture"))
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "start_margins_misi.json"), "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)
            f.write("\n")
    print(MARGINS)
    assert all(v["max_error_over_bound"] <= 1.0 for v in MARGINS["entry"].values())
    assert all(v["max_rel_l2_over_bar"] <= 1.0 for g in ("whole", "stream") for k, v in MARGINS[g].items() if k != "same_bits_as_misi_la_dev")
