"""GPU: streaming online MISI (MisiLaStream, k_misi_la_stream of lws_gla.hip): rows and mixture samples pushed as they arrive, the
state on the device.

The definition is the host's misi_la(..., open_end=True) of everything pushed (tests/misi_la_stream_cases.py has the inputs and the
references).  What is held here: however the input is cut into chunks the stream returns the same bits; it meets the host definition
by the bars of tests/test_gpu_misi_la.py, measured from the host (per mixture and source: the rel-L2 distance the host iteration
moves under a 1e-6 perturbation of every projection, times 3; at most 0.1 % of the bins further than 1e-3 max A_k; magnitudes within
2e-6 max A_k; |sum_k s_k - y| within mixture_bound of tests/test_gpu_misi.py and each signal within the bar_s that file and
test_gpu_misi_la.py use, 3 x what the model moves it + 3e-6 max|s_k|); it agrees with the one-shot misi_la_dev wherever the two
definitions coincide; streams do not see each other.  Every figure is printed before it is asserted (pytest -s)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import lws_amd
import misi_la_stream_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_misi import mixture_bound  # noqa: E402
from test_gpu_rtisi import assert_placement  # noqa: E402

MARGINS = {}   # "fsize,fshift,perfectrec" -> figures against the host; ["vs_misi_la_dev"]: against the one-shot kernel


def chunkings(T):
    return [[T], [1] * T, [2, 0, 1, T - 3]]


def run_stream(p, c0, y, LA, n, chunks, magnitudes=None, batch="stack", disturb=False):
    """Push c0 (B, K, T, F) and y (B, need(T)) -- or (K, T, F) and (need(T),) with batch=None -- in `chunks`, finish; returns the
    concatenated frames and signals.  disturb: before every push, one with a sample too few, which must raise and change nothing."""
    B = None if batch is None else c0.shape[0]
    K, T = c0.shape[-3], c0.shape[-2]
    assert sum(chunks) == T
    t, ty = torch.from_numpy(np.array(c0)).cuda(), torch.from_numpy(np.array(y)).cuda()   # (copies: the cases are read-only)
    A = None if magnitudes is None else torch.from_numpy(np.ascontiguousarray(magnitudes, dtype=np.float32)).cuda()
    s = p.misi_la_stream(K, n, look_ahead=LA, batch=B, return_signals=True)
    key = (p.fsize, p.fshift, p.perfectrec)
    lo = sc.lead_in(key)
    frames, sig, entered, committed, at, yat = [], [], 0, 0, 0, 0
    for k in chunks:
        ns = s.samples_needed(k)
        assert ns == sc.need(key, entered + k) - sc.need(key, entered)
        if disturb and ns > 0:
            with pytest.raises(ValueError):
                s.push(t[..., at:at + k, :], ty[..., yat:yat + ns - 1])
        out, x = s.push(t[..., at:at + k, :], ty[..., yat:yat + ns], None if A is None else A[..., at:at + k, :])
        at, yat, entered = at + k, yat + ns, entered + k
        want = max(0, entered - LA) - committed
        want_x = max(0, p.fshift * (committed + want) - max(p.fshift * committed, lo)) if want else 0
        assert out.shape[-2] == want and x.shape[-1] == want_x, (chunks, k, tuple(out.shape), want, tuple(x.shape), want_x)
        assert out.dtype == torch.complex64 and x.dtype == torch.float32
        committed += want
        frames.append(out)
        sig.append(x)
    assert yat == ty.shape[-1]
    out, x = s.finish()
    assert out.shape[-2] == T - committed
    frames.append(out)
    sig.append(x)
    s.close()
    frames, sig = torch.cat(frames, dim=-2), torch.cat(sig, dim=-1)
    assert tuple(frames.shape) == c0.shape
    assert sig.shape[-1] == max(lws_amd._capi.istft_length(T, p.fsize, p.fshift, p.perfectrec), 0) and sig.shape[:-1] == frames.shape[:-2]
    return frames, sig


def inputs(key, rows=None):
    p, A, c0, y = sc.open_case(*key)
    T1 = key[3] if rows is None else rows
    return p, A[:, :, :T1], c0[:, :, :T1], y[:, :sc.need(key, T1)]


@functools.lru_cache(maxsize=None)
def streamed(key, LA, n):
    """The stream's result for the whole case pushed at once (chunking changes no bit: test_chunking_changes_no_bit)."""
    p, A, c0, y = inputs(key)
    return run_stream(p, c0, y, LA, n, [key[3]])


def margins(key):
    return MARGINS.setdefault("%d,%d,%s" % key[:3], {"cases": 0, "max_rel_l2": 0.0, "max_rel_l2_over_bar": 0.0, "max_far_fraction": 0.0,
                                                     "max_magnitude_error": 0.0, "max_mixture_error_over_bound": 0.0,
                                                     "max_signal_error_over_bar": 0.0})


def check_against_host(key, LA, n, chunks=None, explicit=False, rows=None):
    p, A, c0, y = inputs(key, rows)
    B, K, T = c0.shape[:3]
    ref, ref_s = sc.host_open(key, LA, n, explicit, rows)
    per, per_s = sc.host_open_perturbed(key, LA, n, explicit, rows)
    target = sc.magnitudes_of(A) if explicit else A
    if explicit or rows is not None or chunks is not None:
        out, s = run_stream(p, c0, y, LA, n, chunks or [T], magnitudes=target if explicit else None)
    else:
        out, s = streamed(key, LA, n)
    out, s = out.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
    assert s.shape == ref_s.shape
    tag = "misi_la stream %s T=%d LA=%d n=%d%s" % (sc.key_id(key), T, LA, n, " explicit A" if explicit else "")
    m = margins(key)
    for b in range(B):
        if s.shape[-1]:
            x_host = [p.istft(ref[b, k]) for k in range(K)]
            yb = y[b, :s.shape[-1]]
            mix, mix_bar = np.abs(s[b].sum(axis=0) - yb).max(), mixture_bound(K, yb, x_host)
            print("%s b=%d: |sum s - y| %.2e (bound %.2e)" % (tag, b, mix, mix_bar))
            m["max_mixture_error_over_bound"] = max(m["max_mixture_error_over_bound"], float(mix / mix_bar))
            assert mix <= mix_bar, (b, mix, mix_bar)
        for k in range(K):
            top = target[b, k].max()
            dist, bar = sc.rel(out[b, k], ref[b, k]), 3 * sc.rel(per[b, k], ref[b, k])
            far = np.mean(np.abs(out[b, k] - ref[b, k]) > 1e-3 * top)
            mag = np.abs(np.abs(out[b, k]) - target[b, k]).max() / top
            ds = bar_s = 0.0
            if s.shape[-1]:
                ds = np.abs(s[b, k] - ref_s[b, k]).max()
                bar_s = 3 * np.abs(per_s[b, k] - ref_s[b, k]).max() + 3e-6 * np.abs(ref_s[b, k]).max()
            print("%s b=%d k=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal off %.2e (bar %.2e)"
                  % (tag, b, k, dist, bar, 100 * far, mag, ds, bar_s))
            m["cases"] += 1
            for name, v in (("max_rel_l2", dist), ("max_rel_l2_over_bar", dist / bar), ("max_far_fraction", far),
                            ("max_magnitude_error", mag), ("max_signal_error_over_bar", ds / bar_s if bar_s else 0.0)):
                m[name] = max(m[name], float(v))
            assert dist <= bar, (b, k, dist, bar)
            assert far <= 1e-3, (b, k, far)
            assert mag <= 2e-6, (b, k, mag)
            assert ds <= bar_s, (b, k, ds, bar_s)


def check_chunking(key, LA, n):
    p, A, c0, y = inputs(key)
    whole, whole_x = streamed(key, LA, n)
    for chunks in chunkings(key[3])[1:]:
        out, x = run_stream(p, c0, y, LA, n, chunks)
        assert torch.equal(out, whole) and torch.equal(x, whole_x), (LA, n, chunks)


@pytest.mark.parametrize("key", sc.GPU_KEYS, ids=sc.key_id)
def test_chunking_changes_no_bit(key):
    """Pushed whole, a row at a time, and with a chunk shorter than LA + 1 and an empty one: the same frames, signals and counts."""
    for LA, n in sc.STEPS:
        check_chunking(key, LA, n)


@pytest.mark.parametrize("key", sc.GPU_KEYS, ids=sc.key_id)
def test_matches_host_open_end(key):
    for LA, n in sc.STEPS:
        check_against_host(key, LA, n)


@pytest.mark.parametrize("key", sc.GPU_KEYS, ids=sc.key_id)
def test_against_the_one_shot_kernel(key):
    """misi_la_dev knows the end: its denominator stops at the last frame and, under perfectrec, it cuts the tail inside the iteration.
    Where neither reaches -- the frames < P and the samples they finalise -- the stream computes the same thing with another kernel.
    Held to the bars of the host comparison; whether the bits are equal is measured and recorded, not required."""
    p, A, c0, y = inputs(key)
    closed_y = sc.case(*key)[3]
    B, K, T = c0.shape[:3]
    rec = margins(key).setdefault("vs_misi_la_dev", {"bits_equal": True, "frames_compared": 0, "max_abs_diff_over_max_A": 0.0,
                                                     "max_signal_diff_over_bar": 0.0})
    for LA, n in sc.STEPS:
        P, k = sc.coincide(key, LA)
        out, x = streamed(key, LA, n)
        one, one_x = p.misi_la_dev(c0, closed_y, n, look_ahead=LA, return_signals=True)
        same = torch.equal(out[:, :, :P], one[:, :, :P]) and torch.equal(x[..., :k], one_x[..., :k])
        a, b = out[:, :, :P].cpu().numpy().astype(np.complex128), one[:, :, :P].cpu().numpy().astype(np.complex128)
        xa, xb = x[..., :k].cpu().numpy().astype(np.float64), one_x[..., :k].cpu().numpy().astype(np.float64)
        ref, ref_s = sc.host_open(key, LA, n)
        per, per_s = sc.host_open_perturbed(key, LA, n)
        diff = sdiff = 0.0
        for i in range(B):
            for j in range(K):
                top = A[i, j].max()
                if P:
                    dist, bar = sc.rel(a[i, j], b[i, j]), 3 * sc.rel(per[i, j, :P], ref[i, j, :P])
                    far = np.mean(np.abs(a[i, j] - b[i, j]) > 1e-3 * top)
                    diff = max(diff, np.abs(a[i, j] - b[i, j]).max() / top)
                    assert dist <= bar, (LA, n, i, j, dist, bar)
                    assert far <= 1e-3, (LA, n, i, j, far)
                if k:
                    sd = np.abs(xa[i, j] - xb[i, j]).max()
                    bar_s = 3 * np.abs(per_s[i, j, :k] - ref_s[i, j, :k]).max() + 3e-6 * np.abs(ref_s[i, j, :k]).max()
                    sdiff = max(sdiff, sd / bar_s)
                    assert sd <= bar_s, (LA, n, i, j, sd, bar_s)
        print("misi_la stream vs misi_la_dev %s LA=%d n=%d: %d of %d frames compared, bits equal: %s, largest difference %.2e max A, "
              "signal %.2e of its bar" % (sc.key_id(key), LA, n, P, T, same, diff, sdiff))
        rec["bits_equal"] = bool(rec["bits_equal"] and same)
        rec["frames_compared"] += P
        rec["max_abs_diff_over_max_A"] = max(rec["max_abs_diff_over_max_A"], float(diff))
        rec["max_signal_diff_over_bar"] = max(rec["max_signal_diff_over_bar"], float(sdiff))


@pytest.mark.parametrize("key", sorted(sc.PLACEMENTS), ids=sc.key_id)
def test_placements(key):
    """On both sides of the LDS boundary, at the cap, with a workgroup of 768 threads and with more active frames than overlap: the
    stream is placed as lws_rtisi_la_placement says, returns the same bits however it is chunked, and meets the host."""
    threads, steps = sc.PLACEMENTS[key]
    for LA, n, in_lds in steps:
        assert_placement(key, LA, in_lds, threads, K=key[4])
        if key[:2] == (2048, 512):
            assert lws_amd._capi.rtisi_la_placement(2048, 512, LA, 1)[2] == 160 * 1024   # the cap, to the byte
        check_chunking(key, LA, n)
        check_against_host(key, LA, n)


@pytest.mark.parametrize("run", sc.EARLY_END, ids=lambda r: "%s-rows%d" % (sc.key_id(r[0]), r[3]))
def test_end_before_the_first_commit_closes_with_the_clamped_plan(run):
    """A stream created with its state in scratch that ends after rows <= LA frames closes with a look-ahead of rows - 1, on the state
    buffer sized and strided at creation."""
    key, LA, n, rows = run
    assert_placement(key, LA, False, 1024, K=key[4])                                    # as created
    print("closing placement:", lws_amd._capi.rtisi_la_placement(key[0], key[1], rows - 1, key[4]))
    check_against_host(key, LA, n, chunks=[1] * rows, rows=rows)
    p, A, c0, y = inputs(key, rows)
    a, b = run_stream(p, c0, y, LA, n, [1] * rows), run_stream(p, c0, y, LA, n, [rows])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("run", sc.SHORT, ids=lambda r: "%s-LA%d-rows%d" % (sc.key_id(r[0]), r[1], r[3]))
def test_fewer_frames_than_the_look_ahead(run):
    """T <= LA: no push can commit anything (run_stream checks the counts); finish() runs them as one call on T frames would."""
    key, LA, n, rows = run
    check_against_host(key, LA, n, chunks=[1] * rows, rows=rows)
    p, A, c0, y = inputs(key, rows)
    a, b = run_stream(p, c0, y, LA, n, [1] * rows), run_stream(p, c0, y, LA, n, [rows])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("key", [(64, 16, True, 12, 3), (48, 16, False, 7, 2)], ids=sc.key_id)
def test_explicit_magnitudes_chunk_by_chunk(key):
    T = key[3]
    check_against_host(key, 3, 3, chunks=[1] * T, explicit=True)
    p, A, c0, y = inputs(key)
    a = run_stream(p, c0, y, 3, 3, [1] * T, magnitudes=sc.magnitudes_of(A))
    b = run_stream(p, c0, y, 3, 3, [T], magnitudes=sc.magnitudes_of(A))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_streams_do_not_see_each_other():
    key, LA, n = (64, 16, True, 12, 3), 3, 3
    p, A, c0, y = inputs(key)
    whole, whole_x = streamed(key, LA, n)
    # a batch=3 stream against its members as single streams
    for b in range(c0.shape[0]):
        one, one_x = run_stream(p, c0[b], y[b], LA, n, [5, 7], batch=None)
        assert tuple(one.shape) == c0.shape[1:] and one_x.dim() == 2
        assert torch.equal(one, whole[b]) and torch.equal(one_x, whole_x[b])
    # two streams pushed alternately against each alone
    t, ty = torch.from_numpy(np.array(c0)).cuda(), torch.from_numpy(np.array(y)).cuda()
    other, other_y = torch.flip(t, dims=[0]), torch.flip(ty, dims=[0])
    alone = run_stream(p, other.cpu().numpy(), other_y.cpu().numpy(), LA, n, [12])
    s1, s2 = (p.misi_la_stream(3, n, look_ahead=LA, batch=3, return_signals=True) for _ in range(2))
    got1, got2, yat = [], [], 0
    for at in range(0, 12, 3):
        ns = s1.samples_needed(3)
        assert ns == s2.samples_needed(3)
        got1.append(s1.push(t[:, :, at:at + 3], ty[:, yat:yat + ns]))
        got2.append(s2.push(other[:, :, at:at + 3], other_y[:, yat:yat + ns]))
        yat += ns
    got1.append(s1.finish())
    got2.append(s2.finish())
    for got, (want, want_x) in ((got1, (whole, whole_x)), (got2, alone)):
        assert torch.equal(torch.cat([g[0] for g in got], dim=2), want)
        assert torch.equal(torch.cat([g[1] for g in got], dim=2), want_x)
    # a stream created after others were closed against the first one
    s1.close()
    s2.close()
    again, again_x = run_stream(p, c0, y, LA, n, [4, 8])
    assert torch.equal(again, whole) and torch.equal(again_x, whole_x)


def test_wrong_sample_count_raises_and_the_stream_goes_on():
    """Before every push one with a sample too few, through the Python check and, once, through the C entry point's own: both raise,
    and the stream then continues to the bits of an undisturbed one."""
    key, LA, n = (64, 16, True, 12, 3), 3, 3
    p, A, c0, y = inputs(key)
    whole, whole_x = streamed(key, LA, n)
    out, x = run_stream(p, c0, y, LA, n, [2, 3, 1, 6], disturb=True)
    assert torch.equal(out, whole) and torch.equal(x, whole_x)
    t, ty = torch.from_numpy(np.array(c0)).cuda(), torch.from_numpy(np.array(y)).cuda()
    s = p.misi_la_stream(3, n, look_ahead=LA, batch=3, return_signals=True)
    ns = s.samples_needed(5)
    first = s.push(t[:, :, :5], ty[:, :ns])
    res, sig = torch.empty((3, 3, 7, 33), dtype=torch.complex64, device="cuda"), torch.empty((3, 3, 7 * 16), device="cuda")
    bad = ty[:, ns:-1].contiguous()
    assert bad.shape[1] == s.samples_needed(7) - 1
    with pytest.raises(ValueError, match="mixture samples"):
        lws_amd._capi.misi_stream_push(s._h, t[:, :, 5:].contiguous().data_ptr(), None, bad.data_ptr(), 7, bad.shape[1], res.data_ptr(),
                                       sig.data_ptr())
    rest = s.push(t[:, :, 5:], ty[:, ns:])
    last = s.finish()
    assert torch.equal(torch.cat([first[0], rest[0], last[0]], dim=2), whole)
    assert torch.equal(torch.cat([first[1], rest[1], last[1]], dim=2), whole_x)


def test_edges():
    key = (64, 16, True, 12, 3)
    p, A, c0, y = inputs(key)
    F = c0.shape[3]
    # nothing pushed
    s = p.misi_la_stream(3, 3, return_signals=True)
    out, x = s.finish()
    assert tuple(out.shape) == (3, 0, F) and tuple(x.shape) == (3, 0) and out.dtype == torch.complex64 and x.dtype == torch.float32
    s = p.misi_la_stream(3, 3, batch=3)
    assert s.samples_needed(0) == 0
    assert tuple(s.push(c0[:, :, :0], y[:, :0]).shape) == (3, 3, 0, F) and tuple(s.finish().shape) == (3, 3, 0, F)
    # no iterations: the rows themselves, LA frames late, and the signals of the definition
    t = torch.from_numpy(np.array(c0)).cuda()
    ref_s = sc.host_open(key, 3, 0)[1]
    for chunks in ([12], [1] * 12, [5, 7]):
        out, x = run_stream(p, c0, y, 3, 0, chunks)
        assert torch.equal(out, t)
        assert (np.abs(x.cpu().numpy() - ref_s).max(axis=2) <= 3e-6 * np.abs(ref_s).max(axis=2)).all()
    # digital silence, with a zero mixture
    out, x = run_stream(p, np.zeros_like(c0), np.zeros_like(y), 3, 3, [5, 7])
    assert (out.cpu().numpy() == 0).all() and (x.cpu().numpy() == 0).all()
    # misuse, before anything is enqueued
    s = p.misi_la_stream(3, 3, batch=3)
    n4 = s.samples_needed(4)
    for bad in (c0[:, :, :4, :-1], c0[:2, :, :4], c0[0, :, :4], c0[:, :2, :4]):
        with pytest.raises(ValueError):
            s.push(bad, y[:, :n4])
    for bad in (y[:, :n4 - 1], y[:, :n4 + 1], y[0, :n4], y[:2, :n4]):
        with pytest.raises(ValueError):
            s.push(c0[:, :, :4], bad)
    with pytest.raises(ValueError):
        s.push(c0[:, :, :4], y[:, :n4], magnitudes=A[:, :, :3])
    assert tuple(s.push(c0[:, :, :4], y[:, :n4]).shape) == (3, 3, 1, F)
    s.finish()
    with pytest.raises(ValueError):
        s.push(c0[:, :, 4:8], y[:, n4:n4 + 64])
    with pytest.raises(ValueError):
        s.finish()
    s.close()
    with pytest.raises(ValueError):
        s.push(c0[:, :, 4:8], y[:, n4:n4 + 64])
    for bad in (dict(K=0), dict(iterations=-1), dict(look_ahead=-1), dict(batch=0)):
        kw = dict(dict(K=3, iterations=3), **bad)
        with pytest.raises(ValueError):
            p.misi_la_stream(**kw)


def test_c_abi_misuse_returns_invalid_and_leaves_the_library_usable():
    key = (64, 16, True, 12, 3)
    p, A, c0, y = inputs(key)
    lib, INVALID = lws_amd._capi.load(), lws_amd._capi.LWS_ERR_INVALID
    t, ty = torch.from_numpy(np.array(c0)).cuda(), torch.from_numpy(np.array(y)).cuda()
    out = torch.empty_like(t)
    nf, ns = ctypes.c_int(-1), ctypes.c_int(-1)
    fo, so = ctypes.byref(nf), ctypes.byref(ns)
    assert lib.lws_misi_stream_push(None, t.data_ptr(), None, ty.data_ptr(), 12, y.shape[1], out.data_ptr(), None, fo, so, None) == INVALID
    assert lib.lws_misi_stream_finish(None, out.data_ptr(), None, fo, so, None) == INVALID
    aw, sw = (np.ascontiguousarray(w, dtype=np.float64) for w in (p.awin, p.swin))
    h = ctypes.c_void_p()
    for B, K, iters, LA in ((0, 3, 3, 3), (3, 0, 3, 3), (3, 3, -1, 3), (3, 3, 3, -1)):
        assert lib.lws_misi_stream_create(0, B, K, 64, 16, aw.ctypes.data, sw.ctypes.data, 1, iters, LA, ctypes.byref(h)) == INVALID
    assert lib.lws_misi_stream_create(0, 3, 3, 64, 16, aw.ctypes.data, sw.ctypes.data, 1, 3, 3, ctypes.byref(h)) == 0 and h.value
    full = y.shape[1]
    assert lib.lws_misi_stream_push(h, t.data_ptr(), None, ty.data_ptr(), -1, 0, out.data_ptr(), None, fo, so, None) == INVALID
    assert lib.lws_misi_stream_push(h, None, None, ty.data_ptr(), 12, full, out.data_ptr(), None, fo, so, None) == INVALID
    assert lib.lws_misi_stream_push(h, t.data_ptr(), None, None, 12, full, out.data_ptr(), None, fo, so, None) == INVALID
    assert lib.lws_misi_stream_push(h, t.data_ptr(), None, ty.data_ptr(), 12, full - 1, out.data_ptr(), None, fo, so, None) == INVALID
    assert b"mixture samples" in lib.lws_last_error()
    assert lib.lws_misi_stream_push(h, None, None, None, 0, 1, None, None, fo, so, None) == INVALID
    assert lib.lws_misi_stream_push(h, None, None, None, 0, 0, None, None, fo, so, None) == 0 and (nf.value, ns.value) == (0, 0)
    assert lib.lws_misi_stream_push(h, t.data_ptr(), None, ty.data_ptr(), 12, full, None, None, fo, so, None) == INVALID   # rows to return
    assert lib.lws_misi_stream_finish(h, out.data_ptr(), None, fo, so, None) == 0 and nf.value == 0
    assert lib.lws_misi_stream_push(h, t.data_ptr(), None, ty.data_ptr(), 12, full, out.data_ptr(), None, fo, so, None) == INVALID
    assert b"finish" in lib.lws_last_error()
    lib.lws_misi_stream_destroy(h)
    lib.lws_misi_stream_destroy(None)
    whole, whole_x = streamed(key, 3, 3)          # ... and a fresh handle works
    again, again_x = run_stream(p, c0, y, 3, 3, [12])
    assert torch.equal(again, whole) and torch.equal(again_x, whole_x)


def test_zz_margins_actually_achieved():
    """What the cases above reached, per shape (written to $LWS_MARGINS_DIR/misi_la_stream_margins.json when that variable names a
    directory; profiles/misi_la_stream_margins.json is a copy).  On an MI355X, 234 rows, 87 of them at the rows of sc.PLACEMENTS and
    at the streams that end before their first commit: rel-L2 at most 2.8e-6 and at most 6.2 % of its bar, no bin beyond 1e-3 max A,
    magnitudes within 2.2e-7 max A, the signal sum within 7.1 % of its bound (at lws(2048,512), K = 1) and each signal within 5.0 % of
    its bar; where misi_la_dev computes the same thing (201 frames) the stream had its bits at every shape and step of sc.GPU_KEYS; the
    whole file in 4.1 s."""
    if not MARGINS:
        check_against_host((64, 16, True, 12, 3), 3, 3)
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "misi_la_stream_margins.json"), "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)
            f.write("\n")
    print(MARGINS)
    assert all(v.get("max_rel_l2_over_bar", 0.0) <= 1.0 and v.get("max_mixture_error_over_bound", 0.0) <= 1.0 and
               v.get("max_signal_error_over_bar", 0.0) <= 1.0 for v in MARGINS.values())
