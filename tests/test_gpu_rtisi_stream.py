"""GPU: streaming RTISI-LA (RtisiLaStream, k_rtisi_stream of lws_gla.hip): rows pushed as they arrive, the state on the device.

The definition is the host's rtisi_la(..., open_end=True) of everything pushed.  What is held here: however the rows are cut into
chunks the stream returns the same bits; it meets the host definition by the bars of tests/test_gpu_rtisi.py (the rel-L2 distance the
host iteration moves under a 1e-6 perturbation of every projection, times 3, per spectrogram; at most 0.1 % of the bins further than
1e-3 max A; magnitudes within 2e-6 max A; the signal within 3e-6 max|x| of istft of the result); it agrees with the one-shot
rtisi_la_dev wherever the two definitions coincide; streams do not see each other.  Every figure is printed before it is asserted."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import lws_amd
from lws_amd.lws import _perfectrec_prepad

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_rtisi import EDGE_SHAPES, assert_placement, case, magnitudes_of, perturbation, rel   # noqa: E402

KEYS = [
    (64, 16, True, 12),        # power of two
    (48, 16, False, 7),        # odd factor
    (256, 96, True, 9),        # hop does not divide the frame
    (512, 128, False, 40),     # the ring wraps
    (4096, 1024, False, 6),    # the state does not fit in LDS: scratch placement
]
STEPS = [(0, 2), (1, 3), (3, 3), (5, 2)]   # (look_ahead, iterations)
# rows of EDGE_SHAPES of tests/test_gpu_rtisi.py with their steps there: N = 2 workgroups on both sides of the LDS boundary, 16 bytes
# under the cap, more active frames than overlap, no overlap.  (threads, [(look_ahead, iterations, state in LDS)])
EDGE_KEYS = {k: EDGE_SHAPES[k] for k in [(2048, 512, False, 8), (2048, 1228, False, 8), (64, 8, True, 20), (64, 64, False, 6)]}
MARGINS = {}   # "fsize,fshift,perfectrec" -> figures against the host; ["vs_rtisi_la_dev"]: against the one-shot kernel


def steps_of(key):
    """(look_ahead, iterations) of a key; an edge key first asserts the placement and workgroup of a stream created for each."""
    if key not in EDGE_KEYS:
        return STEPS
    threads, steps = EDGE_KEYS[key]
    for LA, n, in_lds in steps:
        assert_placement(key, LA, in_lds, threads)
    return [(LA, n) for LA, n, in_lds in steps]


def chunkings(T):
    return [[T], [1] * T, [2, 0, 1, T - 3]]


def run_stream(p, c0, LA, n, chunks, magnitudes=None, batch="stack", check_counts=True):
    """Push c0 (B, T, F) -- or (T, F) with batch=None -- in `chunks`, finish; returns the concatenated frames and signal."""
    B = None if batch is None else c0.shape[0]
    T = c0.shape[-2]
    assert sum(chunks) == T
    t = torch.from_numpy(np.array(c0)).cuda()   # (a copy: the cases are read-only)
    A = None if magnitudes is None else torch.from_numpy(np.ascontiguousarray(magnitudes, dtype=np.float32)).cuda()
    s = p.rtisi_la_stream(n, look_ahead=LA, batch=B, return_signal=True)
    lo = _perfectrec_prepad(p.fsize, p.fshift) if p.perfectrec else 0
    frames, sig, entered, committed, at = [], [], 0, 0, 0
    for k in chunks:
        out, x = s.push(t[..., at:at + k, :], None if A is None else A[..., at:at + k, :])
        at, entered = at + k, entered + k
        want = max(0, entered - LA) - committed
        want_x = max(0, p.fshift * (committed + want) - max(p.fshift * committed, lo)) if want else 0
        if check_counts:
            assert out.shape[-2] == want and x.shape[-1] == want_x, (chunks, k, tuple(out.shape), want, tuple(x.shape), want_x)
        assert out.dtype == torch.complex64 and x.dtype == torch.float32
        committed += want
        frames.append(out)
        sig.append(x)
    out, x = s.finish()
    assert out.shape[-2] == T - committed
    frames.append(out)
    sig.append(x)
    s.close()
    frames, sig = torch.cat(frames, dim=-2), torch.cat(sig, dim=-1)
    assert frames.shape[-2] == T and sig.shape[-1] == max(lws_amd._capi.istft_length(T, p.fsize, p.fshift, p.perfectrec), 0)
    return frames, sig


@functools.lru_cache(maxsize=None)
def host(key, LA, n, explicit=False, rows=None):
    """The host fp64 definition (open end) of the first `rows` frames of the case, and the same under the perturbation model."""
    p, A, c0 = case(*key)
    c0, A = c0[:, :rows], A[:, :rows]
    kw = dict(look_ahead=LA, magnitudes=magnitudes_of(A) if explicit else None, perfectrec=p.perfectrec, open_end=True)
    ref = lws_amd.rtisi_la(c0, p.fsize, p.fshift, p.awin, p.swin, n, **kw)
    per = lws_amd.rtisi_la(c0, p.fsize, p.fshift, p.awin, p.swin, n, _perturb=perturbation(n + 17), **kw)
    return ref, per


@functools.lru_cache(maxsize=None)
def streamed(key, LA, n):
    """The stream's result for the whole case pushed at once (chunking changes no bit: test_chunking_changes_no_bit)."""
    p, A, c0 = case(*key)
    return run_stream(p, c0, LA, n, [c0.shape[1]])


def margins(key):
    return MARGINS.setdefault("%d,%d,%s" % key[:3], {"cases": 0, "max_rel_l2": 0.0, "max_rel_l2_over_bar": 0.0, "max_far_fraction": 0.0,
                                                     "max_magnitude_error": 0.0, "max_signal_error": 0.0})


def check_against_host(key, LA, n, chunks, explicit=False, rows=None):
    p, A, c0 = case(*key)
    c0, A = c0[:, :rows], A[:, :rows]
    ref, per = host(key, LA, n, explicit, rows)
    target = magnitudes_of(A) if explicit else A
    if explicit or rows is not None or chunks != [c0.shape[1]]:
        out, sig = run_stream(p, c0, LA, n, chunks, magnitudes=target if explicit else None)
    else:
        out, sig = streamed(key, LA, n)
    out, sig = out.cpu().numpy().astype(np.complex128), sig.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(sig).all()
    m = margins(key)
    for b in range(c0.shape[0]):
        top = target[b].max()
        dist, bar = rel(out[b], ref[b]), 3 * rel(per[b], ref[b])
        far = np.mean(np.abs(out[b] - ref[b]) > 1e-3 * top)
        mag = np.abs(np.abs(out[b]) - target[b]).max() / top
        x = p.istft(out[b])
        serr = np.abs(sig[b] - x).max() / np.abs(x).max() if x.size else 0.0
        print("stream %s T=%d LA=%d n=%d%s b=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal %.2e max|x|"
              % (key[:3], c0.shape[1], LA, n, " explicit A" if explicit else "", b, dist, bar, 100 * far, mag, serr))
        m["cases"] += 1
        for name, v in (("max_rel_l2", dist), ("max_rel_l2_over_bar", dist / bar), ("max_far_fraction", far), ("max_magnitude_error", mag),
                        ("max_signal_error", serr)):
            m[name] = max(m[name], float(v))
        assert dist <= bar, (b, dist, bar)
        assert far <= 1e-3, (b, far)
        assert mag <= 2e-6, (b, mag)
        assert serr <= 3e-6, (b, serr)


@pytest.mark.parametrize("key", KEYS + sorted(EDGE_KEYS))
def test_chunking_changes_no_bit(key):
    """Pushed whole, a row at a time, and with a chunk shorter than LA + 1 and an empty one: the same frames, signals and counts."""
    p, A, c0 = case(*key)
    T = c0.shape[1]
    for LA, n in steps_of(key):
        whole, whole_x = streamed(key, LA, n)
        assert tuple(whole.shape) == c0.shape
        for chunks in chunkings(T)[1:]:
            out, x = run_stream(p, c0, LA, n, chunks)
            assert torch.equal(out, whole) and torch.equal(x, whole_x), (LA, n, chunks)


@pytest.mark.parametrize("key", KEYS + sorted(EDGE_KEYS))
def test_matches_host_open_end(key):
    for LA, n in steps_of(key):
        check_against_host(key, LA, n, [case(*key)[2].shape[1]])


@pytest.mark.parametrize("key", KEYS)
def test_against_the_one_shot_kernel(key):
    """rtisi_la_dev closes the end inside the iteration under perfectrec; where it does not reach -- all of it without perfectrec, the
    frames < P and the samples < hop P - lo with it -- the stream computes the same thing with another kernel.  Held to the bar of the
    host comparison; whether the bits are equal is measured and recorded, not required (two kernels need not contract alike)."""
    p, A, c0 = case(*key)
    T, hop, N = c0.shape[1], p.fshift, p.fsize
    lo = _perfectrec_prepad(N, hop) if p.perfectrec else 0
    rec = margins(key).setdefault("vs_rtisi_la_dev", {"bits_equal": True, "max_abs_diff_over_max_A": 0.0, "max_signal_diff_over_max_x": 0.0})
    for LA, n in STEPS:
        P = sum(1 for m in range(T) if hop * min(m + LA, T - 1) + N <= hop * T) if p.perfectrec else T
        k = max(hop * P - lo, 0) if p.perfectrec else None
        out, x = streamed(key, LA, n)
        one, one_x = p.rtisi_la_dev(c0, n, look_ahead=LA, return_signal=True)
        same = torch.equal(out[:, :P], one[:, :P]) and torch.equal(x[:, :k], one_x[:, :k])
        a, b = out[:, :P].cpu().numpy().astype(np.complex128), one[:, :P].cpu().numpy().astype(np.complex128)
        xa, xb = x[:, :k].cpu().numpy().astype(np.float64), one_x[:, :k].cpu().numpy().astype(np.float64)
        ref, per = host(key, LA, n)
        diff = sdiff = 0.0
        for s in range(c0.shape[0]):
            top = A[s].max()
            if P:
                dist, bar = rel(a[s], b[s]), 3 * rel(per[s][:P], ref[s][:P])
                far = np.mean(np.abs(a[s] - b[s]) > 1e-3 * top)
                diff = max(diff, np.abs(a[s] - b[s]).max() / top)
                assert dist <= bar, (LA, n, s, dist, bar)
                assert far <= 1e-3, (LA, n, s, far)
            if xa.shape[1]:
                sd = np.abs(xa[s] - xb[s]).max() / np.abs(xb[s]).max()
                sdiff = max(sdiff, sd)
                assert sd <= 3e-6, (LA, n, s, sd)
        print("stream vs rtisi_la_dev %s LA=%d n=%d: %d of %d frames compared, bits equal: %s, largest difference %.2e max A, signal %.2e max|x|"
              % (key[:3], LA, n, P, T, same, diff, sdiff))
        rec["bits_equal"] = bool(rec["bits_equal"] and same)
        rec["max_abs_diff_over_max_A"] = max(rec["max_abs_diff_over_max_A"], float(diff))
        rec["max_signal_diff_over_max_x"] = max(rec["max_signal_diff_over_max_x"], float(sdiff))


@pytest.mark.parametrize("key", [(64, 16, True, 12), (256, 96, False, 2)])
def test_explicit_magnitudes_chunk_by_chunk(key):
    T = key[3]
    check_against_host(key, 3, 3, [1] * T, explicit=True)
    p, A, c0 = case(*key)
    a = run_stream(p, c0, 3, 3, [1] * T, magnitudes=magnitudes_of(A))
    b = run_stream(p, c0, 3, 3, [T], magnitudes=magnitudes_of(A))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_streams_do_not_see_each_other():
    key, LA, n = (64, 16, True, 12), 3, 3
    p, A, c0 = case(*key)
    whole, whole_x = streamed(key, LA, n)
    # a stack against its members as single streams
    for b in range(c0.shape[0]):
        one, one_x = run_stream(p, c0[b], LA, n, [5, 7], batch=None)
        assert tuple(one.shape) == c0.shape[1:] and one_x.dim() == 1
        assert torch.equal(one, whole[b]) and torch.equal(one_x, whole_x[b])
    # two streams pushed alternately against each alone
    t = torch.from_numpy(np.array(c0)).cuda()
    other = torch.flip(t, dims=[0])
    alone = run_stream(p, other.cpu().numpy(), LA, n, [12])
    s1, s2 = (p.rtisi_la_stream(n, look_ahead=LA, batch=3, return_signal=True) for _ in range(2))
    got1, got2 = [], []
    for at in range(0, 12, 3):
        got1.append(s1.push(t[:, at:at + 3]))
        got2.append(s2.push(other[:, at:at + 3]))
    got1.append(s1.finish())
    got2.append(s2.finish())
    for got, (want, want_x) in ((got1, (whole, whole_x)), (got2, alone)):
        assert torch.equal(torch.cat([g[0] for g in got], dim=1), want)
        assert torch.equal(torch.cat([g[1] for g in got], dim=1), want_x)
    # a stream created after others were closed against the first one
    s1.close()
    s2.close()
    again, again_x = run_stream(p, c0, LA, n, [4, 8])
    assert torch.equal(again, whole) and torch.equal(again_x, whole_x)


@pytest.mark.parametrize("key,LA,T", [((64, 16, True, 12), 3, 1), ((64, 16, True, 12), 3, 3), ((48, 16, False, 7), 5, 1),
                                      ((48, 16, False, 7), 5, 5)])
def test_fewer_frames_than_the_look_ahead(key, LA, T):
    """T <= LA: no push can commit anything; finish() runs them as one call on T frames would."""
    check_against_host(key, LA, 3, [1] * T, rows=T)
    p, A, c0 = case(*key)
    s = p.rtisi_la_stream(3, look_ahead=LA, batch=3)
    for m in range(T):
        assert tuple(s.push(c0[:, m:m + 1]).shape) == (3, 0, c0.shape[2])
    assert tuple(s.finish().shape) == (3, T, c0.shape[2])


@pytest.mark.parametrize("key,LA,n,T", [((4096, 1024, False, 6), 3, 3, 1), ((2048, 512, False, 8), 6, 2, 2)])
def test_end_before_the_first_commit_changes_the_placement(key, LA, n, T):
    """A stream created with its state in scratch that ends after T <= LA frames closes with a look-ahead of T - 1, for which the
    state fits in LDS: the closing launch is the LDS kernel, on a state buffer sized and strided for the scratch one."""
    assert_placement(key, LA, False, 1024)                               # as created
    assert_placement(key[:3] + (T,), LA, True, 1024)                     # as closed: look-ahead T - 1
    check_against_host(key, LA, n, [1] * T, rows=T)
    p, A, c0 = case(*key)
    a, b = run_stream(p, c0[:, :T], LA, n, [1] * T), run_stream(p, c0[:, :T], LA, n, [T])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_edges():
    p, A, c0 = case(64, 16, True, 12)
    F = c0.shape[2]
    # nothing pushed
    s = p.rtisi_la_stream(3, return_signal=True)
    out, x = s.finish()
    assert tuple(out.shape) == (0, F) and tuple(x.shape) == (0,) and out.dtype == torch.complex64 and x.dtype == torch.float32
    s = p.rtisi_la_stream(3, batch=3)
    assert tuple(s.push(c0[:, :0]).shape) == (3, 0, F) and tuple(s.finish().shape) == (3, 0, F)
    # no iterations: the rows themselves, LA frames late, and their istft
    t = torch.from_numpy(np.array(c0)).cuda()
    for chunks in ([12], [1] * 12, [5, 7]):
        s = p.rtisi_la_stream(0, batch=3, return_signal=True)
        assert tuple(s.push(t[:, :2])[0].shape) == (3, 0, F)
        s.close()
        out, x = run_stream(p, c0, 3, 0, chunks)
        assert torch.equal(out, t)
        ref = np.stack([p.istft(c.astype(np.complex128)) for c in c0])
        assert (np.abs(x.cpu().numpy() - ref).max(axis=1) <= 3e-6 * np.abs(ref).max(axis=1)).all()
    # digital silence
    out, x = run_stream(p, np.zeros_like(c0), 3, 3, [5, 7])
    assert (out.cpu().numpy() == 0).all() and (x.cpu().numpy() == 0).all()
    # misuse, before anything is enqueued
    s = p.rtisi_la_stream(3, batch=3)
    for bad in (c0[:, :4, :-1], c0[:2, :4], c0[0, :4]):
        with pytest.raises(ValueError):
            s.push(bad)
    with pytest.raises(ValueError):
        s.push(c0[:, :4], magnitudes=A[:, :3])
    assert tuple(s.push(c0[:, :4]).shape) == (3, 1, F)
    s.finish()
    with pytest.raises(ValueError):
        s.push(c0[:, 4:8])
    with pytest.raises(ValueError):
        p.rtisi_la_stream(-1)
    with pytest.raises(ValueError):
        p.rtisi_la_stream(3, look_ahead=-1)
    with pytest.raises(ValueError):
        p.rtisi_la_stream(3, batch=0)


def test_c_abi_misuse_returns_invalid_and_leaves_the_library_usable():
    p, A, c0 = case(64, 16, True, 12)
    lib, INVALID = lws_amd._capi.load(), lws_amd._capi.LWS_ERR_INVALID
    t = torch.from_numpy(np.array(c0)).cuda()
    out = torch.empty_like(t)
    nf, ns = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.lws_rtisi_stream_push(None, t.data_ptr(), None, 12, out.data_ptr(), None, ctypes.byref(nf), ctypes.byref(ns), None) == INVALID
    assert lib.lws_rtisi_stream_finish(None, out.data_ptr(), None, ctypes.byref(nf), ctypes.byref(ns), None) == INVALID
    aw, sw = (np.ascontiguousarray(w, dtype=np.float64) for w in (p.awin, p.swin))
    h = ctypes.c_void_p()
    for bad in ((0, 3, 3), (3, -1, 3), (3, 3, -1)):   # (B, iterations, look-ahead)
        assert lib.lws_rtisi_stream_create(0, bad[0], 64, 16, aw.ctypes.data, sw.ctypes.data, 1, bad[1], bad[2], ctypes.byref(h)) == INVALID
    assert lib.lws_rtisi_stream_create(0, 3, 64, 16, aw.ctypes.data, sw.ctypes.data, 1, 3, 3, ctypes.byref(h)) == 0 and h.value
    assert lib.lws_rtisi_stream_push(h, t.data_ptr(), None, -1, out.data_ptr(), None, ctypes.byref(nf), ctypes.byref(ns), None) == INVALID
    assert lib.lws_rtisi_stream_push(h, None, None, 4, out.data_ptr(), None, ctypes.byref(nf), ctypes.byref(ns), None) == INVALID
    assert lib.lws_rtisi_stream_push(h, None, None, 0, None, None, ctypes.byref(nf), ctypes.byref(ns), None) == 0 and (nf.value, ns.value) == (0, 0)
    assert lib.lws_rtisi_stream_finish(h, out.data_ptr(), None, ctypes.byref(nf), ctypes.byref(ns), None) == 0 and nf.value == 0
    assert lib.lws_rtisi_stream_push(h, t.data_ptr(), None, 12, out.data_ptr(), None, ctypes.byref(nf), ctypes.byref(ns), None) == INVALID
    assert b"finish" in lib.lws_last_error()
    lib.lws_rtisi_stream_destroy(h)
    lib.lws_rtisi_stream_destroy(None)
    whole, whole_x = streamed((64, 16, True, 12), 3, 3)          # ... and a fresh handle works
    again, again_x = run_stream(p, c0, 3, 3, [12])
    assert torch.equal(again, whole) and torch.equal(again_x, whole_x)


def test_zz_margins_actually_achieved():
    """What the cases above reached, per shape (written to $LWS_MARGINS_DIR/rtisi_stream_margins.json when that variable names a
    directory; profiles/rtisi_stream_margins.json is a copy).  On an MI355X, 108 rows, 30 of them at EDGE_KEYS and at the streams that end
    before their first commit: rel-L2 at most 4.0e-6 and at most 5.0 % of its bar, no bin beyond 1e-3 max A, magnitudes within 2.0e-7 max A,
    signals within 1.8e-7 max|x|; where rtisi_la_dev computes the same thing the stream had its bits at every shape and step of KEYS; the
    whole file in 3.1 s."""
    if not MARGINS:
        check_against_host((64, 16, True, 12), 3, 3, [12])
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "rtisi_stream_margins.json"), "w") as f:
            json.dump(MARGINS, f, indent=1, sort_keys=True)
            f.write("\n")
    print(MARGINS)
    assert all(v.get("max_rel_l2_over_bar", 0.0) <= 1.0 for v in MARGINS.values())
