"""GPU: online MISI on the device (k_misi_la of lws_gla.hip) against the host fp64 definition (lws_amd.misi_la).

Inputs, error model and host references are those of tests/misi_la_cases.py.  As in tests/test_gpu_rtisi.py and test_gpu_misi.py the
value check has no fixed tolerance: its bar is measured here, on the host side only, as the rel-L2 distance the host iteration moves
under the error model, times 3 (tests/test_misi_la_host.py holds the model itself to at most 0.02 % of far bins on every row of the
table).  Distances, caps and bars are taken per mixture and per source, so that the weak source of a mixture and the small-scale
members of a stack are held as tightly as the loud ones.  Every figure is printed before it is asserted (pytest -s)."""
import json
import os

import numpy as np
import pytest

import lws_amd
import misi_la_cases as mc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_misi import mixture_bound  # noqa: E402
from test_gpu_rtisi import STEPS, assert_placement  # noqa: E402

# per (fsize, fshift, perfectrec): [cases, max rel-L2, max rel-L2 / bar, max far fraction, max magnitude error, max |sum s - y| / bound,
# max signal error / bar]
MARGINS = {}


def check_against_host(key, LA, n, explicit=False):
    p, A, c0, y = mc.case(*key)
    B, K = c0.shape[:2]
    (ref, ref_s), (per, per_s) = mc.host(key, LA, n, explicit)
    target = mc.magnitudes_of(A) if explicit else A
    out, s = p.misi_la_dev(c0, y, n, look_ahead=LA, magnitudes=target if explicit else None, return_signals=True)
    assert out.dtype == torch.complex64 and tuple(out.shape) == c0.shape
    assert s.dtype == torch.float32 and tuple(s.shape) == (B, K, y.shape[1])
    out, s = out.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.float64)
    assert np.isfinite(out.view(np.float64)).all() and np.isfinite(s).all()
    tag = "misi_la %s LA=%d n=%d%s" % (mc.key_id(key), LA, n, " explicit A" if explicit else "")
    m = MARGINS.setdefault(key[:3], [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for b in range(B):
        x_host = [p.istft(ref[b, k]) for k in range(K)]
        mix, mix_bar = np.abs(s[b].sum(axis=0) - y[b]).max(), mixture_bound(K, y[b], x_host)
        print("%s b=%d: |sum s - y| %.2e (bound %.2e)" % (tag, b, mix, mix_bar))
        m[5] = max(m[5], mix / mix_bar)
        assert mix <= mix_bar, (b, mix, mix_bar)
        for k in range(K):
            top = target[b, k].max()
            dist, bar = mc.rel(out[b, k], ref[b, k]), 3 * mc.rel(per[b, k], ref[b, k])
            far = np.mean(np.abs(out[b, k] - ref[b, k]) > 1e-3 * top)
            mag = np.abs(np.abs(out[b, k]) - target[b, k]).max() / top
            ds = np.abs(s[b, k] - ref_s[b, k]).max()
            bar_s = 3 * np.abs(per_s[b, k] - ref_s[b, k]).max() + 3e-6 * np.abs(ref_s[b, k]).max()
            print("%s b=%d k=%d: rel-L2 %.3e (bar %.3e)  far bins %.4f%%  |mag - A| %.2e max A  signal off %.2e (bar %.2e)"
                  % (tag, b, k, dist, bar, 100 * far, mag, ds, bar_s))
            m[:5] = [m[0] + 1, max(m[1], dist), max(m[2], dist / bar), max(m[3], far), max(m[4], mag)]
            m[6] = max(m[6], ds / bar_s)
            assert dist <= bar, (b, k, dist, bar)
            assert far <= 1e-3, (b, k, far)
            assert mag <= 2e-6, (b, k, mag)
            assert ds <= bar_s, (b, k, ds, bar_s)


def test_steps_are_those_of_the_rtisi_test():
    assert list(mc.STEPS) == list(STEPS)


@pytest.mark.parametrize("key", mc.keys(), ids=mc.key_id)
def test_matches_host(key):
    for LA, n in mc.STEPS:
        check_against_host(key, LA, n)


@pytest.mark.parametrize("key", sorted(mc.EDGE_SHAPES), ids=mc.key_id)
def test_edge_shapes_match_host(key):
    threads, steps = mc.EDGE_SHAPES[key]
    for LA, n, in_lds in steps:
        assert_placement(key, LA, in_lds, threads, K=key[4])
        check_against_host(key, LA, n)


@pytest.mark.parametrize("key,LA,n", [((4096, 1024, False, 6, 1), 0, 3),      # N = 4096 with its state in LDS
                                      ((64, 16, True, 12, 4), 3, 3),          # four sources
                                      ((1024, 256, False, 6, 4), 3, 2)],      # four sources whose state goes to scratch
                         ids=["4096-in-LDS", "K4", "K4-scratch"])
def test_placements_and_four_sources(key, LA, n):
    check_against_host(key, LA, n)


@pytest.mark.parametrize("key", [(64, 16, True, 12, 3), (256, 96, False, 2, 3)], ids=mc.key_id)
def test_explicit_magnitudes(key):
    check_against_host(key, 3, 3, explicit=True)
    check_against_host(key, 1, 4, explicit=True)


@pytest.mark.parametrize("key", [(64, 16, True, 12, 3), (512, 128, False, 40, 2)], ids=mc.key_id)
def test_causality_bit_for_bit(key):
    """With explicit magnitudes, LA = 3 and n = 3: other phases in the input frames >= 6, or another mixture from the uncut sample
    hop 5 + N on, leave the output frames 0..2 as they are and change frame 3."""
    p, A, c0, y = mc.case(*key)
    rng = np.random.default_rng(3)
    c1 = c0.copy()
    c1[:, :, 6:] = (A[:, :, 6:] * np.exp(2j * np.pi * rng.random(A[:, :, 6:].shape))).astype(np.complex64)
    lo = (p.fsize - p.fshift if p.fsize % p.fshift == 0 else p.fsize - p.fsize % p.fshift) if p.perfectrec else 0
    first = p.fshift * 5 + p.fsize - lo
    assert 0 < first < y.shape[1]
    y1 = y.copy()
    y1[:, first:] += (np.abs(y).max(axis=1, keepdims=True) * rng.standard_normal(y1[:, first:].shape)).astype(np.float32)
    a = p.misi_la_dev(c0, y, 3, look_ahead=3, magnitudes=A).cpu().numpy()
    for other in (p.misi_la_dev(c1, y, 3, look_ahead=3, magnitudes=A).cpu().numpy(),
                  p.misi_la_dev(c0, y1, 3, look_ahead=3, magnitudes=A).cpu().numpy()):
        assert np.array_equal(a[:, :, :3], other[:, :, :3])
        for b in range(c0.shape[0]):
            for k in range(c0.shape[1]):
                assert not np.array_equal(a[b, k, 3], other[b, k, 3])


@pytest.mark.parametrize("key", [(64, 16, False, 9, 2), (1000, 250, True, 5, 2), (4096, 1024, False, 6, 2)], ids=mc.key_id)
def test_stack_equals_members_and_repeats_bit_for_bit(key):
    p, A, c0, y = mc.case(*key)
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    out, s = p.misi_la_dev(t, ty, 3, return_signals=True)
    again, s2 = p.misi_la_dev(t, ty, 3, return_signals=True)
    assert torch.equal(out, again) and torch.equal(s, s2)
    assert torch.equal(out, p.misi_la_dev(t, ty, 3))                     # with and without the signals
    for b in range(c0.shape[0]):
        one, one_s = p.misi_la_dev(t[b], ty[b], 3, return_signals=True)
        assert tuple(one.shape) == c0.shape[1:] and tuple(one_s.shape) == tuple(s.shape[1:])
        assert torch.equal(one, out[b]) and torch.equal(one_s, s[b])


def test_concurrent_streams_do_not_share_windows_or_scratch():
    """Calls with different windows and shapes -- two whose state is in the context's scratch, which each of them grows and reuses (as
    rtisi_la_dev does: tests/test_gpu_rtisi.py), and one whose state is in LDS -- enqueued on two streams with no host synchronisation
    in between give what they give one at a time."""
    keys = [((4096, 1024, False, 6, 2), 3, False), ((1024, 256, False, 6, 4), 3, False), ((64, 16, True, 12, 3), 3, True)]
    calls = []
    for key, LA, in_lds in keys:
        assert_placement(key, LA, in_lds, 1024 if key[0] >= 1024 else 256, K=key[4])
        p, A, c0, y = mc.case(*key)
        calls.append((p, torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda(), LA))
    refs = [p.misi_la_dev(t, ty, 2, look_ahead=LA, return_signals=True) for p, t, ty, LA in calls]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for rep in range(6):
        for i, (p, t, ty, LA) in enumerate(calls):
            with torch.cuda.stream(streams[(rep + i) % 2]):
                outs.append((i, p.misi_la_dev(t, ty, 2, look_ahead=LA, return_signals=True)))
    torch.cuda.synchronize()
    for i, (out, s) in outs:
        assert torch.equal(out, refs[i][0]) and torch.equal(s, refs[i][1]), i


def test_zero_iterations_and_unmodified_input():
    key = (64, 16, False, 9, 2)
    p, A, c0, y = mc.case(*key)
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    keep, keep_y = t.clone(), ty.clone()
    out = p.misi_la_dev(t, ty, 0)
    assert torch.equal(out, keep) and out.data_ptr() != t.data_ptr()
    out, s = p.misi_la_dev(t, ty, 0, return_signals=True)               # the signals of the start itself
    assert torch.equal(out, keep)
    (ref, ref_s), _ = mc.host(key, 3, 0)
    s = s.cpu().numpy().astype(np.float64)
    for b in range(3):
        x = [p.istft(c0[b, k].astype(np.complex128)) for k in range(2)]
        mix, bound = np.abs(s[b].sum(axis=0) - y[b]).max(), mixture_bound(2, y[b], x)
        off = np.abs(s[b] - ref_s[b]).max(axis=1) / np.abs(ref_s[b]).max(axis=1)
        print("misi_la zero iterations b=%d: |sum s - y| %.2e (bound %.2e), signals off %s max|s|" % (b, mix, bound, off))
        assert mix <= bound and (off <= 3e-6).all()
    out = p.misi_la_dev(t, ty, 4)
    assert torch.equal(t, keep) and torch.equal(ty, keep_y) and not torch.equal(out, keep)
    assert out.data_ptr() != t.data_ptr()
    single = p.misi_la_dev(c0[0], y[0], 0)
    assert tuple(single.shape) == c0.shape[1:] and np.array_equal(single.cpu().numpy(), c0[0])
    single, s1 = p.misi_la_dev(c0[0], y[0], 2, return_signals=True)
    assert tuple(single.shape) == c0.shape[1:] and tuple(s1.shape) == (2, y.shape[1])


def test_silence_gives_exact_zeros():
    p, A, c0, y = mc.case(64, 16, True, 12, 3)
    Z, y0 = np.zeros(A.shape), np.zeros_like(y)
    for start, mags in ((np.zeros_like(c0), None), (c0, Z)):
        out, s = p.misi_la_dev(start, y0, 5, magnitudes=mags, return_signals=True)
        out, s = out.cpu().numpy(), s.cpu().numpy()
        assert (out == 0).all() and (s == 0).all()
    # one silent source among sounding ones stays silent in the spectrogram
    A1 = A.copy()
    A1[:, 1] = 0.0
    out, s = p.misi_la_dev(c0, y, 5, magnitudes=A1, return_signals=True)
    out, s = out.cpu().numpy(), s.cpu().numpy()
    assert np.isfinite(out.view(np.float32)).all() and np.isfinite(s).all() and (out[:, 1] == 0).all()
    assert np.abs(np.abs(out) - A1).max() <= 2e-6 * A1.max()


def test_one_source_with_the_whole_future_starts_as_misi():
    """K = 1, LA >= T - 1 and n = 1: the first commit is one step of misi_dev, whose frame 0 is final (to the value bar: the two
    kernels add the frames of a sample in other groupings)."""
    key = (48, 16, True, 7, 1)
    p, A, c0, y = mc.case(*key)
    (ref, _), (per, _) = mc.host(key, 6, 1)
    a = p.misi_la_dev(c0, y, 1, look_ahead=6).cpu().numpy().astype(np.complex128)
    b = p.misi_dev(c0, y, 1).cpu().numpy().astype(np.complex128)
    for i in range(3):
        dist, bar = mc.rel(a[i, 0, 0], b[i, 0, 0]), 3 * mc.rel(per[i, 0, 0], ref[i, 0, 0])
        print("misi_la K=1 whole future b=%d: frame 0 against misi_dev rel-L2 %.3e (bar %.3e)" % (i, dist, bar))
        assert dist <= bar


def test_method_uses_the_plans_look_ahead():
    p, A, c0, y = mc.case(64, 16, True, 12, 3)
    assert p.look_ahead == 3
    p1 = lws_amd.lws(64, 16, perfectrec=True, look_ahead=1)
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    assert torch.equal(p.misi_la_dev(t, ty, 2), p.misi_la_dev(t, ty, 2, look_ahead=3))
    assert torch.equal(p1.misi_la_dev(t, ty, 2), p.misi_la_dev(t, ty, 2, look_ahead=1))
    assert not torch.equal(p1.misi_la_dev(t, ty, 2), p.misi_la_dev(t, ty, 2))
    assert torch.equal(p.misi_la_dev(t, ty, 2, look_ahead=11), p.misi_la_dev(t, ty, 2, look_ahead=40))   # clamped to T - 1
    assert torch.equal(p.misi_la_dev(t, ty, 2), lws_amd.misi_la_dev(t, ty, 64, 16, p.awin, p.swin, 2, perfectrec=True))


def test_unsupported_and_invalid_arguments_raise():
    p = lws_amd.lws(8192, 2048)                  # beyond the LDS-resident transform (even sizes up to 4096)
    with pytest.raises(lws_amd.LwsHipError):
        p.misi_la_dev(np.ones((2, 5, 4097), complex), np.zeros(p.istft(np.ones((5, 4097), complex)).shape[0]), 2)
    p, A, c0, y = mc.case(64, 16, False, 9, 2)
    for bad in (dict(iterations=-1), dict(iterations=2, look_ahead=-1), dict(iterations=2, look_ahead=1.5),
                dict(iterations=2, magnitudes=A[:, :, :-1])):
        with pytest.raises(ValueError):
            p.misi_la_dev(c0, y, **bad)
    with pytest.raises(ValueError):
        p.misi_la_dev(c0, y[:, :-1], 3)          # wrong mixture length
    with pytest.raises(ValueError):
        p.misi_la_dev(c0, y[0], 3)               # one mixture for a stack
    with pytest.raises(ValueError):
        p.misi_la_dev(c0[0, 0], y[0], 3)         # a 2-D S
    with pytest.raises(ValueError):
        p.misi_la_dev(c0[:, :0], y, 3)           # no sources
    with pytest.raises(ValueError):
        p.misi_la_dev(c0[:, :, :, :-1], y, 3)
    q = lws_amd.lws(64, 16, perfectrec=True)     # two frames come back from the round trip as three
    with pytest.raises(ValueError, match="too few frames for perfectrec"):
        q.misi_la_dev(c0[:, :, :2], np.zeros((3, 0), np.float32), 1)
    # the C entry point checks for itself
    lib = lws_amd._capi.load()
    t, ty = torch.from_numpy(c0).cuda(), torch.from_numpy(y).cuda()
    w = np.ascontiguousarray(p.awin, dtype=np.float64)
    for K, iters, LA, yp in ((0, 2, 3, ty.data_ptr()), (2, -1, 3, ty.data_ptr()), (2, 2, -1, ty.data_ptr()), (2, 2, 3, None)):
        rc = lib.lws_misi_la_dev(0, t.data_ptr(), None, yp, None, 3, K, 9, 64, 16, w.ctypes.data, w.ctypes.data, 0, iters, LA, None)
        assert rc == lws_amd._capi.LWS_ERR_INVALID
    rc = lib.lws_misi_la_dev(0, t.data_ptr(), None, ty.data_ptr(), None, 3, 2, 2, 64, 16, w.ctypes.data, w.ctypes.data, 1, 1, 3, None)
    assert rc == lws_amd._capi.LWS_ERR_INVALID   # perfectrec does not keep two frames
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), c0)


def test_zz_margins_actually_achieved():
    """What the cases above reached, per shape (written to $LWS_MARGINS_DIR/misi_la_margins.json when that variable names a
    directory; profiles/misi_la_margins.json is a copy).  On an MI355X, 669 rows, 78 of them at the rows of mc.EDGE_SHAPES: rel-L2 at most
    8.6e-6 and at most 7.8 % of its bar, no bin beyond 1e-3 max A, magnitudes within 2.7e-7 max A, the signal sum within 7.1 % of its bound
    (at lws(2048,512), K = 1) and each signal within 7.1 % of its bar; the whole file in 4.9 s."""
    if not MARGINS:
        check_against_host((64, 16, True, 12, 3), 3, 3)
    report = {"%d,%d,%s" % k: {"cases": v[0], "max_rel_l2": v[1], "max_rel_l2_over_bar": v[2], "max_far_fraction": v[3],
                               "max_magnitude_error": v[4], "max_mixture_error_over_bound": v[5], "max_signal_error_over_bar": v[6]}
              for k, v in sorted(MARGINS.items())}
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "misi_la_margins.json"), "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    print(report)
    assert all(v[2] <= 1.0 and v[5] <= 1.0 and v[6] <= 1.0 for v in MARGINS.values())
