"""GPU (-m gpu): the consistency-residual pair [sum |acc + w00 S|^2, sum |S|^2] (lws_residual_dev, lws_residual,
lws_residual_allreduce_dev, lws_multi_residual; include/lws_hip.h) against the fp64 restatement of tests/residual_model.py, which
tests/test_residual_model.py pins to the oracle.  The residual always runs the generic accumulate, whatever engine the plan's sweeps
use, so the cases here are plan kinds, shapes, entry points and stream ordering.

Bars:
  * sum |S|^2: rtol 1e-12 on every plan kind (an fp64 sum of the values the plan holds: the model gets S rounded to complex64 for
    fp32 plans);
  * sum |res|^2: rtol 1e-12 on fp64 plans; rtol 1e-4 on fp32 plans against the model of the fp32-rounded S (fp32 taps and fp32
    weights; cancelling inputs cost most).  Worst measured on the MI355X: 2.0e-7 (lws(16,4,L=7) on its own batch output), so the
    bar leaves a wide margin for rounding and none for a wrong tap, weight row or frame;
  * Q = 1: every weight is zero, so sum |res|^2 is exactly 0.0 (not NaN).
"""
import numpy as np
import pytest

import lws_amd
from lws_amd import _capi
from residual_model import db, residual_pairs

pytestmark = pytest.mark.gpu

RTOL_FP32 = 1e-4

# (name, lws() arguments, lws() keywords, general weights, frame counts T): T = 1 and T < Q - 1 replicate frames into the stencil
SHAPES = [
    ("q1", (16, 16), {}, False, (1, 5)),
    ("q2", (64, 32), {}, False, (1, 7)),
    ("q3", (48, 16), {}, False, (1, 6)),
    ("q4", (64, 16), {}, False, (1, 2, 9, 80)),
    ("q8", (64, 8), {}, False, (3, 12)),
    ("q16", (256, 16), {}, False, (1, 10, 40)),
    ("fracq", (400, 160), {}, False, (1, 8)),
    ("general", (64, 16), {}, True, (2, 8)),
    ("L1", (64, 16), {"L": 1}, False, (6,)),
    ("L10", (128, 32), {"L": 10}, False, (6,)),
    ("LFm2", (16, 4), {"L": 7}, False, (2, 6)),
    ("F2049", (4096, 1024), {}, False, (3,)),
]
KINDS = ["fp32", "fp64"]


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


def _plan(args, kw, general, precision="fp32", storage="fp32"):
    p = lws_amd.lws(*args, precision=precision, storage=storage, **kw)
    if general:
        W = lws_amd.create_weights(p.awin, p.swin, p.fshift, p.L, use_summarized_weights=False)
        assert W.shape[0] == p.fsize
        return p, W, _capi.Plan(p.fsize // 2 + 1, W, precision=precision, storage=storage)
    return p, p.W, p.plan()


def _rand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _held(S, precision):
    """The values a plan of this precision holds for S."""
    return S.astype(np.complex128 if precision == "fp64" else np.complex64).astype(np.complex128)


def _check(got, S_held, W, precision, what=""):
    """got (B, 2) from the device against the model of the values the plan holds."""
    ref = residual_pairs(S_held, W)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)), (what, got)
    np.testing.assert_allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0, err_msg=what)
    if W.shape[1] == 1:
        assert (got[:, 0] == 0.0).all() and (ref[:, 0] == 0.0).all(), (what, got)
        return 0.0
    ratio = np.abs(got[:, 0] / ref[:, 0] - 1).max()
    assert ratio < (1e-12 if precision == "fp64" else RTOL_FP32), (what, ratio)
    if precision == "fp32":
        print("RESID fp32 %-40s ratio %.3e" % (what, ratio))
    return ratio


def _inputs(p, T, B, rng):
    """Random complex, a consistent STFT (the cancelling case), both (B, T, F) complex128."""
    F = p.fsize // 2 + 1
    X = np.stack([p.stft(rng.standard_normal(p.fshift * (T + 8)))[:T] for _ in range(B)])
    assert X.shape == (B, T, F)
    return {"random": _rand(rng, (B, T, F)), "consistent": X}


@pytest.mark.parametrize("precision", KINDS)
@pytest.mark.parametrize("name,args,kw,general,Ts", SHAPES, ids=[s[0] for s in SHAPES])
def test_residual_dev_and_host_match_model(name, args, kw, general, Ts, precision):
    torch = _torch()
    p, W, plan = _plan(args, kw, general, precision)
    rng = np.random.default_rng(sum(args) + len(Ts))
    B = 1 if args[0] == 4096 else 2
    for T in Ts:
        for kind, S in _inputs(p, T, B, rng).items():
            what = "%s T=%d %s" % (name, T, kind)
            Sh = _held(S, precision)
            t = torch.from_numpy(Sh.astype(np.complex128 if precision == "fp64" else np.complex64)).cuda()
            before = t.clone()
            _check(plan.residual_dev(t.data_ptr(), B, T), Sh, W, precision, what + " dev")
            assert torch.equal(t, before)                                     # the input is left as it was
            _check(plan.residual(S), Sh, W, precision, what + " host")
            if kind == "random" and W.shape[1] > 1:
                # a spectrogram of this plan's own batch sweeps (at Q = 1 every weight is zero and a sweep changes nothing)
                thr = lws_amd.get_thresholds(20, 2.0, 0.2, 1)
                M = torch.from_numpy(np.abs(Sh).astype(np.complex128 if precision == "fp64" else np.complex64)).cuda()
                plan.batch_dev(M.data_ptr(), B, T, thr, stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                _check(plan.residual_dev(M.data_ptr(), B, T), M.cpu().numpy().astype(np.complex128), W, precision,
                       what + " lws")


@pytest.mark.parametrize("mode,storage", [("music", "fp32"), (None, "fp16")])
def test_music_mode_and_fp16_storage(mode, storage):
    """A music-mode plan's residual uses W (not W_ai / W_af); an fp16-storage plan stages the residual in fp32 like an fp32 plan,
    so the two give the same bits."""
    torch = _torch()
    rng = np.random.default_rng(21)
    p = lws_amd.lws(512, 128, mode=mode, storage=storage)
    ref_plan = lws_amd.lws(512, 128).plan()
    B, T = 3, 30
    S = _inputs(p, T, B, rng)
    for kind, X in S.items():
        Sh = _held(X, "fp32")
        t = torch.from_numpy(Sh.astype(np.complex64)).cuda()
        got = p.plan().residual_dev(t.data_ptr(), B, T)
        _check(got, Sh, p.W, "fp32", "%s/%s %s" % (mode, storage, kind))
        assert np.array_equal(got, ref_plan.residual_dev(t.data_ptr(), B, T))
        assert np.array_equal(p.plan().residual(X), ref_plan.residual(X))


@pytest.mark.parametrize("precision", KINDS)
def test_long_and_wide_calls(precision):
    """T > 256 (k_residual_sum loops over the frames), B = 300 (k_sum_pairs loops over more than its 256 threads), B = 1, and a plan
    whose scratch grows and shrinks between calls (B = 3, 300, 3)."""
    torch = _torch()
    p, W, plan = _plan((64, 16), {}, False, precision)
    np_dt = np.complex128 if precision == "fp64" else np.complex64
    rng = np.random.default_rng(5)
    for B, T in ((1, 300), (2, 517), (3, 4), (300, 3), (3, 5), (1, 1)):
        S = _held(_rand(rng, (B, T, 33)), precision)
        t = torch.from_numpy(S.astype(np_dt)).cuda()
        got = plan.residual_dev(t.data_ptr(), B, T)
        _check(got, S, W, precision, "B=%d T=%d" % (B, T))
        tot = plan.residual_allreduce_dev(t.data_ptr(), B, T, comm=None)
        ref = residual_pairs(S, W).sum(axis=0)
        np.testing.assert_allclose(tot[1], ref[1], rtol=1e-12, atol=0)
        np.testing.assert_allclose(tot[0], ref[0], rtol=1e-12 if precision == "fp64" else RTOL_FP32, atol=0)
        np.testing.assert_allclose(tot, got.sum(axis=0), rtol=1e-13, atol=0)


@pytest.mark.parametrize("precision", KINDS)
def test_multiplan_residual(precision):
    """Two shards on one device (the code path of two GPUs): the job's pair equals the model's column sums."""
    _torch()
    p = lws_amd.lws(64, 16)
    mp = _capi.MultiPlan(33, p.W, p.W_ai, p.W_af, devices=[0, 0], precision=precision)
    try:
        S = _rand(np.random.default_rng(6), (5, 11, 33))
        got = mp.residual(S)
        ref = residual_pairs(_held(S, precision), p.W).sum(axis=0)
        np.testing.assert_allclose(got[1], ref[1], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[0], ref[0], rtol=1e-12 if precision == "fp64" else RTOL_FP32, atol=0)
    finally:
        mp.close()


@pytest.mark.parametrize("variant", ["fp32", "fp64", "generic"])
def test_residual_between_batches_changes_nothing(variant):
    """batch -> residual -> batch gives the bits of batch -> batch: the residual's use of the plan's scratch leaves nothing behind."""
    torch = _torch()
    kw = {"precision": "fp64"} if variant == "fp64" else ({"force_generic": True} if variant == "generic" else {})
    dt = torch.complex128 if variant == "fp64" else torch.complex64
    plan = lws_amd.lws(64, 16, **kw).plan()
    rng = np.random.default_rng(7)
    B, T = 3, 40
    M = np.abs(_rand(rng, (B, T, 33)))
    R = _rand(rng, (2, 9, 33))
    thr = lws_amd.get_thresholds(10, 2.0, 0.2, 1)
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    for with_residual in (False, True):
        t = torch.from_numpy(M).to(dt).cuda()
        plan.batch_dev(t.data_ptr(), B, T, thr, stream=s)
        if with_residual:
            r = torch.from_numpy(R).to(dt).cuda()
            plan.residual_dev(r.data_ptr(), 2, 9, stream=s)
        plan.batch_dev(t.data_ptr(), B, T, thr, stream=s)
        torch.cuda.synchronize()
        outs.append(t.cpu())
    assert torch.equal(outs[0], outs[1])


def test_residual_on_second_stream_after_large_batch():
    """A residual enqueued on a second stream right after a large batch on the first, with no host synchronisation: it shares the
    plan's scratch with the batch, and only the plan's ordering keeps them apart.  Both results are those of a serial run."""
    torch = _torch()
    p = lws_amd.lws(512, 128, force_generic=True)
    plan = p.plan()
    rng = np.random.default_rng(11)
    B, T = 8, 200
    M = np.abs(_rand(rng, (B, T, 257))).astype(np.complex64)
    R = _held(_rand(rng, (3, 50, 257)), "fp32")
    thr = lws_amd.get_thresholds(30, 2.0, 0.1, 1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    serial = torch.from_numpy(M).cuda()
    plan.batch_dev(serial.data_ptr(), B, T, thr, stream=s1.cuda_stream)
    torch.cuda.synchronize()
    t = torch.from_numpy(M).cuda()
    r = torch.from_numpy(R.astype(np.complex64)).cuda()
    torch.cuda.synchronize()
    plan.batch_dev(t.data_ptr(), B, T, thr, stream=s1.cuda_stream)
    got = plan.residual_dev(r.data_ptr(), 3, 50, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    _check(got, R, p.W, "fp32", "second stream")
    assert torch.equal(t, serial)


def test_probe13_on_device():
    """SURVEY probe 13 on the device: the per-spectrogram dB of batch_dev output (100 iterations) from residual_dev equals the
    model's to 0.01 dB (measured: equal to 1e-4 dB, at 19.3-19.6 dB)."""
    torch = _torch()
    p = lws_amd.lws(1024, 256)
    rng = np.random.default_rng(13)
    B, T = 4, 200
    M = np.stack([np.abs(p.stft(rng.standard_normal(256 * (T + 8))))[:T] for _ in range(B)]).astype(np.complex64)
    t = torch.from_numpy(M).cuda()
    p.plan().batch_dev(t.data_ptr(), B, T, lws_amd.get_thresholds(100, 2.0, 0.1, 1),
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = t.cpu().numpy().astype(np.complex128)
    got = db(p.plan().residual_dev(t.data_ptr(), B, T))
    ref = db(residual_pairs(out, p.W))
    print("probe13 dB dev %s model %s" % (np.round(got, 4), np.round(ref, 4)))
    assert np.abs(got - ref).max() < 0.01, (got, ref)
    assert (got > 10).all()          # LWS converged well away from the zero-phase start (~0 dB)
