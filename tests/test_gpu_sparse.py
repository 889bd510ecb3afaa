"""GPU (-m gpu): every LWS sweep engine against the fp64 oracle on silent and sparse spectrograms (tests/sparse_cases.py; their
properties in the oracle alone: tests/test_sparse_cases.py).  The other value tests feed dense Gaussian data: no bin is ever exactly
zero and no weighted sum ever vanishes, so the two branches of the reference that only such data reaches (a bin is updated only if
its magnitude is strictly above the threshold, and only if the weighted sum of its neighbourhood is non-zero: lwslib.cpp:295-296,
356-360) -- which every engine restates in its own way, next to machinery keyed on a spectrogram's largest or mean magnitude -- were
held by nothing.

Per engine and pattern.  Exact: the output is finite; every zero bin is zero; exactly the reference's bins were written; the isolated
atoms (and every other bin whose neighbourhood is silent) equal the input bit for bit -- the caller's complex128 values through the
host-array entry points, which hand back the caller's value for a bin that came back unchanged, the complex64 values in place through
the device-resident ones.  (The few bins of sparse_cases.ambiguous, which the reference rewrites with their own phase, are compared by value only.)
Values: the bars of the neighbouring files, restated in BARS below.  Engine reached: the kernel name the plan reports.
Then, on one representative of each engine family: the one-frame, one-bin-row and batch patterns, and exact homogeneity under
powers of two (LWS is homogeneous, and a power of two scales every fp operation exactly while nothing leaves the range)."""
import json
import os
import warnings

import numpy as np
import pytest

import lws_amd
from lws_amd import _capi
import sparse_cases as sc

pytestmark = pytest.mark.gpu

MARGINS = {}      # kernel name -> [cases, worst rel-L2, worst median |d| / mean |S|, worst magnitude error / max |S|]
COVARIANCE = {}   # family -> {k: "holds" | "range: finite, same bins, magnitudes"}


def rel_l2(a, b):
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


def c64(S):
    return S.astype(np.complex64).astype(np.complex128)


def make(name, monkeypatch, **more):
    """(lws configuration, plan, stage, expected kernel name) of a row of sparse_cases.ENGINES: the plan is created after the
    environment is set (some switches are read at plan creation)."""
    fsize, fshift, L, T, stage, kw, env, kernel = sc.ENGINES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = sc.config(fsize, fshift, L, kw)
    kw = {k: v for k, v in kw.items() if k != "use_simplifications"}
    kw.update(more)
    plan = _capi.Plan(fsize // 2 + 1, cfg.W, cfg.W_ai, cfg.W_af, **kw)
    return cfg, plan, stage, kernel


def run(plan, cfg, stage, S, thr, kernel):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # (the generic engine's notice)
        if stage == "batch":
            out = plan.batch(S, thr)
        elif stage == "nofuture":
            out = plan.nofuture(S, thr, wsel=_capi.LWS_W_AI)   # W_ai, as class lws calls it (lws.pyx:475)
        else:
            out = plan.online(S, thr, cfg.look_ahead, cfg.fsize / cfg.fshift)
    got = plan.last_kernel()["name"]
    # a shape silently routed elsewhere fails here, it does not pass on another kernel
    assert got.startswith(kernel[:-1]) if kernel.endswith("*") else got == kernel, (got, kernel)
    return out, got


def check_exact(out, S, A, ref, cfg, stage, plan_kw, base=None):
    """`base`: what a bin that no sweep wrote must equal bit for bit -- the caller's complex128 values S through the host-array entry
    points (they hand back the caller's value for a bin whose complex64 value came back unchanged, lws_capi.hip: widen_c64; so this
    holds on fp32 plans too and is stronger than equality with the complex64 rounding), c64(S) in place through the device-resident
    ones."""
    base = S if base is None else base
    Q, L = cfg.W.shape[1], cfg.W.shape[2] - 1
    po = sc.past_only(stage, Q, plan_kw)
    assert np.isfinite(out.real).all() and np.isfinite(out.imag).all()
    assert np.all(out[A == 0] == 0), np.argwhere((A == 0) & (out != 0))[:5]
    iso = sc.isolated(A, Q, L, po)
    if plan_kw.get("storage") == "fp16":
        # fp16 storage hands back the PHASE of its half state on the caller's fp32 magnitude for every bin that some sweep of the call
        # could have updated -- magnitude above the smallest threshold in effect, here 0 -- written or not (lws_systolic_layout.h, "fp16
        # storage"; bins below that threshold keep their bits: test_fp16_storage_keeps_the_bits_below_the_thresholds).  The state is
        # stored scaled by a power of two that brings the largest magnitude to [1, 2): each component is off by at most half an
        # ulp of that binade, 2^-11, times at most the largest magnitude; the two components together by sqrt(2) of that.
        assert np.abs(out - base)[iso].max(initial=0.0) <= 2.0 ** -10.5 * A.max() * (1 + 1e-3)
        assert np.abs(np.abs(out) - A)[iso].max(initial=0.0) < 2e-6 * A.max()
        return
    assert np.array_equal(out[iso], base[iso]), np.argwhere(iso & (out != base))[:5]
    amb = sc.ambiguous(ref, S, A, Q, L, po)
    wrong = ((out != base) != (ref != S)) & ~amb
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:5])


# The value bars, restated from the files that own them (rel-L2, median |d| / mean |S|, magnitude error / max |S|, and for the
# no-future engines the bars on the first frames after a silence, where rounding is still rounding):
BARS = {
    "batch_fp32": dict(rel=1e-3, med=1e-6, mag=1e-6),          # tests/test_gpu_systolic.py: run_case
    "batch_fp16": dict(rel=0.3, med=2e-3, mag=2e-6),           # tests/test_gpu_fp16.py: test_fp16_storage_structure_and_tolerance
    "online_fp32": dict(rel=5e-3, med=2e-6, mag=2e-6),         # tests/test_gpu_online.py: test_small_shapes_vs_oracle
    "online_team_fp32": dict(rel=2e-2, med=None, mag=2e-6, first8_rel=1e-4),    # tests/test_gpu_team.py: test_online_fp32_against_the_oracle
    "nofuture_team_fp32": dict(rel=1e-3, med=None, mag=2e-6),  # tests/test_gpu_team.py: test_nofuture_against_the_oracle
    "nofuture_fp32": dict(rel=5e-2, med=1e-4, mag=2e-6, first_med=2e-6),           # tests/test_gpu_nofuture.py, canonical addressing
    "nofuture_compat_fp32": dict(rel=None, med=None, mag=2e-6, first_med=2e-6, first_q99=1e-3),   # ... the shipped Q = 4 addressing
    "fp64": dict(abs=1e-8),                                    # run_case's fp64 plan, tests/test_gpu_online64.py
}


def bars_of(stage, kernel, plan_kw):
    if plan_kw.get("precision") == "fp64":
        return "fp64"
    if stage == "batch":
        return "batch_fp16" if plan_kw.get("storage") == "fp16" else "batch_fp32"
    if stage == "online":
        return "online_team_fp32" if kernel.startswith("team") else "online_fp32"
    if kernel.startswith("team"):
        return "nofuture_team_fp32"
    return "nofuture_compat_fp32" if kernel.startswith("nofuture_lds_q4compat") else "nofuture_fp32"


def first_frames(A):
    """The first two frames with energy after each silence: a no-future sweep chains a frame to its predecessors, and its own test
    file compares values where the chain is short."""
    live = A.any(axis=1)
    idx = []
    for t in np.flatnonzero(live):
        if (t == 0 or not live[t - 1]) or (t >= 2 and live[t - 1] and not live[t - 2]) or (t == 1 and live[0]):
            idx.append(t)
    return np.array(idx, dtype=int)


def check_values(out, S, A, ref, stage, kernel, plan_kw, record=True):
    which = bars_of(stage, kernel, plan_kw)
    bars = BARS[which]
    d = np.abs(out - ref)
    # mean |S| and the medians are taken over the non-zero bins -- the dense tests' statistics on the support: the zero bins are
    # exact (asserted), and there are enough of them to make a median over all bins 0 and the bar on it empty
    mean, top = float(np.mean(A[A > 0])) if (A > 0).any() else 0.0, float(A.max())
    figures = [rel_l2(out, ref), float(np.median(d[A > 0]) / mean) if (A > 0).any() else 0.0,
               float(np.abs(np.abs(out) - A).max() / top) if top > 0 else 0.0]
    print("%s [%s]: rel-L2 %.3e, median |d| / mean %.3e, magnitudes %.3e" % (kernel, which, *figures))
    if record:
        m = MARGINS.setdefault(kernel, [0, 0.0, 0.0, 0.0])
        m[0] += 1
        m[1:] = [max(a, b) for a, b in zip(m[1:], figures)]
    if which == "fp64":
        assert d.max(initial=0.0) < bars["abs"], d.max()
        return
    assert figures[2] < bars["mag"], figures
    if bars.get("rel") is not None:
        assert figures[0] < bars["rel"], figures
    if bars.get("med") is not None:
        assert figures[1] < bars["med"], figures
    if "first8_rel" in bars:
        f8 = np.flatnonzero(A.any(axis=1))[:8]                   # the first eight frames with energy: the short-run bar
        if f8.size:
            assert rel_l2(out[f8], ref[f8]) < bars["first8_rel"], rel_l2(out[f8], ref[f8])
    if "first_med" in bars:
        ff = first_frames(A)
        sel = d[ff][A[ff] > 0]
        if sel.size:
            assert np.median(sel) < bars["first_med"] * mean, np.median(sel) / mean
            if "first_q99" in bars:
                assert np.quantile(sel, 0.99) < bars["first_q99"] * mean, np.quantile(sel, 0.99) / mean


# ---------------------------------------------------------------------------------------------------------- every engine
@pytest.mark.parametrize("name", list(sc.ENGINES))
def test_sparse_case(oracle, name, monkeypatch):
    fsize, fshift, L, T, _, plan_kw, _, _ = sc.ENGINES[name]
    cfg, plan, stage, kernel = make(name, monkeypatch)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, thr = sc.sparse_case(T, F, Q, L, sc.case_seed(name))
    out, got = run(plan, cfg, stage, S, thr, kernel)
    ref = sc.oracle_stage(oracle, cfg, stage, S, thr, plan_kw.get("nofuture_q4_compat", True))
    check_exact(out, S, A, ref, cfg, stage, plan_kw)
    for t, f in sc.atoms(T, F, Q, L):
        assert out[t, f] != 0 and (out[t, f] == S[t, f] or plan_kw.get("storage") == "fp16")
    check_values(out, S, A, ref, stage, got, plan_kw)
    if name.endswith("_serial"):
        # the one-lane verification variant sums the taps in the generic engine's order: the same bits, on sparse data too
        gen = _capi.Plan(F, cfg.W, cfg.W_ai, cfg.W_af, force_generic=True, **plan_kw)
        g = gen.nofuture(S, thr, wsel=_capi.LWS_W_AI)
        assert gen.last_kernel()["name"] == "generic_fp32" and np.array_equal(out, g)
        gen.close()
    plan.close()


@pytest.mark.parametrize("name", ["fp16_quarter", "fp16_narrow"])
def test_fp16_storage_keeps_the_bits_below_the_thresholds(oracle, name, monkeypatch):
    """The sparse case with its three positive thresholds only: no sweep can touch a bin of magnitude 0.25 (below the smallest scaled
    threshold, 0.375), fp16 storage hands such a bin back with the caller's bits; the zeros stay zero, the louder atoms keep their
    magnitude and -- nothing reaches them -- their phase to the rounding of the half state."""
    fsize, fshift, L, T, _, plan_kw, _, _ = sc.ENGINES[name]
    cfg, plan, stage, kernel = make(name, monkeypatch)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, thr = sc.sparse_case(T, F, Q, L, sc.case_seed(name))
    out, got = run(plan, cfg, stage, S, thr[:3], kernel)
    quiet = A < 0.3
    assert np.array_equal(out[quiet], S[quiet]) and (quiet & (A > 0)).sum() > 20
    ref = oracle.batch_lws(S, cfg.W, thr[:3])
    check_exact(out, S, A, ref, cfg, stage, plan_kw)
    check_values(out, S, A, ref, stage, got, plan_kw, record=False)
    plan.close()


@pytest.mark.parametrize("name", list(sc.MUSIC))
def test_run_lws_music_end_to_end(oracle, name):
    fsize, fshift, L, T = sc.MUSIC[name]
    cfg = sc.config(fsize, fshift, L)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, _ = sc.sparse_case(T, F, Q, L, sc.case_seed(name))
    p = lws_amd.lws(fsize, fshift, L=L, **sc.music_schedule(A))
    out = p.run_lws(S)
    got = p.plan().last_kernel()["name"]
    assert got.startswith("systolic_quarter_q4" if Q == 4 else "systolic_half_q3"), got
    assert p.plan()._lib.lws_generic_stage(p.plan()._h).decode() == ""
    ref = sc.music_reference(oracle, p, S)
    check_exact(out, S, A, ref, cfg, "batch", {})
    # (three stages: the online stage's bars, the widest of the three)
    check_values(out, S, A, ref, "online", "run_lws_music_q%d" % Q, {})


# ---------------------------------------------------------------------------------------------------------- the further patterns
@pytest.mark.parametrize("family", list(sc.FAMILIES))
@pytest.mark.parametrize("pattern", ["one-frame", "one-bin-row"])
def test_further_patterns(oracle, family, pattern, monkeypatch):
    name = sc.FAMILIES[family]
    fsize, fshift, L, T, _, plan_kw, _, _ = sc.ENGINES[name]
    cfg, plan, stage, kernel = make(name, monkeypatch)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, thr = sc.sparse_case(T, F, Q, L, sc.case_seed(family), pattern=pattern)
    out, got = run(plan, cfg, stage, S, thr, kernel)
    ref = sc.oracle_stage(oracle, cfg, stage, S, thr, plan_kw.get("nofuture_q4_compat", True))
    check_exact(out, S, A, ref, cfg, stage, plan_kw)
    check_values(out, S, A, ref, stage, got, plan_kw)
    plan.close()


@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_batch_of_loud_silent_sparse_and_scaled(oracle, family, monkeypatch):
    """[loud x 40, all-zero, sparse, sparse x 2^-12] in one call: the all-zero spectrogram (mean and largest magnitude 0) comes back
    all zero, its neighbours equal what they give when run alone, the 2^-12 copy equals 2^-12 times its twin -- all bit for bit."""
    name = sc.FAMILIES[family]
    fsize, fshift, L, T, _, plan_kw, _, _ = sc.ENGINES[name]
    cfg, plan, stage, kernel = make(name, monkeypatch)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    Sb, Ab, thr = sc.batch_case(T, F, Q, L, sc.case_seed(family))
    out, got = run(plan, cfg, stage, Sb, thr, kernel)
    assert np.isfinite(out.real).all() and np.isfinite(out.imag).all()
    assert not out[1].any() and not np.signbit(out[1].real).any() and not np.signbit(out[1].imag).any()
    for b in (0, 2, 3):
        alone, _ = run(plan, cfg, stage, Sb[b], thr, kernel)
        assert np.array_equal(out[b], alone), (b, int(np.sum(out[b] != alone)))
    assert np.array_equal(out[3], out[2] * 2.0 ** -12)
    compat = plan_kw.get("nofuture_q4_compat", True)
    for b in (0, 2):
        ref = sc.oracle_stage(oracle, cfg, stage, Sb[b], thr, compat)
        check_exact(out[b], Sb[b], Ab[b], ref, cfg, stage, plan_kw)
        check_values(out[b], Sb[b], Ab[b], ref, stage, got, plan_kw)
    plan.close()


# ---------------------------------------------------------------------------------------------------------- device-resident entries
@pytest.mark.parametrize("name", ["quarter", "narrow", "band_44_11"])
def test_device_resident_entry(oracle, name, monkeypatch):
    """batch_dev on complex64 with direct I/O: the load kernel computes mean |S| itself (0 for the all-zero spectrogram)."""
    import torch
    fsize, fshift, L, T, _, plan_kw, _, _ = sc.ENGINES[name]
    cfg, plan, stage, kernel = make(name, monkeypatch)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    Sb, Ab, thr = sc.batch_case(T, F, Q, L, sc.case_seed(name))
    t = torch.from_numpy(Sb.astype(np.complex64)).cuda()
    plan.batch_dev(t.data_ptr(), 4, T, thr, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert plan.last_kernel()["name"] == kernel
    out = t.cpu().numpy().astype(np.complex128)
    assert np.isfinite(out.real).all() and np.isfinite(out.imag).all() and not out[1].any()
    assert np.array_equal(out[3], out[2] * 2.0 ** -12)
    for b in (0, 2):
        ref = oracle.batch_lws(Sb[b], cfg.W, thr)
        check_exact(out[b], Sb[b], Ab[b], ref, cfg, stage, plan_kw, base=c64(Sb[b]))
        check_values(out[b], Sb[b], Ab[b], ref, stage, kernel + " (batch_dev)", plan_kw)
    plan.close()


@pytest.mark.parametrize("name", ["quarter", "narrow", "wide"])
def test_workgroup_counts_on_sparse_data(name, monkeypatch):
    """Twenty sweeps are several passes over HBM, dealt to 1, 2 or 3 workgroups per spectrogram: a pass may be a no-op for one
    spectrogram (all of its sweeps dropped; every pass of the all-zero one) and live for its neighbour.  Identical bits."""
    fsize, fshift, L, T, _, plan_kw, _, _ = sc.ENGINES[name]
    cfg, plan, stage, kernel = make(name, monkeypatch)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    Sb, Ab, thr = sc.batch_case(T, F, Q, L, sc.case_seed(name))
    thr = np.concatenate([thr, [60.0 * thr[0]], thr, thr, thr[:4]])     # (a sweep dropped for all but the loud spectrogram)
    assert len(thr) == 20
    monkeypatch.setenv("LWS_SYSTOLIC_NWG", "1")
    ref, _ = run(plan, cfg, stage, Sb, thr, kernel)
    assert not ref[1].any() and np.all(ref[Ab == 0] == 0)
    for nwg in ("2", "3"):
        monkeypatch.setenv("LWS_SYSTOLIC_NWG", nwg)
        out, _ = run(plan, cfg, stage, Sb, thr, kernel)
        assert np.array_equal(out, ref), nwg
    monkeypatch.delenv("LWS_SYSTOLIC_NWG")
    out, _ = run(plan, cfg, stage, Sb, thr, kernel)
    assert np.array_equal(out, ref)
    plan.close()


# ---------------------------------------------------------------------------------------------------------- power-of-two covariance
@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_power_of_two_covariance(family, monkeypatch):
    """out(S 2^k) == out(S) 2^k bit for bit at k = +-30 in every engine and precision; at k = +-66 (about 1e+-20) in the engines that
    state scale handling and in fp64.  The fp32 band, team and generic engines square their sums in plain
    fp32: at k = +-66 they are held to a finite output, the written set of k = 0 and magnitudes within 1e-6 of the targets."""
    name = sc.FAMILIES[family]
    fsize, fshift, L, T, _, plan_kw, _, _ = sc.ENGINES[name]
    cfg, plan, stage, kernel = make(name, monkeypatch)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, thr = sc.sparse_case(T, F, Q, L, sc.case_seed(family))
    base, _ = run(plan, cfg, stage, S, thr, kernel)
    exact66 = family in sc.SCALE_EXACT or plan_kw.get("precision") == "fp64"
    state = COVARIANCE.setdefault(family, {})
    failures = []
    for k in (30, -30, 66, -66):
        out, _ = run(plan, cfg, stage, S * 2.0 ** k, thr, kernel)
        same = np.array_equal(out, base * 2.0 ** k)
        print("%s k=%+d: %s (%d bins differ)" % (kernel, k, "bit for bit" if same else "NOT bit for bit", int(np.sum(out != base * 2.0 ** k))))
        if abs(k) == 30 or exact66:
            state[k] = "holds" if same else "FAILS"
            if not same:
                failures.append(k)
            continue
        ok = (np.isfinite(out.real).all() and np.isfinite(out.imag).all()
              and np.array_equal(out != S * 2.0 ** k, base != S)
              and np.abs(np.abs(out) - A * 2.0 ** k).max() < 1e-6 * A.max() * 2.0 ** k)
        state[k] = ("holds" if same else "range: finite, same bins, magnitudes") if ok else "FAILS"
        if not ok:
            failures.append(k)
    plan.close()
    assert not failures, (family, kernel, state)


# ---------------------------------------------------------------------------------------------------------- the report
def test_zz_sparse_margins_actually_achieved():
    """What the cases above reached, per kernel name (written to $LWS_MARGINS_DIR/sparse_margins.json when that variable names a
    directory; profiles/sparse_margins.json is a copy).  100 cases in 3.4 s, the slowest 1.6 s (the first: it loads the library).  39 kernel
    names; fp32: rel-L2 <= 2.4e-6 (online LDS), medians <= 2.3e-7, magnitudes <= 2.3e-7; fp64: <= 2.5e-15; fp16 storage: rel-L2
    <= 3.5e-3, medians <= 1.1e-4, magnitudes <= 1.2e-7.  No pattern needed a bar of its own.  Power-of-two covariance: bit for bit at
    k = +-30 and +-66 in all eleven families (before the range fixes of this file's commit: band, generic and both team routes failed at
    +-66, the no-future LDS kernel at +66)."""
    if not MARGINS:
        pytest.skip("run with the rest of the file")
    report = {"kernels": {k: {"cases": v[0], "max_rel_l2": v[1], "max_median_over_mean": v[2], "max_magnitude_error": v[3]}
                          for k, v in sorted(MARGINS.items())},
              "covariance": {f: {"%+d" % k: v for k, v in st.items()} for f, st in COVARIANCE.items()}}
    out = os.environ.get("LWS_MARGINS_DIR", "")
    if out and os.path.isdir(out):
        json.dump(report, open(os.path.join(out, "sparse_margins.json"), "w"), indent=1)
    print(report)
    expected = set()
    for name, row in sc.ENGINES.items():
        expected.add(row[7].rstrip("*"))
    for want in expected:
        assert any(k.startswith(want) for k in MARGINS), want
