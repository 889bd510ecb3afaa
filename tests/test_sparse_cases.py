"""CPU: the silent / sparse patterns of tests/sparse_cases.py have, in the fp64 oracle alone, the properties that
tests/test_gpu_sparse.py relies on -- for every shape, stage and pattern that file uses:
  * no bin is within 1e-3 (relative) of a scaled threshold, so fp32 rounding cannot move a bin across one;
  * zeros stay zero, and the two isolated atoms keep their input bits (their weighted sums are structurally zero);
  * the set of bins written is the same when the input is first rounded to complex64 (what an fp32 engine is given) -- but for
    the few (< 0.5 %) bins of sparse_cases.ambiguous, which the reference rewrites with their own phase: whether their bits change
    is decided by the last rounding, in the oracle too;
  * batch sweeps update at least 99.5 % of the other non-zero bins (the final thresholds are 0: only a vanishing sum stops one);
  * batch sweeps are well conditioned here: a perturbation of 1.4e-7 rel-L2 of the input (1e-7 in each of the real and the imaginary
    part) moves the result by less than 1e-5 rel-L2 -- an amplification below 70, which keeps fp32 rounding (6e-8) two orders of
    magnitude under the 1e-3 bar of the dense tests, so those bars apply unchanged (observed: 2e-7 .. 1.3e-6);
  * no-future sweeps at Q = 2 update nothing in the reference (the weights of the past frame vanish): the GPU cases use Q >= 3.
"""
import numpy as np
import pytest

import sparse_cases as sc


def written(out, S):
    return out != S


def perturbed(S, seed, eps=1e-7):
    rng = np.random.default_rng(seed)
    return S * (1.0 + eps * (rng.standard_normal(S.shape) + 1j * rng.standard_normal(S.shape)))


def check_pattern(oracle, cfg, stage, S, A, thr, compat, atom_list=()):
    """The exact properties; returns (fraction of the non-zero, non-atom bins written, rel-L2 movement under a 1e-7 perturbation)."""
    assert sc.margin_to_thresholds(A, thr) > 1e-3
    assert np.array_equal(np.abs(S) > 0, A > 0)
    ref = sc.oracle_stage(oracle, cfg, stage, S, thr, compat)
    assert np.isfinite(ref).all()
    assert np.all(ref[A == 0] == 0)
    for t, f in atom_list:
        assert A[t, f] > 0 and ref[t, f] == S[t, f], (t, f)
    S32 = S.astype(np.complex64).astype(np.complex128)
    ref32 = sc.oracle_stage(oracle, cfg, stage, S32, thr, compat)
    Q, L = cfg.W.shape[1], cfg.W.shape[2] - 1
    po = sc.past_only(stage, Q, {'nofuture_q4_compat': compat})
    iso, amb = sc.isolated(A, Q, L, po), sc.ambiguous(ref, S, A, Q, L, po)
    assert np.all(ref[iso] == S[iso]) and np.all(ref32[iso] == S32[iso])
    print('ambiguous', int(amb.sum()), 'of', int(np.count_nonzero(A)), 'exactly equal', int((amb & (ref == S)).sum()))
    assert np.array_equal(written(ref32, S32)[~amb], written(ref, S)[~amb])
    others = A > 0
    for t, f in atom_list:
        others[t, f] = False
    frac = float(np.mean(written(ref, S)[others])) if others.any() else 1.0
    moved = sc.oracle_stage(oracle, cfg, stage, perturbed(S, 1), thr, compat)
    return frac, float(np.linalg.norm(moved - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("name", list(sc.ENGINES))
def test_sparse_case_in_the_oracle(oracle, name):
    fsize, fshift, L, T, stage, kw, env, kernel = sc.ENGINES[name]
    cfg = sc.config(fsize, fshift, L, kw)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    assert stage != "nofuture" or Q >= 3
    S, A, thr = sc.sparse_case(T, F, Q, L, sc.case_seed(name))
    assert 0.3 < np.mean(A[A.any(axis=1)][:, 1:int(0.7 * F)] == 0) < 0.5          # about 3/8 exact zeros where there is energy
    compat = kw.get("nofuture_q4_compat", True)
    frac, moved = check_pattern(oracle, cfg, stage, S, A, thr, compat, sc.atoms(T, F, Q, L))
    print("%s: %.4f of the non-zero bins written, 1e-7 perturbation -> %.2e" % (name, frac, moved))
    if stage == "batch":
        assert frac >= 0.995, frac
        assert moved < 1e-5, moved


@pytest.mark.parametrize("family", list(sc.FAMILIES))
@pytest.mark.parametrize("pattern", ["one-frame", "one-bin-row"])
def test_further_patterns_in_the_oracle(oracle, family, pattern):
    fsize, fshift, L, T, stage, kw, env, kernel = sc.ENGINES[sc.FAMILIES[family]]
    cfg = sc.config(fsize, fshift, L, kw)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, thr = sc.sparse_case(T, F, Q, L, sc.case_seed(family), pattern=pattern)
    if pattern == "one-frame":
        assert np.count_nonzero(A.any(axis=1)) == 1
    else:
        assert np.array_equal(np.flatnonzero(A.any(axis=0)), [sc.ROW_BIN]) and A[:, sc.ROW_BIN].all()
    check_pattern(oracle, cfg, stage, S, A, thr, kw.get("nofuture_q4_compat", True))


@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_batch_case_in_the_oracle(oracle, family):
    """One relative threshold vector serves the four spectrograms; the all-zero one comes back all zero, and the oracle is exactly
    homogeneous under the power of two."""
    fsize, fshift, L, T, stage, kw, env, kernel = sc.ENGINES[sc.FAMILIES[family]]
    cfg = sc.config(fsize, fshift, L, kw)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    Sb, Ab, thr = sc.batch_case(T, F, Q, L, sc.case_seed(family))
    compat = kw.get("nofuture_q4_compat", True)
    for b in (0, 2, 3):
        check_pattern(oracle, cfg, stage, Sb[b], Ab[b], thr, compat, sc.atoms(T, F, Q, L))
    assert not sc.oracle_stage(oracle, cfg, stage, Sb[1], thr, compat).any()
    assert np.array_equal(sc.oracle_stage(oracle, cfg, stage, Sb[3], thr, compat),
                          sc.oracle_stage(oracle, cfg, stage, Sb[2], thr, compat) * 2.0 ** -12)


@pytest.mark.parametrize("family", list(sc.FAMILIES))
@pytest.mark.parametrize("k", [30, -30, 66, -66, 200, -200])
def test_oracle_is_homogeneous_under_powers_of_two(oracle, family, k):
    fsize, fshift, L, T, stage, kw, env, kernel = sc.ENGINES[sc.FAMILIES[family]]
    cfg = sc.config(fsize, fshift, L, kw)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, thr = sc.sparse_case(T, F, Q, L, sc.case_seed(family))
    compat = kw.get("nofuture_q4_compat", True)
    assert np.array_equal(sc.oracle_stage(oracle, cfg, stage, S * 2.0 ** k, thr, compat),
                          sc.oracle_stage(oracle, cfg, stage, S, thr, compat) * 2.0 ** k)


@pytest.mark.parametrize("name", list(sc.MUSIC))
def test_music_schedules_stay_clear_of_the_levels(oracle, name):
    """run_lws(mode='music') end to end: the thresholds of its three stages, each scaled by the mean magnitude (which the sweeps
    preserve), stay clear of the magnitude levels."""
    import lws_amd
    fsize, fshift, L, T = sc.MUSIC[name]
    cfg = sc.config(fsize, fshift, L)
    F, Q = fsize // 2 + 1, cfg.W.shape[1]
    S, A, _ = sc.sparse_case(T, F, Q, L, sc.case_seed(name))
    p = lws_amd.lws(fsize, fshift, L=L, **sc.music_schedule(A))
    assert (p.nofuture_iterations, p.online_iterations, p.batch_iterations) == (1, 10, 5)
    for stage in ("nofuture", "online", "batch"):
        thr = lws_amd.get_thresholds(*[getattr(p, "%s_%s" % (stage, k)) for k in ("iterations", "alpha", "beta", "gamma")])
        assert sc.margin_to_thresholds(A, thr) > 1e-2, stage
    ref = sc.music_reference(oracle, p, S)
    ref32 = sc.music_reference(oracle, p, S.astype(np.complex64).astype(np.complex128))
    iso, amb = sc.isolated(A, Q, L), sc.ambiguous(ref, S, A, Q, L)
    assert np.isfinite(ref).all() and np.all(ref[A == 0] == 0) and np.all(ref[iso] == S[iso]) and iso.sum() >= 2
    assert np.array_equal(written(ref32, S.astype(np.complex64))[~amb], written(ref, S)[~amb])
    assert np.mean(written(ref, S)[(A > 0) & ~iso]) >= 0.995


def test_nofuture_sweeps_at_q2_update_nothing(oracle):
    cfg = sc.config(64, 32, 5)
    S, A, thr = sc.sparse_case(70, 33, 2, 5, 1)
    assert np.array_equal(oracle.nofuture_lws(S, cfg.W_ai, thr), S)
    rng = np.random.default_rng(0)
    D = rng.standard_normal((20, 33)) + 1j * rng.standard_normal((20, 33))
    assert np.array_equal(oracle.nofuture_lws(D, cfg.W_ai, [0.0]), D)
