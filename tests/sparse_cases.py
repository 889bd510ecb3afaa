"""Silent and sparse spectrograms for the LWS sweep engines (a helper, not a conftest): tests/test_sparse_cases.py proves on the CPU,
with the fp64 oracle alone, that the patterns have the properties stated below; tests/test_gpu_sparse.py holds every engine to the
oracle on them.  The dense Gaussian spectrograms of the other value tests never contain an exact zero, and never a weighted sum
that is exactly zero; the reference has two branches that only such data reaches (lwslib.cpp:295-296, 356-360): a bin is updated
only if its magnitude is strictly above the threshold (a zero bin never is, even at threshold 0), and only if the weighted sum of
its neighbourhood is non-zero (an isolated bin keeps its input value bit for bit).

sparse_case(T, F, Q, L, seed) -> (S, A, thr):
  magnitudes A   drawn from {0, 0, 0, 0.25, 0.5, 1, 2, 4} (3/8 exact zeros, as after a ReLU); each non-zero bin a uniform phase;
  silence        the first 2Q+3 and the last Q+2 frames, the band bin >= int(0.7 F) (Nyquist included), DC, and a silent middle
                 (frames 30..44; 20..30 for frames above 513 bins; wider for Q > 8) -- except two ISOLATED ATOMS in the middle
                 frame (37 / 25), at bins 8 and 8+L+2: more than L bins and Q-1 frames from any other energy, so that their
                 weighted sums are structurally zero;
  thresholds     thr = [3.0, 0.75, 0.375, 0.0, 0.0] / mean|S| -- the engines multiply by mean|S|, so every scaled threshold falls
                 strictly between two magnitude levels and no fp32 rounding of a magnitude or of the mean moves a bin across one.
Further patterns built the same way: "one-frame" (a single non-silent frame), "one-bin-row" (a single non-silent frequency across
all frames) and batch_case (loud x 40, all-zero, sparse, sparse x 2^-12).
"""
import numpy as np

LEVELS = np.array([0.0, 0.0, 0.0, 0.25, 0.5, 1.0, 2.0, 4.0])
THR_LEVELS = np.array([3.0, 0.75, 0.375, 0.0, 0.0])
ROW_BIN = 8                                        # the one-bin-row pattern's frequency, and the first atom's


def middle(T, F, Q):
    """(first, last, atom frame) of the silent middle: the atom frame is more than Q - 1 frames from the energy either side."""
    if Q > 8:
        c = (2 * Q + 3 + T - (Q + 2)) // 2
        return c - Q, c + Q, c
    return (20, 30, 25) if F > 513 else (30, 44, 37)


def atoms(T, F, Q, L):
    """[(frame, bin)] of the two isolated atoms of sparse_case."""
    m = middle(T, F, Q)[2]
    return [(m, ROW_BIN), (m, ROW_BIN + L + 2)]


def thresholds(A):
    return THR_LEVELS / np.mean(A)


def sparse_case(T, F, Q, L, seed, pattern="sparse"):
    """(S complex128, A float64, thr): see the module docstring.  Q: frames per stencil row (W.shape[1]); L: stencil half-width."""
    rng = np.random.default_rng(seed)
    A = rng.choice(LEVELS, size=(T, F))
    phase = rng.uniform(-np.pi, np.pi, size=(T, F))
    cut = int(0.7 * F)
    A[:, cut:] = 0.0
    A[:, 0] = 0.0
    if pattern == "sparse":
        lo, hi, m = middle(T, F, Q)
        assert 2 * Q + 3 < lo - 2 and hi + 3 < T - (Q + 2) and L <= ROW_BIN and ROW_BIN + L + 2 < cut, (T, F, Q, L)
        A[:2 * Q + 3] = 0.0
        A[T - (Q + 2):] = 0.0
        A[lo:hi + 1] = 0.0
        A[m, ROW_BIN], A[m, ROW_BIN + L + 2] = 1.0, 2.0
    elif pattern == "one-frame":
        keep = T // 2
        A[:keep] = 0.0
        A[keep + 1:] = 0.0
    elif pattern == "one-bin-row":
        row = np.where(A[:, ROW_BIN] == 0.0, 0.5, A[:, ROW_BIN])      # (no frame of the row is silent)
        A[:] = 0.0
        A[:, ROW_BIN] = row
    else:
        raise ValueError(pattern)
    S = A * np.exp(1j * phase)
    S[A == 0.0] = 0.0
    return S, A, thresholds(A)


def batch_case(T, F, Q, L, seed):
    """(S (4, T, F), A, thr): [loud x 40, all-zero, sparse, sparse x 2^-12].  One relative threshold vector serves all four: the
    spectrograms' means differ by a few percent (and by the factors 40 and 2^-12, which the scaling by mean|S| removes), the
    scaled thresholds stay strictly between the levels (asserted by tests/test_sparse_cases.py)."""
    loud, A_loud, _ = sparse_case(T, F, Q, L, seed + 1000)
    S, A, thr = sparse_case(T, F, Q, L, seed)
    Sb = np.stack([40.0 * loud, np.zeros_like(S), S, S * 2.0 ** -12])
    Ab = np.stack([40.0 * A_loud, np.zeros_like(A), A, A * 2.0 ** -12])
    return Sb, Ab, thr


def margin_to_thresholds(A, thr):
    """min over the non-zero bins and the thresholds of |A - thr_k mean| / A: how far the nearest bin is from changing sides."""
    mean = np.mean(A)
    nz = A[A > 0]
    if nz.size == 0:
        return np.inf
    return min(float(np.min(np.abs(nz - t * mean) / nz)) for t in np.asarray(thr))


def isolated(A, Q, L, past_only=False):
    """The non-zero bins with no other non-zero bin within L bins and Q - 1 frames (the Hermitian images of the bins below DC and
    above Nyquist lie inside that window too): their weighted sums are structurally zero, every engine must leave their bits.
    past_only: the window of a no-future sweep in the reference's canonical addressing -- the Q - 1 frames before the bin's own,
    and of its own frame the bin alone."""
    T, F = A.shape
    nz = np.zeros((T + 2 * (Q - 1), F + 2 * L))
    nz[:, L:L + F] = np.pad(A > 0, ((Q - 1, Q - 1), (0, 0)), mode="edge")      # (the reference repeats the first and the last frame)
    count = np.zeros((T, F))
    for dt in range(Q - 1 if past_only else 2 * Q - 1):
        for df in range(2 * L + 1):
            count += nz[dt:dt + T, df:df + F]
    return (A > 0) & (count == (0 if past_only else 1))


def ambiguous(ref, S, A, Q, L, past_only=False):
    """The non-zero, non-isolated bins that the reference leaves within 1e-5 |S| of their input: a bin whose neighbourhood reaches it
    only through weights that vanish, or whose weighted sum is (almost) collinear with the bin itself, is rewritten with its own
    phase; whether the new bits equal the old ones is then a matter of the last rounding (the fp64 oracle itself answers differently
    for an input and for its complex64 rounding, tests/test_sparse_cases.py).  Such bins are compared by value, not by
    written / not written."""
    return (A > 0) & ~isolated(A, Q, L, past_only) & (np.abs(ref - S) < 1e-5 * A)


def music_schedule(A):
    """Keyword arguments for lws(..., mode='music') whose three schedules (1 no-future sweep, 10 online iterations, 5 batch sweeps)
    stay clear of the magnitude levels of A: run_lws end to end."""
    m = float(np.mean(A))
    return dict(mode="music", nofuture_alpha=0.75 / m, online_alpha=3.0 / m, online_beta=0.35, batch_iterations=5,
                batch_alpha=3.0 / m, batch_beta=0.7)


# ---------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_sparse.py.  id: (fsize, fshift, L, T, stage, plan keywords, environment, kernel name)
#   stage: batch / nofuture / online; plan keywords as _capi.Plan takes them (plus use_simplifications=False: general weights);
#   the name is matched exactly, or as a prefix when it ends in "*".  T = 70 unless the frame is wider than 513 bins.
ENGINES = {
    # -- the seventeen systolic builds (lws_systolic_builds.h), in plan creation's order
    "quarter_r16": (64, 32, 5, 70, "batch", {}, {}, "systolic_quarter_r16_q2_l5_hann"),
    "quarter": (64, 16, 5, 70, "batch", {}, {}, "systolic_quarter_q4_l5_hann"),
    "quarter_end_in_block": (60, 15, 5, 70, "batch", {}, {}, "systolic_quarter_q4_*"),
    "half_r16": (512, 256, 5, 70, "batch", {}, {}, "systolic_half_r16_q2_l5_hann"),
    "half": (512, 128, 5, 70, "batch", {}, {}, "systolic_half_q4_l5_hann"),
    "r16": (1024, 512, 5, 70, "batch", {}, {}, "systolic_r16_q2_l5_hann"),
    "narrow": (1024, 256, 5, 70, "batch", {}, {}, "systolic_q4_l5_hann"),
    "q8": (64, 8, 5, 70, "batch", {}, {}, "systolic_q8_l5_hann"),
    "q8_end_in_block": (56, 7, 5, 70, "batch", {}, {}, "systolic_q8_l5_hann"),
    "wide_r16": (1056, 528, 5, 40, "batch", {}, {}, "systolic_wide_r16_q2_l5_hann"),
    "wide": (1056, 264, 5, 40, "batch", {}, {}, "systolic_wide_q4_l5_hann"),
    "xwide": (2056, 514, 5, 40, "batch", {}, {}, "systolic_xwide_q4_*"),
    "l7": (64, 16, 7, 70, "batch", {}, {}, "systolic_q4_l7_allmask"),
    "tw_half": (48, 16, 5, 70, "batch", {}, {}, "systolic_half_q3_l5_hannmask_tw"),
    "tw_half_fractional": (400, 160, 5, 70, "batch", {}, {}, "systolic_half_q3_*"),
    "tw": (768, 256, 5, 70, "batch", {}, {}, "systolic_q3_l5_hannmask_tw"),
    "tw_wide": (1536, 512, 5, 40, "batch", {}, {}, "systolic_wide_q3_l5_hannmask_tw"),
    "tw_r40": (80, 16, 5, 70, "batch", {}, {}, "systolic_r40_q5_l5_tw"),
    "tw_r48": (96, 16, 5, 70, "batch", {}, {}, "systolic_r48_q6_l5_tw"),
    "tw_r64": (112, 16, 5, 70, "batch", {}, {}, "systolic_r64_q7_l5_tw"),
    # -- fp16 storage
    "fp16_quarter": (64, 16, 5, 70, "batch", {"storage": "fp16"}, {}, "systolic_quarter_q4_l5_hann_f16"),
    "fp16_narrow": (1024, 256, 5, 70, "batch", {"storage": "fp16"}, {}, "systolic_q4_l5_hann_f16"),
    # -- the band engine, fp32 and fp64
    "band_44_11": (44, 11, 5, 70, "batch", {}, {}, "band_fp32"),
    "band_q16": (128, 8, 5, 120, "batch", {}, {}, "band_fp32"),
    "band_l8": (64, 16, 8, 70, "batch", {}, {}, "band_fp32"),
    "band64_44_11": (44, 11, 5, 70, "batch", {"precision": "fp64"}, {"LWS_NO_SYS64": "1"}, "band_fp64"),     # (else: the fp64 systolic engine)
    "band64_q16": (128, 8, 5, 120, "batch", {"precision": "fp64"}, {}, "band_fp64"),
    "band64_l8": (64, 16, 8, 70, "batch", {"precision": "fp64"}, {}, "band_fp64"),
    # -- the fp64 systolic engine
    "sys64_q2": (64, 32, 5, 70, "batch", {"precision": "fp64"}, {}, "systolic_fp64_q2"),
    "sys64_q4": (64, 16, 5, 70, "batch", {"precision": "fp64"}, {}, "systolic_fp64_q4"),
    # -- the generic engine, skewed and plain layout
    "generic_skew": (64, 16, 5, 70, "batch", {"force_generic": True}, {}, "generic_skew_fp32"),
    "generic_plain": (64, 16, 5, 70, "batch", {"force_generic": True, "generic_plain_layout": True}, {}, "generic_fp32"),
    "generic64_skew": (64, 16, 5, 70, "batch", {"force_generic": True, "precision": "fp64"}, {}, "generic_skew_fp64"),
    "generic64_plain": (64, 16, 5, 70, "batch", {"force_generic": True, "generic_plain_layout": True, "precision": "fp64"}, {}, "generic_fp64"),
    # -- no-future sweeps (Q >= 3: at Q = 2 the reference's no-future sweep updates nothing, tests/test_sparse_cases.py)
    "nf_compat": (64, 16, 5, 70, "nofuture", {}, {}, "nofuture_lds_q4compat_fp32"),
    "nf_compat_serial": (64, 16, 5, 70, "nofuture", {}, {"LWS_NOFUTURE_SERIAL_TAPS": "1"}, "nofuture_lds_q4compat_fp32"),
    "nf_canonical": (64, 16, 5, 70, "nofuture", {"nofuture_q4_compat": False}, {}, "nofuture_lds_fp32"),
    "nf_canonical_serial": (64, 16, 5, 70, "nofuture", {"nofuture_q4_compat": False}, {"LWS_NOFUTURE_SERIAL_TAPS": "1"}, "nofuture_lds_fp32"),
    "nf_canonical_q3": (48, 16, 5, 70, "nofuture", {}, {}, "nofuture_lds_fp32"),
    "nf_team": (64, 16, 5, 70, "nofuture", {"nofuture_q4_compat": False}, {"LWS_TEAM_FIRST": "1"}, "team_nofuture_fp32"),
    # -- online sweeps
    "on_layout2": (64, 16, 5, 70, "online", {}, {"LWS_ONLINE_LAYOUT": "2"}, "online_lds_fp32"),
    "on_layout4": (64, 16, 5, 70, "online", {}, {"LWS_ONLINE_LAYOUT": "4"}, "online_lds_fp32"),
    "on_tw_q3": (48, 16, 5, 70, "online", {}, {}, "online_lds_fp32"),
    "on_fp64": (64, 16, 5, 70, "online", {"precision": "fp64"}, {}, "online_lds_fp64"),
    "on_team": (64, 16, 5, 70, "online", {}, {"LWS_TEAM_FIRST": "1"}, "team_online_fp32"),
}

# one representative of each engine family: the further patterns, the batch case and the power-of-two covariance
FAMILIES = {"systolic": "quarter", "systolic_fp16": "fp16_quarter", "band": "band_44_11", "band64": "band64_44_11", "sys64": "sys64_q4",
            "generic": "generic_skew", "nofuture_lds": "nf_canonical", "nofuture_team": "nf_team", "online_lds": "on_layout4",
            "online64": "on_fp64", "online_team": "on_team"}
# the engines that state scale handling: bit for bit at 2^+-66 too
SCALE_EXACT = ("systolic", "systolic_fp16", "nofuture_lds", "online_lds")
LOOK_AHEAD = 3
MUSIC = {"music_q4": (64, 16, 5, 70), "music_q3": (48, 16, 5, 70)}


def config(fsize, fshift, L, kw=()):
    """The lws object (weights of the three sweeps; pure numpy) of a case."""
    import lws_amd
    return lws_amd.lws(fsize, fshift, L=L, look_ahead=LOOK_AHEAD, use_simplifications=dict(kw).get("use_simplifications", True))


def oracle_stage(oracle, cfg, stage, S, thr, compat=True):
    """The fp64 reference of one stage, as class lws calls it (no-future sweeps use W_ai: lws.pyx:475)."""
    if stage == "batch":
        return oracle.batch_lws(S, cfg.W, thr)
    if stage == "nofuture":
        return oracle.nofuture_lws(S, cfg.W_ai, thr, compat=compat)
    return oracle.online_lws(S, cfg.W, cfg.W_ai, cfg.W_af, thr, cfg.look_ahead, cfg.fshift)


def music_reference(oracle, p, S):
    """run_lws in the fp64 oracle: no-future (W_ai, the shipped Q = 4 addressing), online, batch -- each stage with the thresholds
    class lws derives from its schedule, scaled by the mean magnitude of the stage's input (lws.pyx:470-499)."""
    import lws_amd
    thr = {st: lws_amd.get_thresholds(*[getattr(p, "%s_%s" % (st, k)) for k in ("iterations", "alpha", "beta", "gamma")])
           for st in ("nofuture", "online", "batch")}
    r = oracle.nofuture_lws(S, p.W_ai, thr["nofuture"], compat=True)
    r = oracle.online_lws(r, p.W, p.W_ai, p.W_af, thr["online"], p.look_ahead, p.fshift)
    return oracle.batch_lws(r, p.W, thr["batch"])


def past_only(stage, Q, kw):
    """Whether the stage is a no-future sweep in the canonical addressing (the shipped Q = 4 kernel's flat offset reads other bins)."""
    return stage == "nofuture" and not (Q == 4 and dict(kw).get("nofuture_q4_compat", True))


def case_seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name))
