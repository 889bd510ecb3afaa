"""GPU (-m gpu): which engine serves a stage (lws_capi.hip: choose_engine).  A table of small plans, one per branch of the chooser and
per routing switch, in both precisions and all four sweep modes; each row pins the kernel name the plan reports and the stage, if any,
that ran on the generic engine.  The expected values were recorded on the library before the chooser was factored out of run_stage."""
import contextlib
import warnings

import numpy as np
import pytest

import lws_amd
from lws_amd import _capi

pytestmark = pytest.mark.gpu

B, T, ITERS, LA = 2, 16, 2, 2

# id: (precision, fsize, fshift, L, stage, plan keywords, environment, (kernel name, lws_generic_stage))
#   stage: batch / nofuture / online.  Plans are created AFTER the environment is set (LWS_NO_SYSTOLIC and the LWS_SYSTOLIC_NO_*
#   switches are read at plan creation, the others at each launch).  Plan keywords: use_simplifications=False asks for general weights.
ROUTES = {
    # -- fp32 batch: the systolic builds, in plan creation's order, and the switches that skip some of them
    "sys_short_q4": ("fp32", 64, 16, 5, "batch", {}, {}, ("systolic_quarter_q4_l5_hann", "")),
    "sys_short_q2": ("fp32", 64, 32, 5, "batch", {}, {}, ("systolic_quarter_r16_q2_l5_hann", "")),
    "sys_quarter_q4_f129": ("fp32", 256, 64, 5, "batch", {}, {}, ("systolic_quarter_q4_l5_hann", "")),
    "sys_half_q4": ("fp32", 512, 128, 5, "batch", {}, {}, ("systolic_half_q4_l5_hann", "")),
    "sys_half_q2": ("fp32", 512, 256, 5, "batch", {}, {}, ("systolic_half_r16_q2_l5_hann", "")),
    "sys_half_q2_no_r16": ("fp32", 512, 256, 5, "batch", {}, {"LWS_SYSTOLIC_NO_R16": "1"}, ("systolic_half_q2_l5_hann", "")),
    "sys_no_short": ("fp32", 256, 64, 5, "batch", {}, {"LWS_SYSTOLIC_NO_SHORT": "1"}, ("systolic_q4_l5_hann", "")),
    "sys_q4": ("fp32", 1024, 256, 5, "batch", {}, {}, ("systolic_q4_l5_hann", "")),
    "sys_q2": ("fp32", 1024, 512, 5, "batch", {}, {}, ("systolic_r16_q2_l5_hann", "")),
    "sys_q2_no_r16": ("fp32", 1024, 512, 5, "batch", {}, {"LWS_SYSTOLIC_NO_R16": "1"}, ("systolic_q2_l5_hann", "")),
    "sys_q8": ("fp32", 1024, 128, 5, "batch", {}, {}, ("systolic_q8_l5_hann", "")),
    "sys_wide_q4": ("fp32", 2048, 512, 5, "batch", {}, {}, ("systolic_wide_q4_l5_hann", "")),
    "sys_wide_q2": ("fp32", 2048, 1024, 5, "batch", {}, {}, ("systolic_wide_r16_q2_l5_hann", "")),
    "sys_xwide_q4": ("fp32", 4096, 1024, 5, "batch", {}, {}, ("systolic_xwide_q4_l5_hann", "")),
    "sys_l7": ("fp32", 1024, 256, 7, "batch", {}, {}, ("systolic_q4_l7_allmask", "")),
    "sys_tw_q3": ("fp32", 768, 256, 5, "batch", {}, {}, ("systolic_q3_l5_hannmask_tw", "")),
    "sys_tw_short_q3": ("fp32", 192, 64, 5, "batch", {}, {}, ("systolic_half_q3_l5_hannmask_tw", "")),
    "sys_no_tw_q3": ("fp32", 768, 256, 5, "batch", {}, {"LWS_SYSTOLIC_NO_TW": "1"}, ("band_fp32", "")),
    "sys_tw_wide_q3": ("fp32", 1536, 512, 5, "batch", {}, {}, ("systolic_wide_q3_l5_hannmask_tw", "")),
    "band_general_fractional_q": ("fp32", 1000, 120, 5, "batch", {"use_simplifications": False}, {}, ("band_fp32", "")),
    "sys_tw_q5": ("fp32", 640, 128, 5, "batch", {}, {}, ("systolic_r40_q5_l5_tw", "")),
    "sys_tw_q6": ("fp32", 768, 128, 5, "batch", {}, {}, ("systolic_r48_q6_l5_tw", "")),
    "sys_no_tw_q5": ("fp32", 640, 128, 5, "batch", {}, {"LWS_SYSTOLIC_NO_TW": "1"}, ("band_fp32", "")),
    "sys_general_q4": ("fp32", 1024, 256, 5, "batch", {"use_simplifications": False}, {}, ("systolic_q4_l5_hann", "")),
    "sys_fp16": ("fp32", 1024, 256, 5, "batch", {"storage": "fp16"}, {}, ("systolic_q4_l5_hann_f16", "")),
    "sys_plain_layout": ("fp32", 1024, 256, 5, "batch", {"generic_plain_layout": True}, {}, ("systolic_q4_l5_hann", "")),
    # -- fp32 batch beyond the systolic builds: band, the skewed generic engine, the plain generic engine
    "no_systolic_band": ("fp32", 1024, 256, 5, "batch", {}, {"LWS_NO_SYSTOLIC": "1"}, ("band_fp32", "")),
    "band_q16": ("fp32", 1024, 64, 5, "batch", {}, {}, ("band_fp32", "")),
    "band_l8": ("fp32", 1024, 256, 8, "batch", {}, {}, ("band_fp32", "")),
    "plain_generic": ("fp32", 1024, 256, 5, "batch", {"generic_plain_layout": True}, {"LWS_NO_SYSTOLIC": "1"}, ("generic_fp32", "batch")),
    "force_generic_batch": ("fp32", 1024, 256, 5, "batch", {"force_generic": True}, {}, ("generic_skew_fp32", "batch")),
    "force_generic_plain": ("fp32", 1024, 256, 5, "batch", {"force_generic": True, "generic_plain_layout": True}, {}, ("generic_fp32", "batch")),
    # -- fp32 no-future: Q4-compat and plain LDS engine, the team engine first or as the fallback, the generic engine
    "nf_q4compat": ("fp32", 1024, 256, 5, "nofuture", {}, {}, ("nofuture_lds_q4compat_fp32", "")),
    "nf_q4": ("fp32", 1024, 256, 5, "nofuture", {"nofuture_q4_compat": False}, {}, ("nofuture_lds_fp32", "")),
    "nf_q2": ("fp32", 1024, 512, 5, "nofuture", {}, {}, ("nofuture_lds_fp32", "")),
    "nf_q4_team_first": ("fp32", 1024, 256, 5, "nofuture", {"nofuture_q4_compat": False}, {"LWS_TEAM_FIRST": "1"}, ("team_nofuture_fp32", "")),
    "nf_q4compat_team_first": ("fp32", 1024, 256, 5, "nofuture", {}, {"LWS_TEAM_FIRST": "1"}, ("nofuture_lds_q4compat_fp32", "")),
    "nf_q16_team": ("fp32", 1024, 64, 5, "nofuture", {}, {}, ("team_nofuture_fp32", "")),
    "nf_q16_no_team": ("fp32", 1024, 64, 5, "nofuture", {}, {"LWS_NO_TEAM": "1"}, ("generic_fp32", "no-future")),
    "nf_q16_serial": ("fp32", 1024, 64, 5, "nofuture", {}, {"LWS_NOFUTURE_SERIAL_TAPS": "1"}, ("generic_fp32", "no-future")),
    "nf_q4_serial": ("fp32", 1024, 256, 5, "nofuture", {"nofuture_q4_compat": False}, {"LWS_NOFUTURE_SERIAL_TAPS": "1"}, ("nofuture_lds_fp32", "")),
    "nf_force_generic": ("fp32", 1024, 256, 5, "nofuture", {"force_generic": True}, {}, ("generic_fp32", "no-future")),
    # -- fp32 online
    "on_q4": ("fp32", 1024, 256, 5, "online", {}, {}, ("online_lds_fp32", "")),
    "on_q3": ("fp32", 768, 256, 5, "online", {}, {}, ("online_lds_fp32", "")),
    "on_q4_serial": ("fp32", 1024, 256, 5, "online", {}, {"LWS_ONLINE_SERIAL_TAPS": "1"}, ("online_lds_fp32", "")),
    "on_q4_team_first": ("fp32", 1024, 256, 5, "online", {}, {"LWS_TEAM_FIRST": "1"}, ("team_online_fp32", "")),
    "on_q4_team_first_ordered": ("fp32", 1024, 256, 5, "online", {}, {"LWS_TEAM_FIRST": "1", "LWS_TEAM_ORDERED": "1"}, ("team_online_ordered_fp32", "")),
    "on_q16_team": ("fp32", 1024, 64, 5, "online", {}, {}, ("team_online_fp32", "")),
    "on_q16_team_ordered": ("fp32", 1024, 64, 5, "online", {}, {"LWS_TEAM_ORDERED": "1"}, ("team_online_ordered_fp32", "")),
    "on_q16_no_team": ("fp32", 1024, 64, 5, "online", {}, {"LWS_NO_TEAM": "1"}, ("generic_fp32", "online")),
    "on_q16_serial": ("fp32", 1024, 64, 5, "online", {}, {"LWS_ONLINE_SERIAL_TAPS": "1"}, ("generic_fp32", "online")),
    "on_force_generic": ("fp32", 1024, 256, 5, "online", {"force_generic": True}, {}, ("generic_fp32", "online")),
    # -- fp64 batch: sys64, band, the skewed and plain generic engine
    "f64_sys_q4": ("fp64", 1024, 256, 5, "batch", {}, {}, ("systolic_fp64_q4", "")),
    "f64_sys_q2": ("fp64", 1024, 512, 5, "batch", {}, {}, ("systolic_fp64_q2", "")),
    "f64_no_sys64": ("fp64", 1024, 256, 5, "batch", {}, {"LWS_NO_SYS64": "1"}, ("band_fp64", "")),
    "f64_band_q3": ("fp64", 768, 256, 5, "batch", {}, {}, ("band_fp64", "")),
    "f64_plain_layout": ("fp64", 1024, 256, 5, "batch", {"generic_plain_layout": True}, {}, ("generic_fp64", "batch")),
    "f64_force_generic": ("fp64", 1024, 256, 5, "batch", {"force_generic": True}, {}, ("generic_skew_fp64", "batch")),
    # -- fp64 no-future
    "f64_nf_q4compat": ("fp64", 1024, 256, 5, "nofuture", {}, {}, ("nofuture_lds_q4compat_fp64", "")),
    "f64_nf_q4": ("fp64", 1024, 256, 5, "nofuture", {"nofuture_q4_compat": False}, {}, ("nofuture_lds_fp64", "")),
    "f64_nf_q4_team_first": ("fp64", 1024, 256, 5, "nofuture", {"nofuture_q4_compat": False}, {"LWS_TEAM_FIRST": "1"}, ("nofuture_lds_fp64", "")),
    "f64_nf_q4_team_first_fp64": ("fp64", 1024, 256, 5, "nofuture", {"nofuture_q4_compat": False}, {"LWS_TEAM_FIRST": "1", "LWS_TEAM_FP64": "1"},
                                  ("team_nofuture_fp64", "")),
    "f64_nf_q16": ("fp64", 1024, 64, 5, "nofuture", {}, {}, ("generic_fp64", "no-future")),
    "f64_nf_q16_team_fp64": ("fp64", 1024, 64, 5, "nofuture", {}, {"LWS_TEAM_FP64": "1"}, ("team_nofuture_fp64", "")),
    "f64_nf_force_generic": ("fp64", 1024, 256, 5, "nofuture", {"force_generic": True}, {}, ("generic_fp64", "no-future")),
    # -- fp64 online: online64 (and its one-wave kernel), the Q = 8 team case and its switches, the team engine's fallback
    "f64_on_q4": ("fp64", 1024, 256, 5, "online", {}, {}, ("online_lds_fp64", "")),
    "f64_on_q4_one_wave": ("fp64", 1024, 256, 5, "online", {}, {"LWS_ONLINE64_ONE_WAVE": "1"}, ("online_lds_fp64_1w", "")),
    "f64_on_q4_team_first": ("fp64", 1024, 256, 5, "online", {}, {"LWS_TEAM_FIRST": "1"}, ("team_online_ordered_fp64", "")),
    "f64_on_q8": ("fp64", 1024, 128, 5, "online", {}, {}, ("team_online_ordered_fp64", "")),
    "f64_on_q8_no_team_q8": ("fp64", 1024, 128, 5, "online", {}, {"LWS_NO_TEAM_Q8": "1"}, ("online_lds_fp64", "")),
    "f64_on_q8_no_team": ("fp64", 1024, 128, 5, "online", {}, {"LWS_NO_TEAM": "1"}, ("online_lds_fp64", "")),
    "f64_on_q8_serial": ("fp64", 1024, 128, 5, "online", {}, {"LWS_ONLINE_SERIAL_TAPS": "1"}, ("online_lds_fp64", "")),
    "f64_on_q8_team_fp64": ("fp64", 1024, 128, 5, "online", {}, {"LWS_TEAM_FP64": "1"}, ("team_online_fp64", "")),
    "f64_on_q16": ("fp64", 1024, 64, 5, "online", {}, {}, ("team_online_ordered_fp64", "")),
    "f64_on_q16_no_team": ("fp64", 1024, 64, 5, "online", {}, {"LWS_NO_TEAM": "1"}, ("generic_fp64", "online")),
    "f64_on_force_generic": ("fp64", 1024, 256, 5, "online", {"force_generic": True}, {}, ("generic_fp64", "online")),
}


def spectrograms(F, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, T, F)) + 1j * rng.standard_normal((B, T, F))


def route(precision, fsize, fshift, L, stage, kw, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(kw)
    simple = kw.pop("use_simplifications", True)
    cfg = lws_amd.lws(fsize, fshift, L=L, use_simplifications=simple)
    F = fsize // 2 + 1
    plan = _capi.Plan(F, cfg.W, cfg.W_ai, cfg.W_af, precision=precision, **kw)
    S = spectrograms(F, fsize + fshift + L)
    thr = lws_amd.get_thresholds(ITERS, 1.0, 0.1, 1)
    with quiet():
        if stage == "batch":
            out = plan.batch(S, thr)
        elif stage == "nofuture":
            out = plan.nofuture(S, thr)
        else:
            out = plan.online(S, thr, LA, fsize / fshift)
    got = (plan.last_kernel()["name"], plan._lib.lws_generic_stage(plan._h).decode())
    assert np.isfinite(out).all()
    plan.close()
    return got


@contextlib.contextmanager
def quiet():
    """(the generic-engine RuntimeWarning of Plan._note_engine is expected for some rows)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


@pytest.mark.parametrize("rid", list(ROUTES))
def test_route(rid, monkeypatch):
    precision, fsize, fshift, L, stage, kw, env, expected = ROUTES[rid]
    assert route(precision, fsize, fshift, L, stage, kw, env, monkeypatch) == expected


def test_pipeline_reports_every_stage(monkeypatch):
    """A three-stage call (no-future, online, batch): the name is the last stage's, the generic stage any stage's."""
    cfg = lws_amd.lws(1024, 64, L=5)
    F = 513
    plan = _capi.Plan(F, cfg.W, cfg.W_ai, cfg.W_af)
    S = spectrograms(F, 7)
    thr = lws_amd.get_thresholds(ITERS, 1.0, 0.1, 1)
    monkeypatch.setenv("LWS_NO_TEAM", "1")
    with quiet():
        plan.run(S, thr, thr, LA, 16.0, thr)
    assert (plan.last_kernel()["name"], plan._lib.lws_generic_stage(plan._h).decode()) == ("band_fp32", "online")
    plan.close()


@pytest.mark.parametrize("fshift,chunks,name", [(256, 2, "systolic_q4_l5_hann"), (64, 1, "band_fp32")])
def test_host_chunking_follows_the_engine(fshift, chunks, name, monkeypatch, capfd):
    """Host-array calls of an fp32 plan are cut into chunks; a stage that is not on the systolic engine (whole_device) keeps a device's
    worth of spectrograms per chunk.  With a one-bin chunk target, two spectrograms are two chunks only on the systolic engine."""
    monkeypatch.setenv("LWS_HOST_CHUNK_BINS", "1")
    monkeypatch.setenv("LWS_HOST_TRACE", "1")
    cfg = lws_amd.lws(1024, fshift, L=5)
    plan = _capi.Plan(513, cfg.W, cfg.W_ai, cfg.W_af)
    plan.batch(spectrograms(513, 3), lws_amd.get_thresholds(ITERS, 1.0, 0.1, 1))
    assert plan.last_kernel()["name"] == name
    err = capfd.readouterr().err
    assert ("pool up, chunks: %d\n" % chunks) in err, err
    plan.close()


def test_a_switch_binds_per_call_or_at_plan_creation(monkeypatch):
    """When a switch binds (lws_switches.h: CALL / CREATE).  LWS_NO_TEAM is read by every call: one plan follows the environment from
    call to call.  LWS_NO_SYSTOLIC is read by plan creation: what it decided stays with the plan whatever the environment says later."""
    thr = lws_amd.get_thresholds(ITERS, 1.0, 0.1, 1)
    S = spectrograms(513, 11)
    monkeypatch.delenv("LWS_NO_TEAM", raising=False)
    monkeypatch.delenv("LWS_NO_SYSTOLIC", raising=False)
    cfg = lws_amd.lws(1024, 64, L=5)                       # (the nf_q16_team row)
    plan = _capi.Plan(513, cfg.W, cfg.W_ai, cfg.W_af)
    names = []
    for no_team in (None, "1", None):
        if no_team is None:
            monkeypatch.delenv("LWS_NO_TEAM", raising=False)
        else:
            monkeypatch.setenv("LWS_NO_TEAM", no_team)
        with quiet():
            plan.nofuture(S, thr)
        names.append(plan.last_kernel()["name"])
    plan.close()
    assert names == ["team_nofuture_fp32", "generic_fp32", "team_nofuture_fp32"]

    cfg = lws_amd.lws(1024, 256, L=5)
    early = _capi.Plan(513, cfg.W, cfg.W_ai, cfg.W_af)     # created with LWS_NO_SYSTOLIC unset
    monkeypatch.setenv("LWS_NO_SYSTOLIC", "1")
    late = _capi.Plan(513, cfg.W, cfg.W_ai, cfg.W_af)
    early.batch(S, thr)
    late.batch(S, thr)
    names = (early.last_kernel()["name"], late.last_kernel()["name"])
    early.close()
    late.close()
    assert names == ("systolic_q4_l5_hann", "band_fp32")
