"""CPU: the shapes of a call of the systolic engine are plain host code (lws_amd/csrc/lws_systolic_geom.h), a function of a build's
constants, the plan's (F, Q), the call's (B, T, sweeps), the CU count, LWS_SYSTOLIC_NWG and the storage format.
tests/systolic_geometry_main.cpp is that header with a main of its own, compiled with g++; here: the invariants its comments state, over
every build of lws_systolic_builds.h x a grid of calls, and a few values worked out by hand from the formulas."""
import itertools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
MAX_ITERS = 440


def build_dims():
    """{build: (rowl_shift, skew, lag, nslots, wps)} from the rows of lws_systolic_builds.h, by the rules of lws_systolic.hip's header
    comment: a ring row holds 64 frames x waves per slot / slots per wave; frames 8 steps apart (L7: 16); the lag between sweeps is
    the ring's depth: 32 steps, 16 (R16), 64 (Q8, L7), 8 TWQ."""
    with open(os.path.join(ROOT, "lws_amd", "csrc", "lws_systolic_builds.h"), encoding="utf-8") as f:
        text = f.read()
    dims = {}
    for name, fields in re.findall(r"^#define LWS_BUILD_(\w+)\s+[\w:]+,\s*\"[^\"]*\",((?:\s*\d+,){7}\s*\d+)", text, re.M):
        wide, q8, spw, l7, r16, tw, twq, slots = (int(x) for x in fields.replace(" ", "").split(","))
        wps = {0: 1, 1: 2, 2: 4}[wide]
        rowl = 64 * wps // spw
        ring = 8 * twq if twq else (64 if (q8 or l7) else (16 if r16 else 32))
        dims[name] = (rowl.bit_length() - 1, 16 if l7 else 8, ring, slots, wps)
    order = re.findall(r"X\((\w+)\)", text)
    assert sorted(order) == sorted(dims) and len(dims) == 17
    return dims


DIMS = build_dims()


@pytest.fixture(scope="module")
def geometry():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "systolic_geometry_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "systolic_geometry_main.cpp"), "-o", exe],
                   check=True)

    def run(cases):
        """cases: (build, F, Q, B, T, iters, n_cu, forced, h16) -> one dict of the printed fields each"""
        text = "".join(" ".join(str(int(x)) for x in DIMS[c[0]] + tuple(c[1:])) + "\n" for c in cases)
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [{k: int(v) for k, v in (f.split("=") for f in line.split())} for line in out]
    return run


def test_the_six_geometry_classes():
    """the layout passes see a build through (row length, skew) alone"""
    assert sorted({(1 << d[0], d[1]) for d in DIMS.values()}) == [(16, 8), (32, 8), (64, 8), (64, 16), (128, 8), (256, 8)]


def test_values_worked_out_by_hand(geometry):
    narrow, quarter, one = geometry([("narrow", 513, 4, 256, 500, 100, 256, 0, 0), ("quarter", 129, 4, 3, 70, 100, 256, 0, 1),
                                     ("narrow", 513, 4, 1, 500, 100, 256, 0, 0)])
    want = dict(Tp=506, Kr=8, Kt=8, G=4096, TpPad=512, NT=16, nwg=1, n_full=256, nwg_rest=1, cb=8, rb=4, io_partials=128)
    assert {k: narrow[k] for k in want} == want
    # rows of 16 frames, rounds of 128 steps, 24 slots 32 steps apart: a pass of at least 24 * 32 + 96 = 864 rows is 7 rounds, where the
    # 76 frames fill 5; 8 * 63 + 128 steps of a group are 10 tiles of 64; one workgroup: a second one's lag does not fit the pass
    want = dict(Tp=76, Kr=7, Kt=2, G=896, TpPad=128, NT=10, ring_max=1, nwg=1, cb=4, rb=2, n_w=3 * 896 * 16, n_n=3 * 128)
    assert {k: quarter[k] for k in want} == want
    # one spectrogram on 256 CUs: 15 passes of 7 sweeps to share out, but only 4096 / (7 * 32 + 96) = 12 lags fit the pass
    assert (one["ring_max"], one["nwg"], one["n_full"], one["nwg_rest"]) == (12, 12, 1, 1)
    # 300 spectrograms on 256 CUs: the 44 of the second round share the CUs, 5 workgroups each
    (rest,) = geometry([("narrow", 513, 4, 300, 500, 100, 256, 0, 0)])
    assert (rest["nwg"], rest["n_full"], rest["nwg_rest"]) == (1, 256, 5)


def test_the_invariants_hold_for_every_build_on_a_grid_of_calls(geometry):
    grid = list(itertools.product((17, None), (2, 4), (1, 3, 64, 257, 300), (1, 70, 500, 6000), (1, 100, 441), (256, 80), (0, 2, 1000), (0, 1)))
    for name, (shift, skew, lag, nslots, wps) in DIMS.items():
        rowl, rowp = 1 << shift, skew << shift
        cases = [(name, rowp + 1 if F is None else F) + tuple(rest) for F, *rest in grid]   # (the longest frames of the build)
        results = geometry(cases)
        unforced = {c[1:]: g for c, g in zip(cases, results) if c[7] == 0}
        for (_, F, Q, B, T, iters, n_cu, forced, h16), g in zip(cases, results):
            case = (name, F, Q, B, T, iters, n_cu, forced, h16)
            passes = -(-min(iters, MAX_ITERS) // nslots)
            assert g["Tp"] == T + 2 * (Q - 1)
            # a pass: whole rounds that hold every frame, and longer than the last slot's lag behind the loader plus its read-ahead
            assert g["G"] == rowp * g["Kr"] and g["Kr"] * rowl >= g["Tp"] and g["G"] >= nslots * lag + 96, case
            assert g["Kr"] == max(-(-g["Tp"] // rowl), -(-(nslots * lag + 96) // rowp)), case
            assert g["TpPad"] % 64 == 0 and g["Tp"] <= g["TpPad"] < g["Tp"] + 64, case
            # the tiles cover the frames and a group's production times, with less than a tile to spare
            assert 0 <= 64 * g["Kt"] - g["Tp"] < 64 and 0 <= 64 * g["NT"] - (skew * 63 + F - 1) < 64, case
            assert g["io_partials"] == g["Kt"] * g["NT"]
            # workgroups per spectrogram: all resident, their lags within a pass, none without a pass -- unless the count is forced
            nwg, free = g["nwg"], unforced[(F, Q, B, T, iters, n_cu, 0, h16)]
            assert 1 <= nwg <= g["ring_max"] == g["G"] // (nslots * lag + 96), case
            assert nwg == 1 or nwg * B <= n_cu, case
            if forced >= 1 and forced * B <= n_cu:
                assert nwg == min(forced, g["ring_max"]), case
            else:   # a forced count that does not fit is not honoured
                assert nwg <= passes and nwg == free["nwg"], case
                assert nwg == max(1, min(n_cu // B, passes, g["ring_max"])), case
            # a batch larger than the chip: whole rounds with one workgroup each, the rest shares the CUs
            rest = B - g["n_full"]
            assert 0 <= rest < n_cu and (rest == 0) == (g["nwg_rest"] == 1), case
            if rest:
                assert nwg == 1 and B > n_cu and rest == B % n_cu and g["nwg_rest"] * rest <= n_cu and g["nwg_rest"] <= g["ring_max"], case
            # the scratch: the regions in their order, disjoint, each inside its block; 16-byte boundaries where the kernels want them
            assert (g["cb"], g["rb"]) == ((4, 2) if h16 else (8, 4))
            assert g["n_w"] == B * g["G"] * rowl and g["n_n"] == B * g["TpPad"]
            assert g["off_state_nyq"] == g["n_w"] * g["cb"] and g["need_s"] == g["off_state_nyq"] + g["n_n"] * g["cb"], case
            assert g["off_state_nyq"] % 16 == 0 and g["off_amp_nyq"] % 16 == 0 and g["off_amax"] % 16 == 0, case
            assert g["off_amp_nyq"] == g["n_w"] * g["rb"] and 0 <= g["off_amax"] - (g["off_amp_nyq"] + g["n_n"] * g["rb"]) < 16, case
            assert g["off_thr_min"] == g["off_amax"] + 4 * B and g["off_progress"] == g["off_thr_min"] + 4 * B, case
            assert g["off_err"] == g["off_progress"] + 4 * (g["n_prog"] - 1) and g["need_a"] == g["off_err"] + 4, case
            # progress counters: one per workgroup and wave of a slot, the rest's after those of B spectrograms; the flag after all
            assert (B * nwg + rest * g["nwg_rest"]) * wps <= g["n_prog"] - 1, case
            # the scratch of a shape does not grow with the schedule, nor with a forced count
            same = unforced[(F, Q, B, T, 1, n_cu, 0, h16)]
            assert (g["need_s"], g["need_a"], g["off_err"]) == (same["need_s"], same["need_a"], same["off_err"]), case
