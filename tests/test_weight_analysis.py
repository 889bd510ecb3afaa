"""CPU: the analysis of a weight tensor (lws_amd/csrc/lws_weights.cpp), made once per tensor at plan creation, says what the
functions it replaced said -- weights_twiddle (lws_online.hip) at every cap in use, weights_row_period (lws_nofuture.hip),
rows_are_twiddles (lws_band.hip) at both tolerances, base_weights<2|4> (lws_sys64.hip).  Their answers were recorded from the
last commit that had them (tests/golden/weight_analysis.json; recipe: tests/golden/make_golden.py weight_analysis) on the tensors
of cases() below, which the recorder imports.  lws_weights.cpp is plain C++: compiled here with g++, no GPU needed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import lws_amd

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lws_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
CAPS = (4, 16, 128, 512, 4096)      # ... and the tensor's own Q: the caps weights_twiddle was called with (4: the r = 2 case below)

CONFIGS = [(1024, 256, 5), (1024, 512, 5), (512, 64, 5), (768, 256, 5), (640, 128, 5), (1024, 64, 5), (1024, 256, 7), (1024, 256, 8),
           (2048, 320, 5), (1000, 120, 5), (1000, 250, 2), (144, 16, 5)]
STRUCTURE_CONFIGS = [(64, 16), (64, 32), (64, 8), (48, 16), (1024, 256), (400, 160), (512, 160), (1024, 384), (1000, 400), (1000, 200),
                     (768, 128), (1024, 160), (512, 300), (1024, 176), (2048, 768), (100, 30), (1024, 100)]   # test_weights_structure.py

SHIM = r"""
#include "lws_weights.h"
extern "C" void weight_analysis(const double *W, int Q, int Qp, int L, const int *caps, int ncaps, int *tw, int *flags, double *scale) {
    const lws::WeightStructure ws = lws::analyse_weights(W, Q, Qp, L);
    for (int i = 0; i < ncaps; ++i) {
        tw[3 * i + 1] = tw[3 * i + 2] = -1;
        tw[3 * i] = ws.twiddle(caps[i], &tw[3 * i + 1], &tw[3 * i + 2]);
    }
    flags[0] = ws.row_period; flags[1] = ws.band_rows_fp64; flags[2] = ws.band_rows_fp32; flags[3] = ws.quarter_turns;
    *scale = ws.scale;
}
"""


def cases():
    """(name, W[Qp][Q][L+1] complex128), in a fixed order."""
    for fsize, fshift, L in CONFIGS:
        for simp in (True, False):
            p = lws_amd.lws(fsize, fshift, L=L, use_simplifications=simp)
            for name in ("W", "W_ai", "W_af"):
                yield "lws(%d,%d,L=%d)%s.%s" % (fsize, fshift, L, "" if simp else "[general]", name), getattr(p, name)
    # the tensors of tests/test_weights_structure.py
    for fsize, fshift in STRUCTURE_CONFIGS:
        p = lws_amd.lws(fsize, fshift)
        for name in ("W", "W_ai", "W_af"):
            yield "lws(%d,%d).%s" % (fsize, fshift, name), getattr(p, name)
        if fsize % fshift == 0:
            yield "lws(%d,%d)[general].W" % (fsize, fshift), lws_amd.lws(fsize, fshift, use_simplifications=False).W
    W = np.array(lws_amd.lws(64, 16).W)
    W[1, 1, 3] *= 1.01
    yield "lws(64,16).W, one weight off by 1 %", W
    W = np.array(lws_amd.lws(400, 160).W)
    W[37, 1, 0] += 1e-6
    yield "lws(400,160).W, one weight off by 1e-6", W
    rng = np.random.default_rng(0)
    yield "random (4,4,6)", rng.standard_normal((4, 4, 6)) + 1j * rng.standard_normal((4, 4, 6))
    base = rng.standard_normal((3, 6)) + 1j * rng.standard_normal((3, 6))
    pp = np.arange(14)[:, None, None]
    yield "hand-made, period 7, step 3", base[None] * np.exp(2j * np.pi * pp * np.arange(3)[None, :, None] * 3 / 7)
    # neighbour-frame weights at r = 2 only, turned by a third per bin: theta = 1/6 and theta = 2/3 both fit, and the first
    # candidate has the longer period -- a small cap and a large one answer differently
    base = rng.standard_normal((3, 6)) + 1j * rng.standard_normal((3, 6))
    base[1] = 0
    pp = np.arange(6)[:, None, None]
    yield "hand-made, r = 2 only, a third of a turn", base[None] * np.exp(2j * np.pi * pp * np.arange(3)[None, :, None] / 6)
    # a summarised tensor with one row 1e-11 of a turn off: good enough for fp32 arithmetic (1e-9), not for fp64's promise (1e-13)
    W = np.array(lws_amd.lws(1024, 256).W)
    W[1] *= np.exp(2j * np.pi * 1e-11)
    yield "lws(1024,256).W, row 1 turned by 1e-11", W
    # ... and one whose rows disagree about a weight the reference skips by its magnitude (|w| <= 1e-12)
    W = np.array(lws_amd.lws(1024, 256).W)
    W[:, 1, 5] *= 2e-12 / abs(W[0, 1, 5])
    W[0, 1, 5] *= 0.25
    yield "lws(1024,256).W, a weight of 0.5e-12 in row 0 and 2e-12 in the others", W


@pytest.fixture(scope="module")
def analyse():
    os.makedirs(BUILD, exist_ok=True)
    so, shim = os.path.join(BUILD, "libweight_analysis.so"), os.path.join(BUILD, "weight_analysis_shim.cpp")
    with open(shim, "w") as f:
        f.write(SHIM)
    # no contraction, as in the library's build of the same text
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, shim, os.path.join(CSRC, "lws_weights.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.weight_analysis.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp, vp]

    def run(W):
        W = np.ascontiguousarray(W, dtype=np.complex128)
        Qp, Q, K1 = W.shape
        caps = np.array((Q,) + CAPS, dtype=np.intc)
        tw, flags, scale = np.zeros((len(caps), 3), dtype=np.intc), np.zeros(4, dtype=np.intc), np.zeros(1)
        lib.weight_analysis(W.ctypes.data, Q, Qp, K1 - 1, caps.ctypes.data, len(caps), tw.ctypes.data, flags.ctypes.data, scale.ctypes.data)
        twiddle = {("Q" if i == 0 else str(c)): ([int(tw[i, 1]), int(tw[i, 2])] if tw[i, 0] else None) for i, c in enumerate(caps)}
        return {"shape": [Qp, Q, K1], "twiddle": twiddle, "row_period": int(flags[0]), "rows_1e-13": bool(flags[1]), "rows_1e-9": bool(flags[2]),
                "quarter_turns": bool(flags[3]), "scale": float(scale[0])}
    return run


def test_the_analysis_says_what_the_functions_it_replaced_said(analyse):
    with open(os.path.join(HERE, "golden", "weight_analysis.json")) as f:
        golden = json.load(f)
    seen = []
    for name, W in cases():
        want, got = golden[name], analyse(W)
        seen.append(name)
        assert got["shape"] == want["shape"], name
        assert got["twiddle"] == want["twiddle"], (name, got["twiddle"], want["twiddle"])       # weights_twiddle(W, ..., cap), every cap
        # weights_row_period(W, ..., 256); plan creation took Q for a summarised tensor without asking
        assert got["row_period"] == (want["shape"][1] if want["shape"][0] == want["shape"][1] else want["row_period"]), name
        # rows_are_twiddles on the fit of cap 4096, as band_plan called it (null: band_plan had refused the tensor before it got there)
        assert got["rows_1e-13"] == bool(want["rows_1e-13"]) and got["rows_1e-9"] == bool(want["rows_1e-9"]), (name, got, want)
        # base_weights<Q>, which read six columns whatever L is: recorded where the tensor has six (null otherwise)
        if want["base_weights"] is not None:
            assert got["quarter_turns"] == want["base_weights"], name
        # (numpy's |.| against std::hypot: each within half an ulp of the true value)
        assert got["scale"] == pytest.approx(np.abs(W).max(), rel=1e-15, abs=0), name
    assert sorted(seen) == sorted(golden), "the fixture and cases() name different tensors"


def test_the_recorded_cases_tell_the_questions_apart():
    """The fixture is only a check if its tensors make the old functions disagree with each other where they should."""
    with open(os.path.join(HERE, "golden", "weight_analysis.json")) as f:
        g = json.load(f)
    r2 = g["hand-made, r = 2 only, a third of a turn"]["twiddle"]
    assert r2["Q"] == r2["4"] == [3, 2] and r2["16"] == r2["4096"] == [6, 1]              # first fit under the cap, not the smallest period
    turned = g["lws(1024,256).W, row 1 turned by 1e-11"]
    assert turned["rows_1e-9"] and not turned["rows_1e-13"] and not turned["base_weights"]
    skipped = g["lws(1024,256).W, a weight of 0.5e-12 in row 0 and 2e-12 in the others"]
    assert skipped["twiddle"]["4096"] == [4, 1] and not skipped["rows_1e-9"]              # fits to 1e-9; the rows disagree about the skip
    assert g["lws(1024,512,L=5).W_ai"]["twiddle"]["4096"] == [0, 0]                       # no neighbour-frame weight: any twiddle
    assert g["lws(2048,320,L=5).W"]["twiddle"]["16"] is None and g["lws(2048,320,L=5).W"]["twiddle"]["128"] == [32, 5]
    assert g["lws(2048,320,L=5).W"]["row_period"] == 32 and g["lws(1000,120,L=5).W"]["row_period"] == 25
    assert any(c["twiddle"]["4096"] is None for c in g.values())
