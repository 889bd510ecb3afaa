"""CPU: the decode of an online sweep is one function (lws_amd/csrc/lws_online_unit.h: sweep number s, frame position j -> the frame
to update, its weight tensor, whether its own bins take part, how many frames to its right are usable, valid or not), called by every
engine that runs the online driver.  tests/online_unit_main.cpp is that header with a main of its own, compiled with g++; here its
units, in (s, j) order, are held to TF_RTISI_LA's loop nest (lwslib.cpp:1432-1491) and the frame loop of the Asym_UpdatePhase* calls
it makes (lwslib.cpp:1141-1151), restated call by call."""
import functools
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")

W, W_AI, W_AF = 0, 1, 2     # LWS_W, LWS_W_AI, LWS_W_AF: the order of GenericArgs::w

GRID = list(itertools.product((1, 2, 5), (0, 1, 3), (1, 3), (2, 4, 8)))    # T, LA, n_thr, Q


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "online_unit_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "online_unit_main.cpp"), "-o", exe], check=True)

    @functools.lru_cache(maxsize=None)
    def run(T, LA, n_thr, Q):
        out = subprocess.run([exe, str(T), str(LA), str(n_thr), str(Q)], check=True, capture_output=True, text=True).stdout
        keys = ("s", "j", "valid", "m", "q", "rho", "wset", "centre", "ts")
        return [dict(zip(keys, map(int, line.split()))) for line in out.splitlines()]
    return run


def asym_update_phase(first, M, M0, wset, thr_index, Q):
    """One Asym_UpdatePhase* call on frames first .. first + M - 1 with M0 frames usable from the first one on -- the frame loop of
    lwslib.cpp:1141-1151: local frame i uses rframe - 1 frames on its right (at most Q - 1) and its own bins, cframe, unless M0 - i < 1."""
    for i in range(M):
        rframe = min(M0 - i, Q)
        cframe = 1
        if rframe < 1:
            cframe, rframe = 0, 1
        yield (first + i, wset, cframe, rframe, thr_index)


def tf_rtisi_la(T, LA, n_thr, Q):
    """(frame, weight tensor, centre, usable right-hand frames + 1, threshold index or None) of every frame update, in the reference's order"""
    for m in range(T):
        lframe, nframe = m - LA, LA
        if lframe < 0:
            lframe, nframe = 0, m
        yield from asym_update_phase(m, 1, 0, W_AI, None, Q)                      # first estimate of the newest frame, threshold 0
        for h in range(n_thr):
            if LA > 0:
                yield from asym_update_phase(lframe, nframe, nframe + 1, W, h, Q)  # the look-ahead frames
            yield from asym_update_phase(m, 1, 1, W_AF, h, Q)                     # the newest frame


@pytest.mark.parametrize("T,LA,n_thr,Q", GRID)
def test_the_valid_units_are_the_references_frame_updates_in_its_order(driver, T, LA, n_thr, Q):
    units = driver(T, LA, n_thr, Q)
    per = n_thr + 1
    assert [(u["s"], u["j"]) for u in units] == [(s, j) for s in range(T * per) for j in range(LA + 1)]
    got = [(u["rho"], u["wset"], u["centre"], u["ts"], u["q"] - 1 if u["q"] else None) for u in units if u["valid"]]
    want = list(tf_rtisi_la(T, LA, n_thr, Q))
    assert got == want
    # ... which is, in closed form: frames max(0, m - LA) .. m, the newest with W_af, min(Q, m - rho + 1) usable frames
    for u in units:
        assert (u["m"], u["q"]) == divmod(u["s"], per)
        if u["valid"] and u["q"]:
            assert u["ts"] == min(Q, u["m"] - u["rho"] + 1) and u["wset"] == (W_AF if u["rho"] == u["m"] else W)


@pytest.mark.parametrize("T,LA,n_thr,Q", GRID)
def test_valid_units_stay_inside_the_frames_there_are_and_invalid_ones_drop_none(driver, T, LA, n_thr, Q):
    """A valid unit names a frame 0 .. m (< T).  An (s, j) is invalid only where the sweep has no such frame: a position past the
    first in a first estimate, or one whose frame max(0, m - LA) + j would lie beyond the newest frame m -- never a frame of 0 .. m."""
    for u in driver(T, LA, n_thr, Q):
        m, first = u["m"], max(0, u["m"] - LA)
        if u["valid"]:
            assert 0 <= u["rho"] <= m < T
            assert u["rho"] == (m if u["q"] == 0 else first + u["j"])
        elif u["q"] == 0:
            assert u["j"] != 0
        else:
            assert first + u["j"] > m and u["rho"] == first + u["j"]
