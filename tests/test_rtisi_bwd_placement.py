"""CPU: lws_rtisi_la_bwd_placement -- where k_rtisi_bwd keeps its state and with how many threads it runs -- against a restatement in
Python of the layout DESIGN section 7k describes, over the grid of tests/test_rtisi_placement.py without its K, at the rows on either
side of the LDS boundary that the GPU tests run, and at every row the GPU tables claim.  The query calls the function the launch site
calls; tests/test_gpu_rtisi_grad.py and tests/test_gpu_windows_grad.py assert through it the placement their comments claim."""
import ctypes

import pytest

import rtisi_grad_cases as rc
import window_cases as wc
from lws_amd import _capi
from test_rtisi_placement import CAP, GRID, layout as forward_layout

GRID3 = sorted({(N, hop, LA) for N, hop, LA, K in GRID})


def layout(N, hop, LA):
    """(in_lds, threads, dynamic LDS bytes), restated: gdone, G and Gn, three vectors of N + LA hop floats; in front, two N-point
    complex buffers and, where N is not a power of two, a third; the threads by the forward kernels' rule."""
    state = 3 * (N + LA * hop)
    transform = (2 if N & (N - 1) == 0 else 3) * N * 8
    total = transform + 4 * state
    threads = 256 if N <= 256 else 1024 if N >= 1024 else -(-N // 256) * 256
    return total <= CAP, threads, total if total <= CAP else transform


def test_query_is_the_layout_over_a_grid():
    both = set()
    for N, hop, LA in GRID3:
        got, want = _capi.rtisi_la_bwd_placement(N, hop, LA), layout(N, hop, LA)
        assert got == want, ((N, hop, LA), got, want)
        assert got[1] == _capi.rtisi_la_placement(N, hop, LA, 0)[1]
        both.add(want[:2])
    # the grid reaches both placements at every thread count
    assert both == {(lds, th) for lds in (False, True) for th in (256, 512, 768, 1024)}


# (N, hop, LA) on the LDS side with its bytes, then the neighbour on the scratch side
BOUNDARY = [
    ((3000, 1500, 3), 162000, (3000, 1500, 4)),            # three transform buffers: 1840 bytes under the cap; LA = 4 asks for 180000
    ((4096, 1024, 4), 163840, (4096, 1024, 5)),            # two: the cap to the byte; LA = 5 asks for 176128
]


@pytest.mark.parametrize("lds_side,nbytes,scratch_side", BOUNDARY)
def test_boundary_rows(lds_side, nbytes, scratch_side):
    in_lds, threads, got = _capi.rtisi_la_bwd_placement(*lds_side)
    print("backward placement %s: in LDS %s, %d threads, %d bytes" % (lds_side, in_lds, threads, got))
    assert in_lds and got == nbytes and got <= CAP and threads == 1024
    N = lds_side[0]
    transform = (2 if N & (N - 1) == 0 else 3) * N * 8
    in_lds, threads2, got = _capi.rtisi_la_bwd_placement(*scratch_side)
    print("backward placement %s: in LDS %s, %d threads, %d bytes" % (scratch_side, in_lds, threads2, got))
    assert not in_lds and got == transform and threads2 == threads
    assert layout(*lds_side) == (True, 1024, nbytes) and layout(*scratch_side) == (False, 1024, transform)


def test_boundary_arithmetic():
    assert 3 * 3000 * 8 + 12 * (3000 + 3 * 1500) == 162000 == CAP - 1840
    assert 3 * 3000 * 8 + 12 * (3000 + 4 * 1500) == 180000 > CAP
    assert 2 * 4096 * 8 + 12 * (4096 + 4 * 1024) == CAP
    assert 2 * 4096 * 8 + 12 * (4096 + 5 * 1024) == 176128 > CAP


def test_the_gpu_tables_claim_what_the_layout_gives():
    """Every row of rtisi_grad_cases.PLACEMENTS claims the placement of the restated layout at 1024 threads, both placements are there
    with two transform buffers and with three; the scratch rows of tests/window_cases.py are in scratch and its other rows in LDS."""
    reached = set()
    for key, steps in rc.PLACEMENTS.items():
        for LA, n, in_lds in steps:
            want = layout(key[0], key[1], min(LA, key[3] - 1))
            assert want[:2] == (in_lds, 1024), (key, LA, want)
            assert _capi.rtisi_la_bwd_placement(key[0], key[1], min(LA, key[3] - 1)) == want
            reached.add((key[0] & (key[0] - 1) == 0, in_lds))
    assert reached == {(pow2, lds) for pow2 in (False, True) for lds in (False, True)}
    for key, LA, n in wc.SCRATCH_RTISI_GRAD:
        want = layout(key[0], key[1], min(LA, key[3] - 1))
        assert want[:2] == (False, 1024) and _capi.rtisi_la_bwd_placement(key[0], key[1], min(LA, key[3] - 1)) == want
    assert {key[0] & (key[0] - 1) == 0 for key, LA, n in wc.SCRATCH_RTISI_GRAD} == {False, True}
    for key in wc.SHAPES:
        for LA, n in wc.LA_STEPS:
            want = layout(key[0], key[1], min(LA, key[3] - 1))
            assert want[0] and _capi.rtisi_la_bwd_placement(key[0], key[1], min(LA, key[3] - 1)) == want


def test_backward_state_never_exceeds_the_forward_state():
    """3 (N + LA hop) <= N + LA hop + 2 (LA + 1) N, since hop <= N: wherever the forward kernel's state fits LDS the backward's does,
    and the scratch the forward call sized serves the backward call."""
    for N, hop, LA in GRID3:
        bwd, fwd = 3 * (N + LA * hop), N + LA * hop + 2 * (LA + 1) * N
        assert bwd <= fwd, (N, hop, LA)
        if forward_layout(N, hop, LA)[0]:
            assert layout(N, hop, LA)[0] and _capi.rtisi_la_bwd_placement(N, hop, LA)[0], (N, hop, LA)
            assert _capi.rtisi_la_bwd_placement(N, hop, LA)[2] <= _capi.rtisi_la_placement(N, hop, LA, 0)[2]


def test_thread_rule():
    for N, want in ((32, 256), (256, 256), (258, 512), (320, 512), (512, 512), (514, 768), (600, 768), (768, 768), (770, 1024),
                    (1000, 1024), (1024, 1024), (1536, 1024), (2048, 1024), (3000, 1024), (4096, 1024)):
        assert _capi.rtisi_la_bwd_placement(N, N // 2, 3)[1] == want


def test_outputs_are_optional_and_bad_arguments_are_invalid():
    lib = _capi.load()
    assert lib.lws_rtisi_la_bwd_placement(64, 16, 3, None, None, None) == _capi.LWS_OK
    th = ctypes.c_int(-1)
    assert lib.lws_rtisi_la_bwd_placement(600, 150, 3, None, ctypes.byref(th), None) == _capi.LWS_OK and th.value == 768
    for bad in ((0, 16, 3), (64, 0, 3), (64, 16, -1)):
        with pytest.raises(ValueError):
            _capi.rtisi_la_bwd_placement(*bad)
