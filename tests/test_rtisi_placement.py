"""CPU: lws_rtisi_la_placement -- where k_rtisi, k_rtisi_stream (K = 0) and k_misi_la (K sources) keep their state and with how many
threads they run -- against a restatement in Python of the layout DESIGN section 7c-e describes, over a grid of (N, hop, LA, K), and
at the rows on either side of the LDS boundary that the GPU tests run.  The query calls the functions the launch sites call; the GPU
tests assert through it the placement their comments claim."""
import ctypes

import pytest

import misi_la_cases as mc
from lws_amd import _capi

CAP = 160 * 1024      # the LDS of a CU: transform buffers and state together may take all of it


def layout(N, hop, LA, K=0):
    """(in_lds, threads, dynamic LDS bytes), restated: a ring of N + LA hop floats and two buffers of LA + 1 windowed frames per
    source; with K >= 1 sources K such states, the gated mixture and K rows of coupled signals, a ring's length each; in front, two
    N-point complex buffers and, where N is not a power of two, a third for the twiddle table."""
    ring = N + LA * hop
    source = ring + 2 * (LA + 1) * N
    floats = source if K == 0 else K * source + (K + 1) * ring
    transform = (2 if N & (N - 1) == 0 else 3) * N * 8
    total = transform + 4 * floats
    threads = 256 if N <= 256 else 1024 if N >= 1024 else -(-N // 256) * 256
    return total <= CAP, threads, total if total <= CAP else transform


GRID = [(N, hop, LA, K)
        for N in (32, 48, 64, 256, 258, 320, 512, 514, 600, 768, 770, 1000, 1024, 1536, 2048, 3000, 4096)
        for hop in sorted({1, N // 16, N // 4, N // 3, N // 2, N // 2 + 1, N})
        for LA in (0, 1, 3, 5, 6, 17, 60, 200)
        for K in (0, 1, 2, 3, 4, 6, 7)]


def test_query_is_the_layout_over_a_grid():
    both = set()
    for N, hop, LA, K in GRID:
        got, want = _capi.rtisi_la_placement(N, hop, LA, K), layout(N, hop, LA, K)
        assert got == want, ((N, hop, LA, K), got, want)
        both.add((K > 0, want[0], want[1]))
    # the grid reaches both placements of both kernels at every thread count
    assert both == {(k, lds, th) for k in (False, True) for lds in (False, True) for th in (256, 512, 768, 1024)}


# (N, hop, LA, K): bytes on the LDS side, then the neighbour on the scratch side
BOUNDARY = [
    ((2048, 512, 5, 0), 149504, (2048, 512, 6, 0)),
    ((2048, 1228, 5, 0), 163824, (2048, 1229, 5, 0)),      # 16 bytes under the cap; 4 over it
    ((1024, 256, 3, 2), None, (1024, 256, 3, 3)),
    ((512, 128, 5, 4), 147968, (512, 128, 6, 4)),
    ((512, 128, 3, 6), 153088, (512, 128, 3, 7)),          # the README: lws(512,128) at LA = 3 stays in LDS up to K = 6
    ((4096, 1024, 1, 0), 151552, (4096, 1024, 2, 0)),      # a stream created at LA = 3 (scratch) that ends after two frames or one
]


@pytest.mark.parametrize("lds_side,nbytes,scratch_side", BOUNDARY)
def test_boundary_rows(lds_side, nbytes, scratch_side):
    in_lds, threads, got = _capi.rtisi_la_placement(*lds_side)
    print("placement %s: in LDS %s, %d threads, %d bytes" % (lds_side, in_lds, threads, got))
    assert in_lds and got <= CAP and (nbytes is None or got == nbytes)
    N = lds_side[0]
    transform = (2 if N & (N - 1) == 0 else 3) * N * 8
    in_lds, threads2, got = _capi.rtisi_la_placement(*scratch_side)
    print("placement %s: in LDS %s, %d threads, %d bytes" % (scratch_side, in_lds, threads2, got))
    assert not in_lds and got == transform and threads2 == threads
    assert layout(*scratch_side)[0] is False and layout(*lds_side)[2] == (nbytes or layout(*lds_side)[2])


def test_the_misi_edge_table_claims_what_the_layout_gives_and_reaches_the_cap():
    """Every row of the second table of tests/test_gpu_misi_la.py claims the placement and workgroup of the restated layout, both
    placements are there, and one LDS row is within 1 KB of the cap: lws(2048,512), K = 1, LA = 4 asks for the LDS of a CU to the byte."""
    nearest, placements = CAP, set()
    for key, (threads, steps) in mc.EDGE_SHAPES.items():
        for LA, n, in_lds in steps:
            want = layout(key[0], key[1], min(LA, key[3] - 1), key[4])
            assert want[:2] == (in_lds, threads), (key, LA, want)
            placements.add(in_lds)
            if in_lds:
                nearest = min(nearest, CAP - want[2])
    assert placements == {True, False} and nearest == 0
    assert _capi.rtisi_la_placement(2048, 512, 4, 1) == (True, 1024, CAP)


def test_over_the_cap_by_four_bytes():
    N, hop, LA = 2048, 1229, 5
    assert 2 * N * 8 + 4 * (N + LA * hop + 2 * (LA + 1) * N) == CAP + 4


def test_thread_rule():
    for N, want in ((32, 256), (256, 256), (258, 512), (320, 512), (512, 512), (514, 768), (600, 768), (768, 768), (770, 1024),
                    (1000, 1024), (1024, 1024), (1536, 1024), (2048, 1024), (4096, 1024)):
        assert _capi.rtisi_la_placement(N, N // 2, 3)[1] == want
        assert _capi.rtisi_la_placement(N, N // 2, 3, 2)[1] == want


def test_outputs_are_optional_and_bad_arguments_are_invalid():
    lib = _capi.load()
    assert lib.lws_rtisi_la_placement(64, 16, 3, 0, None, None, None) == _capi.LWS_OK
    th = ctypes.c_int(-1)
    assert lib.lws_rtisi_la_placement(600, 150, 3, 2, None, ctypes.byref(th), None) == _capi.LWS_OK and th.value == 768
    for bad in ((0, 16, 3, 0), (64, 0, 3, 0), (64, 16, -1, 0), (64, 16, 3, -1)):
        with pytest.raises(ValueError):
            _capi.rtisi_la_placement(*bad)
