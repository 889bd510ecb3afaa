"""Inputs and host references of the streaming online-MISI tests (lws_amd.misi_la(..., open_end=True) / MisiLaStream), shared by
tests/test_misi_la_stream_host.py and tests/test_gpu_misi_la_stream.py so that each fp64 reference is computed once.

Starts, levels, mixtures and the error model are those of tests/misi_la_cases.py.  An open end takes every sample under the pushed
frames: with perfectrec the mixture is extended by the fsize - fshift zeros stft pads behind the signal."""
import functools

import numpy as np

import lws_amd
from lws_amd.lws import _perfectrec_prepad
from misi_la_cases import SCALES, SOURCES, case, magnitudes_of, perturbation, rel  # noqa: F401  (re-exported to the tests)

STEPS = [(0, 2), (1, 3), (3, 3), (5, 2)]   # (look_ahead, iterations)
# (fsize, fshift, perfectrec, T, K)
HOST_KEYS = [(64, 16, True, 12, 3), (48, 16, False, 7, 2), (256, 96, True, 9, 2), (128, 32, True, 20, 3)]
GPU_KEYS = [(64, 16, True, 12, 3), (48, 16, False, 7, 2), (256, 96, True, 9, 2), (512, 128, False, 40, 2),
            (4096, 1024, False, 6, 2)]   # the last: the state does not fit in LDS
# key: (threads, [(look_ahead, iterations, state in LDS)]): what lws_rtisi_la_placement must say, and the steps run there
PLACEMENTS = {
    (512, 128, False, 8, 4): (512, [(5, 2, True), (6, 2, False)]),   # LA = 5 in LDS, LA = 6 in scratch
    (1024, 256, False, 6, 2): (1024, [(3, 2, True)]),
    (2048, 512, False, 6, 1): (1024, [(4, 2, True)]),                # the 160 KB asked for to the byte
    (600, 150, True, 7, 2): (768, [(2, 3, True)]),                   # a workgroup of 768 threads
    (64, 8, True, 20, 2): (256, [(9, 2, True)]),                     # more active frames than overlap
}
# (key, look_ahead, iterations, rows): streams that end before their first commit, after `rows` <= look_ahead frames of the case ...
SHORT = [((64, 16, True, 12, 3), 3, 3, 1), ((64, 16, True, 12, 3), 3, 3, 3), ((48, 16, False, 7, 2), 5, 3, 1), ((48, 16, False, 7, 2), 5, 3, 5)]
# ... and one created in scratch that does so after one and after two frames: it closes with the clamped plan
EARLY_END = [((4096, 1024, False, 6, 2), 3, 3, 1), ((4096, 1024, False, 6, 2), 3, 3, 2)]


def key_id(k):
    return "%d-%d-%s-T%d-K%d" % tuple(k[:5])


def gpu_runs():
    """Every (key, look_ahead, iterations, rows) the GPU file compares with the host; rows None: the whole case."""
    runs = [(k, LA, n, None) for k in GPU_KEYS for LA, n in STEPS]
    runs += [(k, LA, n, None) for k, (_, steps) in PLACEMENTS.items() for LA, n, _ in steps]
    return runs + SHORT + EARLY_END


def lead_in(key):
    return _perfectrec_prepad(key[0], key[1]) if key[2] else 0


def need(key, M):
    """Mixture samples under the first M frames."""
    return 0 if M <= 0 else key[1] * (M - 1) + key[0] - lead_in(key)


@functools.lru_cache(maxsize=None)
def open_case(*key):
    """case(*key) with the mixture at the open-end length: p, A, c0, y (B, need(T)) float32."""
    p, A, c0, y = case(*key)
    yo = np.zeros((y.shape[0], need(key, key[3])), dtype=np.float32)
    assert y.shape[1] <= yo.shape[1] and yo.shape[1] - y.shape[1] == (key[0] - key[1] if key[2] else 0)
    yo[:, :y.shape[1]] = y
    yo.setflags(write=False)
    return p, A, c0, yo


@functools.lru_cache(maxsize=None)
def host_open(key, LA, n, explicit=False, rows=None):
    """(c, signals) of misi_la(..., open_end=True) on the first `rows` frames (all) and the mixture under them."""
    p, A, c0, y = open_case(*key)
    T1 = key[3] if rows is None else rows
    mag = magnitudes_of(A)[:, :, :T1] if explicit else None
    return lws_amd.misi_la(c0[:, :, :T1], y[:, :need(key, T1)], p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=mag,
                           perfectrec=p.perfectrec, return_signals=True, open_end=True)


@functools.lru_cache(maxsize=None)
def host_open_perturbed(key, LA, n, explicit=False, rows=None):
    """host_open() under the error model."""
    p, A, c0, y = open_case(*key)
    T1 = key[3] if rows is None else rows
    mag = magnitudes_of(A)[:, :, :T1] if explicit else None
    return lws_amd.misi_la(c0[:, :, :T1], y[:, :need(key, T1)], p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, magnitudes=mag,
                           perfectrec=p.perfectrec, return_signals=True, open_end=True, _perturb=perturbation(n + 17))


@functools.lru_cache(maxsize=None)
def host_closed(key, LA, n):
    """(c, signals) of misi_la without open_end on the mixture cut to its length."""
    p, A, c0, y = case(*key)
    return lws_amd.misi_la(c0, y, p.fsize, p.fshift, p.awin, p.swin, n, look_ahead=LA, perfectrec=p.perfectrec, return_signals=True)


def coincide(key, LA):
    """P: the frames whose steps reach no sample where the closed and the open form differ, and the samples they finalise."""
    N, hop, _, T, _ = key
    P = sum(1 for m in range(T) if hop * min(m + LA, T - 1) + N <= hop * T)
    return P, max(hop * P - lead_in(key), 0)
