"""CPU: tests/residual_model.py (the fp64 restatement of the consistency-residual proxy) pinned to the oracle and to the truth.

(a) The accumulator, bin by bin, against the oracle's sweep (itself pinned to the reference): with target magnitude 1 at one bin and 0
    everywhere else, a sweep at threshold 0.5 updates only that bin, to acc / |acc|, while every neighbour it reads is untouched.
    This pins every row of the tap table -- the DC / Nyquist mirrors and the replicated edge frames included -- at 1e-13.
(b) What the proxy means (SURVEY probe 13): on interior frames (2Q frames left out at each end) 10 log10(sum|S|^2 / sum|res|^2)
    agrees with the true sum |stft(istft(S)) - S|^2 to 0.3 dB, for a zero-phase spectrogram and for an LWS output; for a consistent
    STFT the truth is ~300 dB but the proxy stops at the floor its L-bin truncation leaves (~40 dB at L = 5) -- it is not
    get_consistency.  Over the whole spectrogram the edge frames (which enter with extspec's replicated neighbours) move the proxy away
    from get_consistency by up to ~2.4 dB at Q = 2 (lws(512,256): 26.7 vs 24.3 dB on the LWS output; 0.2-0.4 dB at Q >= 3):
    recorded here, not asserted.  Measured interior margins: 0.00-0.01 dB (zero phase), 0.04-0.21 dB (LWS output); consistent-STFT
    proxy 38.6-40.3 dB.
"""
import numpy as np
import pytest

import lws_amd
from residual_model import residual_pairs, residual_terms

# (constructor arguments, frame counts): T = 1 and T < Q - 1 are the cases where extspec replicates frames into the stencil
PIN_CASES = [
    ((64, 16), {}, (1, 2, 7)),                               # Q = 4
    ((64, 8), {}, (1, 3, 9)),                                # Q = 8
    ((64, 32), {}, (1, 5)),                                  # Q = 2
    ((48, 16), {}, (1, 6)),                                  # Q = 3
    ((40, 16), {}, (1, 6)),                                  # fractional Q: general weights, Qp = 40
    ((64, 16), {"use_simplifications": False}, (4,)),        # general weights at an integer Q: Qp = 64 > F
    ((64, 16), {"L": 1}, (5,)),
    ((16, 4), {"L": 7}, (2, 6)),                             # L = F - 2
]


def _rand(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("args,kw,Ts", PIN_CASES,
                         ids=["64_16", "64_8", "64_32", "48_16", "40_16", "64_16_general", "64_16_L1", "16_4_L7"])
def test_accumulator_matches_oracle_sweep(oracle, args, kw, Ts):
    p = lws_amd.lws(*args, **kw)
    W = p.W
    Qp, Q, L1 = W.shape
    L = L1 - 1
    F = p.fsize // 2 + 1
    rng = np.random.default_rng(sum(args) + 7 * L)
    worst = 0.0
    for T in Ts:
        S = _rand(rng, (T, F))
        acc, res = residual_terms(S, W)
        assert np.array_equal(res, acc + W[np.arange(F) % Qp, 0, 0] * S)
        er0, ei0 = oracle.extend(S, L, Q)
        for m in range(T):
            for n in range(F):
                er, ei = er0.copy(), ei0.copy()
                amp = np.zeros_like(er)
                amp[m + Q - 1, n + L] = 1.0
                oracle.sweep(er, ei, W, amp, F, T, L, Q, 0.5)
                out = er[m + Q - 1, n + L] + 1j * ei[m + Q - 1, n + L]
                a = acc[m, n]
                assert abs(a) > 1e-6
                worst = max(worst, abs(out - a / abs(a)))
    assert worst < 1e-13, worst


@pytest.mark.parametrize("T", [1, 2, 9])
def test_q1_is_exactly_zero(T):
    """Q = 1 (frame == shift): every weight, w00 included, is zero, so the proxy is exactly 0 (not NaN)."""
    p = lws_amd.lws(16, 16)
    assert p.W.shape[1] == 1
    S = _rand(np.random.default_rng(T), (T, 9))
    acc, res = residual_terms(S, p.W)
    assert not acc.any() and not res.any()
    pair = residual_pairs(S, p.W)
    assert pair[0, 0] == 0.0 and pair[0, 1] > 0


def test_pairs_of_a_stack():
    p = lws_amd.lws(64, 16)
    S = _rand(np.random.default_rng(3), (3, 5, 33))
    pairs = residual_pairs(S, p.W)
    for b in range(3):
        _, res = residual_terms(S[b], p.W)
        assert np.allclose(pairs[b], [np.sum(np.abs(res) ** 2), np.sum(np.abs(S[b]) ** 2)], rtol=1e-14, atol=0)
    assert np.array_equal(residual_pairs(S[1], p.W), pairs[1:2])


# ---- (b) probe 13: the proxy against the true inconsistency ----------------------------------------------------------------------
PROBE_SHAPES = [(512, 128), (512, 64), (512, 256), (400, 160), (1024, 256)]


def _interior_db(p, S):
    """(proxy dB, true dB) over the frames 2Q .. T-2Q-1."""
    Q = p.W.shape[1]
    _, res = residual_terms(S, p.W)
    diff = p.stft(p.istft(S)) - S
    assert diff.shape == S.shape
    sl = slice(2 * Q, S.shape[0] - 2 * Q)
    pw = np.sum(np.abs(S[sl]) ** 2)
    return 10 * np.log10(pw / np.sum(np.abs(res[sl]) ** 2)), 10 * np.log10(pw / np.sum(np.abs(diff[sl]) ** 2))


@pytest.mark.parametrize("shape", PROBE_SHAPES, ids=lambda s: "%d_%d" % s)
def test_proxy_tracks_true_inconsistency(oracle, shape):
    fsize, fshift = shape
    p = lws_amd.lws(fsize, fshift)
    x = np.random.default_rng(fsize + fshift).standard_normal(200 * fshift)
    X = p.stft(x)
    M = np.abs(X)
    lws_out = oracle.batch_lws(M, p.W, lws_amd.get_thresholds(100, 2.0, 0.1, 1))
    for S in (M.astype(np.complex128), lws_out):
        proxy, true = _interior_db(p, S)
        assert abs(proxy - true) < 0.3, (proxy, true)
    # a consistent STFT: the truth is at the rounding floor, the proxy at its truncation floor (~40 dB at L = 5)
    proxy, true = _interior_db(p, X)
    assert true > 200, true
    assert 35 <= proxy <= 45, proxy
