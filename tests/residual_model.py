"""The consistency-residual proxy (lws_residual_dev and its siblings, include/lws_hip.h) restated on the CPU in fp64 --

  * E = extspec(S, L, Q): L Hermitian columns each side, Q-1 copies of the first / last frame each end (lws.pyx:146-157);
  * row = n % Qp, rowneg = (Qp - row) % Qp; a weight with |w| <= 1e-12 counts as zero (the flags of lws.pyx:227-232);
  * acc[m, n] is the LWS weighted sum of bin (m, n) without its centre tap, one tap per (frame offset, bin offset):

        (0, -k)  W[row,0,k]          (0, +k)  conj(W[row,0,k])          k = 1..L
        (-r, 0)  W[row,r,0]          (+r, 0)  conj(W[row,r,0])          r = 1..Q-1
        (-r, -k) W[row,r,k]          (+r, -k) conj(W[row,r,k])
        (+r, +k) W[rowneg,r,k]       (-r, +k) conj(W[rowneg,r,k])

  * res = acc + W[row,0,0] S (create_weights already subtracted 1 from W[.,0,0], lws.pyx:177), so res is the truncated
    F(S) - S, and the pair of one spectrogram is [sum |res|^2, sum |S|^2].

Test infrastructure: tests/test_residual_model.py pins the tap table to the oracle's sweep bin by bin; tests/test_gpu_residual.py
compares the device with it.  Each tap term is a slice of E -- no loop over bins."""
import numpy as np

from lws_amd import extspec


def residual_terms(S, W):
    """One spectrogram S (T, F) and weights W (Qp, Q, L+1).  Returns (acc, res), complex128 (T, F)."""
    S = np.asarray(S).astype(np.complex128)
    W = np.asarray(W, dtype=np.complex128)
    W = np.where(np.abs(W) > 1.0e-12, W, 0)
    Qp, Q, L1 = W.shape
    L = L1 - 1
    T, F = S.shape
    E = extspec(S, L, Q)
    row = np.arange(F) % Qp
    Wa, Wb = W[row], W[(Qp - row) % Qp]          # (F, Q, L+1): the weights of each bin's row and of its mirror row
    cj = np.conjugate

    def at(dr, dk):                               # the neighbour (dr frames, dk bins) away of every bin
        return E[Q - 1 + dr:Q - 1 + dr + T, L + dk:L + dk + F]

    acc = np.zeros((T, F), dtype=np.complex128)
    for k in range(1, L + 1):
        acc += Wa[:, 0, k] * at(0, -k) + cj(Wa[:, 0, k]) * at(0, k)
    for r in range(1, Q):
        acc += Wa[:, r, 0] * at(-r, 0) + cj(Wa[:, r, 0]) * at(r, 0)
        for k in range(1, L + 1):
            acc += Wa[:, r, k] * at(-r, -k) + cj(Wa[:, r, k]) * at(r, -k)
            acc += Wb[:, r, k] * at(r, k) + cj(Wb[:, r, k]) * at(-r, k)
    return acc, acc + Wa[:, 0, 0] * S


def residual_pairs(S, W):
    """S (T, F) or (B, T, F).  Returns (B, 2) float64: [sum |res|^2, sum |S|^2] of each spectrogram."""
    S = np.asarray(S)
    S3 = S[None] if S.ndim == 2 else S
    out = np.empty((S3.shape[0], 2))
    for b, Sb in enumerate(S3):
        _, res = residual_terms(Sb, W)
        Sb = Sb.astype(np.complex128)
        out[b] = [np.sum(res.real ** 2 + res.imag ** 2), np.sum(Sb.real ** 2 + Sb.imag ** 2)]
    return out


def db(pair):
    """The proxy's consistency in dB, 10 log10(sum |S|^2 / sum |res|^2), of one pair or of each row of a (B, 2) array."""
    pair = np.asarray(pair, dtype=np.float64)
    return 10 * np.log10(pair[..., 1] / pair[..., 0])
