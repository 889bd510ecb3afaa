"""The device transform (fft_lds, lws_amd/csrc/lws_fft.h) restated on the CPU with every intermediate rounded to one number format:
what the factorisation N = m 2^a costs in accuracy, separated from what a particular kernel makes of it.

  * the gather y[r n2 + j] = x[m j + r] puts the m interleaved subsequences of n2 = 2^a points side by side;
  * `a` radix-2 Stockham stages (decimation in frequency, auto-sort) transform all m blocks, stage twiddle
    exp(j pi sign 2 p / ncur) on the difference of the butterfly;
  * one stage of m-point DFTs combines them, X[o] = sum_r tw[(r o) mod n] Y_r[o mod n2], tw[i] = exp(sign 2 pi j i / n), the m
    terms accumulated in ascending r.

Twiddles are the correctly rounded values (computed in fp64 from an exactly reduced angle); each product, sum and difference is
rounded to `dtype` (no fused multiply-add).  It is the arithmetic that is restated, on whole arrays, not the kernel's loops: with
dtype = float64 it must equal np.fft (tests/test_fft_model.py), with float32 it is the error model that tests/
test_gpu_transform_edges.py holds the kernels to.  stft_model / istft_model put the window product, the Hermitian completion and
the overlap-add of lws_stft.hip around it, in the same format."""
import functools

import numpy as np

import lws_amd
from lws_amd.lws import _perfectrec_prepad


def factor(n):
    """n = m 2^a with m odd: (m, a)."""
    m, a = int(n), 0
    while m % 2 == 0:
        m //= 2
        a += 1
    return m, a


def _unit(num, den, sign, rt):
    """exp(sign 2 pi j num / den) for integer arrays num, correctly rounded to rt: (cos, sin).  The angle is reduced exactly, in
    integers, before anything is rounded."""
    frac = (np.asarray(num, dtype=np.int64) % den) / float(den)            # in [0, 1): exact numerator, one fp64 division
    return np.cos(2 * np.pi * frac).astype(rt), (sign * np.sin(2 * np.pi * frac)).astype(rt)


def fft_model(x, sign, dtype=np.float32):
    """Unnormalised DFT along the last axis of x (n = m 2^a points, n even), sign = -1 forward / +1 inverse, every intermediate
    rounded to the real format `dtype`.  Returns (re, im) as one complex array of the matching complex type."""
    rt = np.dtype(dtype)
    x = np.asarray(x)
    n = x.shape[-1]
    m, a = factor(n)
    n2 = n // m
    lead = x.shape[:-1]
    xr, xi = np.real(x).astype(rt), np.imag(x).astype(rt)
    # gather: block r holds x[m j + r], j = 0..n2-1
    yr = np.ascontiguousarray(np.swapaxes(xr.reshape(lead + (n2, m)), -1, -2))      # (..., m, n2)
    yi = np.ascontiguousarray(np.swapaxes(xi.reshape(lead + (n2, m)), -1, -2))
    # Stockham: the block as (ncur, s), element (p, q) at q + s p; butterflies pair p with p + h and write rows 2p, 2p + 1
    ncur, s = n2, 1
    for _ in range(a):
        h = ncur // 2
        vr, vi = yr.reshape(lead + (m, ncur, s)), yi.reshape(lead + (m, ncur, s))
        ur, ui, wr, wi = vr[..., :h, :], vi[..., :h, :], vr[..., h:, :], vi[..., h:, :]
        cs, sn = _unit(np.arange(h), ncur, sign, rt)
        cs, sn = cs[:, None], sn[:, None]
        dr, di = ur - wr, ui - wi
        outr = np.stack([ur + wr, dr * cs - di * sn], axis=-2)                      # (..., m, h, 2, s)
        outi = np.stack([ui + wi, dr * sn + di * cs], axis=-2)
        yr, yi = outr.reshape(lead + (m, n2)), outi.reshape(lead + (m, n2))
        ncur, s = h, 2 * s
    if m == 1:
        return (yr[..., 0, :] + 1j * yi[..., 0, :]).astype(np.result_type(rt, np.complex64))
    # the odd stage, ascending r
    tr, ti = _unit(np.arange(n), n, sign, rt)
    o = np.ascontiguousarray(np.arange(n, dtype=np.int64).reshape(m, n2).T)         # output o = q n2 + k held at (k, q): o mod n2 = k
    idx = np.zeros((n2, m), dtype=np.int64)                                         # (r o) mod n
    ar, ai = np.zeros(lead + (n2, m), rt), np.zeros(lead + (n2, m), rt)
    t1, t2 = np.empty_like(ar), np.empty_like(ar)
    for r in range(m):
        cs, sn = tr[idx], ti[idx]
        vr, vi = yr[..., r, :, None], yi[..., r, :, None]                           # Y_r[k], the same for every q
        np.multiply(vr, cs, out=t1); np.multiply(vi, sn, out=t2); t1 -= t2; ar += t1
        np.multiply(vr, sn, out=t1); np.multiply(vi, cs, out=t2); t1 += t2; ai += t1
        idx += o
        idx[idx >= n] -= n
    ar, ai = np.swapaxes(ar, -1, -2).reshape(lead + (n,)), np.swapaxes(ai, -1, -2).reshape(lead + (n,))
    return (ar + 1j * ai).astype(np.result_type(rt, np.complex64))


def stft_model(x, fsize, fshift, awin, fftsize=None, perfectrec=False, dtype=np.float32):
    """lws_amd.stft -- of one signal (len,) or of a stack (B, len) -- with the arithmetic of k_stft_frames in `dtype`: the samples
    and the window rounded, their product rounded, fft_model, bins 0..fftsize/2."""
    rt = np.dtype(dtype)
    fftsize = fsize if fftsize is None else fftsize
    x = np.asarray(x, dtype=np.float64).astype(rt)
    if x.ndim == 1:
        return stft_model(x[None], fsize, fshift, awin, fftsize, perfectrec, dtype)[0]
    B, n = x.shape
    if perfectrec:
        x = np.concatenate([np.zeros((B, _perfectrec_prepad(fsize, fshift)), rt), x, np.zeros((B, (-n) % fshift), rt)], axis=1)
        M = x.shape[1] // fshift
    else:
        x = np.concatenate([x, np.zeros((B, (-(n - fsize)) % fshift), rt)], axis=1)
        M = max((x.shape[1] - fsize) // fshift + 1, 0)
    need = (M - 1) * fshift + fsize
    if need > x.shape[1]:
        x = np.concatenate([x, np.zeros((B, need - x.shape[1]), rt)], axis=1)
    if M == 0:
        return np.zeros((B, 0, fftsize // 2 + 1), np.result_type(rt, np.complex64))
    idx = fshift * np.arange(M)[:, None] + np.arange(fsize)[None, :]
    frames = np.zeros((B, M, fftsize), rt)
    frames[:, :, :fsize] = x[:, idx] * np.asarray(awin, dtype=np.float64).astype(rt)[None, None, :]
    return fft_model(frames, -1, rt)[..., :fftsize // 2 + 1]


def istft_model(spec, fshift, swin, perfectrec=False, dtype=np.float32):
    """lws_amd.istft -- of one spectrogram (M, F) or of a stack (B, M, F) -- with the arithmetic of k_istft_frames / k_overlap_add
    in `dtype`: Hermitian completion, fft_model, real part times 1/N times the window, frames added in ascending order."""
    rt = np.dtype(dtype)
    spec = np.asarray(spec).astype(np.result_type(rt, np.complex64))
    if spec.ndim == 2:
        return istft_model(spec[None], fshift, swin, perfectrec, dtype)[0]
    B, M, F = spec.shape
    N = 2 * (F - 1)
    full = np.concatenate([spec, np.conjugate(spec[:, :, -2:0:-1])], axis=2)
    frames = (np.real(fft_model(full, +1, rt)) * rt.type(1.0 / N)).astype(rt) * np.asarray(swin, dtype=np.float64).astype(rt)[None, None, :]
    signal = np.zeros((B, fshift * (M - 1) + N), rt)
    for s in range(M):
        signal[:, fshift * s: fshift * s + N] += frames[:, s]
    if perfectrec:
        signal = signal[:, _perfectrec_prepad(N, fshift):(fshift - N)]
    return signal


def max_rel(a, b):
    """The suite's metric: max |a - b| / max |b|."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def model_error(n, dtype=np.float32, frames=4):
    """max error / max value of fft_model in `dtype` against fp64 np.fft.fft on seeded unit Gaussian input (real and imaginary
    parts), the worse of the two signs."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((frames, n)) + 1j * rng.standard_normal((frames, n))
    fwd = max_rel(fft_model(x, -1, dtype), np.fft.fft(x, axis=1))
    inv = max_rel(fft_model(x, +1, dtype), n * np.fft.ifft(x, axis=1))
    return max(fwd, inv)


def windows(fsize, fshift):
    """sqrt(hann) and its synthesis partner: the window pair of the transform tests."""
    awin = np.sqrt(lws_amd.hann(fsize, symmetric=True, use_offset=False))
    return awin, lws_amd.synthwin(awin, fshift)
