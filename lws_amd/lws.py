"""Python surface of the reference's ``lws`` module (python/lws.pyx, v1.2.8) on the MI355X engine.

Same names, arguments, defaults, return dtypes and error behaviour as the reference; the three LWS
entry points ``batch_lws`` / ``nofuture_lws`` / ``online_lws`` (lws.pyx:209-375) and the methods of
``class lws`` call the HIP engine through the C ABI (include/lws_hip.h) instead of the CPU kernels of
lwslib.cpp.  Everything else in this file is host-side setup (windows, weights, STFT for evaluation):
one-off numpy work that feeds the kernels, restated here so the package is self-contained.

Extensions that do not change 2-D behaviour: the LWS entry points also accept a ``(B, T, F)`` stack of
independent spectrograms, and ``class lws`` takes ``device=`` / ``precision=`` / ``nofuture_q4_compat=``.
"""
from __future__ import annotations

import collections
import hashlib
import threading
import math

import numpy as np

from . import _capi

__version__ = "1.2.8"  # version of the interface mirrored


# --------------------------------------------------------------------------------------------
# windows (lws.pyx:10-40)
# --------------------------------------------------------------------------------------------
def hann(n, symmetric=True, use_offset=False):
    """Hann window of length n (lws.pyx:10-19)."""
    if symmetric:
        phase = (2.0 * np.arange(n) + 1.0) / (2.0 * n)  # sample points at the half-integers
    else:
        phase = (np.arange(n) + (1 if use_offset else 0)) / float(n)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * phase))


def synthwin(awin, fshift, swin=None):
    """Synthesis window normalised for perfect reconstruction (lws.pyx:22-40)."""
    fsize = len(awin)
    Q = int(math.ceil(float(fsize) / float(fshift)))
    if swin is None:
        swin = awin
    prod = np.zeros(Q * fshift)
    prod[:fsize] = np.asarray(awin) * np.asarray(swin)
    overlap = prod.reshape(Q, fshift).sum(axis=0)  # sum of the shifted window products
    norm = np.tile(overlap, Q)[:fsize]
    if norm.min() <= 0:
        raise ValueError('The normalizer is not strictly positive')
    return swin / norm


# --------------------------------------------------------------------------------------------
# STFT / iSTFT / consistency (lws.pyx:43-144) -- evaluation helpers, host numpy
# --------------------------------------------------------------------------------------------
def _perfectrec_prepad(fsize, fshift):
    rem = fsize % fshift
    return fsize - fshift if rem == 0 else fsize - rem


def stft(x, fsize, fshift, awin, fftsize=None, perfectrec=False):
    """STFT with a fixed frame shift; returns (frames, fftsize//2+1) complex128 (lws.pyx:43-90)."""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError('We only deal with single channel signals here')
    if fftsize is None:
        fftsize = fsize
    if fftsize % 2 == 1:
        raise ValueError('Odd ffts not supported.')
    x = x.astype(np.float64, copy=False) if not np.iscomplexobj(x) else x
    if perfectrec is True:
        pre = _perfectrec_prepad(fsize, fshift)
        post = (-len(x)) % fshift
        x = np.concatenate([np.zeros(pre), x, np.zeros(post)])
        M = len(x) // fshift
    else:
        post = (-(len(x) - fsize)) % fshift
        x = np.concatenate([x, np.zeros(post)])
        M = (len(x) - fsize) // fshift + 1
    need = (M - 1) * fshift + fsize
    if need > len(x):
        x = np.concatenate([x, np.zeros(need - len(x))])
    idx = fshift * np.arange(M)[:, None] + np.arange(fsize)[None, :]
    frames = x[idx] * np.asarray(awin)[None, :]
    spec = np.fft.fft(frames, n=fftsize, axis=1)[:, : fftsize // 2 + 1]
    return spec.astype(np.complex128)


def istft(spec, fshift, swin, awin=None, fftsize=None, perfectrec=False):
    """Inverse STFT by weighted overlap-add (lws.pyx:93-137)."""
    spec = np.asarray(spec)
    if spec.ndim != 2:
        raise ValueError('We only deal with single channel signals here')
    M, N = spec.shape
    if N % 2 != 1:
        raise ValueError('We expect the spectrogram to only have non-negative frequencies')
    fsize = 2 * (N - 1)
    if awin is not None:
        swin = synthwin(awin, fshift, swin=swin)
    if fftsize is None:
        fftsize = fsize
    swin = np.asarray(swin, dtype=np.float64)
    if fftsize > len(swin):
        swin = np.concatenate([swin, np.zeros(fftsize - len(swin))])
    full = np.concatenate([spec, np.conjugate(spec[:, -2:0:-1])], axis=1)  # Hermitian completion
    # (as in the reference, lws.pyx:107-126: the frame is 2 (bins - 1) samples, so a window of any other length -- which is what
    # every fftsize > fsize makes of it, and an fftsize < fsize of the frame -- fails to broadcast: ValueError)
    frames = np.real(np.fft.ifft(full, n=fftsize, axis=1))[:, :fsize] * np.squeeze(swin)[None, :]
    if frames.shape[1] != fsize:
        raise ValueError('operands could not be broadcast together with shapes (%d,) (%d,)' % (fsize, frames.shape[1]))
    signal = np.zeros(fshift * (M - 1) + fsize)
    for s in range(M):
        signal[fshift * s: fshift * s + fsize] += frames[s]
    if perfectrec is True:
        signal = signal[_perfectrec_prepad(fsize, fshift):(fshift - fsize)]
    return signal


def get_consistency(S, fsize, fshift, awin, swin, perfectrec=False):
    """20 log10(|S| / |stft(istft(S)) - S|) in dB (lws.pyx:140-144)."""
    back = stft(istft(S, fshift, swin, perfectrec=perfectrec), fsize, fshift, awin, perfectrec=perfectrec)
    return 20 * np.log10(np.linalg.norm(S) / np.linalg.norm(back - S))


def _dev_tensor(a, dtype, device):
    import torch
    dev = torch.device("cuda", int(device))
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


def stft_dev(x, fsize, fshift, awin, fftsize=None, perfectrec=False, device=0):
    """stft() above on the device (lws_stft.hip, float32): x a signal (len,) or a stack (B, len), numpy or torch; returns a complex64
    torch tensor (T, fftsize//2+1) / (B, T, ...).  fftsize > fsize: the fsize windowed samples followed by zeros, as
    np.fft.fft(frame, n=fftsize) does (lws.pyx:49-50,85); any even fftsize in [32, 4096].  A signal too short for one frame gives an
    empty (0, F) / (B, 0, F) tensor, as stft() gives an empty array."""
    import torch
    if fftsize is None:
        fftsize = fsize
    if fftsize % 2 == 1:
        raise ValueError('Odd ffts not supported.')
    t = _dev_tensor(x, torch.float32, device)
    if t.dim() not in (1, 2):
        raise ValueError('We only deal with single channel signals here')
    single = t.dim() == 1
    if single:
        t = t[None]
    B, n = t.shape
    T = _capi.stft_frames(n, fsize, fshift, perfectrec)
    out = torch.empty((B, T, fftsize // 2 + 1), dtype=torch.complex64, device=t.device)
    _capi.stft_dev(t.data_ptr(), B, n, fsize, fshift, np.asarray(awin, dtype=np.float64), perfectrec, out.data_ptr(), device=int(device),
                   stream=torch.cuda.current_stream(t.device).cuda_stream, fftsize=fftsize)
    return out[0] if single else out


def istft_dev(spec, fshift, swin, awin=None, fftsize=None, perfectrec=False, device=0):
    """istft() above on the device: spec (T, F) or (B, T, F), numpy or torch; returns a float32 torch tensor (len,) / (B, len).
    As in the reference (lws.pyx:107-126) the frame is 2 (F - 1) samples and any other fftsize / window length is a ValueError.
    Frames of which perfectrec keeps no sample give an empty (0,) / (B, 0) tensor, as istft() gives an empty array."""
    import torch
    t = _dev_tensor(spec, torch.complex64, device)
    if t.dim() not in (2, 3):
        raise ValueError('We only deal with single channel signals here')
    single = t.dim() == 2
    if single:
        t = t[None]
    B, T, N = t.shape
    if N % 2 != 1:
        raise ValueError('We expect the spectrogram to only have non-negative frequencies')
    fsize = 2 * (N - 1)
    if awin is not None:
        swin = synthwin(awin, fshift, swin=swin)
    swin = np.squeeze(np.asarray(swin, dtype=np.float64))
    if (fftsize is not None and fftsize != fsize) or swin.shape != (fsize,):
        raise ValueError('operands could not be broadcast together with shapes (%d,) (%d,)' % (fsize, max(swin.size, fftsize or 0)))
    n = _capi.istft_length(T, fsize, fshift, perfectrec)
    out = torch.empty((B, n), dtype=torch.float32, device=t.device)
    _capi.istft_dev(t.data_ptr(), B, T, fsize, fshift, swin, perfectrec, out.data_ptr(), device=int(device),
                    stream=torch.cuda.current_stream(t.device).cuda_stream)
    return out[0] if single else out


# --------------------------------------------------------------------------------------------
# Griffin-Lim refinement (no counterpart in the reference): host fp64 definition, and the device form (lws_gla.hip)
# --------------------------------------------------------------------------------------------
def _gla_args(iterations, alpha):
    if int(iterations) != iterations or iterations < 0:
        raise ValueError('iterations must be a non-negative integer, got %r' % (iterations,))
    if not 0.0 <= float(alpha) < 1.0:
        raise ValueError('alpha must be in [0, 1), got %r' % (alpha,))
    return int(iterations), float(alpha)


def _project(X, A):
    """A X / |X|, and A + 0j where |X| == 0: the magnitude projection of every iteration below."""
    mag = np.abs(X)
    return np.where(mag > 0, A * X / np.where(mag > 0, mag, 1.0), A + 0j)


def griffin_lim(S, fsize, fshift, awin, swin, iterations, alpha=0.99, magnitudes=None, perfectrec=False, return_trace=False,
                _perturb=None):
    """(Fast) Griffin-Lim iterations from the start S, (T, F) or a stack (B, T, F), in fp64 on the host: the definition the
    device form is held to.  With P(c) = stft(istft(c)) -- the round trip get_consistency makes -- step i = 1..iterations is
    X = P(c), t_i = A X / |X| (A + 0j where |X| == 0), c = t_i for i = 1 and t_i + alpha (t_i - t_{i-1}) after that.  Returns
    t_n (its magnitudes are A = `magnitudes`, by default |S|); zero iterations return S.  alpha = 0 is plain Griffin-Lim.
    return_trace: also the consistency in dB, 10 log10(sum |c|^2 / sum |P(c) - c|^2), of the iterate entering each step,
    shape (iterations,) / (iterations, B).  (_perturb(i, b, X) -> X: replaces each projection; the error model of the tests.)"""
    n, alpha = _gla_args(iterations, alpha)
    S = np.asarray(S)
    if S.ndim not in (2, 3):
        raise ValueError('expected a (T, F) spectrogram or a (B, T, F) stack')
    A = np.abs(S) if magnitudes is None else np.asarray(magnitudes, dtype=np.float64)
    if A.shape != S.shape:
        raise ValueError('magnitudes of shape %s for a spectrogram of shape %s' % (A.shape, S.shape))
    if n == 0:
        return (S, np.zeros((0,) + S.shape[:-2])) if return_trace else S
    S3, A3 = (S[None], A[None]) if S.ndim == 2 else (S, A)
    out = np.empty(S3.shape, dtype=np.complex128)
    db = np.empty((n, S3.shape[0]))
    for b in range(S3.shape[0]):
        c, t_prev = S3[b].astype(np.complex128), None
        for i in range(1, n + 1):
            X = stft(istft(c, fshift, swin, perfectrec=perfectrec), fsize, fshift, awin, perfectrec=perfectrec)
            if X.shape != c.shape:
                raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (c.shape[0], X.shape[0]))
            if _perturb is not None:
                X = _perturb(i, b, X)
            db[i - 1, b] = 10 * np.log10(np.sum(np.abs(c) ** 2) / np.sum(np.abs(X - c) ** 2))
            t = _project(X, A3[b])
            c = t if i == 1 else t + alpha * (t - t_prev)
            t_prev = t
        out[b] = t_prev
    if S.ndim == 2:
        out, db = out[0], db[:, 0]
    return (out, db) if return_trace else out


def griffin_lim_dev(S, fsize, fshift, awin, swin, iterations, alpha=0.99, magnitudes=None, perfectrec=False, return_trace=False,
                    device=0):
    """griffin_lim() above on the device (lws_gla.hip: float32, the transforms fused with the magnitude projection, two launches
    per iteration): S (T, F) or (B, T, F), numpy or torch; returns a new complex64 torch tensor (S itself is not modified), and
    with return_trace also the dB values as a numpy array.  Runs on the caller's current torch stream; without return_trace
    the call only enqueues work.  Raises ValueError, as griffin_lim() does, for a frame count the round trip does not keep."""
    import torch
    n, alpha = _gla_args(iterations, alpha)
    t = _dev_tensor(S, torch.complex64, device)
    if t.dim() not in (2, 3):
        raise ValueError('expected a (T, F) spectrogram or a (B, T, F) stack')
    single = t.dim() == 2
    t3 = (t[None] if single else t).clone()
    B, T, F = t3.shape
    if F != fsize // 2 + 1:
        raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
    back = _capi.stft_frames(_capi.istft_length(T, fsize, fshift, perfectrec), fsize, fshift, perfectrec)
    if n > 0 and back != T:
        raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, back))
    A = None
    if magnitudes is not None:
        A = _dev_tensor(magnitudes, torch.float32, device)
        if A.shape != t.shape:
            raise ValueError('magnitudes of shape %s for a spectrogram of shape %s' % (tuple(A.shape), tuple(t.shape)))
    trace = _capi.griffin_lim_dev(t3.data_ptr(), None if A is None else A.data_ptr(), B, T, fsize, fshift, awin, swin, perfectrec,
                                  n, alpha, want_trace=return_trace, device=int(device),
                                  stream=torch.cuda.current_stream(t3.device).cuda_stream)
    out = t3[0] if single else t3
    if not return_trace:
        return out
    db = 10 * np.log10(trace[..., 0] / trace[..., 1])
    return out, (db[:, 0] if single else db)


# --------------------------------------------------------------------------------------------
# MISI (Gunawan & Sen 2010; no counterpart in the reference): Griffin-Lim on K sources coupled through their known mixture
# --------------------------------------------------------------------------------------------
def _misi_returns(out, db, sig, return_trace, return_signals):
    res = (out,) + ((db,) if return_trace else ()) + ((sig,) if return_signals else ())
    return res[0] if len(res) == 1 else res


def _misi_share(x, y):
    """The K signals x (K, len) with the mixture error e = y - sum_k x_k (k ascending) shared out equally; also e."""
    tot = x[0].copy()
    for k in range(1, x.shape[0]):
        tot += x[k]
    e = y - tot
    return x + e / x.shape[0], e


def misi(S, mixture, fsize, fshift, awin, swin, iterations, magnitudes=None, perfectrec=False, return_trace=False,
         return_signals=False, _perturb=None):
    """Multiple Input Spectrogram Inversion from the starts S, (K, T, F) or a stack (B, K, T, F), and the real mixture(s)
    `mixture`, (len,) / (B, len) with len that of istft(S[k]), in fp64 on the host: the definition the device form is held to.
    Step i = 1..iterations is x_k = istft(c_k), e = y - sum_k x_k (k ascending), X_k = stft(x_k + e / K), c_k = A_k X_k / |X_k|
    (A_k + 0j where |X_k| == 0); no momentum.  Returns c after the last step (its magnitudes are A = `magnitudes`, by default
    |S|); zero iterations return S.  return_trace: also 10 log10(sum y^2 / sum e^2) of the iterate entering each step, shape
    (iterations,) / (iterations, B).  return_signals: also s_k = istft(out_k) + (y - sum_j istft(out_j)) / K, (K, len) /
    (B, K, len), which sum to the mixture.  Order of the extras: trace, signals.  (_perturb(i, b, k, X) -> X: replaces each
    projection; the error model of the tests.)"""
    n, _ = _gla_args(iterations, 0.0)
    S = np.asarray(S)
    if S.ndim not in (3, 4):
        raise ValueError('expected (K, T, F) spectrograms of the sources or a (B, K, T, F) stack')
    A = np.abs(S) if magnitudes is None else np.asarray(magnitudes, dtype=np.float64)
    if A.shape != S.shape:
        raise ValueError('magnitudes of shape %s for spectrograms of shape %s' % (A.shape, S.shape))
    y = np.asarray(mixture, dtype=np.float64)
    S4, A4, y2 = (S[None], A[None], y[None]) if S.ndim == 3 else (S, A, y)
    B, K, T, F = S4.shape
    if K < 1:
        raise ValueError('no sources')
    length = len(istft(np.zeros((T, F), complex), fshift, swin, perfectrec=perfectrec))
    if y.ndim != S.ndim - 2 or y2.shape != (B, length):
        raise ValueError('mixture of shape %s for %s spectrograms of %d frames: expected %s' %
                         (y.shape, S.shape[:-2], T, S.shape[:-3] + (length,)))
    out = S4.astype(np.complex128)
    db = np.empty((n, B))
    sig = np.empty((B, K, length))
    for b in range(B):
        c = out[b]
        for i in range(1, n + 1):
            x, e = _misi_share(np.stack([istft(c[k], fshift, swin, perfectrec=perfectrec) for k in range(K)]), y2[b])
            with np.errstate(divide='ignore', invalid='ignore'):
                db[i - 1, b] = 10 * np.log10(np.sum(y2[b] ** 2) / np.sum(e ** 2))
            for k in range(K):
                X = stft(x[k], fsize, fshift, awin, perfectrec=perfectrec)
                if X.shape != c[k].shape:
                    raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, X.shape[0]))
                if _perturb is not None:
                    X = _perturb(i, b, k, X)
                c[k] = _project(X, A4[b, k])
        if return_signals:
            sig[b] = _misi_share(np.stack([istft(c[k], fshift, swin, perfectrec=perfectrec) for k in range(K)]), y2[b])[0]
    if n == 0:
        out = S4
    if S.ndim == 3:
        out, db, sig = out[0], db[:, 0], sig[0]
    return _misi_returns(out, db, sig, return_trace, return_signals)


def misi_dev(S, mixture, fsize, fshift, awin, swin, iterations, magnitudes=None, perfectrec=False, return_trace=False,
             return_signals=False, device=0):
    """misi() above on the device (lws_gla.hip: float32; per iteration one inverse launch over all sources, one residual launch
    and one forward launch whose load adds the shared mixture error and whose epilogue is the magnitude projection): S (K, T, F)
    or (B, K, T, F) and mixture (len,) / (B, len), numpy or torch; returns a new complex64 torch tensor (S itself is not
    modified), with return_trace also the dB values as a numpy array, with return_signals also the signals as a float32 torch
    tensor (in that order).  Runs on the caller's current torch stream; without return_trace the call only enqueues work."""
    import torch
    n, _ = _gla_args(iterations, 0.0)
    t = _dev_tensor(S, torch.complex64, device)
    if t.dim() not in (3, 4):
        raise ValueError('expected (K, T, F) spectrograms of the sources or a (B, K, T, F) stack')
    single = t.dim() == 3
    if isinstance(S, torch.Tensor) and t.data_ptr() == S.data_ptr():
        t = t.clone()                              # the iteration is in place: never on the caller's storage
    t4 = t[None] if single else t
    B, K, T, F = t4.shape
    if K < 1:
        raise ValueError('no sources')
    if F != fsize // 2 + 1:
        raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
    A = None
    if magnitudes is not None:
        A = _dev_tensor(magnitudes, torch.float32, device)
        if A.shape != t.shape:
            raise ValueError('magnitudes of shape %s for spectrograms of shape %s' % (tuple(A.shape), tuple(t.shape)))
    y = _dev_tensor(mixture, torch.float32, device)
    length = _capi.istft_length(T, fsize, fshift, perfectrec)
    if y.dim() != t.dim() - 2 or tuple(y.shape)[-1:] != (length,) or (not single and y.shape[0] != B):
        raise ValueError('mixture of shape %s for %s spectrograms of %d frames: expected %s' %
                         (tuple(y.shape), tuple(t.shape[:-2]), T, tuple(t.shape[:-3]) + (length,)))
    if n > 0 and _capi.stft_frames(length, fsize, fshift, perfectrec) != T:
        raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' %
                         (T, _capi.stft_frames(length, fsize, fshift, perfectrec)))
    sig = torch.empty((B, K, length), dtype=torch.float32, device=t4.device) if return_signals else None
    trace = _capi.misi_dev(t4.data_ptr(), None if A is None else A.data_ptr(), y.data_ptr(), B, K, T, fsize, fshift, awin, swin,
                           perfectrec, n, None if sig is None else sig.data_ptr(), want_trace=return_trace, device=int(device),
                           stream=torch.cuda.current_stream(t4.device).cuda_stream)
    db = None
    if return_trace:
        with np.errstate(divide='ignore', invalid='ignore'):
            db = 10 * np.log10(trace[..., 0] / trace[..., 1])
    if single:
        t4, db, sig = t4[0], (None if db is None else db[:, 0]), (None if sig is None else sig[0])
    return _misi_returns(t4, db, sig, return_trace, return_signals)


# --------------------------------------------------------------------------------------------
# Training through MISI (unfolded MISI, Wang, Le Roux & Hershey 2018): the gradient of a loss on misi()'s results, host fp64
# definition and device form.  Complex gradients are g = dL/dRe + j dL/dIm (torch's convention), so that dL = Re sum conj(g) dz.
# --------------------------------------------------------------------------------------------
def _misi_cuts(T, fsize, fshift, perfectrec):
    """(Tfull, lo, hi): istft returns the samples lo..hi of the uncut timeline of Tfull = fshift (T - 1) + fsize samples."""
    full = fshift * (T - 1) + fsize
    if perfectrec is True:
        return full, _perfectrec_prepad(fsize, fshift), full - (fsize - fshift)
    return full, 0, full


def _misi_istft_adjoint(gx, T, fsize, fshift, swin, perfectrec):
    """The gradient on c, (T, F), of a loss whose gradient on istft(c; swin) is gx: (w / N) stft(gx; window swin) with w = 2 on the
    interior bins and 1 at the bins 0 and N/2, whose imaginary parts istft never reads (zero).  gx sits where istft cut it from."""
    full, lo, hi = _misi_cuts(T, fsize, fshift, perfectrec)
    x = np.zeros(full)
    x[lo:hi] = gx
    idx = fshift * np.arange(T)[:, None] + np.arange(fsize)[None, :]
    g = np.fft.fft(x[idx] * np.asarray(swin, dtype=np.float64)[None, :], axis=1)[:, : fsize // 2 + 1] * (2.0 / fsize)
    g[:, 0] = 0.5 * g[:, 0].real
    g[:, -1] = 0.5 * g[:, -1].real
    return g


def _misi_stft_adjoint(gX, fsize, fshift, awin, perfectrec):
    """The gradient on v of a loss whose gradient on stft(v; awin) is gX: N istft(G; window awin) with G = gX / 2 on the interior
    bins and Re gX at the bins 0 and N/2; istft's cut is the adjoint of the zeros stft pads with perfectrec."""
    G = 0.5 * np.asarray(gX, dtype=np.complex128)
    G[:, 0] = gX[:, 0].real
    G[:, -1] = gX[:, -1].real
    return fsize * istft(G, fshift, np.asarray(awin, dtype=np.float64), perfectrec=perfectrec)


# ---- what the three trainings (MISI, Griffin-Lim, RTISI-LA) do alike, stated once: the projection's derivative, the front and back of
# the *_grad definitions, the argument checks of the *_layer operations and the autograd scaffold they are built from
def _project_backward(X, A, g):
    """Step 3 of every backward pass below: (Re q, gX) with u = X / |X|, q = conj(u) g and gX = j u (A / |X|) Im q, g being the
    gradient on _project(X, A); where |X| == 0 the forward gives A + 0j, so u = 1 and gX = 0."""
    mag = np.abs(X)
    safe = np.where(mag > 0, mag, 1.0)
    u = np.where(mag > 0, X / safe, 1.0 + 0j)
    q = np.conj(u) * g
    return q.real, np.where(mag > 0, 1j * u * (A / safe) * q.imag, 0j)


def _grad_call(fn, sources, S, magnitudes, grad_out, grad_sig, _tape, plan):
    """misi_grad (sources: S holds K spectrograms per mixture), griffin_lim_grad and rtisi_la_grad around what is their own: S and
    the required magnitudes as stacks (a single one becomes a stack of one, and the results come back single), the cotangents
    converted and held to their shapes, the tape from _tape or from a recording forward run.  plan(S_stack, A_stack, single) ->
    (tape, forward, backward, length, sig_name): the empty tape, forward() that fills it, backward(gC, gs) -> the gradients as
    stacks, and the length and argument name of the signal cotangent grad_sig (None for a function that takes none)."""
    S = np.asarray(S)
    rank = 3 if sources else 2
    if S.ndim not in (rank, rank + 1):
        raise ValueError('expected (K, T, F) spectrograms of the sources or a (B, K, T, F) stack' if sources else
                         'expected a (T, F) spectrogram or a (B, T, F) stack')
    noun = 'spectrograms' if sources else 'a spectrogram'
    if magnitudes is None:
        raise ValueError('%s differentiates with respect to the magnitudes: give them' % fn)
    A = np.asarray(magnitudes, dtype=np.float64)
    if A.shape != S.shape:
        raise ValueError('magnitudes of shape %s for %s of shape %s' % (A.shape, noun, S.shape))
    single = S.ndim == rank
    tape, forward, backward, length, sig_name = plan(*((S[None], A[None]) if single else (S, A)), single)
    if _tape is None:
        forward()
    else:
        tape[...] = np.asarray(_tape).reshape(tape.shape)
    gC = gs = None
    if grad_out is not None:
        gC = np.asarray(grad_out, dtype=np.complex128)
        if gC.shape != S.shape:
            raise ValueError('grad_out of shape %s for %s of shape %s' % (gC.shape, noun, S.shape))
        gC = gC[None] if single else gC
    if grad_sig is not None:
        gs = np.asarray(grad_sig, dtype=np.float64)
        if gs.shape != S.shape[:-2] + (length,):
            raise ValueError('%s of shape %s: expected %s' % (sig_name, gs.shape, S.shape[:-2] + (length,)))
        gs = gs[None] if single else gs
    grads = backward(gC, gs)
    return tuple(g[0] for g in grads) if single else grads


def _layer_args(A, S, fsize, fshift, awin, swin, n, perfectrec, mixture=None, round_trip_always=True, squeeze_swin=False):
    """The checks of misi_layer (mixture given: K sources per mixture), griffin_lim_layer and rtisi_la_layer (which holds the round
    trip to the frame count under perfectrec only, and squeezes swin): float32 / complex64 device tensors on one device, S a
    single input or a stack, A shaped as S, fsize // 2 + 1 bins, a mixture of istft's length, a frame count the round trip keeps.
    Returns the windows as fp64 arrays."""
    import torch
    sources = mixture is not None
    for name, t, dtype in (('A', A, torch.float32), ('S', S, torch.complex64)) + ((('mixture', mixture, torch.float32),) if sources else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            raise ValueError('%s must be a %s torch tensor on the device' % (name, str(dtype).replace('torch.', '')))
    rank = 3 if sources else 2
    if S.dim() not in (rank, rank + 1):
        raise ValueError('expected (K, T, F) spectrograms of the sources or a (B, K, T, F) stack' if sources else
                         'expected a (T, F) spectrogram or a (B, T, F) stack')
    if A.shape != S.shape:
        raise ValueError('magnitudes of shape %s for %s of shape %s' %
                         (tuple(A.shape), 'spectrograms' if sources else 'a spectrogram', tuple(S.shape)))
    if A.device != S.device or (sources and mixture.device != S.device):
        raise ValueError('A, S and mixture must be on one device' if sources else 'A and S must be on one device')
    T, F = S.shape[-2:]
    if sources and S.shape[-3] < 1:
        raise ValueError('no sources')
    if F != fsize // 2 + 1:
        raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
    length = _capi.istft_length(T, fsize, fshift, perfectrec)
    if sources and tuple(mixture.shape) != tuple(S.shape[:-3]) + (length,):
        raise ValueError('mixture of shape %s for %s spectrograms of %d frames: expected %s' %
                         (tuple(mixture.shape), tuple(S.shape[:-2]), T, tuple(S.shape[:-3]) + (length,)))
    if n > 0 and (perfectrec or round_trip_always):
        back = _capi.stft_frames(length, fsize, fshift, perfectrec)
        if back != T:
            raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, back))
    awin, swin = np.array(awin, dtype=np.float64), np.array(swin, dtype=np.float64)
    return awin, (np.squeeze(swin) if squeeze_swin else swin)


class _Layer(object):
    """What a differentiable layer gives the scaffold below: the rank of a single S, whether it returns signals beside C, the
    shape of its tape, tape_shape(n, dims, extra), and its two _capi calls, forward(p, dims, mid, extra, kw) and backward(...)
    alike, with p the device pointers by name (None where there is no tensor), dims = (B, [K,] T, F) of the stack, mid = (fsize,
    fshift, awin, swin, perfectrec, n) as every call takes them in a row, extra the layer's own numbers (alpha, or the look-ahead),
    kw the device and the stream."""

    def __init__(self, rank, signals, tape_shape, forward, backward):
        self.rank, self.signals, self.tape_shape, self.forward, self.backward = rank, signals, tape_shape, forward, backward


_layer_function = None


def _layer_apply(layer, A, S, y, fsize, fshift, awin, swin, n, perfectrec, *extra):
    """The one torch.autograd.Function behind misi_layer, griffin_lim_layer and rtisi_la_layer, made on first use (importing this
    module needs no torch), applied to checked arguments: y the mixture or None; returns C, or (C, signals)."""
    global _layer_function
    if _layer_function is None:
        import types
        import torch
        from torch.autograd.function import once_differentiable

        def pointers(**tensors):
            return types.SimpleNamespace(**{k: None if t is None else t.data_ptr() for k, t in tensors.items()})

        class Layer(torch.autograd.Function):
            @staticmethod
            def forward(ctx, layer, A, S, y, fsize, fshift, awin, swin, n, perfectrec, *extra):
                dev = S.device
                dims = ((1,) if S.dim() == layer.rank else ()) + tuple(S.shape)
                length = max(_capi.istft_length(dims[-2], fsize, fshift, perfectrec), 0)
                A, y = A.detach().contiguous(), None if y is None else y.detach().contiguous()
                C = S.detach().clone(memory_format=torch.contiguous_format)      # the iteration is in place: never on the caller's storage
                sig = torch.empty(tuple(S.shape[:-2]) + (length,), dtype=torch.float32, device=dev) if layer.signals else None
                tape = torch.empty(layer.tape_shape(n, dims, extra), dtype=torch.complex64, device=dev)
                mid, kw = (fsize, fshift, awin, swin, perfectrec, n), dict(device=dev.index, stream=torch.cuda.current_stream(dev).cuda_stream)
                layer.forward(pointers(C=C, A=A, y=y, sig=sig if length else None, tape=tape if n else None), dims, mid, extra, kw)
                ctx.save_for_backward(A, tape)
                ctx.set_materialize_grads(False)
                ctx.call = (layer, dims, mid, extra, None if y is None else tuple(y.shape))
                return (C, sig) if layer.signals else C

            @staticmethod
            @once_differentiable
            def backward(ctx, gC, gs=None):
                A, tape = ctx.saved_tensors
                layer, dims, mid, extra, y_shape = ctx.call
                dev = A.device
                if gC is not None:
                    gC = gC.to(torch.complex64).contiguous()
                if gs is not None:
                    gs = gs.to(torch.float32).contiguous() if gs.numel() else None
                gA = torch.empty_like(A)
                gS = torch.empty(A.shape, dtype=torch.complex64, device=dev) if ctx.needs_input_grad[2] else None
                gy = torch.empty(y_shape, dtype=torch.float32, device=dev) if y_shape is not None and ctx.needs_input_grad[3] else None
                kw = dict(device=dev.index, stream=torch.cuda.current_stream(dev).cuda_stream)
                layer.backward(pointers(gC=gC, gs=gs, A=A, tape=tape if mid[-1] else None, gA=gA, gS=gS, gy=gy), dims, mid, extra, kw)
                return (None, gA if ctx.needs_input_grad[1] else None, gS, gy) + (None,) * (6 + len(extra))

        _layer_function = Layer
    return _layer_function.apply(layer, A, S, y, int(fsize), int(fshift), awin, swin, n, bool(perfectrec), *extra)


def _misi_backward(tape, A, grad_out, grad_signals, fsize, fshift, awin, swin, perfectrec=False, _perturb=None):
    """The backward pass of misi() from a tape of its projections' arguments: tape (n, B, K, T, F) the X_k of the steps 1..n, A
    (B, K, T, F), and the cotangents grad_out (B, K, T, F) complex of the returned spectrograms and grad_signals (B, K, len) of
    the signals, either None for zeros.  Returns (gA, gS, gy); see misi_grad, which records the tape and calls this."""
    tape, A = np.asarray(tape, dtype=np.complex128), np.asarray(A, dtype=np.float64)
    B, K, T, F = A.shape
    n = tape.shape[0]
    _, lo, hi = _misi_cuts(T, fsize, fshift, perfectrec)
    length = hi - lo
    gA, gS, gy = np.zeros(A.shape), np.zeros(A.shape, dtype=np.complex128), np.zeros((B, length))

    def share_back(gv, b):              # step 1: v_k = x_k + (y - sum_j x_j) / K
        m = gv[0].copy()
        for k in range(1, K):
            m += gv[k]
        m /= K
        gy[b] += m
        return gv - m

    def frames_back(gsig, i, b):        # step 2, for the K sources
        gc = np.stack([_misi_istft_adjoint(gsig[k], T, fsize, fshift, swin, perfectrec) for k in range(K)])
        if _perturb is not None:
            gc = np.stack([_perturb('gc', i, b, k, gc[k]) for k in range(K)])
        return gc

    for b in range(B):
        gv = np.zeros((K, length)) if grad_signals is None else np.array(grad_signals[b], dtype=np.float64)
        gc = frames_back(share_back(gv, b), n, b)
        if grad_out is not None:
            gc = gc + np.asarray(grad_out[b], dtype=np.complex128)
        for i in range(n, 0, -1):
            gv = np.empty((K, length))
            for k in range(K):
                ga, gX = _project_backward(tape[i - 1, b, k], A[b, k], gc[k])          # step 3
                gA[b, k] += ga
                v = _misi_stft_adjoint(gX, fsize, fshift, awin, perfectrec)            # step 4
                gv[k] = v if _perturb is None else np.real(_perturb('gv', i, b, k, v))
            gc = frames_back(share_back(gv, b), i - 1, b)
        gS[b] = gc
    return gA, gS, gy


def misi_grad(S, mixture, fsize, fshift, awin, swin, iterations, magnitudes, grad_out=None, grad_signals=None, perfectrec=False,
              _perturb=None, _tape=None):
    """The gradient of a loss L on the results of misi(S, mixture, ..., magnitudes=A, return_signals=True), in fp64 on the host:
    the definition the device backward pass (misi_layer) is held to.  grad_out: the cotangent dL/dRe + j dL/dIm of the returned
    spectrograms, shaped as S; grad_signals: that of the signals, (K, len) / (B, K, len); either None for zeros.  Returns
    (gA, gS, gy), the gradients on the magnitudes (real), on the start S (complex, same convention) and on the mixture, shaped as
    their arguments.  A is a variable of its own here: `magnitudes` is required.

    Backward through step i = n..1 of misi(), gc being the gradient on c_i and X the argument of that step's projection:
      3. u = X / |X|, q = conj(u) gc;  gA += Re q;  gX = j u (A / |X|) Im q   (where |X| == 0 the forward gives A + 0j: u = 1, gX = 0)
      4. gv_k = N istft(G; window awin), G = gX / 2 on the interior bins and Re gX at the bins 0 and N/2
      1. m = mean_k gv_k (k ascending);  gsig_k = gv_k - m;  gy += m   (the perfectrec cuts carry no gradient)
      2. gc_k = (w / N) stft(gsig_k; window swin), w = 2 on the interior bins, 1 and no imaginary part at the bins 0 and N/2
    and on entry gc = (1 and 2 applied to grad_signals) + grad_out; the gc left at the end is gS.  Zero iterations: gA = 0.
    (_perturb(kind, i, b, k, Z) -> Z: replaces each projection argument, kind 'X', step i; each result of 2, kind 'gc', the
    gradient on c_i; each result of 4, kind 'gv', step i, of which the real part is taken.  The error model of the tests.
    _tape: (n, K, T, F) / (n, B, K, T, F), the X of every step from elsewhere -- a device run's -- instead of this function's own
    forward pass: the backward pass alone, teacher-forced.)"""
    n, _ = _gla_args(iterations, 0.0)

    def plan(S4, A4, single):
        y = np.asarray(mixture, dtype=np.float64)
        tape = np.empty((n,) + S4.shape, dtype=np.complex128)

        def record(i, b, k, X):
            if _perturb is not None:
                X = _perturb('X', i, b, k, X)
            tape[i - 1, b, k] = X
            return X

        def forward():
            misi(S4, y[None] if single else y, fsize, fshift, awin, swin, n, magnitudes=A4, perfectrec=perfectrec, _perturb=record)

        def backward(gC, gs):
            return _misi_backward(tape, A4, gC, gs, fsize, fshift, awin, swin, perfectrec=perfectrec, _perturb=_perturb)

        _, lo, hi = _misi_cuts(S4.shape[2], fsize, fshift, perfectrec)
        return tape, forward, backward, hi - lo, 'grad_signals'

    return _grad_call('misi_grad', True, S, magnitudes, grad_out, grad_signals, _tape, plan)


_MISI_LAYER = _Layer(
    3, True, lambda n, dims, extra: (n,) + dims,
    lambda p, dims, mid, extra, kw: _capi.misi_tape_dev(p.C, p.A, p.y, *dims[:3], *mid, p.sig, p.tape, **kw),
    lambda p, dims, mid, extra, kw: _capi.misi_backward_dev(p.gC, p.gs, p.A, p.tape, *dims[:3], *mid, p.gA, p.gS, p.gy, **kw))


def misi_layer(A, S, mixture, fsize, fshift, awin, swin, iterations, perfectrec=False):
    """misi_dev(S, mixture, ..., magnitudes=A, return_signals=True) as a differentiable torch operation, for training through MISI:
    returns (C, s), the spectrograms after `iterations` steps and their signals, with the bits misi_dev gives them, and
    loss.backward() reaches whichever of A, S and mixture require grad (the others get None).  Takes device tensors, A float32
    and S complex64 of shape (K, T, F) or (B, K, T, F), mixture float32 (len,) / (B, len); does not modify them; runs on the
    current torch stream and only enqueues work, forward and backward.  Once differentiable.  The forward pass keeps the argument
    of every projection for the backward pass: a complex64 tape of `iterations` times the size of S, held by the autograd graph
    until backward() has run (or the results are dropped).  The backward pass is three launches per iteration, as the forward
    pass (lws_gla.hip), and repeats bit for bit; its definition is misi_grad.  Zero iterations: C is a copy of S."""
    n, _ = _gla_args(iterations, 0.0)
    awin, swin = _layer_args(A, S, fsize, fshift, awin, swin, n, perfectrec, mixture=mixture)
    return _layer_apply(_MISI_LAYER, A, S, mixture, fsize, fshift, awin, swin, n, perfectrec)


# --------------------------------------------------------------------------------------------
# Training through (Fast) Griffin-Lim (a few unrolled steps under a waveform or spectral loss, "deep Griffin-Lim"): the gradient of a
# loss on griffin_lim()'s result, host fp64 definition and device form.  Same convention for complex gradients as above.
# --------------------------------------------------------------------------------------------
def _gla_backward(tape, A, grad_out, alpha, fsize, fshift, awin, swin, perfectrec=False, _perturb=None):
    """The backward pass of griffin_lim() from a tape of its projections' arguments: tape (n, B, T, F) the X of the steps 1..n,
    A (B, T, F), grad_out (B, T, F) complex, the cotangent of t_n, or None for zeros.  Returns (gA, gS); see griffin_lim_grad, which
    records the tape and calls this."""
    tape, A = np.asarray(tape, dtype=np.complex128), np.asarray(A, dtype=np.float64)
    B, T, F = A.shape
    n = tape.shape[0]
    gA, gS = np.zeros(A.shape), np.zeros(A.shape, dtype=np.complex128)
    for b in range(B):
        gout = np.zeros((T, F), dtype=np.complex128) if grad_out is None else np.asarray(grad_out[b], dtype=np.complex128)
        gc, gc_next = gout, None            # the gradients on c_i and c_{i+1}; with n == 0 the start is the result
        for i in range(n, 0, -1):
            if i == n:                      # step 0: c_n is never used, t_n is the result
                gt = gout
            else:
                gt = (1.0 + (alpha if i >= 2 else 0.0)) * gc
                if i + 1 < n:               # gc_n = 0
                    gt = gt - alpha * gc_next
            ga, gX = _project_backward(tape[i - 1, b], A[b], gt)                               # step 3
            gA[b] += ga
            gv = _misi_stft_adjoint(gX, fsize, fshift, awin, perfectrec)                       # step 4
            if _perturb is not None:
                gv = np.real(_perturb('gv', i, b, gv))
            new = _misi_istft_adjoint(gv, T, fsize, fshift, swin, perfectrec)                  # step 2
            if _perturb is not None:
                new = _perturb('gc', i - 1, b, new)
            gc_next, gc = gc, new
        gS[b] = gc
    return gA, gS


def griffin_lim_grad(S, fsize, fshift, awin, swin, iterations, magnitudes, alpha=0.99, grad_out=None, perfectrec=False,
                     _perturb=None, _tape=None):
    """The gradient of a loss L on the result of griffin_lim(S, ..., alpha=alpha, magnitudes=A), in fp64 on the host: the definition
    the device backward pass (griffin_lim_layer) is held to.  grad_out: the cotangent dL/dRe + j dL/dIm of the returned
    spectrogram, shaped as S, (T, F) or (B, T, F); None for zeros.  Returns (gA, gS), the gradients on the magnitudes (real) and on
    the start S (complex, same convention), shaped as S.  A is a variable of its own here: `magnitudes` is required.  alpha is a
    number, not a variable: it gets no gradient.

    The update c_i = t_i + alpha_i (t_i - t_{i-1}) (alpha_1 = 0, alpha_i = alpha after that) is linear in the t's, so no t is kept:
    the momentum is a two-term recurrence in the gradients.  With gc_i the gradient on c_i and gc_n = 0 (c_n is never used),
    backward through step i = n..1 of griffin_lim(), X_i the argument of that step's projection:
      0. gt = grad_out for i = n, (1 + alpha_i) gc_i - alpha_{i+1} gc_{i+1} otherwise
      3. u = X_i / |X_i|, q = conj(u) gt;  gA += Re q;  gX = j u (A / |X_i|) Im q   (where |X_i| == 0 the forward gives A + 0j: u = 1, gX = 0)
      4. gv = N istft(G; window awin), G = gX / 2 on the interior bins and Re gX at the bins 0 and N/2
      2. gc_{i-1} = (w / N) stft(gv; window swin), w = 2 on the interior bins, 1 and no imaginary part at the bins 0 and N/2 (the
         perfectrec cuts carry no gradient)
    and gS = gc_0.  Zero iterations: gA = 0, gS = grad_out.
    (_perturb(kind, i, b, Z) -> Z: replaces each projection argument, kind 'X', step i; each result of 4, kind 'gv', step i, of
    which the real part is taken; each result of 2, kind 'gc', the gradient on c_i.  The error model of the tests.
    _tape: (n, T, F) / (n, B, T, F), the X of every step from elsewhere -- a device run's -- instead of this function's own forward
    pass: the backward pass alone, teacher-forced.)"""
    n, alpha = _gla_args(iterations, alpha)

    def plan(S3, A3, single):
        tape = np.empty((n,) + S3.shape, dtype=np.complex128)

        def record(i, b, X):
            if _perturb is not None:
                X = _perturb('X', i, b, X)
            tape[i - 1, b] = X
            return X

        def forward():
            griffin_lim(S3, fsize, fshift, awin, swin, n, alpha=alpha, magnitudes=A3, perfectrec=perfectrec, _perturb=record)

        def backward(gC, _):
            return _gla_backward(tape, A3, gC, alpha, fsize, fshift, awin, swin, perfectrec=perfectrec, _perturb=_perturb)

        return tape, forward, backward, None, None

    return _grad_call('griffin_lim_grad', False, S, magnitudes, grad_out, None, _tape, plan)


_GLA_LAYER = _Layer(
    2, False, lambda n, dims, extra: (n,) + dims,
    lambda p, dims, mid, extra, kw: _capi.griffin_lim_tape_dev(p.C, p.A, *dims[:2], *mid, extra[0], p.tape, **kw),
    lambda p, dims, mid, extra, kw: _capi.griffin_lim_backward_dev(p.gC, p.A, p.tape, *dims[:2], *mid, extra[0], p.gA, p.gS, **kw))


def griffin_lim_layer(A, S, fsize, fshift, awin, swin, iterations, alpha=0.99, perfectrec=False):
    """griffin_lim_dev(S, ..., alpha=alpha, magnitudes=A) as a differentiable torch operation, for training through a few unrolled
    (Fast) Griffin-Lim steps: returns C, the spectrogram after `iterations` steps, with the bits griffin_lim_dev gives it, and
    loss.backward() reaches whichever of A and S require grad (the other gets None).  alpha is a number, not a variable: it gets no
    gradient.  Takes device tensors, A float32 and S complex64 of shape (T, F) or (B, T, F); does not modify them; runs on the
    current torch stream and only enqueues work, forward and backward.  Once differentiable.  The forward pass keeps the argument
    of every projection for the backward pass: a complex64 tape of `iterations` times the size of S, held by the autograd graph
    until backward() has run (or the result is dropped); the momentum needs no tape of its own.  The backward pass is two launches
    per iteration, as the forward pass (lws_gla.hip), and repeats bit for bit; its definition is griffin_lim_grad.  Zero
    iterations: C is a copy of S.  Raises ValueError, as griffin_lim_dev does, for a frame count the round trip does not keep."""
    n, alpha = _gla_args(iterations, alpha)
    awin, swin = _layer_args(A, S, fsize, fshift, awin, swin, n, perfectrec)
    return _layer_apply(_GLA_LAYER, A, S, None, fsize, fshift, awin, swin, n, perfectrec, alpha)


# --------------------------------------------------------------------------------------------
# RTISI-LA (Zhu, Beauregard & Wyse 2007): Griffin-Lim under a look-ahead -- what online LWS approximates, as batch LWS does Griffin-Lim
# --------------------------------------------------------------------------------------------
def _look_ahead_arg(look_ahead):
    if int(look_ahead) != look_ahead or look_ahead < 0:
        raise ValueError('look_ahead must be a non-negative integer, got %r' % (look_ahead,))
    return int(look_ahead)


def _start_arg(start, allowed):
    if start not in allowed:
        raise ValueError('start must be one of %s, got %r' % (', '.join(repr(a) for a in allowed), start))
    return start


def rtisi_la(S, fsize, fshift, awin, swin, iterations, look_ahead=3, magnitudes=None, perfectrec=False, return_signal=False,
             _perturb=None, open_end=False, start='given'):
    """Real-Time Iterative Spectrogram Inversion with Look-Ahead from the start S, (T, F) or a stack (B, T, F), in fp64 on the
    host: the definition the device form is held to.  Frame m of the result depends on no input frame later than m + look_ahead.
    With inv(c) = swin irfft(c) and fwd(y) = rfft(awin y) on the timeline of fshift (T - 1) + fsize samples -- where, with
    perfectrec, the samples istft cuts read as zero -- the frames m = 0 .. T-1 are committed in order: every frame up to
    last = min(m + look_ahead, T - 1) that has not entered does, f_j = inv(c_j); `iterations` times, all active frames are
    projected from the same sum (Jacobi), y = done + sum_{j = m..last} f_j (j ascending), c_j = A_j X_j / |X_j| with
    X_j = fwd(y[fshift j : fshift j + fsize]) (A_j + 0j where |X_j| == 0), f_j = inv(c_j); then done += f_m for good.  Returns c
    (its magnitudes are A = `magnitudes`, by default |S|); zero iterations return S.  With look_ahead >= T - 1 the first commit
    is `iterations` plain Griffin-Lim steps.  return_signal: also done cut as istft cuts it, which is istft(c), (len,) / (B, len).
    open_end: nothing inside the iteration depends on where the spectrogram ends -- with perfectrec the samples from fshift T on are
    not read as zero (the lead-in still is, and the returned signal is still cut as istft cuts it), and the frame count need not be
    one the round trip keeps -- so the rows [:T1 - look_ahead] of a run on S[:T1] are those of a run on any longer S: what a stream
    (RtisiLaStream) computes.  Without perfectrec it changes nothing.
    start: how a frame enters.  'given' (the default): from S, as above.  'overlap': RTISI's own initial estimate, from magnitudes
    alone -- frames enter one at a time, j ascending, and frame j, entering in commit step m, does not compute f_j = inv(S_j) but
    y = keep (done + sum_{i = m..j-1} f_i) (i ascending), X = fwd(y[fshift j : fshift j + fsize]), c_j = A_j X / |X| (A_j + 0j
    where |X| == 0: frame 0, every frame under a silent sum, every frame at fshift == fsize), f_j = inv(c_j).  Only A is read --
    the phases of S are not, and S may be a real array -- and zero iterations return the entry estimates, not S.
    (_perturb(m, it, b, X) -> X: replaces the stacked projections of one inner iteration, and with it = 0 and X[None] the projection
    of an entering frame; the error model of the tests.)"""
    n, _ = _gla_args(iterations, 0.0)
    LA = _look_ahead_arg(look_ahead)
    overlap = _start_arg(start, ('given', 'overlap')) == 'overlap'
    S = np.asarray(S)
    if S.ndim not in (2, 3):
        raise ValueError('expected a (T, F) spectrogram or a (B, T, F) stack')
    A = np.abs(S) if magnitudes is None else np.asarray(magnitudes, dtype=np.float64)
    if A.shape != S.shape:
        raise ValueError('magnitudes of shape %s for a spectrogram of shape %s' % (A.shape, S.shape))
    T, F = S.shape[-2:]
    if F != fsize // 2 + 1 or fsize % 2:
        raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
    awin, swin = np.asarray(awin, dtype=np.float64), np.squeeze(np.asarray(swin, dtype=np.float64))
    total = fshift * (T - 1) + fsize
    keep = np.ones(total)
    lo, hi = 0, total
    if perfectrec is True:
        lo, hi = _perfectrec_prepad(fsize, fshift), total - (fsize - fshift)
        keep[:lo] = 0.0
        if not open_end:
            keep[max(hi, 0):] = 0.0
            back = stft(np.zeros(max(hi - lo, 0)), fsize, fshift, awin, perfectrec=True).shape[0]
            if n > 0 and back != T:
                raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, back))
    S3, A3 = (S[None], A[None]) if S.ndim == 2 else (S, A)
    out = (A3 + 0j) if overlap else S3.astype(np.complex128)
    sig = np.empty((S3.shape[0], max(hi - lo, 0)))
    for b in range(S3.shape[0] if (n > 0 or return_signal or overlap) else 0):
        c, done, f, entered = out[b], np.zeros(total), np.zeros((T, fsize)), 0
        for m in range(T):
            last = min(m + LA, T - 1)
            while entered <= last:
                if overlap:
                    y = done.copy()
                    for i in range(m, entered):
                        y[fshift * i: fshift * i + fsize] += f[i]
                    y *= keep
                    X = np.fft.rfft(awin * y[fshift * entered: fshift * entered + fsize])
                    if _perturb is not None:
                        X = _perturb(m, 0, b, X[None])[0]
                    c[entered] = _project(X, A3[b, entered])
                f[entered] = swin * np.fft.irfft(c[entered], fsize)
                entered += 1
            for it in range(1, n + 1):
                y = done.copy()
                for j in range(m, last + 1):
                    y[fshift * j: fshift * j + fsize] += f[j]
                y *= keep
                X = np.stack([np.fft.rfft(awin * y[fshift * j: fshift * j + fsize]) for j in range(m, last + 1)])
                if _perturb is not None:
                    X = _perturb(m, it, b, X)
                c[m: last + 1] = _project(X, A3[b, m: last + 1])
                for j in range(m, last + 1):
                    f[j] = swin * np.fft.irfft(c[j], fsize)
            done[fshift * m: fshift * m + fsize] += f[m]
        sig[b] = (keep * done)[lo: max(hi, lo)]
    if S.ndim == 2:
        out, sig = out[0], sig[0]
    if n == 0 and not overlap:
        out = S
    return (out, sig) if return_signal else out


def _start_rows(S, magnitudes, start, device):
    """The device tensors a look-ahead call passes down: (rows, magnitudes or None).  Under start='given' the rows are complex64.
    Under another start only magnitudes are read, so rows that are real stay real (float32) and serve as the magnitudes themselves
    -- their absolute values -- when none are given."""
    import torch
    A = None if magnitudes is None else _dev_tensor(magnitudes, torch.float32, device)
    real = start != 'given' and not (S.is_complex() if torch.is_tensor(S) else np.iscomplexobj(S))
    t = _dev_tensor(S, torch.float32 if real else torch.complex64, device)
    if real and A is None:
        A = t.abs()
    return t, A


class _LaStream(object):
    """What RtisiLaStream and MisiLaStream share: the checks of their constructors, what push() and finish() hand back, finish(),
    close().  Tensors are (B,) + _lead + (rows, F) and (B,) + _lead + (samples,), with _lead = (K,) for the sources of a mixture."""
    _other_start = _create = _finish = _destroy = None   # of the subclass: its start besides 'given', its calls in _capi

    def __init__(self, K, fsize, fshift, awin, swin, iterations, look_ahead, perfectrec, batch, return_signals, device, start):
        self._h = None
        n, _ = _gla_args(iterations, 0.0)
        self.look_ahead = _look_ahead_arg(look_ahead)
        self.start = _start_arg(start, ('given', self._other_start))
        if K is not None and (int(K) != K or K < 1):
            raise ValueError('K must be a positive integer, got %r' % (K,))
        if batch is not None and (int(batch) != batch or batch < 1):
            raise ValueError('batch must be None or a positive integer, got %r' % (batch,))
        if fsize % 2:
            raise ValueError('Odd ffts not supported.')
        self.fsize, self.fshift, self.iterations, self.perfectrec = int(fsize), int(fshift), n, perfectrec is True
        self.batch, self.device = None if batch is None else int(batch), int(device)
        self._B, self._F = 1 if batch is None else int(batch), int(fsize) // 2 + 1
        self._lead, self._signals = () if K is None else (int(K),), bool(return_signals)
        self.finished = False
        swin = np.squeeze(np.asarray(swin, dtype=np.float64))
        self._h = type(self)._create(self._B, *self._lead, fsize, fshift, awin, swin, self.perfectrec, n, self.look_ahead,
                                     device=self.device, start=self.start)

    def _returns(self, out, sig, nf, ns):
        out = out[..., :nf, :]
        if self.batch is None:
            out = out[0]
        if not self._signals:
            return out
        sig = sig[..., :ns]
        return out, (sig[0] if self.batch is None else sig)

    def finish(self):
        import torch
        if self._h is None or self.finished:
            raise ValueError('finish on a stream that has finished or been closed')
        dev = torch.device("cuda", self.device)
        lead = (self._B,) + self._lead
        out = torch.empty(lead + (self.look_ahead, self._F), dtype=torch.complex64, device=dev)
        sig = None
        if self._signals:
            sig = torch.empty(lead + (self.fsize + self.look_ahead * self.fshift,), dtype=torch.float32, device=dev)
        nf, ns = type(self)._finish(self._h, out.data_ptr() if out.numel() else None, None if sig is None else sig.data_ptr(),
                                    stream=torch.cuda.current_stream(dev).cuda_stream)
        self.finished = True
        return self._returns(out, sig, nf, ns)

    def close(self):
        h, self._h = self._h, None
        if h is not None:
            type(self)._destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


class RtisiLaStream(_LaStream):
    """rtisi_la_dev() for frames that arrive over time (k_rtisi_stream of lws_gla.hip): push() takes the next rows, (Tc, F) -- or
    (B, Tc, F) for `batch`=B streams side by side -- numpy or torch, and returns the rows that could be committed, a new complex64
    torch tensor (n, F) / (B, n, F): frame m is committed once frame m + look_ahead has been pushed, so n may be 0.  finish() returns
    the remaining look_ahead frames and ends the stream.  With return_signal both also return the float32 samples those commits
    finalised, (k,) / (B, k).  Everything returned, concatenated, is rtisi_la(everything pushed, ..., open_end=True) (and its signal):
    however the rows are cut into chunks, bit for bit.  The state lives on the device between calls; a call runs on the caller's current
    torch stream and only enqueues work.  magnitudes: the targets of the pushed rows (default |S|).  iterations=0 returns the pushed rows
    themselves, with the same latency.  start='overlap' drives the stream from magnitudes alone, as rtisi_la(..., start='overlap')
    does: push(A) then takes real or complex rows, reads only their magnitudes (or `magnitudes`), and iterations=0 returns the entry
    estimates.  close() frees the device state (also on deletion)."""
    _other_start, _create, _finish, _destroy = 'overlap', _capi.rtisi_stream_create, _capi.rtisi_stream_finish, _capi.rtisi_stream_destroy

    def __init__(self, fsize, fshift, awin, swin, iterations, look_ahead=3, perfectrec=False, batch=None, return_signal=False, device=0,
                 start='given'):
        _LaStream.__init__(self, None, fsize, fshift, awin, swin, iterations, look_ahead, perfectrec, batch, return_signal, device, start)
        self.return_signal = self._signals

    def push(self, S, magnitudes=None):
        import torch
        if self._h is None or self.finished:
            raise ValueError('push on a stream that has finished or been closed')
        t, A = _start_rows(S, magnitudes, self.start, self.device)
        want = 2 if self.batch is None else 3
        if t.dim() != want or t.shape[-1] != self._F or (self.batch is not None and t.shape[0] != self._B):
            raise ValueError('expected rows of shape %s, got %s' % (('Tc', self._F) if self.batch is None else (self._B, 'Tc', self._F),
                                                                    tuple(t.shape)))
        if A is not None and A.shape != t.shape:
            raise ValueError('magnitudes of shape %s for rows of shape %s' % (tuple(A.shape), tuple(t.shape)))
        Tc = t.shape[-2]
        out = torch.empty((self._B, Tc, self._F), dtype=torch.complex64, device=t.device)
        sig = torch.empty((self._B, Tc * self.fshift), dtype=torch.float32, device=t.device) if self.return_signal else None
        nf, ns = 0, 0
        if Tc > 0:
            nf, ns = _capi.rtisi_stream_push(self._h, None if t.dtype != torch.complex64 else t.data_ptr(),
                                             None if A is None else A.data_ptr(), Tc, out.data_ptr(),
                                             None if sig is None else sig.data_ptr(),
                                             stream=torch.cuda.current_stream(t.device).cuda_stream)
        return self._returns(out, sig, nf, ns)


def rtisi_la_dev(S, fsize, fshift, awin, swin, iterations, look_ahead=3, magnitudes=None, perfectrec=False, return_signal=False,
                 device=0, start='given'):
    """rtisi_la() above on the device (lws_gla.hip: float32, one workgroup per spectrogram marching over the frames with its
    state in LDS, one launch): S (T, F) or (B, T, F), numpy or torch; returns a new complex64 torch tensor (S itself is not
    modified), and with return_signal also the float32 signals (len,) / (B, len).  Runs on the caller's current torch stream
    and only enqueues work.  start: 'given', or 'overlap' for RTISI's own initial estimate from magnitudes alone (S real or complex,
    its phases not read), as rtisi_la() defines it.  Raises ValueError, as rtisi_la() does, for a frame count the round trip does
    not keep."""
    import torch
    n, _ = _gla_args(iterations, 0.0)
    LA = _look_ahead_arg(look_ahead)
    start = _start_arg(start, ('given', 'overlap'))
    t, A = _start_rows(S, magnitudes, start, device)
    if t.dim() not in (2, 3):
        raise ValueError('expected a (T, F) spectrogram or a (B, T, F) stack')
    single = t.dim() == 2
    t3 = t[None] if single else t
    t3 = t3.clone() if t3.dtype == torch.complex64 else torch.empty(t3.shape, dtype=torch.complex64, device=t3.device)
    B, T, F = t3.shape
    if F != fsize // 2 + 1:
        raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
    length = _capi.istft_length(T, fsize, fshift, perfectrec)
    back = _capi.stft_frames(length, fsize, fshift, perfectrec)
    if n > 0 and perfectrec and back != T:
        raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, back))
    if A is not None and A.shape != t.shape:
        raise ValueError('magnitudes of shape %s for a spectrogram of shape %s' % (tuple(A.shape), tuple(t.shape)))
    sig = torch.empty((B, max(length, 0)), dtype=torch.float32, device=t3.device) if return_signal else None
    _capi.rtisi_la_dev(t3.data_ptr(), None if A is None else A.data_ptr(), None if sig is None or sig.numel() == 0 else sig.data_ptr(),
                       B, T, fsize, fshift, awin, swin, perfectrec, n, LA, device=int(device),
                       stream=torch.cuda.current_stream(t3.device).cuda_stream, start=start)
    out = t3[0] if single else t3
    return (out, sig[0] if single else sig) if return_signal else out


# --------------------------------------------------------------------------------------------
# Training through RTISI-LA: the gradient of a loss on rtisi_la()'s results under start='given', host fp64 definition and device
# form.  Same convention for complex gradients as misi_grad.  Not covered: start='overlap', online MISI, the streams.
# --------------------------------------------------------------------------------------------
def _rtisi_inv_adjoint(g, fsize, swin):
    """The gradient on c_j, (F,), of a loss whose gradient on f_j = swin irfft(c_j) is g: step 2 of griffin_lim_grad for one frame."""
    c = np.fft.rfft(swin * g) * (2.0 / fsize)
    c[0] = 0.5 * c[0].real
    c[-1] = 0.5 * c[-1].real
    return c


def _rtisi_fwd_adjoint(gX, fsize, awin):
    """The gradient on the fsize samples under a frame of a loss whose gradient on X = rfft(awin y) is gX: step 4 of
    griffin_lim_grad for one frame."""
    G = 0.5 * np.asarray(gX, dtype=np.complex128)
    G[0] = gX[0].real
    G[-1] = gX[-1].real
    return fsize * awin * np.fft.irfft(G, fsize)


def _rtisi_backward(tape, A, grad_out, grad_signal, fsize, fshift, awin, swin, LA, perfectrec=False, _perturb=None):
    """The backward pass of rtisi_la() from a tape of its projections' arguments: tape (B, T, n, min(LA, T-1) + 1, F), row
    [b, m, it-1, j-m] the X of frame j in inner iteration it of commit step m; A (B, T, F); the cotangents grad_out (B, T, F)
    complex and grad_signal (B, len), either None for zeros.  Returns (gA, gS); see rtisi_la_grad, which records the tape and
    calls this."""
    tape, A = np.asarray(tape, dtype=np.complex128), np.asarray(A, dtype=np.float64)
    B, T, F = A.shape
    n = tape.shape[2]
    total, lo, hi = _misi_cuts(T, fsize, fshift, perfectrec)
    hi = max(hi, lo)
    keep = np.zeros(total)
    keep[lo:hi] = 1.0
    gA, gS = np.zeros(A.shape), np.zeros(A.shape, dtype=np.complex128)
    pert = (lambda kind, m, it, b, Z: Z) if _perturb is None else _perturb

    def win(j):
        return slice(fshift * j, fshift * j + fsize)

    for b in range(B):
        gdone = np.zeros(total)
        if grad_signal is not None:
            gdone[lo:hi] = grad_signal[b]
        G = np.zeros(total)
        for m in range(T - 1, -1, -1):
            last = min(m + LA, T - 1)
            if n == 0:
                gS[b, m] = pert('gc', m, 0, b, _rtisi_inv_adjoint(gdone[win(m)], fsize, swin))
                if grad_out is not None:
                    gS[b, m] += grad_out[b, m]
                continue
            for it in range(n, 0, -1):
                Gn = np.zeros(total)
                for j in range(m, last + 1):
                    head = it == n and j == m                       # undoing `done += f_m`
                    gc = pert('gc', m, it, b, _rtisi_inv_adjoint(gdone[win(m)] if head else G[win(j)], fsize, swin))
                    if head and grad_out is not None:
                        gc = gc + grad_out[b, m]
                    ga, gX = _project_backward(tape[b, m, it - 1, j - m], A[b, j], gc)
                    gA[b, j] += ga
                    Gn[win(j)] += np.real(pert('gv', m, it, b, _rtisi_fwd_adjoint(gX, fsize, awin)))
                Gn *= keep                                          # Jacobi: one sum fed every active frame and `done`
                gdone += Gn
                G = Gn
            for j in (range(0, last + 1) if m == 0 else range(m + LA, min(m + LA, T - 1) + 1)):   # the frames that entered in step m
                gS[b, j] = pert('gc', m, 0, b, _rtisi_inv_adjoint(G[win(j)], fsize, swin))
    return gA, gS


def rtisi_la_grad(S, fsize, fshift, awin, swin, iterations, magnitudes, look_ahead=3, grad_out=None, grad_signal=None,
                  perfectrec=False, _perturb=None, _tape=None):
    """The gradient of a loss L on the results of rtisi_la(S, ..., magnitudes=A, return_signal=True, start='given'), in fp64 on the
    host: the definition the device backward pass (rtisi_la_layer) is held to.  grad_out: the cotangent dL/dRe + j dL/dIm of the
    returned spectrogram c, shaped as S, (T, F) or (B, T, F); grad_signal: the real cotangent of the returned signal, (len,) /
    (B, len); either None for zeros.  Returns (gA, gS), the gradients on the magnitudes (real) and on the start S (complex, same
    convention), shaped as S.  A is a variable of its own here: `magnitudes` is required.  Frame m of c and the samples it finalises
    depend on no input frame later than m + look_ahead, so rows of gA and gS later than that get nothing from them.

    With N = fsize, hop = fshift, keep and the cuts lo, hi as in rtisi_la, inv_adj(g) = (w / N) rfft(swin g) (w = 2 on the interior
    bins, 1 and no imaginary part at the bins 0 and N/2) and fwd_adj(gX) = N awin irfft(G) (G = gX / 2 on the interior bins, Re gX
    at the bins 0 and N/2) -- steps 2 and 4 of griffin_lim_grad for one frame -- X[m, it, j] the argument of the projection of frame
    j in inner iteration it of commit step m, and v[j] the samples hop j : hop j + N of a timeline vector v:
      gdone = keep (grad_signal placed at lo:hi)          the gradient on `done`
      G = 0                                               the gradient on f_j is G[j] for every active frame but m
      for m = T-1 .. 0, last = min(m + LA, T-1):
        for it = n .. 1:
          Gn = 0
          for j = m .. last, ascending:
            gf = gdone[m] if (it == n and j == m) else G[j]              undoing `done += f_m`
            gc = inv_adj(gf), plus grad_out[m] if (it == n and j == m)
            u = X / |X|, q = conj(u) gc;  gA[j] += Re q;  gX = j u (A_j / |X|) Im q     (u = 1, gX = 0 where |X| == 0)
            Gn[j] += fwd_adj(gX)
          Gn *= keep;  gdone += Gn;  G = Gn               Jacobi: one sum fed every active frame and `done`
        gS[j] = inv_adj(G[j]) for the frames j that entered in step m (0 .. last at m == 0, else m + LA if that is a frame)
    Because every active frame is projected from one sum, the gradients on all f_j are windows of ONE timeline vector.  The
    perfectrec cuts carry no gradient.  Zero iterations: gA = 0, gS[m] = grad_out[m] + inv_adj(gdone[m]), the adjoint of istft.
    (_perturb(kind, m, it, b, Z) -> Z: replaces each stacked projection argument, kind 'X'; each result of inv_adj, kind 'gc' (it
    = 0 for the rows of gS); each result of fwd_adj, kind 'gv', of which the real part is taken.  The error model of the tests.
    _tape: (T, n, W, F) / (B, T, n, W, F) with W = min(look_ahead, T - 1) + 1, row [m, it-1, j-m] the X above, from elsewhere -- a
    device run's -- instead of this function's own forward pass: the backward pass alone, teacher-forced.  Rows beyond `last` are
    not read.)"""
    n, _ = _gla_args(iterations, 0.0)
    LA = _look_ahead_arg(look_ahead)

    def plan(S3, A3, single):
        B, T, F = S3.shape
        if F != fsize // 2 + 1 or fsize % 2:
            raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
        wa, ws = np.asarray(awin, dtype=np.float64), np.squeeze(np.asarray(swin, dtype=np.float64))
        _, lo, hi = _misi_cuts(T, fsize, fshift, perfectrec)
        length = max(hi - lo, 0)
        if perfectrec is True and n > 0:
            back = stft(np.zeros(length), fsize, fshift, wa, perfectrec=True).shape[0]
            if back != T:
                raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, back))
        tape = np.zeros((B, T, n, min(LA, T - 1) + 1, F), dtype=np.complex128)

        def record(m, it, b, X):
            if _perturb is not None:
                X = _perturb('X', m, it, b, X)
            tape[b, m, it - 1, :X.shape[0]] = X
            return X

        def forward():
            rtisi_la(S3, fsize, fshift, wa, ws, n, look_ahead=LA, magnitudes=A3, perfectrec=perfectrec, _perturb=record)

        def backward(gC, gx):
            return _rtisi_backward(tape, A3, gC, gx, fsize, fshift, wa, ws, LA, perfectrec=perfectrec, _perturb=_perturb)

        return tape, forward, backward, length, 'grad_signal'

    return _grad_call('rtisi_la_grad', False, S, magnitudes, grad_out, grad_signal, _tape, plan)


_RTISI_LAYER = _Layer(
    2, True, lambda n, dims, extra: (dims[0], dims[1], n, min(extra[0], dims[1] - 1) + 1, dims[2]),
    lambda p, dims, mid, extra, kw: _capi.rtisi_la_tape_dev(p.C, p.A, p.sig, *dims[:2], *mid, extra[0], p.tape, **kw),
    lambda p, dims, mid, extra, kw: _capi.rtisi_la_backward_dev(p.gC, p.gs, p.A, p.tape, *dims[:2], *mid, extra[0], p.gA, p.gS, **kw))


def rtisi_la_layer(A, S, fsize, fshift, awin, swin, iterations, look_ahead=3, perfectrec=False, return_signal=False):
    """rtisi_la_dev(S, ..., magnitudes=A, return_signal=True) as a differentiable torch operation, for training a model through the
    causal iteration it will run under at inference: returns C, the committed spectrogram, or with return_signal (C, x), with the
    bits rtisi_la_dev gives them, and loss.backward() reaches whichever of A and S require grad (the other gets None), from a loss
    on C, on x or on both.  Takes device tensors, A float32 and S complex64 of shape (T, F) or (B, T, F); does not modify them; runs
    on the current torch stream and only enqueues work, forward and backward.  Once differentiable.  The forward pass keeps the
    argument of every projection for the backward pass: a complex64 tape of iterations * (LA + 1) times the size of S (LA the
    look-ahead, at most T - 1), held by the autograd graph until backward() has run (or the results are dropped).  The backward
    pass is one launch, one workgroup per spectrogram marching over the frames from the last to the first (k_rtisi_bwd of
    lws_gla.hip), and repeats bit for bit; its definition is rtisi_la_grad.  Zero iterations: C is a copy of S.  Not covered:
    start='overlap', online MISI and the stream classes.  Raises ValueError, as rtisi_la_dev does, for a frame count the round
    trip does not keep."""
    n, _ = _gla_args(iterations, 0.0)
    LA = _look_ahead_arg(look_ahead)
    awin, swin = _layer_args(A, S, fsize, fshift, awin, swin, n, perfectrec, round_trip_always=False, squeeze_swin=True)
    C, x = _layer_apply(_RTISI_LAYER, A, S, None, fsize, fshift, awin, swin, n, perfectrec, LA)
    return (C, x) if return_signal else C


# --------------------------------------------------------------------------------------------
# Online MISI: the K sources of a known mixture under a look-ahead -- MISI as RTISI-LA is Griffin-Lim
# --------------------------------------------------------------------------------------------
def misi_la(S, mixture, fsize, fshift, awin, swin, iterations, look_ahead=3, magnitudes=None, perfectrec=False, return_signals=False,
            _perturb=None, open_end=False, start='given'):
    """MISI under a look-ahead from the starts S, (K, T, F) or a stack (B, K, T, F), and the real mixture(s) `mixture`, (len,) /
    (B, len) with len that of istft(S[k]), in fp64 on the host: the definition the device form is held to.  Frame m of every
    source depends on no input frame later than m + look_ahead and on no mixture sample behind the end of that frame.  On the
    timeline and with inv, fwd and the cuts of rtisi_la(), the mixture y sitting where istft would put it, and with
    g_l = (sum_{j <= l} w) / (sum_j w), w = awin swin shifted to the frames that cover a sample (j ascending; 1 where the
    denominator is 0) -- the share of a sample's overlap-add weight that has entered -- the frames m = 0 .. T-1 are committed in
    order: every frame up to last = min(m + look_ahead, T - 1) that has not entered does, f_kj = inv(c_kj) for every source;
    `iterations` times, from the same iterate (Jacobi over frames and sources), y_k = done_k + sum_{j = m..last} f_kj (j ascending),
    e = g_last y - sum_k y_k (k ascending), c_kj = A_kj X / |X| with X = fwd((y_k + e / K)[fshift j : fshift j + fsize]) (A_kj + 0j
    where |X| == 0), f_kj = inv(c_kj); then done_k += f_km for good.  Returns c (its magnitudes are A = `magnitudes`, by default
    |S|); zero iterations return S.  With look_ahead >= T - 1 the first commit is `iterations` steps of misi().  At
    look_ahead = 0 the last active frame is always transformed from a partial sum and the iteration moves away from a good
    start, as RTISI itself does.  return_signals: also s_k = done_k + (y - sum_j done_j) / K cut as istft cuts it, (K, len) /
    (B, K, len), which sum to the mixture.
    open_end: nothing a step with m + look_ahead <= T - 1 computes depends on where the input ends, so the rows [:, :T1 - look_ahead]
    of a run on S[:, :T1] and the mixture under those frames are those of a run on any longer input: what a stream (MisiLaStream)
    computes.  The mixture then has fshift (T - 1) + fsize - lo samples, lo the lead-in perfectrec cuts (else 0): every sample under
    the frames, with perfectrec the fsize - fshift more that stft reads behind what istft returns.  The tail is not read as zero
    inside the iteration (the lead-in still is, and the returned signals are still cut as istft cuts them), the frame count need not
    be one the round trip keeps, and the denominator of g sums w over ALL frames j >= 0 that would cover a sample, as if the input
    never ended, in the steps with m + look_ahead <= T - 1; in the later ones, which know the end, over the frames 0 .. T-1 as
    without open_end, so that g = 1 there and the last frames explain the whole mixture.
    start: how a frame enters.  'given' (the default): from S, as above.  'mixture': with the phase of the mixture, from magnitudes
    alone -- frame j of every source takes c_kj = A_kj X / |X| (A_kj + 0j where |X| == 0) with X = fwd(keep y[fshift j :
    fshift j + fsize]), one transform for all sources, y on the timeline as placed and cut above (open_end included).  Only A is
    read -- the phases of S are not, and S may be a real array -- and zero iterations return these rows, not S.  An entry does not
    depend on the state, so this is misi_la(S0, ...) with S0 built the same way.
    (_perturb(m, it, b, X) -> X: replaces the (K, last - m + 1, F) stack of projections of one inner iteration, and with it = 0 and
    the (1, 1, F) transform that of an entering frame; the error model of the tests.)"""
    n, _ = _gla_args(iterations, 0.0)
    LA = _look_ahead_arg(look_ahead)
    mix = _start_arg(start, ('given', 'mixture')) == 'mixture'
    S = np.asarray(S)
    if S.ndim not in (3, 4):
        raise ValueError('expected (K, T, F) spectrograms of the sources or a (B, K, T, F) stack')
    A = np.abs(S) if magnitudes is None else np.asarray(magnitudes, dtype=np.float64)
    if A.shape != S.shape:
        raise ValueError('magnitudes of shape %s for spectrograms of shape %s' % (A.shape, S.shape))
    y = np.asarray(mixture, dtype=np.float64)
    S4, A4, y2 = (S[None], A[None], y[None]) if S.ndim == 3 else (S, A, y)
    B, K, T, F = S4.shape
    if K < 1:
        raise ValueError('no sources')
    if F != fsize // 2 + 1 or fsize % 2:
        raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
    awin, swin = np.asarray(awin, dtype=np.float64), np.squeeze(np.asarray(swin, dtype=np.float64))
    total = fshift * (T - 1) + fsize
    keep = np.ones(total)
    lo, hi = 0, total
    if perfectrec is True:
        lo, hi = _perfectrec_prepad(fsize, fshift), total - (fsize - fshift)
        keep[:lo] = 0.0
        if not open_end:
            keep[max(hi, 0):] = 0.0
            back = stft(np.zeros(max(hi - lo, 0)), fsize, fshift, awin, perfectrec=True).shape[0]
            if n > 0 and back != T:
                raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, back))
    length = max(hi - lo, 0)            # of the returned signals
    ylen = total - lo if open_end else length
    if y.ndim != S.ndim - 2 or y2.shape != (B, ylen):
        raise ValueError('mixture of shape %s for %s spectrograms of %d frames: expected %s' %
                         (y.shape, S.shape[:-2], T, S.shape[:-3] + (ylen,)))
    w = awin * swin
    den = np.zeros(total)
    for j in range(T):
        den[fshift * j: fshift * j + fsize] += w
    den_open = den
    if open_end:   # over every frame j >= 0 that would cover a sample: the frames behind T - 1 too
        den_open = np.zeros(total + fsize)
        for j in range(T + (fsize - 1) // fshift):
            den_open[fshift * j: fshift * j + fsize] += w[:max(0, min(fsize, total + fsize - fshift * j))]
        den_open = den_open[:total]
    out = (A4 + 0j) if mix else S4.astype(np.complex128)
    sig = np.empty((B, K, length))
    for b in range(B if (n > 0 or return_signals or mix) else 0):
        c, done, f, entered = out[b], np.zeros((K, total)), np.zeros((K, T, fsize)), 0
        yfull, num = np.zeros(total), np.zeros(total)
        yfull[lo: lo + ylen] = y2[b]
        for m in range(T):
            last = min(m + LA, T - 1)
            while entered <= last:
                if mix:
                    X = np.fft.rfft(awin * (keep * yfull)[fshift * entered: fshift * entered + fsize])[None, None]
                    if _perturb is not None:
                        X = _perturb(m, 0, b, X)
                    c[:, entered] = _project(X[0], A4[b, :, entered])
                for k in range(K):
                    f[k, entered] = swin * np.fft.irfft(c[k, entered], fsize)
                num[fshift * entered: fshift * entered + fsize] += w
                entered += 1
            dn = den_open if m + LA <= T - 1 else den
            target = keep * np.where(dn != 0, num / np.where(dn != 0, dn, 1.0), 1.0) * yfull
            for it in range(1, n + 1):
                yk = done.copy()
                for j in range(m, last + 1):
                    yk[:, fshift * j: fshift * j + fsize] += f[:, j]
                yk *= keep
                tot = yk[0].copy()
                for k in range(1, K):
                    tot += yk[k]
                x = yk + keep * (target - tot) / K
                X = np.stack([[np.fft.rfft(awin * x[k, fshift * j: fshift * j + fsize]) for j in range(m, last + 1)]
                              for k in range(K)])
                if _perturb is not None:
                    X = _perturb(m, it, b, X)
                c[:, m: last + 1] = _project(X, A4[b, :, m: last + 1])
                for k in range(K):
                    for j in range(m, last + 1):
                        f[k, j] = swin * np.fft.irfft(c[k, j], fsize)
            done[:, fshift * m: fshift * m + fsize] += f[:, m]
        tot = done[0].copy()
        for k in range(1, K):
            tot += done[k]
        sig[b] = (keep * done + keep * (yfull - tot) / K)[:, lo: lo + length]
    if n == 0 and not mix:
        out = S4
    if S.ndim == 3:
        out, sig = out[0], sig[0]
    return (out, sig) if return_signals else out


def misi_la_dev(S, mixture, fsize, fshift, awin, swin, iterations, look_ahead=3, magnitudes=None, perfectrec=False,
                return_signals=False, device=0, start='given'):
    """misi_la() above on the device (lws_gla.hip: float32, one workgroup per mixture marching over the frames, its sources one
    after another, the state in LDS when it fits; one launch): S (K, T, F) or (B, K, T, F) and mixture (len,) / (B, len), numpy or
    torch; returns a new complex64 torch tensor (S itself is not modified), and with return_signals also the float32 signals
    (K, len) / (B, K, len).  Runs on the caller's current torch stream and only enqueues work.  start: 'given', or 'mixture' for the
    phase of the mixture from magnitudes alone (S real or complex, its phases not read), as misi_la() defines it.  Raises ValueError,
    as misi_la() does, for a frame count the round trip does not keep."""
    import torch
    n, _ = _gla_args(iterations, 0.0)
    LA = _look_ahead_arg(look_ahead)
    start = _start_arg(start, ('given', 'mixture'))
    t, A = _start_rows(S, magnitudes, start, device)
    if t.dim() not in (3, 4):
        raise ValueError('expected (K, T, F) spectrograms of the sources or a (B, K, T, F) stack')
    single = t.dim() == 3
    t4 = t[None] if single else t
    t4 = t4.clone() if t4.dtype == torch.complex64 else torch.empty(t4.shape, dtype=torch.complex64, device=t4.device)
    B, K, T, F = t4.shape
    if K < 1:
        raise ValueError('no sources')
    if F != fsize // 2 + 1:
        raise ValueError('frames of %d samples have %d bins, got %d' % (fsize, fsize // 2 + 1, F))
    if A is not None and A.shape != t.shape:
        raise ValueError('magnitudes of shape %s for spectrograms of shape %s' % (tuple(A.shape), tuple(t.shape)))
    y = _dev_tensor(mixture, torch.float32, device)
    length = max(_capi.istft_length(T, fsize, fshift, perfectrec), 0)
    if y.dim() != t.dim() - 2 or tuple(y.shape)[-1:] != (length,) or (not single and y.shape[0] != B):
        raise ValueError('mixture of shape %s for %s spectrograms of %d frames: expected %s' %
                         (tuple(y.shape), tuple(t.shape[:-2]), T, tuple(t.shape[:-3]) + (length,)))
    back = _capi.stft_frames(length, fsize, fshift, perfectrec)
    if n > 0 and perfectrec and back != T:
        raise ValueError('the round trip turns %d frames into %d (too few frames for perfectrec)' % (T, back))
    sig = torch.empty((B, K, length), dtype=torch.float32, device=t4.device) if return_signals else None
    _capi.misi_la_dev(t4.data_ptr(), None if A is None else A.data_ptr(), y.data_ptr(),
                      None if sig is None or sig.numel() == 0 else sig.data_ptr(), B, K, T, fsize, fshift, awin, swin, perfectrec, n,
                      LA, device=int(device), stream=torch.cuda.current_stream(t4.device).cuda_stream, start=start)
    out = t4[0] if single else t4
    return (out, sig[0] if single else sig) if return_signals else out


class MisiLaStream(_LaStream):
    """misi_la_dev() for frames and mixture that arrive over time (k_misi_la_stream of lws_gla.hip).  push() takes the next rows of the
    K sources, (K, Tc, F) -- or (B, K, Tc, F) for `batch`=B mixtures side by side -- and the next samples_needed(Tc) samples of the
    mixture, (n,) / (B, n), numpy or torch: after M frames the stream has every mixture sample under them, fshift (M - 1) + fsize
    less the lead-in perfectrec cuts, so the first push carries fsize - fshift more than the later ones per frame and, with
    perfectrec, the last the fsize - fshift zeros stft pads with (or the real continuation).  It returns the rows that could be
    committed, a new complex64 torch tensor (K, n_f, F) / (B, K, n_f, F): frame m is committed once frame m + look_ahead has been
    pushed, so n_f may be 0.  finish() returns the remaining look_ahead frames and ends the stream.  With return_signals both also
    return the float32 samples those commits finalised, (K, k) / (B, K, k), which sum to the mixture.  Everything returned,
    concatenated, is misi_la(everything pushed, ..., open_end=True) and its signals: however the input is cut into chunks, bit for bit.
    The state lives on the device between calls; a call runs on the caller's current torch stream, only enqueues work and keeps no
    reference to its arguments.  magnitudes: the targets of the pushed rows (default |S|).  iterations=0 returns the pushed rows
    themselves, with the same latency.  start='mixture' drives the stream from magnitudes alone, as misi_la(..., start='mixture') does:
    push(A, mixture) then takes real or complex rows, reads only their magnitudes (or `magnitudes`), and iterations=0 returns the
    entry estimates.  A push with another sample count raises ValueError and leaves the stream as it was.  close() frees the device
    state (also on deletion)."""
    _other_start, _create, _finish, _destroy = 'mixture', _capi.misi_stream_create, _capi.misi_stream_finish, _capi.misi_stream_destroy

    def __init__(self, K, fsize, fshift, awin, swin, iterations, look_ahead=3, perfectrec=False, batch=None, return_signals=False,
                 device=0, start='given'):
        _LaStream.__init__(self, K, fsize, fshift, awin, swin, iterations, look_ahead, perfectrec, batch, return_signals, device, start)
        self.K, self.return_signals = int(K), self._signals
        self._lo = _perfectrec_prepad(self.fsize, self.fshift) if self.perfectrec else 0
        self._entered = 0

    def _need(self, M):
        return 0 if M <= 0 else self.fshift * (M - 1) + self.fsize - self._lo

    def samples_needed(self, Tc):
        """The mixture samples the next push of Tc frames must carry."""
        return self._need(self._entered + int(Tc)) - self._need(self._entered)

    def push(self, S, mixture, magnitudes=None):
        import torch
        if self._h is None or self.finished:
            raise ValueError('push on a stream that has finished or been closed')
        t, A = _start_rows(S, magnitudes, self.start, self.device)
        want = 3 if self.batch is None else 4
        if t.dim() != want or t.shape[-1] != self._F or t.shape[-3] != self.K or (self.batch is not None and t.shape[0] != self._B):
            raise ValueError('expected rows of shape %s, got %s' %
                             ((self.K, 'Tc', self._F) if self.batch is None else (self._B, self.K, 'Tc', self._F), tuple(t.shape)))
        if A is not None and A.shape != t.shape:
            raise ValueError('magnitudes of shape %s for rows of shape %s' % (tuple(A.shape), tuple(t.shape)))
        Tc = t.shape[-2]
        y = _dev_tensor(mixture, torch.float32, self.device)
        ns_in = self.samples_needed(Tc)
        if y.dim() != want - 2 or y.shape[-1] != ns_in or (self.batch is not None and y.shape[0] != self._B):
            raise ValueError('mixture of shape %s for %d more frames after %d: expected %s' %
                             (tuple(y.shape), Tc, self._entered, ((ns_in,) if self.batch is None else (self._B, ns_in))))
        out = torch.empty((self._B, self.K, Tc, self._F), dtype=torch.complex64, device=t.device)
        sig = torch.empty((self._B, self.K, Tc * self.fshift), dtype=torch.float32, device=t.device) if self.return_signals else None
        nf, ns = 0, 0
        if Tc > 0:
            nf, ns = _capi.misi_stream_push(self._h, None if t.dtype != torch.complex64 else t.data_ptr(),
                                            None if A is None else A.data_ptr(), y.data_ptr(), Tc, ns_in,
                                            out.data_ptr(), None if sig is None else sig.data_ptr(),
                                            stream=torch.cuda.current_stream(t.device).cuda_stream)
            self._entered += Tc
        return self._returns(out, sig, nf, ns)


def extspec(S, L, Q):
    """Extended spectrogram: L Hermitian columns each side, Q-1 repeated frames each end (lws.pyx:146-157)."""
    S = np.asarray(S)
    T, F = S.shape
    E = np.zeros((T + 2 * (Q - 1), F + 2 * L), dtype=S.dtype)
    E[Q - 1:Q - 1 + T, L:L + F] = S
    for j in range(1, L + 1):
        E[:, L - j] = np.conjugate(E[:, L + j])
        E[:, F + L - 1 + j] = np.conjugate(E[:, F + L - 1 - j])
    E[:Q - 1] = E[Q - 1]
    E[Q - 1 + T:] = E[Q - 2 + T]
    return E


# --------------------------------------------------------------------------------------------
# weights (lws.pyx:160-206)
# --------------------------------------------------------------------------------------------
def create_weights(awin, swin, fshift, L, use_summarized_weights=True):
    """Complex LWS weights, shape (Qprime, Q, L+1) (lws.pyx:160-181).

    W[p, q, l] = exp(2j*pi*p*q/Qf) * exp(-2j*pi*l*q/Qf) * sum_t awin[t]*swin[t+q*fshift]/T * exp(-2j*pi*l*t/T)
    with 1 subtracted from the (q=0, l=0) term; Qf = T/fshift; Qprime = Q when the shift divides the
    window and summarised weights are requested, else T.
    """
    awin = np.asarray(awin, dtype=np.float64)
    swin = np.asarray(swin, dtype=np.float64)
    T = len(awin)
    Q = int(math.ceil(float(T) / float(fshift)))
    Qf = float(T) / float(fshift)
    Qprime = Q if (T % fshift == 0 and use_summarized_weights) else T
    lag = np.arange(L + 1)[:, None]
    prod = np.zeros((T, Q))
    for q in range(Q):
        n = T - q * fshift
        prod[:n, q] = awin[:n] * swin[q * fshift:q * fshift + n] / T
    base = np.exp(-2j * np.pi * lag * np.arange(T)[None, :] / T).dot(prod)      # (L+1, Q)
    base = base * np.exp(-2j * np.pi * lag * np.arange(Q)[None, :] / Qf)
    base[0, 0] -= 1
    twiddle = np.exp(2j * np.pi * np.arange(Qprime)[:, None] * np.arange(Q)[None, :] / Qf)  # (Qprime, Q)
    W = base[:, None, :] * twiddle[None, :, :]                                  # (L+1, Qprime, Q)
    return np.ascontiguousarray(W.transpose(1, 2, 0))


def build_asymmetric_windows(awin_swin, fshift):
    """Mirrored envelopes of RTISI-LA from the analysis*synthesis product (lws.pyx:184-200)."""
    awin_swin = np.asarray(awin_swin, dtype=np.float64)
    T = len(awin_swin)
    Q = int(math.ceil(float(T) / float(fshift)))
    shifted = np.zeros((T, Q))
    for q in range(Q):
        n = T - q * fshift
        shifted[:n, q] = awin_swin[q * fshift:q * fshift + n]
    win_ai = shifted[:, 1:].sum(axis=1)[::-1]
    win_af = shifted.sum(axis=1)[::-1]
    if T % fshift == 2:  # kept verbatim from lws.pyx:198 (the MATLAB binding tests Q == 2 instead)
        win_ai = awin_swin
    return win_ai, win_af


def get_thresholds(iterations, alpha, beta, gamma):
    """alpha * exp(-beta * i**gamma), i = 0..iterations-1 (lws.pyx:203-206)."""
    return alpha * np.exp(-beta * np.arange(iterations) ** gamma)


# --------------------------------------------------------------------------------------------
# the hot path (lws.pyx:209-375) -> HIP engine
# --------------------------------------------------------------------------------------------
_PLAN_DEFAULTS = {"device": 0, "precision": "fp32", "nofuture_q4_compat": True, "force_generic": False, "storage": "fp32"}

# The reference's module-level functions take the weights with every call (lws.pyx:209,261,314) and user code calls them
# in loops over spectrograms; a device plan (weight upload, table analysis, scratch, events) per call would dominate small
# calls, so the last few plans are kept, keyed by the weights' bytes and the plan options.  `clear_plan_cache()` releases
# their device memory.  Precision: the engine computes in fp32 by default (`precision="fp64"` selects the reference's
# arithmetic: batch sweeps of Q = 2 / 4 plans on the fp64 systolic engine, lws_sys64.hip, everything else -- and everything
# with `force_generic=True` -- on the order-exact generic engine; tolerances in DESIGN.md section 6); complex128 in, complex128
# out either way.
_PLAN_CACHE_SIZE = 4
# One cache per calling thread: the bindings release the GIL around the C call and an lws_plan (scratch, events, stage
# buffers) serves one call at a time, so a plan shared between threads could be used -- or evicted and destroyed -- while
# another thread is inside the library with it.  A thread's plans die with the thread (Plan.__del__).
_plan_tls = threading.local()


def _thread_cache():
    cache = getattr(_plan_tls, "cache", None)
    if cache is None:
        cache = _plan_tls.cache = collections.OrderedDict()
    return cache


def _cached_plan(F, Ws, plan_kw):
    kw = {**_PLAN_DEFAULTS, **plan_kw}
    key = (int(F),) + tuple(None if w is None else (w.shape, hashlib.sha1(np.ascontiguousarray(w, dtype=np.complex128).tobytes()).hexdigest())
                            for w in Ws) + tuple(sorted(kw.items()))
    cache = _thread_cache()
    plan = cache.pop(key, None)
    if plan is None:
        plan = _capi.Plan(F, *Ws, **kw)
        while len(cache) >= _PLAN_CACHE_SIZE:
            cache.popitem(last=False)[1].close()   # (this thread's own plan, and it is not inside a call)
    cache[key] = plan          # most recently used last
    return plan


def clear_plan_cache():
    """Destroy the calling thread's plans kept for the module-level batch_lws / nofuture_lws / online_lws (frees their
    device memory)."""
    cache = _thread_cache()
    while cache:
        cache.popitem()[1].close()


def _prepare(S, W, use_simplifications, n_extra_w=()):
    """Argument handling shared by the three wrappers (lws.pyx:212-224)."""
    S = np.asarray(S)
    if S.dtype != np.complex128:
        S = S.astype(np.complex128)
    W = np.asarray(W)
    Qp, Q = W.shape[0], W.shape[1]
    F = S.shape[-1]
    return S, W, Qp, Q, F


def _check(S, W, Qp, Q, F, use_simplifications):
    if F % 2 == 0:
        raise ValueError('Please only include non-negative frequencies in the input spectrogram.')
    if Qp != Q and Qp != 2 * (F - 1):
        raise ValueError('Weights have %d rows: expected Q=%d (summarized) or N=%d (general).' % (Qp, Q, 2 * (F - 1)))
    if Qp == Q and not use_simplifications:
        # the reference would index a Q-row tensor with the bin number here (undefined behaviour)
        raise ValueError('use_simplifications=False needs general weights '
                         '(create_weights(..., use_summarized_weights=False)).')


def batch_lws(S, W, thresholds, use_simplifications=True, **plan_kw):
    """Batch LWS (lws.pyx:209-258): ``len(thresholds)`` in-place Gauss-Seidel sweeps."""
    S, W, Qp, Q, F = _prepare(S, W, use_simplifications)
    if len(thresholds) == 0:
        return S
    _check(S, W, Qp, Q, F, use_simplifications)
    return _cached_plan(F, (W, None, None), plan_kw).batch(S, thresholds)


def nofuture_lws(S, W, thresholds, use_simplifications=True, **plan_kw):
    """LWS using past frames only (lws.pyx:261-311); for Q == 4 the default reproduces the
    reference's NoFuture_LWSQ4 addressing (pass ``nofuture_q4_compat=False`` for the anyQ semantics)."""
    S, W, Qp, Q, F = _prepare(S, W, use_simplifications)
    if len(thresholds) == 0:
        return S
    _check(S, W, Qp, Q, F, use_simplifications)
    return _cached_plan(F, (W, None, None), plan_kw).nofuture(S, thresholds)


def online_lws(S, W, W_ai, W_af, thresholds, LA, fshift, use_simplifications=True, **plan_kw):
    """Online LWS / TF-RTISI-LA (lws.pyx:314-375)."""
    thresholds = np.asarray(thresholds, dtype=np.float64)
    if thresholds.ndim != 1:
        raise ValueError('Buffer has wrong number of dimensions (expected 1, got %d)' % thresholds.ndim)
    S, W, Qp, Q, F = _prepare(S, W, use_simplifications)
    if len(thresholds) == 0:
        return S
    _check(S, W, Qp, Q, F, use_simplifications)
    qdiv = float(2 * (F - 1) / int(fshift))  # lws.pyx:339
    return _cached_plan(F, (W, np.asarray(W_ai), np.asarray(W_af)), plan_kw).online(S, thresholds, int(LA), qdiv)


# ---- construction of an lws object: helpers ------------------------------------------------------------------------------
# (the keyword surface, defaults, printed notices and attribute names are the reference's interface, lws.pyx:379-455)
_STAGES = ("nofuture", "online", "batch")
_SCHEDULE_KEYS = ("iterations", "alpha", "beta", "gamma")
# what `mode` overrides (lws.pyx:437-442): stage -> iterations
_MODES = {None: {}, "speech": {"nofuture": 0, "online": 0}, "music": {"nofuture": 1, "online": 10}}


def _resolve_windows(awin_or_fsize, fshift, swin, fftsize, symmetric_win):
    """Analysis window (a frame size stands for the reference's default window: the square root of a Hann window,
    renormalised with its synthesis partner) zero-padded symmetrically to `fftsize`, and the synthesis window the caller
    passed, padded the same way.  Returns (awin, swin or None, padded samples per side)."""
    if isinstance(awin_or_fsize, (int, np.integer)):
        root = np.sqrt(hann(int(awin_or_fsize), symmetric=symmetric_win, use_offset=False))
        awin = np.sqrt(root * synthwin(root, fshift))
    else:
        awin = np.asarray(awin_or_fsize)
        if awin.ndim > 1:   # (lws.pyx:391 compares a shape tuple with an int -- a TypeError on Python 3; the intent is clear)
            if awin.ndim > 2 or min(awin.shape) > 1:
                raise ValueError('The analysis window should be flat')
            awin = awin.ravel()
    extra = 0 if fftsize is None else int(fftsize) - len(awin)
    if extra <= 0:
        return awin, swin, 0
    if extra % 2:
        raise ValueError('The zero-padding should add even length to the original window.')
    side = np.zeros(extra // 2)
    return np.hstack((side, awin, side)), (None if swin is None else np.hstack((side, swin, side))), extra // 2


class lws(object):
    """Configuration object of the reference (lws.pyx:378-499), same keyword arguments."""

    def __init__(self, awin_or_fsize, fshift, L=5, swin=None, look_ahead=3,
                 nofuture_iterations=0, nofuture_alpha=1, nofuture_beta=0.1, nofuture_gamma=1,
                 online_iterations=0, online_alpha=1, online_beta=0.1, online_gamma=1,
                 batch_iterations=100, batch_alpha=100, batch_beta=0.1, batch_gamma=1,
                 symmetric_win=True, mode=None, fftsize=None, perfectrec=True, use_simplifications=True,
                 device=0, precision="fp32", nofuture_q4_compat=True, force_generic=False, storage="fp32"):
        schedule = {"nofuture": (nofuture_iterations, nofuture_alpha, nofuture_beta, nofuture_gamma),
                    "online": (online_iterations, online_alpha, online_beta, online_gamma),
                    "batch": (batch_iterations, batch_alpha, batch_beta, batch_gamma)}
        # windows
        awin, swin_given, padded = _resolve_windows(awin_or_fsize, fshift, swin, fftsize, symmetric_win)
        if padded:
            print('Zero-padding symmetrically around the original windows.\n'
                  'WARNING: for code simplicity, a consequence is that the first/last '
                  '{} samples of the signal will not be '.format(padded) +
                  'in the perfect reconstruction region.')
        if swin_given is not None:
            print('Provided synthesis window is renormalized for perfect reconstruction.')
        self.awin, self.fshift, self.fsize = awin, fshift, len(awin)
        self.swin = synthwin(awin, fshift, swin=swin_given)
        self.perfectrec, self.L, self.use_simplifications, self.look_ahead = perfectrec, L, use_simplifications, look_ahead
        q = self.fsize / self.fshift
        self.Q = int(q) if self.fsize % self.fshift == 0 else q
        # weights of the three sweeps: symmetric windows, and the two asymmetric envelopes of RTISI-LA
        self.win_ai, self.win_af = build_asymmetric_windows(self.awin * self.swin, self.fshift)
        for attr, win in (("W", self.awin), ("W_ai", self.win_ai), ("W_af", self.win_af)):
            setattr(self, attr, create_weights(win, self.swin, self.fshift, self.L, use_summarized_weights=use_simplifications))
        # schedules: <stage>_iterations / _alpha / _beta / _gamma; `mode` presets the first two stages
        if mode not in _MODES:
            mode = None          # (the reference ignores an unknown mode)
        for stage in _STAGES:
            values = list(schedule[stage])
            if stage in _MODES[mode]:
                values[0] = _MODES[mode][stage]
            for key, value in zip(_SCHEDULE_KEYS, values):
                setattr(self, "%s_%s" % (stage, key), value)
        if not np.allclose(awin, awin[::-1]):
            print('WARNING: It appears you are using an analysis window that is not symmetric.\n'
                  'The current code uses simplifications that rely on such symmetry, so the code may not behave properly.')
        self.device = int(device)
        self._plan_kw = dict(device=device, precision=precision, nofuture_q4_compat=nofuture_q4_compat,
                             force_generic=force_generic, storage=storage)
        self._plan = None

    # -- engine plumbing (not part of the reference surface) --
    def plan(self):
        """The cached device plan holding W, W_ai, W_af for this configuration."""
        if self._plan is None:
            self._plan = _capi.Plan(self.fsize // 2 + 1, self.W, self.W_ai, self.W_af, **self._plan_kw)
        return self._plan

    def _qdiv(self):
        return float(self.fsize / self.fshift)

    def _as_c128(self, S):
        S = np.asarray(S)
        return S if S.dtype == np.complex128 else S.astype(np.complex128)

    def _check(self, S):
        F = S.shape[-1]
        if F % 2 == 0:
            raise ValueError('Please only include non-negative frequencies in the input spectrogram.')
        if F != self.fsize // 2 + 1:
            raise ValueError('This lws object works on %d-bin spectrograms, got %d.' % (self.fsize // 2 + 1, F))

    # -- reference surface --
    def get_consistency(self, S):
        return get_consistency(S, self.fsize, self.fshift, self.awin, self.swin, perfectrec=self.perfectrec)

    def stft(self, S):
        return stft(S, self.fsize, self.fshift, self.awin, perfectrec=self.perfectrec)

    # ---- device versions of the three helpers above (float32 transforms; any even frame size in 32..4096).
    # Arguments are torch CUDA tensors (complex64 spectrograms (B, T, F) / float32 signals (B, len)) or numpy arrays,
    # which are moved to the plan's device through torch -- PyTorch is only the owner of the device memory here.
    def _to_dev(self, a, dtype):
        import torch
        dev = torch.device("cuda", self.device)
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=dev, dtype=dtype).contiguous()

    def get_consistency_dev(self, S):
        """Consistency in dB of each spectrogram of the stack S (B, T, F) or of the single spectrogram (T, F), computed
        on the device (lws.pyx:140-144)."""
        import torch
        t = self._to_dev(S, torch.complex64)
        single = t.dim() == 2
        if single:
            t = t[None]
        sums = _capi.consistency_dev(t.data_ptr(), t.shape[0], t.shape[1], self.fsize, self.fshift, self.awin, self.swin,
                                     self.perfectrec, device=self.device,
                                     stream=torch.cuda.current_stream(t.device).cuda_stream)
        db = 10 * np.log10(sums[:, 0] / sums[:, 1])
        return float(db[0]) if single else db

    def stft_dev(self, x):
        """STFT of the signals x (B, len) (or one signal (len,)) on the device: complex64 torch tensor (B, T, F)."""
        import torch
        t = self._to_dev(x, torch.float32)
        single = t.dim() == 1
        if single:
            t = t[None]
        B, n = t.shape
        T = _capi.stft_frames(n, self.fsize, self.fshift, self.perfectrec)
        out = torch.empty((B, T, self.fsize // 2 + 1), dtype=torch.complex64, device=t.device)
        _capi.stft_dev(t.data_ptr(), B, n, self.fsize, self.fshift, self.awin, self.perfectrec, out.data_ptr(),
                       device=self.device, stream=torch.cuda.current_stream(t.device).cuda_stream)
        return out[0] if single else out

    def istft_dev(self, S):
        """Inverse STFT of the spectrograms S (B, T, F) (or one (T, F)) on the device: float32 torch tensor (B, len)."""
        import torch
        t = self._to_dev(S, torch.complex64)
        single = t.dim() == 2
        if single:
            t = t[None]
        B, T, _ = t.shape
        n = _capi.istft_length(T, self.fsize, self.fshift, self.perfectrec)
        out = torch.empty((B, n), dtype=torch.float32, device=t.device)
        _capi.istft_dev(t.data_ptr(), B, T, self.fsize, self.fshift, self.swin, self.perfectrec, out.data_ptr(),
                        device=self.device, stream=torch.cuda.current_stream(t.device).cuda_stream)
        return out[0] if single else out

    def istft(self, S):
        return istft(S, self.fshift, self.swin, perfectrec=self.perfectrec)

    # ---- Griffin-Lim refinement of a phase estimate, e.g. of what run_lws returned (no counterpart in the reference) ----
    def griffin_lim(self, S, iterations, alpha=0.99, magnitudes=None, return_trace=False):
        """Host fp64 form with this object's windows and perfectrec: see the module's griffin_lim."""
        return griffin_lim(S, self.fsize, self.fshift, self.awin, self.swin, iterations, alpha=alpha, magnitudes=magnitudes,
                           perfectrec=self.perfectrec, return_trace=return_trace)

    def griffin_lim_dev(self, S, iterations, alpha=0.99, magnitudes=None, return_trace=False):
        """Device form: a new complex64 torch tensor, see the module's griffin_lim_dev."""
        return griffin_lim_dev(S, self.fsize, self.fshift, self.awin, self.swin, iterations, alpha=alpha, magnitudes=magnitudes,
                               perfectrec=self.perfectrec, return_trace=return_trace, device=self.device)

    # ---- MISI: the phases of K sources under the constraint that they add up to a known mixture ----
    def misi(self, S, mixture, iterations, magnitudes=None, return_trace=False, return_signals=False):
        """Host fp64 form with this object's windows and perfectrec: see the module's misi."""
        return misi(S, mixture, self.fsize, self.fshift, self.awin, self.swin, iterations, magnitudes=magnitudes,
                    perfectrec=self.perfectrec, return_trace=return_trace, return_signals=return_signals)

    def misi_dev(self, S, mixture, iterations, magnitudes=None, return_trace=False, return_signals=False):
        """Device form: a new complex64 torch tensor, see the module's misi_dev."""
        return misi_dev(S, mixture, self.fsize, self.fshift, self.awin, self.swin, iterations, magnitudes=magnitudes,
                        perfectrec=self.perfectrec, return_trace=return_trace, return_signals=return_signals, device=self.device)

    def misi_grad(self, S, mixture, iterations, magnitudes, grad_out=None, grad_signals=None):
        """Host fp64 gradient through misi with this object's windows and perfectrec: (gA, gS, gy), see the module's misi_grad."""
        return misi_grad(S, mixture, self.fsize, self.fshift, self.awin, self.swin, iterations, magnitudes, grad_out=grad_out,
                         grad_signals=grad_signals, perfectrec=self.perfectrec)

    def griffin_lim_grad(self, S, iterations, magnitudes, alpha=0.99, grad_out=None):
        """Host fp64 gradient through griffin_lim with this object's windows and perfectrec: (gA, gS), see the module's
        griffin_lim_grad."""
        return griffin_lim_grad(S, self.fsize, self.fshift, self.awin, self.swin, iterations, magnitudes, alpha=alpha,
                                grad_out=grad_out, perfectrec=self.perfectrec)

    def griffin_lim_layer(self, A, S, iterations, alpha=0.99):
        """griffin_lim_dev as a differentiable torch operation on device tensors: C, see the module's griffin_lim_layer."""
        return griffin_lim_layer(A, S, self.fsize, self.fshift, self.awin, self.swin, iterations, alpha=alpha,
                                 perfectrec=self.perfectrec)

    def misi_layer(self, A, S, mixture, iterations):
        """misi_dev as a differentiable torch operation on device tensors: (C, s), see the module's misi_layer."""
        return misi_layer(A, S, mixture, self.fsize, self.fshift, self.awin, self.swin, iterations, perfectrec=self.perfectrec)

    def rtisi_la(self, S, iterations, look_ahead=None, magnitudes=None, return_signal=False, open_end=False, start='given'):
        """Host fp64 form with this object's windows, perfectrec and (look_ahead=None) look-ahead: see the module's rtisi_la."""
        return rtisi_la(S, self.fsize, self.fshift, self.awin, self.swin, iterations,
                        look_ahead=self.look_ahead if look_ahead is None else look_ahead, magnitudes=magnitudes,
                        perfectrec=self.perfectrec, return_signal=return_signal, open_end=open_end, start=start)

    def rtisi_la_dev(self, S, iterations, look_ahead=None, magnitudes=None, return_signal=False, start='given'):
        """Device form: a new complex64 torch tensor, see the module's rtisi_la_dev."""
        return rtisi_la_dev(S, self.fsize, self.fshift, self.awin, self.swin, iterations,
                            look_ahead=self.look_ahead if look_ahead is None else look_ahead, magnitudes=magnitudes,
                            perfectrec=self.perfectrec, return_signal=return_signal, device=self.device, start=start)

    def rtisi_la_grad(self, S, iterations, magnitudes, look_ahead=None, grad_out=None, grad_signal=None):
        """Host fp64 gradient through rtisi_la with this object's windows, perfectrec and (look_ahead=None) look-ahead: (gA, gS),
        see the module's rtisi_la_grad."""
        return rtisi_la_grad(S, self.fsize, self.fshift, self.awin, self.swin, iterations, magnitudes,
                             look_ahead=self.look_ahead if look_ahead is None else look_ahead, grad_out=grad_out,
                             grad_signal=grad_signal, perfectrec=self.perfectrec)

    def rtisi_la_layer(self, A, S, iterations, look_ahead=None, return_signal=False):
        """rtisi_la_dev as a differentiable torch operation on device tensors: C or (C, x), see the module's rtisi_la_layer."""
        return rtisi_la_layer(A, S, self.fsize, self.fshift, self.awin, self.swin, iterations,
                              look_ahead=self.look_ahead if look_ahead is None else look_ahead, perfectrec=self.perfectrec,
                              return_signal=return_signal)

    def rtisi_la_stream(self, iterations, look_ahead=None, batch=None, return_signal=False, start='given'):
        """A RtisiLaStream with the windows, look-ahead and device of this object: push() rows as they arrive, then finish()."""
        return RtisiLaStream(self.fsize, self.fshift, self.awin, self.swin, iterations,
                             look_ahead=self.look_ahead if look_ahead is None else look_ahead, perfectrec=self.perfectrec, batch=batch,
                             return_signal=return_signal, device=self.device, start=start)

    def misi_la(self, S, mixture, iterations, look_ahead=None, magnitudes=None, return_signals=False, open_end=False, start='given'):
        """Host fp64 form with this object's windows, perfectrec and (look_ahead=None) look-ahead: see the module's misi_la."""
        return misi_la(S, mixture, self.fsize, self.fshift, self.awin, self.swin, iterations,
                       look_ahead=self.look_ahead if look_ahead is None else look_ahead, magnitudes=magnitudes,
                       perfectrec=self.perfectrec, return_signals=return_signals, open_end=open_end, start=start)

    def misi_la_dev(self, S, mixture, iterations, look_ahead=None, magnitudes=None, return_signals=False, start='given'):
        """Device form: a new complex64 torch tensor, see the module's misi_la_dev."""
        return misi_la_dev(S, mixture, self.fsize, self.fshift, self.awin, self.swin, iterations,
                           look_ahead=self.look_ahead if look_ahead is None else look_ahead, magnitudes=magnitudes,
                           perfectrec=self.perfectrec, return_signals=return_signals, device=self.device, start=start)

    def misi_la_stream(self, K, iterations, look_ahead=None, batch=None, return_signals=False, start='given'):
        """A MisiLaStream for K sources with the windows, look-ahead and device of this object: push() rows and mixture samples as
        they arrive, then finish()."""
        return MisiLaStream(K, self.fsize, self.fshift, self.awin, self.swin, iterations,
                            look_ahead=self.look_ahead if look_ahead is None else look_ahead, perfectrec=self.perfectrec, batch=batch,
                            return_signals=return_signals, device=self.device, start=start)

    def nofuture_lws(self, S, iterations=None, thresholds=None):
        if iterations is None:
            iterations = self.nofuture_iterations
        if thresholds is None:
            thresholds = get_thresholds(iterations, self.nofuture_alpha, self.nofuture_beta, self.nofuture_gamma)
        S = self._as_c128(S)
        if len(thresholds) == 0:
            return S
        self._check(S)
        return self.plan().nofuture(S, thresholds, wsel=_capi.LWS_W_AI)  # W_ai on purpose: lws.pyx:475

    def online_lws(self, S, iterations=None, thresholds=None):
        if iterations is None:
            iterations = self.online_iterations
        if thresholds is None:
            thresholds = get_thresholds(iterations, self.online_alpha, self.online_beta, self.online_gamma)
        S = self._as_c128(S)
        if len(thresholds) == 0:
            return S
        self._check(S)
        return self.plan().online(S, thresholds, self.look_ahead, self._qdiv())

    def batch_lws(self, S, iterations=None, thresholds=None):
        if iterations is None:
            iterations = self.batch_iterations
        if thresholds is None:
            thresholds = get_thresholds(iterations, self.batch_alpha, self.batch_beta, self.batch_gamma)
        S = self._as_c128(S)
        if len(thresholds) == 0:
            return S
        self._check(S)
        return self.plan().batch(S, thresholds)

    def run_lws(self, S):
        """nofuture -> online -> batch (lws.pyx:495-499) as one device-resident pipeline."""
        S = self._as_c128(S)
        t0 = get_thresholds(self.nofuture_iterations, self.nofuture_alpha, self.nofuture_beta, self.nofuture_gamma)
        t1 = get_thresholds(self.online_iterations, self.online_alpha, self.online_beta, self.online_gamma)
        t2 = get_thresholds(self.batch_iterations, self.batch_alpha, self.batch_beta, self.batch_gamma)
        if len(t0) + len(t1) + len(t2) == 0:
            return S
        self._check(S)
        return self.plan().run(S, t0, t1, self.look_ahead, self._qdiv(), t2)
