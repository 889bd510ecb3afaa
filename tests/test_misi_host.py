"""CPU: the host fp64 MISI (lws_amd.misi) against its definition written out here: x_k = istft(c_k), e = y - sum_k x_k,
X_k = stft(x_k + e / K), c_k = A_k X_k / |X_k|."""
import numpy as np
import pytest

import lws_amd


def make(fsize, fshift, T, K, seed, perfectrec=False, B=None):
    """An lws object, K noise sources per mixture at different levels, their mixture y, the magnitudes A = |stft(source)| of
    T frames and starts c_0 = A exp(2 pi j u)."""
    rng = np.random.default_rng(seed)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    src = rng.standard_normal((B or 1, K, n)) * np.array([1.0, 0.3, 3.0, 0.5])[:K, None]
    A = np.abs(np.stack([[p.stft(x) for x in s] for s in src]))
    assert A.shape == (B or 1, K, T, F)
    c0 = A * np.exp(2j * np.pi * rng.random(A.shape))
    y = src.sum(axis=1)
    return (p, A, c0, y, src) if B is not None else (p, A[0], c0[0], y[0], src[0])


def one_step(p, c, A, y):
    """The definition, written out."""
    x = [p.istft(ck) for ck in c]
    e = y - sum(x[1:], x[0])
    return np.stack([Ak * np.exp(1j * np.angle(p.stft(xk + e / len(c)))) for Ak, xk in zip(A, x)]), e


@pytest.mark.parametrize("perfectrec", [False, True])
def test_one_step_is_the_written_out_formula(perfectrec):
    p, A, c0, y, _ = make(64, 16, 11, 3, 1, perfectrec)
    got = p.misi(c0, y, 1)
    assert got.dtype == np.complex128 and got.shape == c0.shape
    assert np.abs(got - one_step(p, c0, A, y)[0]).max() < 1e-12 * A.max()
    # the module-level form with the same windows, and explicit magnitudes that differ from |c_0|
    A2 = 2 * A + 1
    got = lws_amd.misi(c0, y, 64, 16, p.awin, p.swin, 1, magnitudes=A2, perfectrec=perfectrec)
    assert np.abs(got - one_step(p, c0, A2, y)[0]).max() < 1e-12 * A2.max()
    # two steps are the step applied twice
    twice = one_step(p, one_step(p, c0, A, y)[0], A, y)[0]
    assert np.abs(p.misi(c0, y, 2) - twice).max() < 1e-12 * A.max()


def test_one_source_takes_the_phase_of_the_mixture():
    """K = 1 with perfectrec: x + (y - x) is y, so every step gives A exp(j angle(stft(y))).  x + (y - x) equals y to a few
    ulp of max|x|, |y|, and the smallest bin of this noise mixture is above 1e-4 max|X|, so the phases agree to 1e-11."""
    p, A, c0, y, _ = make(64, 16, 9, 1, 2, perfectrec=True)
    Y = p.stft(y)
    assert np.abs(Y).min() > 1e-4 * np.abs(Y).max()
    want = A * np.exp(1j * np.angle(Y))
    for n in (1, 2, 5):
        assert np.abs(p.misi(c0, y, n) - want).max() < 1e-9 * A.max()


def test_the_true_sources_are_a_fixed_point():
    p, A, _, y, src = make(64, 16, 10, 3, 3, perfectrec=True)
    S = np.stack([p.stft(x) for x in src])
    out, db = p.misi(S, y, 1, return_trace=True)
    assert np.abs(out - S).max() < 1e-12 * np.abs(S).max()
    assert db.shape == (1,) and db[0] > 200


@pytest.mark.parametrize("perfectrec", [False, True])
@pytest.mark.parametrize("n", [0, 1, 4])
def test_signals_sum_to_the_mixture(perfectrec, n):
    p, A, c0, y, _ = make(48, 16, 8, 3, 4, perfectrec)
    out, s = p.misi(c0, y, n, return_signals=True)
    assert s.shape == (3, len(y)) and s.dtype == np.float64
    assert np.abs(s.sum(axis=0) - y).max() < 1e-12 * np.abs(y).max()
    x = np.stack([p.istft(o) for o in out])
    assert np.abs(s - (x + (y - x.sum(axis=0)) / 3)).max() < 1e-12 * np.abs(y).max()
    if n == 0:
        assert np.array_equal(out, c0)
    # all three extras together: trace before signals
    out2, db, s2 = p.misi(c0, y, n, return_trace=True, return_signals=True)
    assert np.array_equal(out2, out) and np.array_equal(s2, s) and db.shape == (n,)


def test_trace_is_the_mixture_consistency_of_the_entering_iterate():
    p, A, c0, y, _ = make(64, 16, 9, 2, 5)
    out, db = p.misi(c0, y, 3, return_trace=True)
    c = c0
    for i in range(3):
        nxt, e = one_step(p, c, A, y)
        assert abs(db[i] - 10 * np.log10(np.sum(y ** 2) / np.sum(e ** 2))) < 1e-9
        c = nxt
    assert np.abs(out - c).max() < 1e-12 * A.max()


def test_silent_magnitudes_give_exact_zeros():
    p, A, c0, y, _ = make(64, 16, 9, 2, 6, perfectrec=True)
    Z = A.copy()
    Z[0, 2:5] = 0.0                                # a silent stretch of one source
    Z[1] = 0.0                                     # and a silent source
    out, db, s = p.misi(c0, y, 4, magnitudes=Z, return_trace=True, return_signals=True)
    assert np.isfinite(out).all() and np.isfinite(db).all() and np.isfinite(s).all()
    assert (out[0, 2:5] == 0).all() and (out[1] == 0).all()
    assert np.abs(np.abs(out) - Z).max() <= 1e-12 * A.max()
    out = p.misi(np.zeros_like(c0), np.zeros_like(y), 2)      # silence everywhere: |X| == 0 in every bin
    assert (out == 0).all()


def test_a_stack_equals_its_members():
    p, A, c0, y, _ = make(64, 16, 7, 2, 7, B=3)
    scale = np.array([1.0, 1e-3, 40.0])
    c0, y = c0 * scale[:, None, None, None], y * scale[:, None]
    out, db, s = p.misi(c0, y, 3, return_trace=True, return_signals=True)
    assert out.shape == c0.shape and db.shape == (3, 3) and s.shape == (3, 2, y.shape[1])
    for b in range(3):
        one, one_db, one_s = p.misi(c0[b], y[b], 3, return_trace=True, return_signals=True)
        assert np.array_equal(out[b], one) and np.array_equal(db[:, b], one_db) and np.array_equal(s[b], one_s)


def test_argument_errors():
    p, A, c0, y, _ = make(64, 16, 6, 2, 8)
    with pytest.raises(ValueError):
        p.misi(c0, y[:-1], 3)                      # wrong mixture length
    with pytest.raises(ValueError):
        p.misi(c0, np.stack([y, y]), 3)            # a stack of mixtures for one set of sources
    with pytest.raises(ValueError):
        p.misi(c0, y, 3, magnitudes=A[:, :-1])
    with pytest.raises(ValueError):
        p.misi(c0, y, -1)
    with pytest.raises(ValueError):
        lws_amd.misi(c0[0], y, 64, 16, p.awin, p.swin, 3)      # a 2-D S
    # with perfectrec two frames of lws(64, 16) come back from the round trip as three
    q = lws_amd.lws(64, 16, perfectrec=True)
    with pytest.raises(ValueError):
        q.misi(c0[:, :2], np.zeros(len(q.istft(c0[0, :2]))), 1)


def test_the_reference_module_name_exports_it():
    import lws
    assert lws.misi is lws_amd.misi and lws.misi_dev is lws_amd.misi_dev
