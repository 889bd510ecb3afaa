"""CPU: the host fp64 Griffin-Lim (lws_amd.griffin_lim) against its definition written out here, and against Griffin-Lim's own
guarantee (the inconsistency of the magnitude-projected iterates does not increase)."""
import numpy as np
import pytest

import lws_amd


def make(fsize, fshift, T, seed, perfectrec=False, B=None):
    """An lws object, magnitudes A = |stft(noise)| of T frames and a start c_0 = A exp(2 pi j u)."""
    rng = np.random.default_rng(seed)
    p = lws_amd.lws(fsize, fshift, perfectrec=perfectrec)
    F = fsize // 2 + 1
    shape = (T, F) if B is None else (B, T, F)
    n = lws_amd.istft(np.zeros((T, F), complex), fshift, p.swin, perfectrec=perfectrec).shape[0]
    sigs = rng.standard_normal((B or 1, n))
    A = np.abs(np.stack([p.stft(x) for x in sigs])).reshape(shape)
    return p, A, A * np.exp(2j * np.pi * rng.random(shape))


def project(p, c):
    return p.stft(p.istft(c))


@pytest.mark.parametrize("perfectrec", [False, True])
def test_one_plain_step_is_the_written_out_formula(perfectrec):
    p, A, c0 = make(64, 16, 11, 1, perfectrec)
    want = A * np.exp(1j * np.angle(project(p, c0)))
    got = p.griffin_lim(c0, 1, alpha=0.0)
    assert got.dtype == np.complex128 and got.shape == c0.shape
    assert np.abs(got - want).max() < 1e-12 * A.max()
    # the module-level form with the same windows, and explicit magnitudes that differ from |c_0|
    got = lws_amd.griffin_lim(c0, 64, 16, p.awin, p.swin, 1, alpha=0.0, magnitudes=2 * A + 1, perfectrec=perfectrec)
    assert np.abs(got - (2 * A + 1) * np.exp(1j * np.angle(project(p, c0)))).max() < 1e-12 * (2 * A + 1).max()


def test_momentum_steps_are_the_written_out_recursion():
    p, A, c0 = make(96, 32, 9, 2)
    alpha, c, t_prev = 0.5, c0, None
    for i in range(1, 5):
        t = A * np.exp(1j * np.angle(project(p, c)))
        c = t if i == 1 else t + alpha * (t - t_prev)
        t_prev = t
    assert np.abs(p.griffin_lim(c0, 4, alpha=alpha) - t_prev).max() < 1e-12 * A.max()


def test_plain_griffin_lim_does_not_increase_the_inconsistency():
    p, A, c0 = make(64, 16, 14, 3)
    d = []
    for n in range(1, 7):
        t = p.griffin_lim(c0, n, alpha=0.0)
        d.append(np.sum(np.abs(project(p, t) - t) ** 2))
    assert all(b <= a * (1 + 1e-12) for a, b in zip(d, d[1:])), d
    assert d[-1] < d[0]
    # the trace is the consistency of the iterate ENTERING each step: entry 0 is get_consistency(c_0), entry i that of t_i
    _, db = p.griffin_lim(c0, 6, alpha=0.0, return_trace=True)
    assert db.shape == (6,)
    assert abs(db[0] - p.get_consistency(c0)) < 1e-9
    energy = np.sum(A ** 2)
    assert np.allclose(db[1:], 10 * np.log10(energy / np.array(d[:5])), atol=1e-9)


@pytest.mark.parametrize("alpha", [0.0, 0.99])
def test_magnitudes_of_the_result_are_the_target(alpha):
    p, A, c0 = make(48, 16, 8, 4)
    assert np.abs(np.abs(p.griffin_lim(c0, 5, alpha=alpha)) - A).max() <= 1e-12 * A.max()
    Z = A.copy()
    Z[2:5] = 0.0                                   # a silent stretch: exact zeros, nothing undefined
    out = p.griffin_lim(c0, 5, alpha=alpha, magnitudes=Z)
    assert np.isfinite(out).all() and (out[2:5] == 0).all()
    assert np.abs(np.abs(out) - Z).max() <= 1e-12 * A.max()


def test_zero_iterations_return_the_input():
    p, A, c0 = make(64, 16, 6, 5)
    assert np.array_equal(p.griffin_lim(c0, 0), c0)
    out, db = p.griffin_lim(c0, 0, return_trace=True)
    assert np.array_equal(out, c0) and db.shape == (0,)


def test_a_stack_equals_its_members():
    p, A, c0 = make(64, 16, 7, 6, B=3)
    c0 = c0 * np.array([1.0, 1e-3, 40.0])[:, None, None]
    out, db = p.griffin_lim(c0, 3, return_trace=True)
    assert out.shape == c0.shape and db.shape == (3, 3)
    for b in range(3):
        one, one_db = p.griffin_lim(c0[b], 3, return_trace=True)
        assert np.array_equal(out[b], one) and np.array_equal(db[:, b], one_db)


def test_argument_errors():
    p, A, c0 = make(64, 16, 6, 7)
    with pytest.raises(ValueError):
        p.griffin_lim(c0, 3, alpha=1.0)
    with pytest.raises(ValueError):
        p.griffin_lim(c0, -1)
    with pytest.raises(ValueError):
        p.griffin_lim(c0, 3, magnitudes=A[:-1])
    with pytest.raises(ValueError):
        lws_amd.griffin_lim(c0[0], 64, 16, p.awin, p.swin, 3)


def test_the_reference_module_name_exports_it():
    import lws
    assert lws.griffin_lim is lws_amd.griffin_lim and lws.griffin_lim_dev is lws_amd.griffin_lim_dev
