"""CPU: the restatement of the device transform's factorisation (tests/fft_model.py) is a DFT, and what it costs in float32.

In float64 the model must equal np.fft at every frame size the transform tests use; in float32 its error against fp64 np.fft is
the error model of tests/test_gpu_transform_edges.py, printed here per N (pytest -s) next to what the kernels measured."""
import numpy as np
import pytest

import fft_model as fm

# the sizes of tests/test_gpu_transform_edges.py (a = 1: 34 50 62 510 4094; a = 2: 36 100 516 4092; MINN = 32), the sizes the older
# transform tests run (a >= 3), and the largest odd factors the range [32, 4096] holds
SIZES = [32, 34, 36, 50, 62, 64, 96, 100, 510, 516, 1000, 1032, 2050, 3000, 4090, 4092, 4094, 4096]

# max |dev - fp64| / max |fp64| of the kernel's forward transform of real unit Gaussian noise (rectangular window, 8 frames), one
# MI355X run of tests/test_gpu_transform_edges.py::test_forward_error_per_size, which prints it beside the model's figure for the
# same input (within 15 % of it at every size); sizes that test does not run: not measured
DEVICE = {32: 9.71e-08, 34: 1.18e-07, 36: 9.92e-08, 50: 1.10e-07, 62: 1.67e-07, 64: 9.92e-08, 100: 2.61e-07, 510: 4.67e-07,
          516: 3.26e-07, 1000: 2.64e-07, 4092: 8.79e-07, 4094: 1.49e-06, 4096: 1.55e-07}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sign", [-1, 1])
def test_float64_model_is_the_dft(n, sign):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    x[2] = 0
    x[2, 1] = 1.0                                     # an impulse off the origin: one twiddle per bin, sign and order exposed
    ref = np.fft.fft(x, axis=1) if sign < 0 else n * np.fft.ifft(x, axis=1)
    got = fm.fft_model(x, sign, np.float64)
    assert got.dtype == np.complex128 and got.shape == ref.shape
    for b in range(3):
        assert fm.max_rel(got[b], ref[b]) < 1e-12, (n, sign, b)


def test_float64_transform_models_are_the_host_functions():
    import lws_amd
    rng = np.random.default_rng(7)
    for fsize, fshift, fftsize in ((36, 27, None), (100, 30, None), (32, 16, 34), (50, 25, None)):
        awin, swin = fm.windows(fsize, fshift)
        for perfectrec in (True, False):
            for n in (1, fshift, fsize, 2 * fsize + fshift):
                x = rng.standard_normal(n)
                ref = lws_amd.stft(x, fsize, fshift, awin, fftsize=fftsize, perfectrec=perfectrec)
                got = fm.stft_model(x, fsize, fshift, awin, fftsize=fftsize, perfectrec=perfectrec, dtype=np.float64)
                assert got.shape == ref.shape
                if ref.size:
                    assert np.abs(got - ref).max() < 1e-12 * max(np.abs(ref).max(), 1.0)
                if fftsize is None and fsize % 4 == 0 and ref.shape[0] > 0:
                    back_ref = lws_amd.istft(ref, fshift, swin, perfectrec=perfectrec)
                    back = fm.istft_model(ref, fshift, swin, perfectrec=perfectrec, dtype=np.float64)
                    assert back.shape == back_ref.shape
                    if back_ref.size:
                        assert np.abs(back - back_ref).max() < 1e-12 * max(np.abs(back_ref).max(), 1.0)


def test_float32_error_table():
    """The cost of the factorisation in float32: grows with the odd factor m (m accumulated terms per output), and stays within
    the transform tests' 3e-6 of the largest value at every size -- by a factor of two at m = 2045, not by more."""
    print("\n    N     m   a   float32 model   device (MI355X; real input, forward)")
    worst = 0.0
    for n in SIZES:
        m, a = fm.factor(n)
        err = fm.model_error(n)
        worst = max(worst, err)
        dev = DEVICE.get(n)
        print("%5d %5d %3d   %.2e        %s" % (n, m, a, err, "not measured" if dev is None else "%.2e" % dev))
        assert err < 3e-6, (n, err)
        assert err > 2.0 ** -25, (n, err)              # a float32 model that is more exact than float32 rounds nothing
    assert worst > 1e-6                                # the large odd factors do cost: the table's point
