"""CPU-only checks of the frequency module (niwqg_amd/frequency.py): the numpy restatement of the (frequency x shell) table
(Parseval closure, a known line with its sign, the evenness of a real field's table, demean), every refusal raised by the
model-free checker, the shell bookkeeping of the block, and the C entries exported, typed and declared in the header."""
import ctypes
import os
import re

import numpy as np
import pytest

from niwqg_amd import _lib, frequency
from niwqg_amd.spectra import shell_modes, shell_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = 32
K = 5
T = 16


def _series(kind, seed=0, T=T, K=K):
    rng = np.random.default_rng(seed)
    shape = (T, 2 * K + 1, 2 * K + 1 if kind == "phi" else K + 1)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _record_shells(x, kind, dk):
    """S_n(b): the instantaneous shell spectrum of every record, from the definition (full plane of a real field: columns
    1..K count twice)"""
    Tn, R, C = x.shape
    Kb = (R - 1) // 2
    j = frequency.block_numbers(Kb)
    i = j if kind == "phi" else np.arange(Kb + 1)
    a = np.abs(x) ** 2
    if kind != "phi":
        a[:, :, 1:] *= 2.0
    if kind == "psi":
        a = a * (dk ** 2 * (i[None, :] ** 2 + j[:, None] ** 2))[None]
    sh = shell_of(i[None, :], j[:, None]).ravel()
    nb = int(shell_of(Kb, Kb)) + 1
    S = np.zeros((Tn, nb))
    for b in range(nb):
        S[:, b] = a.reshape(Tn, -1)[:, sh == b].sum(axis=1)
    return 0.5 * S / float(NX * NX) ** 2


@pytest.mark.parametrize("kind", ["phi", "q", "psi"])
@pytest.mark.parametrize("window", ["boxcar", "hann"])
def test_parseval_closure(kind, window):
    """sum_p P(p, b) = sum_n w_n^2 S_n(b) / sum_n w_n^2, to 1e-13 of the mass"""
    dk = 0.7
    x = _series(kind, seed=3)
    omega, P = frequency.reference_spectrum(x, 2.0, kind, window, False, NX, NX, dk=dk)
    w = frequency.check_window(window, T)
    want = (w[:, None] ** 2 * _record_shells(x, kind, dk)).sum(axis=0) / (w ** 2).sum()
    assert P.shape == (T, frequency.block_shell_count(K)) and np.all(np.diff(omega) > 0)
    assert np.abs(P.sum(axis=0) - want).max() <= 1e-13 * want.sum()


def test_line_lands_in_the_bin_of_plus_omega():
    """x_n = a e^{-i Omega n Delta} with Omega Delta T = 2 pi p0: everything in the bin of +Omega"""
    p0, delta = 3, 2.5
    Om = 2 * np.pi * p0 / (T * delta)
    x = np.zeros((T, 2 * K + 1, 2 * K + 1), complex)
    x[:, 4, 3] = (0.3 - 0.2j) * np.exp(-1j * Om * delta * np.arange(T))          # (i, j) = (3, 4): shell 5
    omega, P = frequency.reference_spectrum(x, delta, "phi", "boxcar", False, NX, NX)
    ip = int(np.argmin(np.abs(omega - Om)))
    assert abs(omega[ip] - Om) <= 1e-12 * Om
    assert P[ip, 5] > 0 and P[ip, 5] >= (1 - 1e-13) * P.sum()
    rest = P.copy()
    rest[ip, 5] = 0.0
    assert rest.max() <= 1e-28 * P[ip, 5]
    assert np.all(np.delete(P, 5, axis=1) == 0.0)


@pytest.mark.parametrize("kind", ["q", "psi"])
@pytest.mark.parametrize("Tn", [16, 12, 7])
def test_real_field_table_is_even_in_omega(kind, Tn):
    """columns 1..K pair +p with -p term by term; column 0 of a real field is Hermitian in l, so its sum over the rows is even
    too, up to the rounding of the transform (1e-14 of the mass)"""
    x = _series(kind, seed=5, T=Tn)
    x[:, K + 1:, 0] = np.conj(x[:, K:0:-1, 0])
    x[:, 0, 0] = x[:, 0, 0].real
    omega, P = frequency.reference_spectrum(x, 1.0, kind, "hann", False, NX, NX, dk=1.3)
    seen = 0
    for p in range(Tn):
        m = int(np.argmin(np.abs(omega + omega[p])))
        if abs(omega[m] + omega[p]) <= 1e-12:                  # (the Nyquist bin of an even T has no mirror on the axis)
            seen += 1
            assert np.abs(P[p] - P[m]).max() <= 1e-14 * P.sum()
    assert seen >= Tn - 1
    x[:, :, 1:] = 0.0                                          # and not by accident: an un-Hermitian column 0 breaks it
    x[:, 1, 0] *= 3.0
    omega, P = frequency.reference_spectrum(x, 1.0, kind, "hann", False, NX, NX, dk=1.3)
    assert np.abs(P - P[::-1] if Tn % 2 else P[1:] - P[1:][::-1]).max() > 1e-3 * P.max()


@pytest.mark.parametrize("kind", ["phi", "q"])
def test_demean_removes_a_constant_exactly(kind):
    x = _series(kind, seed=7)
    const = np.ones_like(x[0]) * (2.0 - 1.0j)                  # representable: x + const - mean(x + const) differs by rounding only
    a = frequency.reference_spectrum(x, 1.0, kind, "hann", True, NX, NX)[1]
    b = frequency.reference_spectrum(x + const[None], 1.0, kind, "hann", True, NX, NX)[1]
    assert np.abs(a - b).max() <= 1e-13 * a.sum()
    only = np.broadcast_to(const, x.shape)
    assert np.all(frequency.reference_spectrum(only, 1.0, kind, "boxcar", True, NX, NX)[1] == 0.0)
    assert frequency.reference_spectrum(only, 1.0, kind, "boxcar", False, NX, NX)[1].sum() > 0.0


def test_longdouble_restatement_agrees():
    x = _series("q", seed=9, T=12)
    a = frequency.reference_spectrum(x, 1.0, "q", "hann", False, NX, NX)[1]
    b = frequency.reference_spectrum(x.astype(np.clongdouble), 1.0, "q", "hann", False, NX, NX)[1]
    assert b.dtype == np.longdouble
    assert np.abs(a - b).max() <= 1e-14 * float(b.sum())


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(kmax=0), dict(kmax=NX // 2), dict(kmax=-3), dict(kmax=2.5), dict(kmax=True),
                                dict(every=0), dict(every=1.5), dict(length=1), dict(length=0),
                                dict(fields=[]), dict(fields=["phi", "phi"]), dict(fields=["u"])])
def test_attach_arguments_are_refused(kw):
    args = dict(kmax=4, every=1, length=8, fields=None)
    args.update(kw)
    with pytest.raises(ValueError, match="frequency.attach"):
        frequency.check(NX, _lib.COUPLED, **args)


def test_fields_by_class():
    assert frequency.check(NX, _lib.COUPLED, 4)[3] == ("phi", "q", "psi")
    assert frequency.check(NX, _lib.UNCOUPLED, 4)[3] == ("phi", "q", "psi")
    assert frequency.check(NX, _lib.QG, 4)[3] == ("q", "psi")
    assert frequency.check(NX, _lib.YBJ, 4)[3] == ("phi",)
    assert frequency.check(NX, _lib.COUPLED, NX // 2 - 1, 3, 2, "q") == (NX // 2 - 1, 3, 2, ("q",))
    with pytest.raises(ValueError, match=r"'phi' not available for QGModel; valid names: q, psi"):
        frequency.check(NX, _lib.QG, 4, fields=["q", "phi"])
    with pytest.raises(ValueError, match=r"'q', 'psi' not available for YBJModel; valid names: phi"):
        frequency.check(NX, _lib.YBJ, 4, fields=["q", "psi"])


@pytest.mark.parametrize("window", [np.ones(T - 1), np.ones((T, 1)), np.r_[np.ones(T - 1), np.nan], np.r_[np.ones(T - 1), np.inf],
                                    "welch", np.zeros(T), [1j] * T])
def test_windows_are_refused(window):
    with pytest.raises(ValueError, match="frequency.spectrum"):
        frequency.check_window(window, T)


def test_spectrum_needs_two_records():
    with pytest.raises(ValueError, match="at least 2"):
        frequency.check_window("hann", 1)
    assert np.array_equal(frequency.check_window("boxcar", 2), [1.0, 1.0])
    n = np.arange(12)
    assert np.array_equal(frequency.check_window("hann", 12), 0.5 - 0.5 * np.cos(2 * np.pi * n / 12))
    assert np.array_equal(frequency.check_window(range(1, 4), 3), [1.0, 2.0, 3.0])


def test_attach_refuses_before_the_device():
    """the public entry checks through the same function: a model whose context fails on any use"""
    from niwqg_amd.YBJModel import Model

    class NoDevice(object):
        def __getattr__(self, name):
            raise AssertionError("the device was touched: %s" % name)

    m = Model.__new__(Model)
    m.__dict__.update(nx=NX, ny=NX, t=0.0, dt=1.0, dk=1.0, _ctx=NoDevice())
    with pytest.raises(ValueError, match="not available for YBJModel"):
        frequency.attach(m, 4, fields=["q"])
    with pytest.raises(ValueError, match="kmax"):
        frequency.attach(m, NX // 2)


# ---- the block ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, Kb", [(16, 1), (32, 5), (64, 8), (128, 40), (48, 23)])
def test_block_shells_are_the_planes(nx, Kb):
    modes = frequency.block_modes(Kb)
    assert len(modes) == int(shell_of(Kb, Kb)) + 1 == frequency.block_shell_count(Kb)
    assert np.array_equal(modes[:Kb + 1], shell_modes(nx)[:Kb + 1])          # whole shells up to K
    assert np.all(modes[Kb + 1:] <= shell_modes(nx)[Kb + 1:len(modes)]) and modes.sum() == (2 * Kb + 1) ** 2
    rows = frequency.block_index(nx, Kb)
    assert np.array_equal(np.fft.fftfreq(nx, 1.0 / nx)[rows], frequency.block_numbers(Kb))
    assert nx // 2 not in rows                                                # never the Nyquist line
    half = frequency.block_shells(Kb, False)
    assert half.shape == (2 * Kb + 1, Kb + 1) and np.array_equal(half, frequency.block_shells(Kb, True)[:, :Kb + 1])


def test_entries_exported_typed_and_declared():
    import niwqg_amd
    niwqg_amd.build()
    L = _lib.lib()
    names = ("nq_freq_attach", "nq_freq_detach", "nq_freq_info", "nq_freq_series", "nq_freq_spectrum", "nq_any_freq_record",
             "nq_any_freq_spectrum")
    header = open(os.path.join(ROOT, "include", "niwqg_amd.h")).read()
    for name in names:
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert L.nq_freq_spectrum.argtypes[4] is ctypes.c_double and L.nq_freq_spectrum.argtypes[5] is ctypes.c_int
    assert L.nq_any_freq_spectrum.argtypes[11] is ctypes.c_double
    # null contexts and engines are refused without a device
    w = (ctypes.c_double * 4)()
    f = (ctypes.c_int * 1)(0)
    i3 = (ctypes.c_longlong * 3)()
    assert L.nq_freq_attach(None, 4, 1, 8, 1, f) != 0
    assert L.nq_freq_detach(None) != 0
    assert L.nq_freq_info(None, i3) != 0
    assert L.nq_freq_series(None, 0, None, None) != 0
    assert L.nq_freq_spectrum(None, 0, w, 0, 1.0, 4, w) != 0
    assert L.nq_any_freq_record(None, 1, None, None, None, None, 48, 8, 4, 0) != 0
    assert L.nq_any_freq_spectrum(None, None, 48, 8, 1, 0, 4, 0, 4, w, 0, 1.0, 12, w) != 0
