"""CPU-only checks of the isotropic-spectra module (niwqg_amd/spectra.py): the integer shell rule, the shell count and
the mode counts, the name tables per class and the refusal of unknown names."""
import ctypes

import numpy as np
import pytest


def test_integer_shell_rule_is_the_nearest_integer():
    from niwqg_amd.spectra import shell_of
    n = np.arange(-300, 301)
    i, j = np.meshgrid(n, n)
    r = np.hypot(i, j)
    away = np.abs(r - np.floor(r) - 0.5) > 1e-9          # sqrt of an integer is never a half-integer: this keeps all of them
    assert away.all()
    assert np.array_equal(shell_of(i, j)[away], np.floor(r[away] + 0.5).astype(np.int64))
    assert shell_of(0, 0) == 0 and shell_of(1, 0) == 1 and shell_of(1, 1) == 1 and shell_of(2, 1) == 2


def test_isqrt_is_exact_near_squares():
    from niwqg_amd.spectra import isqrt
    r = np.arange(0, 200000, 7, dtype=np.int64)
    for d in (-1, 0, 1):
        v = np.maximum(r * r + d, 0)
        got = isqrt(v)
        assert np.all(got * got <= v) and np.all((got + 1) * (got + 1) > v)


@pytest.mark.parametrize("nx", [4, 8, 16, 64, 96, 100, 128, 512, 1024, 4096, 8192, 16384])
def test_shell_count(nx):
    from niwqg_amd.spectra import shell_count
    assert shell_count(nx) == int(np.floor(nx / np.sqrt(2) + 0.5)) + 1


@pytest.mark.parametrize("nx", [4, 16, 64, 128, 100, 512])
def test_modes_cover_the_plane(nx):
    from niwqg_amd.spectra import shell_modes, shell_count
    m = shell_modes(nx)
    assert m.shape == (shell_count(nx),) and m.sum() == nx * nx and m[0] == 1 and (m > 0).all()
    # full shells inside the square: the number of lattice points with |r - b| < 1/2, counted by brute force
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    r = np.hypot(n[None, :], n[:, None])
    for b in range(0, nx // 2 + 1, max(1, nx // 16)):
        assert m[b] == np.count_nonzero(np.floor(r + 0.5) == b)


def test_name_tables():
    from niwqg_amd import spectra
    assert spectra.KERNEL_NAMES == ("ke_qg", "ens", "ke_niw", "pe_niw", "ep_phi", "ep_psi", "chi_q", "chi_phi", "gamma_r",
                                    "gamma_a", "xi_r", "xi_a")
    assert spectra.QG_NAMES == ("ke_qg", "ens", "ep_psi", "chi_q")
    assert spectra.QG_SCALAR_NAMES == ("C2", "gradC2", "ep_c", "chi_c")

    class FakeQG(object):
        passive_scalar = True
    import niwqg_amd.QGModel as Q
    fake = Q.Model.__new__(Q.Model)
    fake.passive_scalar = False
    assert spectra.available(fake) == list(spectra.QG_NAMES)
    fake.passive_scalar = True
    assert spectra.available(fake) == list(spectra.QG_NAMES + spectra.QG_SCALAR_NAMES)
    assert spectra.available(FakeQG()) == list(spectra.KERNEL_NAMES)


def test_unknown_name_is_refused_before_the_device():
    import niwqg_amd.QGModel as Q
    from niwqg_amd import spectra
    fake = Q.Model.__new__(Q.Model)
    fake.passive_scalar = False
    with pytest.raises(ValueError, match="valid names: ke_qg, ens, ep_psi, chi_q"):
        spectra.isotropic_spectra(fake, names=["C2"])
    with pytest.raises(ValueError, match="'nope'"):
        spectra.isotropic_spectra(fake, names="nope")


def test_binned_entries_are_exported_and_typed():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    L = _lib.lib()
    entries = ("nq_spectrum_shells", "nq_diagnostics_binned", "nq_slab_diagnostics_binned", "nq_any_bin")
    for name in entries:                # untyped, ctypes would pass a device pointer as a 32-bit int
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    assert L.nq_any_bin.argtypes[1] is ctypes.c_void_p
    assert L.nq_spectrum_shells(None) == -1
