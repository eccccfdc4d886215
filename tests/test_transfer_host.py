"""CPU-only checks of the spectral-transfer module (niwqg_amd/transfer.py): the name tables and available() per class, the
refusal of unknown names before the device is touched, the two C entries, and the flux as minus the cumulative transfer."""
import ctypes

import numpy as np
import pytest


def _fake(module, **attrs):
    cls = __import__("niwqg_amd." + module, fromlist=["Model"]).Model
    m = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_name_tables():
    from niwqg_amd import transfer
    assert transfer.KERNEL_NAMES == ("ke_qg", "ens", "ke_niw_adv", "ke_niw_ref")
    assert transfer.YBJ_NAMES == ("ke_niw_adv", "ke_niw_ref")
    assert transfer.QG_NAMES == ("ke_qg", "ens")
    assert transfer.QG_SCALAR_NAMES == ("C2", "gradC2")
    names = transfer.KERNEL_NAMES + transfer.QG_SCALAR_NAMES
    assert sorted(transfer.ROWS) == sorted(names)
    assert sorted(r for r, _ in transfer.ROWS.values()) == list(range(6))


def test_available_per_class():
    from niwqg_amd import transfer
    assert transfer.available(_fake("QGModel", passive_scalar=False)) == ["ke_qg", "ens"]
    assert transfer.available(_fake("QGModel", passive_scalar=True)) == ["ke_qg", "ens", "C2", "gradC2"]
    assert transfer.available(_fake("CoupledModel")) == ["ke_qg", "ens", "ke_niw_adv", "ke_niw_ref"]
    assert transfer.available(_fake("UnCoupledModel")) == ["ke_qg", "ens", "ke_niw_adv", "ke_niw_ref"]
    assert transfer.available(_fake("YBJModel")) == ["ke_niw_adv", "ke_niw_ref"]


def test_unknown_or_unavailable_names_are_refused_before_the_device():
    from niwqg_amd.transfer import spectral_transfer
    qg = _fake("QGModel", passive_scalar=False)          # no context, no grid: any device access would fail otherwise
    with pytest.raises(ValueError, match="valid names: ke_qg, ens$"):
        spectral_transfer(qg, names=["C2"])
    with pytest.raises(ValueError, match="'nope'"):
        spectral_transfer(qg, names="nope")
    with pytest.raises(ValueError, match="valid names: ke_niw_adv, ke_niw_ref"):
        spectral_transfer(_fake("YBJModel"), names=["ke_niw_adv", "ens"])
    with pytest.raises(ValueError, match="'ke_niw_adv'"):
        spectral_transfer(_fake("QGModel", passive_scalar=True), names=["C2", "ke_niw_adv"])


def test_transfer_entries_are_exported_and_typed():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    L = _lib.lib()
    for name in ("nq_transfer_binned", "nq_slab_transfer_binned"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    assert L.nq_transfer_binned.argtypes[1] is ctypes.c_int
    assert L.nq_transfer_binned(None, 1, None) == -1
    assert L.nq_slab_transfer_binned(None, 1, None) == -1
    assert _lib.TRANSFER_ROWS == 6


def test_header_documents_the_row_count():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "niwqg_amd.h")).read()
    assert int(re.search(r"#define NQ_TRANSFER_ROWS (\d+)", header).group(1)) == 6


def test_flux_is_minus_the_cumulative_transfer():
    from niwqg_amd.transfer import SpectralTransfer, flux_of
    rng = np.random.default_rng(3)
    nb, dk = 92, 0.25
    T = {"ke_qg": rng.standard_normal(nb), "ens": rng.standard_normal(nb)}
    st = SpectralTransfer(np.arange(nb, dtype=np.int64), dk, np.ones(nb, dtype=np.int64), 32 * dk, T)
    assert np.allclose(st.k_edge, (np.arange(nb) + 0.5) * dk) and np.allclose(st.k, np.arange(nb) * dk)
    assert np.allclose(st.k_edge - st.k, 0.5 * dk)
    for name, t in T.items():
        assert np.array_equal(st.flux[name], -np.cumsum(t))
        assert np.array_equal(flux_of(t), st.flux[name])
        assert st.flux[name][0] == -t[0]
        assert abs(st.flux[name][-1] + t.sum()) <= 1e-12 * np.abs(t).sum()
    assert set(st.flux) == set(T)
    assert "ens" in repr(st)
