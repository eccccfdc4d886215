"""The coarse-grained flux maps' numpy restatement (niwqg_amd/coarse.py: reference) against a numpy restatement of the transfer
rows written here, a single Fourier mode, the table builders and every refusal of the contract.  No GPU."""
import types

import numpy as np
import pytest


def shim(nx, seed=0, waves=True):
    """a broadband state with energy on the Nyquist lines, as the public reads of a Kernel-family model give it"""
    rng = np.random.default_rng(seed + nx)
    dk = 2 * np.pi / (2 * np.pi * 3.0)
    kk = dk * np.append(np.arange(0., nx / 2), np.arange(-nx / 2, 0.))
    kx, ly = kk[None, :], kk[:, None]
    ph = np.fft.fft2(rng.standard_normal((nx, nx)))
    q = np.fft.ifft2(-(kx ** 2 + ly ** 2) * ph).real + 0.3 * rng.standard_normal((nx, nx))
    m = types.SimpleNamespace(nx=nx, dk=dk, kk=kk, ll=kk.copy(), ph=ph, q=q)
    if waves:
        phih = np.fft.fft2(rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx)))
        m.phih, m.phix, m.phiy = phih, np.fft.ifft2(1j * kx * phih), np.fft.ifft2(1j * ly * phih)
    return m


def transfer_rows(m):
    """T(b) of ke_qg, ens, ke_niw_adv from the host fields (tests/test_gpu_transfer.py: restated)"""
    from niwqg_amd.spectra import shell_of, shell_count
    nx, M2 = m.nx, float(m.nx) ** 4
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    b, nb = shell_of(n[None, :], n[:, None]).ravel(), shell_count(nx)
    kx, ly = m.kk[None, :], m.ll[:, None]
    F = np.fft.fft2
    P = F(np.fft.ifft2(m.ph).real)
    u, v = np.fft.ifft2(-1j * ly * P).real, np.fft.ifft2(1j * kx * P).real
    Jq = 1j * kx * F(u * m.q) + 1j * ly * F(v * m.q)

    def binned(x):
        return np.bincount(b, weights=np.ravel(x), minlength=nb)
    out = dict(ke_qg=binned((np.conj(P) * Jq).real) / M2, ens=-binned((np.conj(F(m.q)) * Jq).real) / M2)
    if hasattr(m, "phih"):
        out["ke_niw_adv"] = -binned((np.conj(m.phih) * F(u * m.phix + v * m.phiy)).real) / M2
    return out


def cuts(nx, name):
    return sorted({1, 2, nx // 8, (nx - 1) // 3} | ({nx // 2 - 1} if name == "ke_qg" else set()))


@pytest.mark.parametrize("nx", [64, 128])
def test_plane_mean_is_the_spectral_flux_through_the_cut(nx):
    from niwqg_amd import coarse
    m = shim(nx)
    T = transfer_rows(m)
    shells = sorted({B for n in coarse.NAMES for B in cuts(nx, n)})
    R = coarse.reference(m, [coarse.sharp(m, B) for B in shells])
    assert sorted(R) == sorted(coarse.NAMES) and all(v.shape == (len(shells), nx, nx) and v.dtype == np.float64 for v in R.values())
    for name in coarse.NAMES:
        flux = -np.cumsum(T[name])
        for B in cuts(nx, name):
            mp = R[name][shells.index(B)]
            err, scale = abs(mp.mean() - flux[B]), np.abs(mp).mean() + np.abs(T[name]).sum()
            print("%d %s B = %d: %.3g" % (nx, name, B, err / scale))
            assert scale > 0 and err <= 1e-12 * scale, (name, B, err, scale)


@pytest.mark.parametrize("nx", [64, 128])
def test_the_identity_is_not_vacuous(nx):
    """at B = nx/2 - 1 the resolved triple product of ens aliases (3 B >= nx): its mean is not zero and the identity fails"""
    from niwqg_amd import coarse
    m = shim(nx)
    T = transfer_rows(m)["ens"]
    B = nx // 2 - 1
    mp = coarse.reference(m, coarse.sharp(m, B), "ens")["ens"][0]
    assert abs(mp.mean() + np.cumsum(T)[B]) > 1e-8 * (np.abs(mp).mean() + np.abs(T).sum())


def test_a_single_mode_below_the_cut_has_no_sub_filter_flux():
    from niwqg_amd import coarse
    nx = 64
    m = shim(nx)
    x = np.arange(nx) * 2 * np.pi * 3.0 / nx
    X, Y = np.meshgrid(x, x)
    a, b = 3, 5                                                   # shell 6
    psi = 0.7 * np.cos(a * m.dk * X + b * m.dk * Y + 0.3)
    m.ph = np.fft.fft2(psi)
    m.q = -(a * a + b * b) * m.dk ** 2 * psi
    for B in (6, 7, 20):                                          # the mode's shell is at or below the cut: G leaves every plane alone
        R = coarse.reference(m, coarse.sharp(m, B), ("ke_qg", "ens"))
        scale = np.abs(m.q).max() ** 2 * 0.7 * np.hypot(a, b) * m.dk
        assert np.abs(R["ke_qg"]).max() <= 1e-12 * scale and np.abs(R["ens"]).max() <= 1e-12 * scale * np.hypot(a, b) * m.dk, B
    # the mode is filtered away: what is left are products of two roundoff residues of fft2(psi) on the other wavenumbers
    R = coarse.reference(m, coarse.sharp(m, 5), ("ke_qg", "ens"))
    assert np.abs(R["ke_qg"]).max() <= 1e-24 * scale and np.abs(R["ens"]).max() <= 1e-24 * scale * np.hypot(a, b) * m.dk


def test_table_builders():
    from niwqg_amd import coarse
    from niwqg_amd.spectra import shell_count
    m = types.SimpleNamespace(nx=64, dk=0.25)
    nb = shell_count(64)
    g = coarse.sharp(m, 8)
    assert g.shape == (nb,) and g.dtype == np.float64 and np.array_equal(g[:9], np.ones(9)) and not g[9:].any()
    assert coarse.sharp(m, 31)[31] == 1 and not coarse.sharp(m, 31)[32:].any()
    h = coarse.gaussian(m, 3.0)
    b = np.arange(32)
    assert h.shape == (nb,) and np.array_equal(h[:32], np.exp(-(b * 0.25 * 3.0) ** 2 / 24.0)) and not h[32:].any() and h[0] == 1
    for bad in (0, 32, -1, 2.5):
        with pytest.raises(ValueError, match="1 .. nx/2 - 1 = 31"):
            coarse.sharp(m, bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="length > 0"):
            coarse.gaussian(m, bad)
    assert coarse.check_table(64, g).shape == (1, nb)
    t = np.tile(g, (2, 1))
    t[1, 32] = 1e-300
    with pytest.raises(ValueError, match="Nyquist rule"):
        coarse.check_table(64, t)
    t[1, 32] = 0
    t[0, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        coarse.check_table(64, t)
    with pytest.raises(ValueError, match="nb = %d" % nb):
        coarse.check_table(64, np.ones(nb - 1))
    with pytest.raises(ValueError, match="nscales <= 64"):
        coarse.check_table(64, np.zeros((65, nb)))


def test_half_plane_psi_of_qgmodel():
    """QGModel's public reads: psi-hat on kx = 0 .. nx/2 and u, v = irfft2 of it, which keep the content of row ny/2 that a full
    plane's real part drops.  The products of the reference are formed with those u, v (what the device's products pass holds),
    and the identities hold against the transfer rows formed the same way (tests/test_gpu_transfer.py: restated)."""
    from niwqg_amd import coarse
    from niwqg_amd.spectra import shell_of, shell_count
    nx = 64
    f = shim(nx, waves=False)
    h = nx // 2 + 1
    ph = np.fft.rfft2(np.fft.ifft2(f.ph).real)
    ph[nx // 2, 1:h - 1] += 3.0 * np.abs(ph).mean() * (1 + 0.5j)       # row ny/2, not Hermitian-consistent: irfft2 keeps it in u
    m = types.SimpleNamespace(nx=nx, dk=f.dk, kk=f.kk[:h].copy(), ll=f.ll, ph=ph, q=f.q)
    m.kk[-1] = abs(m.kk[-1])
    kx, ly, kh = f.kk[None, :], f.ll[:, None], m.kk[None, :]
    u, v = np.fft.irfft2(-1j * ly * ph, s=(nx, nx)), np.fft.irfft2(1j * kh * ph, s=(nx, nx))
    assert np.abs(u - np.fft.ifft2(-1j * ly * np.fft.fft2(np.fft.irfft2(ph, s=(nx, nx)))).real).max() > 1e-3 * np.abs(u).max()
    F = np.fft.fft2
    P, Q = F(np.fft.irfft2(ph, s=(nx, nx))), F(m.q)
    Jq = 1j * kx * F(u * m.q) + 1j * ly * F(v * m.q)
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    b, nb = shell_of(n[None, :], n[:, None]).ravel(), shell_count(nx)
    T = dict(ke_qg=np.bincount(b, weights=np.ravel((np.conj(P) * Jq).real), minlength=nb) / float(nx) ** 4,
             ens=-np.bincount(b, weights=np.ravel((np.conj(Q) * Jq).real), minlength=nb) / float(nx) ** 4)
    for name in ("ke_qg", "ens"):
        for B in cuts(nx, name):
            mp = coarse.reference(m, coarse.sharp(m, B), name)[name][0]
            err, scale = abs(mp.mean() + np.cumsum(T[name])[B]), np.abs(mp).mean() + np.abs(T[name]).sum()
            assert err <= 1e-12 * scale, (name, B, err, scale)


def _fake(module, **attrs):
    cls = __import__("niwqg_amd." + module, fromlist=["Model"]).Model
    m = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_available_per_class_and_the_constants():
    from niwqg_amd import coarse, _lib
    import niwqg_amd
    assert niwqg_amd.coarse is coarse
    assert coarse.NAMES == ("ke_qg", "ens", "ke_niw_adv")
    assert coarse.available(_fake("QGModel")) == ["ke_qg", "ens"]
    assert coarse.available(_fake("CoupledModel", model_id=_lib.COUPLED)) == list(coarse.NAMES)
    assert coarse.available(_fake("UnCoupledModel", model_id=_lib.UNCOUPLED)) == list(coarse.NAMES)
    assert coarse.available(_fake("YBJModel", model_id=_lib.YBJ)) == ["ke_niw_adv"]
    assert [coarse.BITS[n] for n in coarse.NAMES] == [1, 2, 4] == [_lib.CG_KE, _lib.CG_ENS, _lib.CG_NIW]
    assert coarse.MAX_SCALES == _lib.CG_MAX_SCALES == 64
    assert "nq_coarse_flux" in _lib.EXPORTS


def test_every_refusal_comes_before_the_device():
    """models without a context: any device access would raise AttributeError instead"""
    from niwqg_amd import coarse, _lib
    qg = _fake("QGModel", nx=64, dk=0.25)
    with pytest.raises(ValueError, match="valid names: ke_qg, ens$"):
        coarse.flux_maps(qg, [4], names=["ke_niw_adv"])
    with pytest.raises(ValueError, match="valid names: ke_niw_adv$"):
        coarse.flux_maps(_fake("YBJModel", nx=64, dk=0.25, model_id=_lib.YBJ), [4], names="ens")
    c = _fake("CoupledModel", nx=64, dk=0.25, model_id=_lib.COUPLED)
    with pytest.raises(ValueError, match="valid names: ke_qg, ens, ke_niw_adv"):
        coarse.flux_maps(c, [4], names=["zeta"])
    with pytest.raises(ValueError, match="valid names"):
        coarse.flux_maps(c, [4], names=["ens", "ens"])
    with pytest.raises(ValueError, match="valid: sharp, gaussian"):
        coarse.flux_maps(c, [4], kind="tophat")
    with pytest.raises(ValueError, match="1 .. nx/2 - 1 = 31"):
        coarse.flux_maps(c, [4, 32])
    with pytest.raises(ValueError, match="length > 0"):
        coarse.flux_maps(c, [4.0, 0.0], kind="gaussian")
    with pytest.raises(ValueError, match="1 to 64"):
        coarse.flux_maps(c, [])
    with pytest.raises(ValueError, match="1 to 64"):
        coarse.flux_maps(c, list(range(1, 32)) * 3)
    with pytest.raises(ValueError, match="not both"):
        coarse.flux_maps(c, [4], table=coarse.sharp(c, 4))
    bad = coarse.sharp(c, 4)
    bad[32] = 0.5
    with pytest.raises(ValueError, match="Nyquist rule"):
        coarse.flux_maps(c, table=bad)
    with pytest.raises(ValueError, match="nb = "):
        coarse.flux_maps(c, table=np.ones(7))
    with pytest.raises(ValueError, match="valid: ke_qg, ens, ke_niw_adv"):
        coarse.reference(shim(64), coarse.sharp(c, 4), ["zeta"])
    # the grids and models without the maps: NotImplementedError that points at DESIGN.md section 7
    a = _fake("CoupledModel", nx=96, dk=0.25, model_id=_lib.COUPLED, _any_size=True)
    with pytest.raises(NotImplementedError, match="any-size.*section 7"):
        coarse.flux_maps(a, [4])
    s = _fake("CoupledModel", nx=64, dk=0.25, model_id=_lib.COUPLED, _ctx=object())
    with pytest.raises(NotImplementedError, match="slab.*section 7"):
        coarse.flux_maps(s, [4])
    big = _fake("CoupledModel", nx=8192, dk=0.25, model_id=_lib.COUPLED, _ctx=_lib.Context.__new__(_lib.Context))
    big._ctx.h = None
    with pytest.raises(NotImplementedError, match="8192.*section 7"):
        coarse.flux_maps(big, [4])


def test_entry_is_exported_and_refuses_a_null_context():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    L = _lib.lib()
    assert L.nq_coarse_flux(None, 1, 1, None, 1, None, None) == -1
