"""The shell-to-shell transfers' numpy restatement (niwqg_amd/shelltoshell.py: reference) against a numpy restatement of the four
transfer rows written here: closure over the donor bands, antisymmetry of the band-to-band matrices where it holds and its
failure where it does not, a single triad, the band builder and every refusal of the contract.  No GPU.

Bounds: 1e-12 of sum_{Q, b} |T(b | Q)| of the name, the figures of DESIGN.md section 5p (closure <= 1.1e-15, antisymmetry
<= 1e-15 on 64^2 .. 256^2)."""
import types

import numpy as np
import pytest

NAMES = ("ke_qg", "ens", "ke_niw_adv", "ke_niw_ref")


def shells(nx):
    from niwqg_amd.spectra import shell_of
    n = np.append(np.arange(0, nx // 2), np.arange(-(nx // 2), 0))
    return shell_of(n[None, :], n[:, None])


def shim(nx, top, seed=0):
    """a broadband (white) state with nothing on the shells > top, as the public reads of a Kernel-family model give it"""
    rng = np.random.default_rng(seed + nx)
    dk = 2 * np.pi / (2 * np.pi * 3.0)
    kk = dk * np.append(np.arange(0., nx / 2), np.arange(-nx / 2, 0.))
    kx, ly = kk[None, :], kk[:, None]
    keep = shells(nx) <= top

    def field(cplx):
        z = rng.standard_normal((nx, nx)) + (1j * rng.standard_normal((nx, nx)) if cplx else 0)
        z = np.fft.ifft2(np.fft.fft2(z) * keep)
        return z if cplx else z.real
    psi = field(False)
    ph = np.fft.fft2(psi)
    q = np.fft.ifft2(-(kx ** 2 + ly ** 2) * ph).real / (dk * top) ** 2 + 0.3 * field(False)
    return types.SimpleNamespace(nx=nx, dk=dk, kk=kk, ll=kk.copy(), ph=ph, q=q, q_psi=q - 0.4 * field(False), phih=np.fft.fft2(field(True)))


def transfer_rows(m):
    """T(b) of the four names from the host fields (tests/test_gpu_transfer.py: restated)"""
    from niwqg_amd.spectra import shell_count
    nx, M2 = m.nx, float(m.nx) ** 4
    b, nb = shells(nx).ravel(), shell_count(nx)
    kx, ly = m.kk[None, :], m.ll[:, None]
    F, Fi = np.fft.fft2, np.fft.ifft2
    P = F(Fi(m.ph).real)
    u, v = Fi(-1j * ly * P).real, Fi(1j * kx * P).real
    Jq = 1j * kx * F(u * m.q) + 1j * ly * F(v * m.q)
    W = m.phih
    J = F(u * Fi(1j * kx * W) + v * Fi(1j * ly * W))
    R = 1j * F(Fi(W) * m.q_psi)

    def binned(x):
        return np.bincount(b, weights=np.ravel(x), minlength=nb)
    return dict(ke_qg=binned((np.conj(P) * Jq).real) / M2, ens=-binned((np.conj(F(m.q)) * Jq).real) / M2,
                ke_niw_adv=-binned((np.conj(W) * J).real) / M2, ke_niw_ref=-0.5 * binned((np.conj(W) * R).real) / M2)


def sharp_edges(nx):
    """0, 1, 2, 3, 4, 6, 8, 12, ... , nx/2"""
    e, x = [0, 1, 2, 3], 4
    while x < nx // 2:
        e += [x, x + x // 2]
        x *= 2
    return [i for i in e if i < nx // 2] + [nx // 2]


def smooth_tables(nx):
    """overlapping Gaussian bumps on a logarithmic ladder of centres, normalised to sum to one on every shell below nx/2"""
    from niwqg_amd.spectra import shell_count
    b = np.arange(shell_count(nx), dtype=np.float64)
    centres = [0.0, 1.5, 3.0, 6.0, 12.0, 24.0, 48.0][:5 + (nx > 64)]
    t = np.array([np.exp(-((b - c) / (0.6 * c + 1.0)) ** 2) for c in centres]) + 1e-3
    t /= t.sum(axis=0)
    t[:, nx // 2:] = 0.0
    return t


def tables(nx, which):
    from niwqg_amd import shelltoshell
    m = types.SimpleNamespace(nx=nx)
    return shelltoshell.bands(m, sharp_edges(nx)) if which == "sharp" else smooth_tables(nx)


def antisymmetry(tab, rows):
    """(max |M + M^T|, sum |T(b | Q)|) of M[K, Q] = sum_b g_K[b] T(b | Q)"""
    M = tab @ rows.T
    return np.abs(M + M.T).max(), np.abs(rows).sum()


@pytest.fixture(scope="module")
def refs():
    """(nx, top, which) -> (state, tables, reference rows), formed once"""
    cache = {}

    def get(nx, top, which):
        from niwqg_amd import shelltoshell
        if (nx, top, which) not in cache:
            m, tab = shim(nx, top), tables(nx, which)
            cache[(nx, top, which)] = (m, tab, shelltoshell.reference(m, tab))
        return cache[(nx, top, which)]
    return get


def test_the_edges_of_the_issue():
    assert sharp_edges(64) == [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32]
    assert sharp_edges(128) == [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64]
    for nx in (64, 128):
        t = smooth_tables(nx)
        assert np.allclose(t[:, :nx // 2].sum(axis=0), 1.0, rtol=0, atol=4e-16) and not t[:, nx // 2:].any()
        assert ((t[:, :nx // 2] > 1e-4).sum(axis=0) >= 2).all()            # they overlap on every shell


@pytest.mark.parametrize("which", ["sharp", "smooth"])
@pytest.mark.parametrize("nx", [64, 128])
def test_closure_over_the_donor_bands(refs, nx, which):
    from niwqg_amd.spectra import shell_count
    m, tab, R = refs(nx, nx // 2 - 1, which)
    T = transfer_rows(m)
    assert sorted(R) == sorted(NAMES)
    for name in NAMES:
        assert R[name].shape == (len(tab), shell_count(nx)) and R[name].dtype == np.float64
        err, scale = np.abs(R[name].sum(axis=0) - T[name]).max(), np.abs(R[name]).sum()
        print("%d %s %s: closure %.3g" % (nx, which, name, err / scale))
        assert scale > 0 and np.abs(T[name]).sum() > 1e-3 * scale and err <= 1e-12 * scale, (name, err, scale)


@pytest.mark.parametrize("which", ["sharp", "smooth"])
@pytest.mark.parametrize("nx", [64, 128])
def test_antisymmetry_and_zero_diagonal(refs, nx, which):
    m, tab, R = refs(nx, nx // 2 - 1, which)
    err, scale = antisymmetry(tab, R["ke_niw_ref"])                    # any state, aliased or not
    print("%d %s ke_niw_ref: %.3g" % (nx, which, err / scale))
    assert scale > 0 and err <= 1e-12 * scale
    m, tab, R = refs(nx, (nx - 1) // 3, which)                         # alias-free triple products
    for name in ("ens", "ke_niw_adv", "ke_niw_ref"):
        err, scale = antisymmetry(tab, R[name])
        print("%d %s %s: %.3g" % (nx, which, name, err / scale))
        assert scale > 0 and err <= 1e-12 * scale, (name, err, scale)
        assert np.abs(np.diag(tab @ R[name].T)).max() <= 1e-12 * scale
        assert np.abs(tab @ R[name].T).max() > 1e-3 * scale            # the matrix itself is not small


@pytest.mark.parametrize("which", ["sharp", "smooth"])
@pytest.mark.parametrize("nx", [64, 128])
def test_the_antisymmetry_is_not_vacuous(refs, nx, which):
    """with the band limit at nx/2 - 1 the triple products alias: ens and ke_niw_adv miss antisymmetry by more than 1e-3 of
    sum |T|; ke_qg (receiver psi, donor q: different fields) is not antisymmetric on any state"""
    m, tab, R = refs(nx, nx // 2 - 1, which)
    for name in ("ens", "ke_niw_adv", "ke_qg"):
        err, scale = antisymmetry(tab, R[name])
        print("%d %s %s at nx/2 - 1: %.3g" % (nx, which, name, err / scale))
        assert err > 1e-3 * scale, (name, err, scale)
    m, tab, R = refs(nx, (nx - 1) // 3, which)
    err, scale = antisymmetry(tab, R["ke_qg"])
    print("%d %s ke_qg at (nx - 1) // 3: %.3g" % (nx, which, err / scale))
    assert err > 1e-3 * scale


def test_single_triad():
    """psi on one mode p, q on p and one other mode r: u . grad q^Q vanishes for the donor band of p (parallel wavevectors) and
    lives on p +- r for the donor band of r, so the ens rows are zero outside (donor band of r, receiver shells of p +- r).  With
    q on p + r as well the triad is closed and those entries are there: band(r) -> shell(p + r) and band(p + r) -> shell(r)."""
    from niwqg_amd import shelltoshell
    from niwqg_amd.spectra import shell_of
    nx = 64
    m = shim(nx, 8)
    x = np.arange(nx) * 2 * np.pi * 3.0 / nx
    X, Y = np.meshgrid(x, x)
    p, r = (3, 1), (2, 9)                                              # shells 3 and 9; p + r = (5, 10): 11, p - r = (1, -8): 8

    def wave(a, amp, phase):
        return amp * np.cos(a[0] * m.dk * X + a[1] * m.dk * Y + phase)
    sh = lambda a: int(shell_of(a[0], a[1]))
    assert (sh(p), sh(r), sh((5, 10)), sh((1, -8))) == (3, 9, 11, 8)
    edges = [0, 2, 5, 9, 10, 12, 32]                                   # bands: p in 1, r in 3, p - r in 2, p + r in 4
    tab = shelltoshell.bands(m, edges)
    m.ph = np.fft.fft2(wave(p, 0.7, 0.3))
    scale = 0.7 * np.hypot(*p) * m.dk * np.hypot(*r) * m.dk * 1.0       # |u| |grad q| |q| of unit-amplitude q modes
    for closed in (False, True):
        m.q = wave(p, 1.0, 0.3) + wave(r, 1.0, 1.1) + (wave((5, 10), 1.0, -0.4) if closed else 0.0)
        E = shelltoshell.reference(m, tab, "ens")["ens"]
        allowed = np.zeros_like(E, dtype=bool)
        allowed[3, [8, 11]] = True                                     # donor band of r, receiver shells of p -+ r
        if closed:
            allowed[4, [9]] = True                                     # donor p + r: (p + r) - p = r  [(p + r) + p is not in q]
        assert np.abs(E[~allowed]).max() <= 1e-12 * scale, np.abs(E[~allowed]).max() / scale
        if closed:
            assert abs(E[3, 11]) > 1e-2 * scale and abs(E[4, 9]) > 1e-2 * scale
            assert abs(E[3, 11] + E[4, 9]) <= 1e-12 * scale            # what shell 11 gains from r, r's shell loses to p + r
            assert abs(E[3, 8]) <= 1e-12 * scale                       # nothing of q at p - r to receive it


def test_band_builder():
    from niwqg_amd import shelltoshell
    from niwqg_amd.spectra import shell_count
    m = types.SimpleNamespace(nx=64, dk=0.25)
    nb = shell_count(64)
    t = shelltoshell.bands(m, [0, 1, 2, 4, 8, 16, 32])
    assert t.shape == (6, nb) and t.dtype == np.float64 and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t.sum(axis=0), (np.arange(nb) < 32).astype(float))
    assert np.array_equal(np.nonzero(t[3])[0], [4, 5, 6, 7]) and np.array_equal(np.nonzero(t[0])[0], [0])
    assert np.array_equal(shelltoshell.bands(m, [3, 7])[0], ((np.arange(nb) >= 3) & (np.arange(nb) < 7)).astype(float))
    assert shelltoshell.bands(m, np.arange(33)).shape == (32, nb)
    for bad in ([0], [], [0, 0, 4], [4, 2], [0, 33], [-1, 4], [0, 2.5], [0, np.nan], [[0, 1], [2, 3]], 5):
        with pytest.raises(ValueError, match=r"valid: increasing integer shells .* nx/2 = 32 .* 64 bands"):
            shelltoshell.bands(m, bad)
    big = types.SimpleNamespace(nx=256)
    assert shelltoshell.bands(big, np.arange(65)).shape == (64, shell_count(256))
    with pytest.raises(ValueError, match="64 bands"):
        shelltoshell.bands(big, np.arange(66))
    # tables: coarse.check_table's contract under this module's name
    assert shelltoshell.check_table(64, t[2]).shape == (1, nb)
    bad = t.copy()
    bad[1, 32] = 1e-300
    with pytest.raises(ValueError, match="shelltoshell: .*Nyquist rule"):
        shelltoshell.check_table(64, bad)
    bad = t.copy()
    bad[0, 3] = np.inf
    with pytest.raises(ValueError, match="finite"):
        shelltoshell.check_table(64, bad)
    with pytest.raises(ValueError, match="nb = %d" % nb):
        shelltoshell.check_table(64, np.ones(nb - 1))
    with pytest.raises(ValueError, match="1 <= nbands <= 64"):
        shelltoshell.check_table(64, np.zeros((65, nb)))


def _fake(module, **attrs):
    cls = __import__("niwqg_amd." + module, fromlist=["Model"]).Model
    m = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_available_per_class_and_the_constants():
    from niwqg_amd import shelltoshell, transfer, _lib
    import niwqg_amd
    assert niwqg_amd.shelltoshell is shelltoshell
    assert shelltoshell.NAMES == NAMES
    assert shelltoshell.available(_fake("QGModel")) == ["ke_qg", "ens"]
    assert shelltoshell.available(_fake("CoupledModel", model_id=_lib.COUPLED)) == list(NAMES)
    assert shelltoshell.available(_fake("UnCoupledModel", model_id=_lib.UNCOUPLED)) == list(NAMES)
    assert shelltoshell.available(_fake("YBJModel", model_id=_lib.YBJ)) == ["ke_niw_adv", "ke_niw_ref"]
    assert (_lib.S2S_Q, _lib.S2S_ADV, _lib.S2S_REF, _lib.S2S_ROWS, _lib.S2S_MAX_BANDS) == (1, 2, 4, 4, 64)
    assert [shelltoshell.BITS[n] for n in NAMES] == [1, 1, 2, 4] and shelltoshell.MAX_BANDS == 64
    assert shelltoshell.ROWS == {n: transfer.ROWS[n] for n in NAMES}   # the rows and factors of nq_transfer_binned
    assert "nq_shell_transfer" in _lib.EXPORTS


def test_every_refusal_comes_before_the_device():
    """models without a context: any device access would raise AttributeError instead"""
    from niwqg_amd import shelltoshell, _lib
    s2s = shelltoshell.shell_to_shell
    qg = _fake("QGModel", nx=64, dk=0.25)
    with pytest.raises(ValueError, match="valid names: ke_qg, ens$"):
        s2s(qg, [0, 4], names=["ke_niw_ref"])
    with pytest.raises(ValueError, match="valid names: ke_niw_adv, ke_niw_ref$"):
        s2s(_fake("YBJModel", nx=64, dk=0.25, model_id=_lib.YBJ), [0, 4], names="ens")
    c = _fake("CoupledModel", nx=64, dk=0.25, model_id=_lib.COUPLED)
    with pytest.raises(ValueError, match="valid names: ke_qg, ens, ke_niw_adv, ke_niw_ref"):
        s2s(c, [0, 4], names=["zeta"])
    with pytest.raises(ValueError, match="valid names"):
        s2s(c, [0, 4], names=["ens", "ens"])
    with pytest.raises(ValueError, match="valid names"):
        s2s(c, [0, 4], names=[])
    with pytest.raises(ValueError, match="valid: increasing integer shells"):
        s2s(c, [0, 4, 33])
    with pytest.raises(ValueError, match="valid: increasing integer shells"):
        s2s(c, [4])
    with pytest.raises(ValueError, match="valid: one of them"):
        s2s(c, [0, 4], table=shelltoshell.bands(c, [0, 4]))
    with pytest.raises(ValueError, match="valid: one of them"):
        s2s(c)
    bad = shelltoshell.bands(c, [0, 4])
    bad[0, 32] = 0.5
    with pytest.raises(ValueError, match="Nyquist rule"):
        s2s(c, table=bad)
    with pytest.raises(ValueError, match="nb = "):
        s2s(c, table=np.ones(7))
    with pytest.raises(ValueError, match="valid: ke_qg, ens, ke_niw_adv, ke_niw_ref"):
        shelltoshell.reference(shim(64, 8), shelltoshell.bands(c, [0, 4]), ["zeta"])
    # the grids and models without the transfers: NotImplementedError that points at DESIGN.md section 7
    a = _fake("CoupledModel", nx=96, dk=0.25, model_id=_lib.COUPLED, _any_size=True)
    with pytest.raises(NotImplementedError, match="any-size.*section 7"):
        s2s(a, [0, 4])
    s = _fake("CoupledModel", nx=64, dk=0.25, model_id=_lib.COUPLED, _ctx=object())
    with pytest.raises(NotImplementedError, match="slab.*section 7"):
        s2s(s, [0, 4])
    big = _fake("CoupledModel", nx=8192, dk=0.25, model_id=_lib.COUPLED, _ctx=_lib.Context.__new__(_lib.Context))
    big._ctx.h = None
    with pytest.raises(NotImplementedError, match="8192.*section 7"):
        s2s(big, [0, 4])


def test_half_plane_psi_of_qgmodel():
    """QGModel's public reads: psi-hat on kx = 0 .. nx/2; reference forms u, v with irfft2 as coarse.reference does, and closes on
    the transfer rows formed the same way"""
    from niwqg_amd import shelltoshell
    from niwqg_amd.spectra import shell_count
    nx = 64
    f = shim(nx, nx // 2 - 1)
    h = nx // 2 + 1
    ph = np.fft.rfft2(np.fft.ifft2(f.ph).real)
    m = types.SimpleNamespace(nx=nx, dk=f.dk, kk=f.kk[:h].copy(), ll=f.ll, ph=ph, q=f.q)
    m.kk[-1] = abs(m.kk[-1])
    tab = tables(nx, "sharp")
    R = shelltoshell.reference(m, tab)
    assert sorted(R) == ["ens", "ke_qg"]
    T = transfer_rows(f)
    for name in R:
        err, scale = np.abs(R[name].sum(axis=0) - T[name]).max(), np.abs(R[name]).sum()
        assert R[name].shape == (len(tab), shell_count(nx)) and err <= 1e-12 * scale, (name, err, scale)


def test_entry_is_exported_and_refuses_a_null_context():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    L = _lib.lib()
    assert L.nq_shell_transfer(None, 1, 1, None, 1, None) == -1
