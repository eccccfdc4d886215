"""The low-mode recorder and its frequency - wavenumber spectra (niwqg_amd/frequency.py, nq_freq_*, nq_any_freq_*; DESIGN.md
section 5j): the ring against the state bit for bit, batching and wrap, no side effects, the device table against the numpy
restatement (double and extended precision), closure on the package's own spectra, a known line with its sign, determinism
and lifecycle."""
import numpy as np
import pytest

from test_gpu_forcing import pair, amplitudes
from test_oracle_golden import notebook_kwargs

pytestmark = pytest.mark.gpu

# (kind, nx, mask, K): the fused plans at 64^2; 128^2 / K = 40 crosses the 64-column wave boundary of the gather; 48^2 is the
# any-size path; "mask" (dealias without the filter) is the dual-copy context
CASES = [("coupled", 64, "filter", 8), ("qg", 64, "filter", 8), ("ybj", 64, "filter", 8), ("uncoupled", 64, "filter", 8),
         ("coupled", 64, "mask", 8), ("coupled", 128, "filter", 40), ("coupled", 48, "filter", 8)]


def model(kind, nx, mask="filter"):
    m, _, init, _ = pair(kind, nx, mask, oracle=False)
    init(m)
    return m


def block(a, nx, K, full):
    from niwqg_amd import frequency
    rows = frequency.block_index(nx, K)
    a = np.asarray(a)[rows]
    return a[:, rows] if full else a[:, :K + 1]


def state_blocks(m, fields, K):
    src = dict(phi="phih", q="qh", psi="ph")
    return {n: block(getattr(m, src[n]), m.nx, K, n == "phi") for n in fields}


# ---- 1. the ring is the state, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, nx, mask, K", CASES)
def test_ring_is_the_state(kind, nx, mask, K):
    from niwqg_amd import frequency
    m = model(kind, nx, mask)
    if mask == "mask":
        assert m._dual
    R = frequency.attach(m, K, length=16)
    assert R.fields == {"qg": ("q", "psi"), "ybj": ("phi",)}.get(kind, ("phi", "q", "psi"))
    for step in range(7):
        if step:
            m._step_forward()
        want = state_blocks(m, R.fields, K)
        for n in R.fields:
            ts = R.series(n)
            assert ts.values.shape == (step + 1, 2 * K + 1, 2 * K + 1 if n == "phi" else K + 1) and ts.values.dtype == np.complex128
            assert np.array_equal(ts.step, np.arange(step + 1)) and np.allclose(ts.t, ts.t[0] + m.dt * ts.step, rtol=1e-15, atol=0)
            assert np.any(ts.values[-1] != 0)
            assert np.array_equal(ts.values[-1], want[n]), (n, step, np.abs(ts.values[-1] - want[n]).max())
            if step:
                assert not np.array_equal(ts.values[-1], ts.values[-2]), n
    assert R.info() == {"written": 7, "held": 7, "steps": 6}
    R.detach()


# ---- 2. batching and wrap -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 48])
def test_batching_and_wrap(nx):
    from niwqg_amd import frequency
    A, B = model("coupled", nx), model("coupled", nx)
    RA, RB = (frequency.attach(m, 8, every=3, length=4) for m in (A, B))
    if nx == 64:
        A._ctx.step(11)                       # one batched call: the records are written without a host visit
    else:
        for _ in range(11):                   # (the any-size path steps from Python)
            A._step_forward()
    for i in range(11):
        B._step_forward()
    assert RA.info() == RB.info() == {"written": 4, "held": 4, "steps": 11}
    for n in RA.fields:
        a, b = RA.series(n), RB.series(n)
        assert np.array_equal(a.step, [0, 3, 6, 9]) and np.array_equal(b.step, [0, 3, 6, 9])
        assert np.array_equal(a.values, b.values), n
    if nx == 64:
        A._ctx.step(4)                        # the fifth and sixth record wrap the ring: the attach record goes first
        for _ in range(4):
            B._step_forward()
        a, b = RA.series("phi"), RB.series("phi")
        assert np.array_equal(a.step, [6, 9, 12, 15]) and np.array_equal(a.values, b.values)
        assert np.array_equal(b.values[-1], block(B.phih, 64, 8, True))
        assert RA.info() == {"written": 6, "held": 4, "steps": 15}


# ---- 3. no side effects ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
def test_no_side_effects(forced):
    from niwqg_amd import frequency, forcing
    nx = 64
    A, B = model("coupled", nx), model("coupled", nx)
    if forced:
        Aq, Aphi = amplitudes(nx, "q+phi")
        FA, FB = (forcing.attach(m, q=Aq, phi=Aphi, seed=5) for m in (A, B))
    R = frequency.attach(A, 8, length=16)
    for i in range(20):
        A._step_forward()
        B._step_forward()
        if i in (3, 11):
            R.series("q")
            R.spectrum("hann", demean=True)
    for n in ("qh", "phih", "ph"):
        assert np.array_equal(np.array(getattr(A, n)), np.array(getattr(B, n))), n
    # the hook order: the record of a forced step is the forced, re-inverted state
    for n, want in state_blocks(B, R.fields, 8).items():
        assert np.array_equal(R.series(n).values[-1], want), n


# ---- 4. the device table against the restatement -------------------------------------------------------------------------------
def run_recorded(nx, length, steps, kind="coupled"):
    from niwqg_amd import frequency
    m = model(kind, nx)
    R = frequency.attach(m, 8, length=length)
    if nx == 64:
        m._ctx.step(steps)
    else:
        for _ in range(steps):
            m._step_forward()
    return m, R


@pytest.fixture(scope="module")
def recorded():
    """(nx, length, steps) -> model and recorder, run once and only read afterwards"""
    cache = {}

    def get(nx, length, steps):
        key = (nx, length, steps)
        if key not in cache:
            cache[key] = run_recorded(nx, length, steps)
        return cache[key]
    return get


ARRAY_WINDOW = "array"


def window_of(name, T):
    if name != ARRAY_WINDOW:
        return name
    return 0.2 + np.sin(np.pi * (np.arange(T) + 0.5) / T) ** 2 * np.linspace(1.0, 1.5, T)


# T = 16 (a full ring, run past the wrap), T = 12 (Bluestein), T = 7 of 16 (a ring not yet full), the any-size model
@pytest.mark.parametrize("nx, length, steps, T", [(64, 16, 20, 16), (64, 12, 14, 12), (64, 16, 6, 7), (48, 16, 15, 16)])
@pytest.mark.parametrize("window", ["boxcar", "hann", ARRAY_WINDOW])
@pytest.mark.parametrize("demean", [False, True])
def test_spectrum_against_the_restatement(recorded, nx, length, steps, T, window, demean):
    """max |device - numpy| <= 1e-12 of the field's total sum P (the bar of the shell tables).
    Measured on MI355X over all these cases: at most 1.9e-16."""
    from niwqg_amd import frequency
    m, R = recorded(nx, length, steps)
    w = window_of(window, T)
    S = R.spectrum(w, demean=demean)
    assert len(S.omega) == T and np.all(np.diff(S.omega) > 0) and len(S.step) == T
    assert np.array_equal(S.modes, frequency.block_modes(8)) and S.k_iso_max == 8 * m.dk
    for n in R.fields:
        ts = R.series(n)
        assert len(ts.step) == T and np.array_equal(ts.step, S.step)
        omega, P = frequency.reference_spectrum(ts.values, m.dt, n, w, demean, m.nx, m.ny, dk=m.dk)
        got = S.values[n]
        assert got.shape == P.shape == (T, frequency.block_shell_count(8)) and np.array_equal(omega, S.omega)
        err = np.abs(got - P).max() / P.sum()
        print("spectrum %s nx %d T %d %s demean %d: max |device - numpy| / sum P = %.3e" % (n, nx, T, window, demean, err))
        assert P.sum() > 0 and np.all(got >= 0)
        assert err <= 1e-12


def test_spectrum_against_extended_precision(recorded):
    """the same bar against the longdouble restatement; measured on MI355X: at most 9.9e-17"""
    from niwqg_amd import frequency
    m, R = recorded(64, 16, 20)
    S = R.spectrum("hann", demean=True)
    for n in R.fields:
        x = R.series(n).values.astype(np.clongdouble)
        P = frequency.reference_spectrum(x, m.dt, n, "hann", True, m.nx, m.ny, dk=m.dk)[1]
        err = float(np.abs(S.values[n] - P).max() / P.sum())
        print("spectrum %s against longdouble: max |device - restatement| / sum P = %.3e" % (n, err))
        assert err <= 1e-12


# ---- 5. closure on the package's own spectra ------------------------------------------------------------------------------------
def test_closure_on_isotropic_spectra():
    """boxcar, b <= K: sum_p P_phi(p, b) = the mean over the records of isotropic_spectra(m, "ke_niw"), to 1e-12 of the mass"""
    from niwqg_amd import frequency
    from niwqg_amd.spectra import isotropic_spectra
    m = model("coupled", 64)
    K = 8
    R = frequency.attach(m, K, length=16)
    acc = isotropic_spectra(m, "ke_niw").values["ke_niw"].copy()
    for _ in range(15):
        m._step_forward()
        acc += isotropic_spectra(m, "ke_niw").values["ke_niw"]
    acc /= 16.0
    S = R.spectrum("boxcar")
    got = S.values["phi"].sum(axis=0)
    err = np.abs(got[:K + 1] - acc[:K + 1]).max() / acc.sum()
    print("closure on ke_niw: max over b <= K of |sum_p P - mean S| / mass = %.3e" % err)
    assert acc[:K + 1].min() > 0 and acc[:K + 1].sum() > 0.05 * acc.sum()      # the shells of the block hold energy
    assert err <= 1e-12
    assert np.abs(got[:K + 1] - acc[:K + 1]).max() <= 1e-12 * acc[:K + 1].sum()      # ... and of the block's own share of it
    assert np.all(got[K + 1:] <= acc[K + 1:len(got)] * (1 + 1e-12))      # cut shells hold part of theirs


# ---- 6. a known answer with a sign ---------------------------------------------------------------------------------------------------
def test_free_wave_lands_at_plus_omega():
    """YBJModel without flow or dissipation: phi-hat(l, k) turns as e^{-i hslash kappa^2 t / 2}.  Two modes of shell 5, dt such
    that Omega dt T = 2 pi 3: at least 1 - 1e-10 of the shell in the bin of +Omega, every other shell exactly zero."""
    import niwqg_amd
    from niwqg_amd import frequency, _lib
    nx, T, p0 = 64, 16, 3
    kw = notebook_kwargs(nx, False)
    kw.update(U=0.0, nuw=0.0, nu4w=0.0, muw=0.0, use_filter=False)
    probe = niwqg_amd.YBJModel.Model(**kw)
    Om = 0.5 * probe.f * 25 * probe.dk ** 2 / probe.kappa2
    kw["dt"] = 2 * np.pi * p0 / (Om * T)
    m = niwqg_amd.YBJModel.Model(**kw)
    m.set_q(np.zeros((nx, nx)))
    ph = np.zeros((nx, nx), complex)
    ph[4, 3] = (0.3 - 0.4j) * nx * nx
    ph[5, 0] = (0.1 + 0.2j) * nx * nx
    m.set_phi(np.fft.ifft2(ph))
    # the transform of set_phi leaves rounding in every other mode: the two-mode phi-hat itself goes in (the C ABI's upload)
    c = m._ctx
    c._chk(c.L.nq_upload_spectral(c.h, 1, _lib._dptr(np.ascontiguousarray(ph).view(np.float64))), "nq_upload_spectral")
    assert np.array_equal(m._ctx.field(_lib.F_PHIH), ph)
    R = frequency.attach(m, 8, length=T)
    m._ctx.step(T - 1)
    S = R.spectrum("boxcar")
    P = S.values["phi"]
    ip = int(np.argmin(np.abs(S.omega - Om)))
    assert abs(S.omega[ip] - Om) <= 1e-12 * Om and S.omega[ip] > 0
    frac = P[ip, 5] / P[:, 5].sum()
    print("free wave: fraction of shell 5 in the bin of +Omega: 1 - %.3e" % (1 - frac))
    assert P[:, 5].sum() > 0 and frac >= 1 - 1e-10
    assert np.all(np.delete(P, 5, axis=1) == 0.0)
    want = 0.5 * (abs(0.3 - 0.4j) ** 2 + abs(0.1 + 0.2j) ** 2)               # ke_niw of the two modes
    assert abs(P[:, 5].sum() - want) <= 1e-12 * want


# ---- 7. determinism and lifecycle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 48])
def test_determinism_and_lifecycle(nx):
    from niwqg_amd import frequency
    m = model("coupled", nx)
    m._step_forward()                         # (what the first step allocates on its own is there before the count)
    b0 = m._ctx.device_bytes()
    with pytest.raises(ValueError, match="not available for CoupledModel; valid names: phi, q, psi"):
        frequency.attach(m, 8, fields=["phi", "u"])
    R = frequency.attach(m, 8, length=12)
    if nx == 64:
        assert m._ctx.device_bytes() >= b0 + 12 * 17 * (17 + 9 + 9) * 16
    with pytest.raises(ValueError, match="attached already"):
        frequency.attach(m, 4)
    with pytest.raises(ValueError, match="at least 2"):
        R.spectrum()
    for _ in range(8):
        m._step_forward()
    with pytest.raises(ValueError, match="9 records are held"):
        R.spectrum(np.ones(12))
    a, b = R.spectrum("hann"), R.spectrum("hann")
    for n in R.fields:
        assert np.array_equal(a.values[n], b.values[n]) and a.values[n].sum() > 0, n
    only = R.spectrum("hann", fields="q")
    assert list(only.values) == ["q"] and np.array_equal(only.values["q"], a.values["q"])
    R.detach()
    R.detach()
    if nx == 64:
        assert m._ctx.device_bytes() == b0
        with pytest.raises(RuntimeError, match="nq_freq_info"):
            m._ctx.freq_info()
    with pytest.raises(RuntimeError, match="detached"):
        R.series("phi")
    frequency.attach(m, 4, length=2, fields="psi").detach()


def test_one_recorder_per_context_in_the_library():
    m = model("qg", 64)
    c = m._ctx
    with pytest.raises(RuntimeError, match="no wave field"):
        c.freq_attach(8, 1, 4, [0])
    c.freq_attach(8, 1, 4, [1, 2])
    assert c.L.nq_freq_attach(c.h, 8, 1, 4, 0, None) == -4
    with pytest.raises(RuntimeError, match="attached already"):
        c.freq_attach(8, 1, 4, [1])
    with pytest.raises(RuntimeError, match="not recorded"):
        c.freq_series(0, 1, 17, 17)
    c.freq_detach()
    with pytest.raises(RuntimeError, match="kmax = 32"):
        c.freq_attach(32, 1, 4, [1])


def test_slab_ranks_refuse():
    import ctypes
    import niwqg_amd
    from niwqg_amd import frequency, _lib
    m = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        frequency.attach(m, 8)
    lib = _lib.lib()
    h = m._ctx.sim.ranks[0].h
    f = (ctypes.c_int * 1)(0)
    i3 = (ctypes.c_longlong * 3)()
    w = np.ones(4)
    assert lib.nq_freq_attach(h, 8, 1, 4, 1, f) == -4
    assert lib.nq_freq_detach(h) == -4
    assert lib.nq_freq_info(h, i3) == -4
    assert lib.nq_freq_series(h, 0, None, None) == -4
    assert lib.nq_freq_spectrum(h, 0, _lib._dptr(w), 0, 1.0, 12, _lib._dptr(w)) == -4
