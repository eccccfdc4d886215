"""Lagrangian particles (niwqg_amd/particles.py, nq_particles_*, nq_any_particles_rk4 / nq_any_interp): positions against a
numpy restatement of the contract written here (velocity from m.ph, Keys interpolation, RK4 linear in time), bit-identical
model outputs with and without particles, state changes between steps, exact flows, records and sampling, the any-size grids,
determinism, non-finite states, slab ranks and ensembles."""
import numpy as np
import pytest

from test_gpu_spectra import make, LEFTOVERS, ATOMIC
from test_particles_host import interp as interpolate

pytestmark = pytest.mark.gpu


# ---- the restatement -----------------------------------------------------------------------------------------------------
def velocity(m):
    """(u, v) of the psi-hat the model holds: u = -d psi/dy, v = d psi/dx (Kernel family: Re ifft2 of the full plane; QGModel:
    irfft2 of its half plane)"""
    nx = m.nx
    k = np.fft.fftfreq(nx, 1.0 / nx) * m.dk
    kx, ly = k[None, :], k[:, None]
    ph = np.array(m.ph)
    if ph.shape[1] == nx:
        return np.fft.ifft2(-1j * ly * ph).real, np.fft.ifft2(1j * kx * ph).real
    kh = np.fft.rfftfreq(nx, 1.0 / nx)[None, :] * m.dk
    return np.fft.irfft2(-1j * ly * ph, s=(nx, nx)), np.fft.irfft2(1j * kh * ph, s=(nx, nx))


def rk4(x, y, U0, U1, Ub, dt, L):
    a, b = U0[0] + 1j * U0[1], U1[0] + 1j * U1[1]

    def vel(px, py, which):
        if which == 0:
            w = interpolate(a, px, py, L)
        elif which == 1:
            w = interpolate(b, px, py, L)
        else:
            w = 0.5 * (interpolate(a, px, py, L) + interpolate(b, px, py, L))
        return w.real + Ub, w.imag
    k1 = vel(x, y, 0)
    k2 = vel(x + 0.5 * dt * k1[0], y + 0.5 * dt * k1[1], 2)
    k3 = vel(x + 0.5 * dt * k2[0], y + 0.5 * dt * k2[1], 2)
    k4 = vel(x + dt * k3[0], y + dt * k3[1], 1)
    return (x + dt / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0]), y + dt / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1]))


def particle_set(m, n, seed=5):
    """random points plus nodes, the periodic seam, negative and far-out coordinates"""
    L, dx = m.L, m.L / m.nx
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
    special = [((i + 0.5) * dx, (j + 0.5) * dx) for i, j in ((0, 0), (3, 7), (m.nx - 1, m.nx - 1))]
    special += [(0.0, 0.0), (L, 0.5 * L), (np.nextafter(L, 0), np.nextafter(L, 0)), (-0.3 * L, -2.7 * L), (41.2 * L, -17.9 * L),
                (-1e-300, 3 * L), (350.5 * L, 0.25 * L)]
    for i, (a, b) in enumerate(special[:n]):
        x[i], y[i] = a, b
    return x, y


def set_tmax(m, nsteps):
    m.tmax = m.t + (nsteps - 0.5) * m.dt


def outputs(m, kind):
    """everything a run leaves that particles must not change"""
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    out = {"qh": np.array(m.qh), "ph": np.array(m.ph), "u": np.array(m.u), "v": np.array(m.v), "q": np.array(m.q)}
    if kind in ("coupled", "uncoupled", "ybj"):
        out["phih"] = np.array(m.phih)
    for name in LEFTOVERS.get(kind, ()):
        try:
            out["left_" + name] = np.array(getattr(m, name))
        except AttributeError:
            pass
    for name, d in m.diagnostics.items():
        if d.get("active"):
            out["diag_" + name] = np.array([d["value"], d["count"]], dtype=object)
    for name in ("ke", "kew", "pew", "cfl", "Ke", "Pw", "Kw", "t", "tc"):
        if name in m.__dict__:
            out["s_" + name] = np.array(m.__dict__[name])
    out.update({"spec_" + k: v for k, v in isotropic_spectra(m).values.items()})
    out.update({"tr_" + k: v for k, v in spectral_transfer(m).transfer.items()})
    return out


def _rounded(key, kind):
    """the outputs the package reduces with floating-point atomics (test_gpu_spectra.ATOMIC): their last bits differ between ANY
    two runs, with or without particles.  Besides those, the status line's ke, kew and pew are nq_get_scalar values that
    k_reduce sums with atomicAdd (the tick's ke_niw series is not: it is compared bit for bit).  Everything else is compared bit
    for bit."""
    if not key.startswith(("diag_", "s_", "left_")):
        return False
    name = key.split("_", 1)[1]
    if key.startswith("diag_"):
        name = "diag:" + name
        if name in ("diag:ep_phi", "diag:chi_phi") and kind == "coupled":
            return False
        return name in ATOMIC
    if key.startswith(("s_", "left_")):
        return name in ATOMIC or (key.startswith("s_") and name in ("ke", "kew", "pew"))
    return False


def assert_same(a, b, kind):
    assert sorted(a) == sorted(b)
    for k in a:
        p, q = a[k], b[k]
        if p.dtype == object:                              # a diagnostics series: [value, count]
            p, q = [np.asarray(v, float) for v in p], [np.asarray(v, float) for v in q]
        else:
            p, q = [p], [q]
        for u, w in zip(p, q):
            if _rounded(k, kind):
                assert np.allclose(u, w, rtol=1e-12, atol=0, equal_nan=True), k
            else:
                assert np.array_equal(u, w, equal_nan=True), k


def check_run(kind, nx, mask="filter", n=1000, nsteps=20, **extra):
    from niwqg_amd import particles
    A = make(kind, nx, mask, tdiags=3, **extra)
    C = make(kind, nx, mask, tdiags=3, **extra)
    B = make(kind, nx, mask, tdiags=3, **extra)
    for m in (A, B, C):
        m.twrite = 5
        set_tmax(m, nsteps)
    x, y = particle_set(A, n)
    P = particles.attach(A, x, y)
    A.run()
    C.run()
    # the restatement on the twin, one step at a time
    U0 = velocity(B)
    for _ in range(nsteps):
        B._step_forward()
        U1 = velocity(B)
        x, y = rk4(x, y, U0, U1, B.U, B.dt, B.L)
        U0 = U1
    assert A.tc == B.tc == nsteps
    xa, ya = P.positions()
    tol = 1e-12 * A.L
    assert np.max(np.abs(xa - x)) <= tol and np.max(np.abs(ya - y)) <= tol, (np.max(np.abs(xa - x)), np.max(np.abs(ya - y)))
    assert np.max(np.abs(xa - x0(A, n)[0])) > 1e-5 * A.L                # they did move (far beyond the tolerance)
    assert_same(outputs(A, kind), outputs(C, kind), kind)
    P.detach()
    if not getattr(A, "_any_size", False):           # the twin without particles made the same lazy allocations
        assert A._ctx.device_bytes() == C._ctx.device_bytes()


def x0(m, n):
    return particle_set(m, n)


CLASSES = ("coupled", "uncoupled", "ybj", "qg")


@pytest.mark.parametrize("nx", [64, 256, 1024])
@pytest.mark.parametrize("kind", CLASSES)
def test_restatement_fused(kind, nx):
    check_run(kind, nx)


@pytest.mark.parametrize("kind,mask", [("coupled", "mask"), ("uncoupled", "mask"), ("coupled", "none"), ("ybj", "none"),
                                       ("qgc", "filter"), ("coupled", "dual"), ("qgc", "none")])
def test_restatement_masks_and_scalar(kind, mask):
    check_run(kind, 128, mask)


@pytest.mark.parametrize("kind,nx", [("coupled", 128), ("qg", 128), ("uncoupled", 512), ("qg", 512), ("coupled", 2048),
                                     ("coupled", 4096), ("ybj", 4096), ("qg", 8192)])
def test_restatement_every_size(kind, nx):
    if nx > 1024:
        check_run(kind, nx, n=10 ** 4, nsteps=3)
    else:
        check_run(kind, nx, nsteps=8)


@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj", "qgc"])
def test_state_changes_between_steps(kind):
    from niwqg_amd import particles
    m = make(kind, 128, "filter")
    rng = np.random.default_rng(9)
    x, y = particle_set(m, 500)
    P = particles.attach(m, x, y)
    U0 = velocity(m)

    def step():
        nonlocal x, y, U0
        m._step_forward()
        U1 = velocity(m)
        x, y = rk4(x, y, U0, U1, m.U, m.dt, m.L)
        U0 = U1
    step()
    step()
    m.set_q(m.q * 0.7 + 0.1 * m.q.std() * rng.standard_normal(m.q.shape))
    U0 = velocity(m)
    step()
    if kind != "qgc":
        ph_before = np.array(m.ph)
        m.set_phi(m.phi * 1.3)
        if kind == "coupled":                      # quirk Q2: set_phi does not re-invert; U0 is what the first stage sees
            assert np.array_equal(np.array(m.ph), ph_before)
        U0 = velocity(m)
        step()
    else:
        m.set_c(np.roll(m.c, 3, axis=0))
        U0 = velocity(m)
        step()
    if kind != "ybj":
        m._invert()
        U0 = velocity(m)
    step()
    step()
    xa, ya = P.positions()
    assert max(np.max(np.abs(xa - x)), np.max(np.abs(ya - y))) <= 1e-12 * m.L


# ---- exact flows -----------------------------------------------------------------------------------------------------------
def _euler_model(kind, nx, dt, U=0.0):
    import niwqg_amd
    L = 2 * np.pi * 1e5
    kw = dict(nx=nx, L=L, dt=dt, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9, use_filter=False, nu4=0.0, nu=0.0, mu=0.0, U=U)
    if kind == "qg":
        return niwqg_amd.QGModel.Model(beta=0.0, **kw)
    return niwqg_amd.YBJModel.Model(nu4w=0.0, nuw=0.0, muw=0.0, **kw)


def _cellular(m, B=1e4, k0=3):
    """psi = B sin(k0 X) sin(k0 Y), X = 2 pi x / L: a steady Euler state (q = -2 k^2 psi)"""
    X, Y = np.meshgrid((np.arange(m.nx) + 0.5) * m.L / m.nx, (np.arange(m.nx) + 0.5) * m.L / m.nx)
    k = k0 * 2 * np.pi / m.L
    psi = B * np.sin(k * X) * np.sin(k * Y)
    m.set_q(-2 * k * k * psi)
    return B, k


def _analytic_rk4(x, y, B, k, dt, n):
    for _ in range(n):
        def f(px, py):
            return -B * k * np.sin(k * px) * np.cos(k * py), B * k * np.cos(k * px) * np.sin(k * py)
        k1 = f(x, y)
        k2 = f(x + dt / 2 * k1[0], y + dt / 2 * k1[1])
        k3 = f(x + dt / 2 * k2[0], y + dt / 2 * k2[1])
        k4 = f(x + dt * k3[0], y + dt * k3[1])
        x, y = x + dt / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0]), y + dt / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1])
    return x, y


@pytest.mark.parametrize("kind", ["qg", "ybj"])
def test_exact_cellular_flow(kind):
    from niwqg_amd import particles
    T = 4.0e4
    n = 64
    rng = np.random.default_rng(3)
    errs_t, errs_x, psis = [], [], []
    for dt in (4000.0, 2000.0, 1000.0):
        m = _euler_model(kind, 64, dt)
        B, k = _cellular(m)
        x0_, y0_ = rng.uniform(0, m.L, n), rng.uniform(0, m.L, n)
        P = particles.attach(m, x0_, y0_)
        m._ctx.step(int(round(T / dt)))
        x, y = P.positions()
        # the same interpolated field, fine dt
        U = velocity(m)
        xf, yf = x0_.copy(), y0_.copy()
        for _ in range(int(round(T / 50.0))):
            xf, yf = rk4(xf, yf, U, U, 0.0, 50.0, m.L)
        errs_t.append(np.max(np.hypot(x - xf, y - yf)))
        psis.append(np.max(np.abs(np.sin(k * x) * np.sin(k * y) - np.sin(k * x0_) * np.sin(k * y0_))))
        rng = np.random.default_rng(3)
    # Keys' kernel is C^1: its second derivative jumps at every grid line, so RK4 on the interpolated field commits an O(dt^3)
    # local error at each crossing; the crossings over a fixed time do not depend on dt, so the global error is third order
    assert errs_t[0] / errs_t[1] >= 7 and errs_t[1] / errs_t[2] >= 7, errs_t
    assert max(psis) < 1e-2, psis
    # space: against the analytic field at a fine dt, 64^2 then 128^2
    for nx in (64, 128):
        m = _euler_model(kind, nx, 500.0)
        B, k = _cellular(m)
        rng = np.random.default_rng(4)
        x0_, y0_ = rng.uniform(0, m.L, n), rng.uniform(0, m.L, n)
        P = particles.attach(m, x0_, y0_)
        m._ctx.step(80)
        x, y = P.positions()
        xa, ya = _analytic_rk4(x0_, y0_, B, k, 500.0, 80)
        errs_x.append(np.max(np.hypot(x - xa, y - ya)))
    assert errs_x[0] / errs_x[1] >= 6, errs_x


def test_zonal_jet_with_uniform_flow():
    from niwqg_amd import particles
    m = _euler_model("qg", 64, 1000.0, U=0.3)
    X, Y = np.meshgrid((np.arange(64) + 0.5) * m.L / 64, (np.arange(64) + 0.5) * m.L / 64)
    k = 2 * 2 * np.pi / m.L
    m.set_q(-k * k * 1e4 * np.cos(k * Y))                     # psi = 1e4 cos(k y): u = 1e4 k sin(k y), v = 0
    x0_, y0_ = particle_set(m, 100)
    y0_ = np.fmod(np.abs(y0_), m.L)
    P = particles.attach(m, x0_, y0_)
    m._ctx.step(30)
    x, y = P.positions()
    assert np.max(np.abs(y - y0_)) <= 1e-12 * m.L            # v = 0 up to the rounding of the transforms
    u = velocity(m)[0][:, 0]
    uy = interpolate(np.tile(u[:, None], (1, 64)), x0_, y0_, m.L)
    want = x0_ + (0.3 + uy) * 30 * 1000.0
    assert np.max(np.abs(x - want)) <= 1e-9 * m.L


# ---- records and sampling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "ybj", "qg"])
def test_records_and_sampling(kind):
    from niwqg_amd import particles
    m = make(kind, 128, "filter", tdiags=3)
    m.twrite = 5
    names = ("u", "v", "q") if kind == "qg" else ("u", "v", "q", "phi")
    x, y = particle_set(m, 300)
    P = particles.attach(m, x, y, record_every=3, capacity=4, record=names)
    seen = []
    t, tc = m.t, m.tc
    times = {0: t}
    for s in range(1, 14):
        m._step_forward()
        t += m.dt
        times[s] = t
        if s % 3 == 0:
            seen.append((s, P.positions(), P.sample(names), {"q": np.array(m.q), "phi": np.array(m.phi) if kind != "qg" else None,
                                                               "uv": velocity(m)}))
    tr = P.trajectory()
    assert list(tr.step) == [tc + s for s, *_ in seen[-4:]]
    assert np.array_equal(tr.t, [times[s] for s, *_ in seen[-4:]])
    for r, (s, (px, py), smp, ref) in enumerate(seen[-4:]):
        assert np.array_equal(tr.x[r], px) and np.array_equal(tr.y[r], py)
        for nm in names:
            assert np.array_equal(tr.values[nm][r], smp[nm]), nm
        assert np.max(np.abs(smp["q"] - interpolate(ref["q"], px, py, m.L))) <= 1e-10 * np.abs(ref["q"]).max()
        U = ref["uv"]
        assert np.max(np.abs(smp["u"] - interpolate(U[0], px, py, m.L))) <= 1e-10 * np.abs(U[0]).max()
        assert np.max(np.abs(smp["v"] - interpolate(U[1], px, py, m.L))) <= 1e-10 * np.abs(U[1]).max()
        if ref["phi"] is not None:
            assert np.max(np.abs(smp["phi"] - interpolate(ref["phi"], px, py, m.L))) <= 1e-10 * np.abs(ref["phi"]).max()
    # at nodes, the sample is the field itself
    dx = m.L / m.nx
    Pn_m = make(kind, 128, "filter")
    Pn = particles.attach(Pn_m, np.array([0.5 * dx, 10.5 * dx]), np.array([3.5 * dx, 100.5 * dx]))
    s = Pn.sample(names)
    q = np.array(Pn_m.q)
    assert np.allclose(s["q"], [q[3, 0], q[100, 10]], rtol=0, atol=1e-12 * np.abs(q).max())
    if "phi" in names:
        phi = np.array(Pn_m.phi)
        assert np.allclose(s["phi"], [phi[3, 0], phi[100, 10]], rtol=0, atol=1e-12 * np.abs(phi).max())
    Pn.detach()
    twin = make(kind, 128, "filter", tdiags=3)
    twin.twrite = 5
    while twin.tc < m.tc:
        twin._step_forward()
    np.array(twin.q), np.array(twin.ph), (np.array(twin.phi) if kind != "qg" else None)   # the same lazy download buffers
    P.detach()
    assert m._ctx.device_bytes() == twin._ctx.device_bytes()
    with pytest.raises(RuntimeError):
        P.positions()
    P2 = particles.attach(m, x, y)
    with pytest.raises(RuntimeError, match="attached already"):
        particles.attach(m, x, y)
    P2.detach()


# ---- any-size -----------------------------------------------------------------------------------------------------------------
def _check_anysize(kind, nx):
    from niwqg_amd import particles
    A = make(kind, nx, "filter", tdiags=3)
    B = make(kind, nx, "filter", tdiags=3)
    C = make(kind, nx, "filter", tdiags=3)
    assert getattr(A, "_any_size", False)
    for m in (A, B, C):
        m.twrite = 5
        set_tmax(m, 8)
    x, y = particle_set(A, 200)
    names = ("u", "v", "q") if kind == "qg" else ("u", "v", "q", "phi")
    P = particles.attach(A, x, y, record_every=2, capacity=3, record=names)
    A.run()
    C.run()
    U0 = velocity(B)
    for _ in range(8):
        B._step_forward()
        U1 = velocity(B)
        x, y = rk4(x, y, U0, U1, B.U, B.dt, B.L)
        U0 = U1
    xa, ya = P.positions()
    assert max(np.max(np.abs(xa - x)), np.max(np.abs(ya - y))) <= 1e-12 * A.L
    assert_same(outputs(A, kind), outputs(C, kind), kind)
    tr = P.trajectory()
    assert list(tr.step) == [4, 6, 8]
    assert np.array_equal(tr.x[-1], xa)
    s = P.sample(names)
    for nm in names:
        assert np.array_equal(tr.values[nm][-1], s[nm]), nm
    assert np.max(np.abs(s["q"] - interpolate(np.array(A.q), xa, ya, A.L))) <= 1e-10 * np.abs(A.q).max()
    P.detach()


@pytest.mark.parametrize("nx", [96, 100])
@pytest.mark.parametrize("kind", ["coupled", "qg"])
def test_anysize(kind, nx):
    _check_anysize(kind, nx)


# ---- determinism, non-finite, slabs, ensembles ---------------------------------------------------------------------------
def test_determinism():
    from niwqg_amd import particles
    res = []
    for _ in range(2):
        m = make("coupled", 256, "filter")
        x, y = particle_set(m, 20000)
        P = particles.attach(m, x, y, record_every=2, capacity=8, record=("phi", "q"))
        m._ctx.step(10)
        tr = P.trajectory()
        res.append((P.positions(), tr.x, tr.values["phi"], tr.values["q"]))
    for a, b in zip(res[0], res[1]):
        if isinstance(a, tuple):
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
        else:
            assert np.array_equal(a, b)


def test_non_finite_state_turns_particles_nan():
    from niwqg_amd import particles
    m = make("coupled", 64, "filter")
    q = np.array(m.q)
    q[5, 7] = np.nan                                     # the blow-up recipe of test_gpu_nonfinite.py: a NaN in the state
    m.set_q(q)
    x, y = particle_set(m, 100)
    P = particles.attach(m, x, y, record_every=1, capacity=2, record=("u", "phi"))
    m._ctx.step(2)
    xa, ya = P.positions()
    assert np.all(np.isnan(xa) | np.isnan(ya))
    tr = P.trajectory()
    assert np.all(np.isnan(tr.values["u"][-1]))
    P.detach()


def test_slab_ranks_refuse():
    import niwqg_amd
    from niwqg_amd import particles
    from test_oracle_golden import notebook_kwargs
    m = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        particles.attach(m, [1.0], [2.0])


def test_ensemble_member():
    """particles on member 0 of a two-member ensemble: member 1 is bit-identical to an ensemble without particles, member 0's
    state too, and member 0's particles follow the restatement of a twin stepped one step at a time"""
    from niwqg_amd import ensemble, particles
    ens = ensemble.Ensemble(lambda j: ensemble.config5_member(j, nx=128), 2)
    solo = ensemble.Ensemble(lambda j: ensemble.config5_member(j, nx=128), 2)
    twin = ensemble.config5_member(0, nx=128)
    m0 = ens.members[0]
    x, y = particle_set(m0, 1000)
    P = particles.attach(m0, x, y)
    ens.step(6)
    solo.step(6)
    for name in ("qh", "phih", "ph"):
        assert np.array_equal(np.array(getattr(ens.members[1], name)), np.array(getattr(solo.members[1], name))), name
        assert np.array_equal(np.array(getattr(ens.members[0], name)), np.array(getattr(solo.members[0], name))), name
    U0 = velocity(twin)
    for _ in range(6):
        twin._step_forward()
        U1 = velocity(twin)
        x, y = rk4(x, y, U0, U1, twin.U, twin.dt, twin.L)
        U0 = U1
    xa, ya = P.positions()
    assert max(np.max(np.abs(xa - x)), np.max(np.abs(ya - y))) <= 1e-12 * m0.L
    assert np.max(np.hypot(xa - particle_set(m0, 1000)[0], ya - particle_set(m0, 1000)[1])) > 1e-5 * m0.L
    P.detach()
