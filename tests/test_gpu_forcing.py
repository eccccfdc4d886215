"""Stochastic forcing (niwqg_amd/forcing.py, nq_forcing_*, nq_any_forcing): the device's increments against
the numpy restatement of the noise, forced runs against the oracle driven step by step with the restated increments, the work
identities, the injection rate of a ring, off means off, particles beside forcing, refusals, restart and determinism."""
import numpy as np
import pytest

from test_gpu_spectra import make, MASKS
from test_gpu_particles import outputs, assert_same, set_tmax, particle_set, velocity
from test_oracle_golden import notebook_kwargs, K0, U0, L, rel

pytestmark = pytest.mark.gpu

KERNEL = ("coupled", "uncoupled", "ybj")


def amplitudes(nx, which, seed=3):
    """random amplitude planes inside a box of low wavenumbers, non-zero on the lines the q rule must leave alone too"""
    rng = np.random.default_rng(seed)
    Aq = Aphi = None
    if "q" in which:
        Aq = np.zeros((nx, nx // 2 + 1))
        b = 9
        Aq[:b, :b] = rng.uniform(0.5, 1.5, (b, b))
        Aq[-b + 1:, :b] = rng.uniform(0.5, 1.5, (b - 1, b))
        Aq[nx // 2 + 1:, 0] = Aq[1:nx // 2, 0][::-1]               # the forcing of q is a real field
        Aq[nx // 2, :3] = 1.0                                    # never forced, whatever A holds
        Aq[:3, nx // 2] = 1.0
        Aq *= 1e-9 * nx * nx                                      # (spectral values scale with the number of points)
    if "phi" in which:
        Aphi = np.zeros((nx, nx))
        b = 7
        for rs in (slice(0, b), slice(-b, None)):
            for cs in (slice(0, b), slice(-b, None)):
                Aphi[rs, cs] = rng.uniform(0.5, 1.5, (b, b))
        Aphi[nx // 2, nx // 2] = 1.0                             # phi draws everywhere, the Nyquist lines included
        Aphi *= 2e-6 * nx * nx
    return Aq, Aphi


def which_of(kind):
    return {"qg": ("q",), "ybj": ("phi",)}.get(kind, ("q", "phi", "q+phi"))


def restated(nx, dt, A, step, stream, seed):
    from niwqg_amd import forcing
    return np.sqrt(dt) * A * forcing.noise_plane(nx, step, stream, seed)


# ---- noise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 128, 96])
@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "ybj", "qg"])
def test_increment_is_the_restated_noise(kind, nx):
    """F.increment against sqrt(dt) A noise at 1e-13 max A: device log / sincos and numpy's differ by a few ulp on values of order
    one, a wrong bit in Philox gives order-one differences."""
    from niwqg_amd import forcing
    m = make(kind, nx)
    which = "q" if kind == "qg" else ("phi" if kind == "ybj" else "q+phi")
    Aq, Aphi = amplitudes(nx, which)
    seed = (0x9e3779b9 << 32) | 0x7f4a7c15
    F = forcing.attach(m, q=Aq, phi=Aphi, seed=seed)
    sdt = np.sqrt(m.dt)
    h = nx // 2
    for step in (0, 1, 2 ** 31):
        if Aq is not None:
            d = F.increment("q", step)
            want = restated(nx, m.dt, Aq, step, 0, seed)
            err = np.max(np.abs(d - want))
            print("increment q %s %d step %d: max err %.3e (%.3e in units of sqrt(dt)), bound %.3e" % (kind, nx, step, err, err / sdt, 1e-13 * Aq.max()))
            assert err <= 1e-13 * Aq.max()
            assert np.max(np.abs(d)) > 0.1 * sdt * Aq.max()
            assert np.array_equal(d[h + 1:, 0], np.conj(d[1:h, 0][::-1]))              # Hermitian on column 0, bit for bit
            assert not d[h, :].any() and not d[:, h].any() and d[0, 0] == 0          # ... and nothing where A is non-zero there
        if Aphi is not None:
            d = F.increment("phi", step)
            want = restated(nx, m.dt, Aphi, step, 1, seed)
            err = np.max(np.abs(d - want))
            print("increment phi %s %d step %d: max err %.3e (%.3e in units of sqrt(dt)), bound %.3e" % (kind, nx, step, err, err / sdt, 1e-13 * Aphi.max()))
            assert err <= 1e-13 * Aphi.max()
            assert d[h, h] != 0
    assert F.state() == {"seed": seed, "step": 0}                                     # increment() leaves the sequence alone
    F.detach()


# ---- against the oracle --------------------------------------------------------------------------------------------------------
def pair(kind, nx, mask, oracle=True):
    import niwqg_amd
    from oracle import niwqg_oracle as O
    kw = notebook_kwargs(nx, False)
    kw.update({k: v for k, v in MASKS[mask].items() if k != "exact_qh"})
    rng = np.random.default_rng(7)
    if kind == "qg":
        for k in ("m", "N", "f", "nu4w", "nuw", "muw", "dealias"):
            kw.pop(k)
        kw.update(mu=2e-8, nu=0.0)
        m, o = niwqg_amd.QGModel.Model(**kw), (O.QGOracle(**kw) if oracle else None)
    else:
        kw.update(nu4w=3e9 * (128.0 / nx) ** 4, muw=1e-7, mu=2e-8)
        cls = {"coupled": niwqg_amd.CoupledModel, "uncoupled": niwqg_amd.UnCoupledModel, "ybj": niwqg_amd.YBJModel}[kind]
        m, o = cls.Model(**kw), (O.NIWQGOracle(kind, **kw) if oracle else None)
    grid = O.SpectralGrid(nx, L, half=False)
    q0 = O.lamb_dipole(grid, U=U0, R=2 * np.pi / K0) + 2e-6 * rng.standard_normal((nx, nx))
    phi0 = 0.1 * O.wave_packet(grid, k=2 * K0, l=K0, R=L / 6, x0=L / 2, y0=L / 2) + 0.02 * (
        rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx)))

    def init(x):
        x.set_q(q0)
        if kind != "qg":
            x.set_phi(phi0)
    return m, o, init, kw


def full_hermitian(half):
    n = half.shape[0]
    v = np.zeros((n, n), complex)
    v[:, :n // 2 + 1] = half
    v[:, n // 2 + 1:] = np.conj(np.roll(half[::-1, 1:n // 2], 1, axis=0))[:, ::-1]
    return v


def drive_oracle(o, kind, nsteps, Aq, Aphi, seed, step0=0):
    nx = o.nx
    for s in range(step0, step0 + nsteps):
        o._step_etdrk4()
        if Aq is not None:
            d = restated(nx, o.dt, Aq, s, 0, seed)
            o.qh = o.qh + (d if kind == "qg" else full_hermitian(d))
        if Aphi is not None:
            o.phih = o.phih + restated(nx, o.dt, Aphi, s, 1, seed)
        if kind == "qg":
            o._invert()
            o.q = o.ifft(o.qh)
        elif kind == "ybj":
            o.phi = o.ifft(o.phih)
        else:
            o._to_physical()
        o._increment_diagnostics()          # the rest of _step_forward: a tick at tc = 0 refreshes UnCoupledModel's phix, phiy (Q1)
        o._print_status()


def compare(m, o, kind, tag):
    names = ("q", "p", "u", "v", "qh") if kind == "qg" else ("q", "p", "phi", "u", "v", "qh", "phih")
    if kind == "ybj":        # YBJModel._invert is purely spectral (YBJModel.py:141-146): the oracle's p stays zero for ever, ph is what it holds
        names = tuple("ph" if n == "p" else n for n in names)
    for name in names:
        e = rel(np.array(getattr(m, name)), getattr(o, name))
        print("%s %s: %.2e" % (tag, name, e))
        assert e < 1e-11, (tag, name, e)


ORACLE_CASES = [(k, msk, w) for k in ("coupled", "uncoupled", "ybj", "qg") for msk in ("filter", "none", "mask") for w in which_of(k)
                if not (k == "qg" and msk == "mask")]


@pytest.mark.parametrize("nx", [64, 128])
@pytest.mark.parametrize("kind,mask,which", ORACLE_CASES)
def test_forced_run_against_the_oracle(kind, mask, which, nx):
    from niwqg_amd import forcing
    Aq, Aphi = amplitudes(nx, which)
    seed, nsteps = 12345, 10
    m, o, init, kw = pair(kind, nx, mask)
    init(o)
    drive_oracle(o, kind, nsteps, Aq, Aphi, seed)
    # one step at a time
    init(m)
    F = forcing.attach(m, q=Aq, phi=Aphi, seed=seed)
    for _ in range(nsteps):
        m._step_forward()
    compare(m, o, kind, "%s %s %s %d stepwise" % (kind, mask, which, nx))
    assert F.state()["step"] == nsteps
    state = [np.array(m.qh)] + ([np.array(m.phih)] if kind != "qg" else [])
    # batched run() of a second model: the same state bit for bit
    b, _, initb, _ = pair(kind, nx, mask, oracle=False)
    initb(b)
    forcing.attach(b, q=Aq, phi=Aphi, seed=seed)
    set_tmax(b, nsteps)
    b.run()
    assert b.tc == nsteps
    compare(b, o, kind, "%s %s %s %d run()" % (kind, mask, which, nx))
    for x, y in zip(state, [np.array(b.qh)] + ([np.array(b.phih)] if kind != "qg" else [])):
        assert np.array_equal(x, y)
    # nq_step(10) in one call and in ten calls (no diagnostics tick in between on either side)
    got = []
    for calls in (1, nsteps):
        b, _, initb, _ = pair(kind, nx, mask, oracle=False)
        initb(b)
        forcing.attach(b, q=Aq, phi=Aphi, seed=seed)
        for _ in range(calls):
            b._ctx.step(nsteps // calls)
        b._after_steps()
        got.append([np.array(b.qh), np.array(b.ph)] + ([np.array(b.phih)] if kind != "qg" else []))
    for x, y in zip(*got):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", ["coupled", "qg"])
def test_forced_run_on_an_any_size_grid_against_the_oracle(kind):
    from niwqg_amd import forcing
    nx = 96
    Aq, Aphi = amplitudes(nx, "q" if kind == "qg" else "q+phi")
    m, o, init, kw = pair(kind, nx, "filter")
    assert getattr(m, "_any_size", False)
    init(o)
    init(m)
    drive_oracle(o, kind, 5, Aq, Aphi, 99)
    F = forcing.attach(m, q=Aq, phi=Aphi, seed=99)
    for _ in range(5):
        m._step_forward()
    compare(m, o, kind, "%s any-size" % kind)
    assert F.state() == {"seed": 99, "step": 5}
    # the work identity of a kick on this path
    k0, w0 = m._calc_ke_qg(), F.work()
    if kind == "coupled":
        F.detach()
        F = forcing.attach(m, q=Aq, seed=99, step0=5)
        w0 = F.work()
    F.kick()
    k1, w1 = m._calc_ke_qg(), F.work()
    assert abs((k1 - k0) - (w1["q"] - w0["q"])) <= 1e-12 * k1 and w1["q"] != w0["q"]
    F.detach()


# ---- work ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 128])
@pytest.mark.parametrize("kind", ["qg", "uncoupled", "coupled"])
def test_work_of_a_q_kick_is_the_change_of_ke_qg(kind, nx):
    from niwqg_amd import forcing
    m = make(kind, nx)
    m._ctx.step(2)
    m._after_steps()
    Aq, _ = amplitudes(nx, "q")
    F = forcing.attach(m, q=Aq, seed=5)
    for i in range(3):
        k0, w0 = m._calc_ke_qg(), F.work()["q"]
        F.kick()
        k1, w1 = m._calc_ke_qg(), F.work()["q"]
        print("work q %s %d kick %d: dke %.6e dwork %.6e ke %.6e" % (kind, nx, i, k1 - k0, w1 - w0, k1))
        assert abs((k1 - k0) - (w1 - w0)) <= 1e-12 * k1
        assert abs(w1 - w0) > 1e-9 * k1                        # the kick did something the bound resolves
    assert F.state()["step"] == 3 and F.work()["phi"] == 0.0


@pytest.mark.parametrize("nx", [64, 128])
@pytest.mark.parametrize("kind", KERNEL)
def test_work_of_a_phi_kick_is_the_change_of_ke_niw(kind, nx):
    from niwqg_amd import forcing
    m = make(kind, nx)
    m._ctx.step(2)
    m._after_steps()
    _, Aphi = amplitudes(nx, "phi")
    F = forcing.attach(m, phi=Aphi, seed=6)
    for i in range(3):
        k0, w0 = m._calc_ke_niw(), F.work()["phi"]
        F.kick()
        k1, w1 = m._calc_ke_niw(), F.work()["phi"]
        print("work phi %s %d kick %d: dke %.6e dwork %.6e ke %.6e" % (kind, nx, i, k1 - k0, w1 - w0, k1))
        assert abs((k1 - k0) - (w1 - w0)) <= 1e-12 * k1
        assert abs(w1 - w0) > 1e-9 * k1
    assert F.work()["q"] == 0.0


# ---- injection rate -------------------------------------------------------------------------------------------------------
def quiet_model(kind, nx, dt):
    import niwqg_amd
    kw = dict(L=L, nx=nx, tmax=1e30, dt=dt, twrite=10 ** 9, tdiags=10 ** 9, use_filter=False, U=0.0, nu4=0.0, nu=0.0, mu=0.0)
    if kind == "qg":
        m = niwqg_amd.QGModel.Model(**kw)
    else:
        kw.update(m=2 * np.pi / 280.0, N=0.01, f=1e-4, nu4w=0.0, nuw=0.0, muw=0.0)
        m = {"uncoupled": niwqg_amd.UnCoupledModel, "ybj": niwqg_amd.YBJModel}[kind].Model(**kw)
    m.set_q(np.zeros((nx, nx)))
    if kind != "qg":
        m.set_phi(np.zeros((nx, nx), complex))
    return m


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("kind", ["qg", "uncoupled"])
def test_injection_rate_of_a_q_ring(kind, seed):
    """64 steps from rest without dissipation: ke_qg / (64 eps dt) within 4 / sqrt(N_eff) of 1, N_eff = (sum e)^2 / sum e^2 over
    the expected energies e of the independent modes (each mode's energy is exponentially distributed).  On the CPU with the
    restated noise and no advection: N_eff = 349, bound 0.21, seeds 1, 2, 3 give 1.040, 0.961, 0.985."""
    from niwqg_amd import forcing
    nx, dt, eps, nsteps = 128, 100.0, 8e-11, 64
    m = quiet_model(kind, nx, dt)
    dk = m.dk
    A = forcing.ring(m, 16 * dk, 2 * dk, eps)
    wv2 = m.kk[None, :nx // 2 + 1] ** 2 + m.ll[:, None] ** 2
    wv2[0, 0] = 1.0
    e = A ** 2 / wv2                       # a mode (l, k) and its mirror image; column 0: rows 1..nx/2-1 with their mirror rows
    e[nx // 2:, 0] = 0.0
    neff = e.sum() ** 2 / (e ** 2).sum()
    F = forcing.attach(m, q=A, seed=seed)
    m._ctx.step(nsteps)
    m._after_steps()
    ratio = m._calc_ke_qg() / (nsteps * eps * dt)
    cfl = m._calc_cfl()
    print("injection q %s seed %d: ratio %.4f, N_eff %.1f, bound %.3f, cfl %.2e, work/ke %.6f" % (
        kind, seed, ratio, neff, 4 / np.sqrt(neff), cfl, F.work()["q"] / m._calc_ke_qg()))
    assert 300 < neff < 400
    assert cfl < 0.1
    assert abs(ratio - 1.0) <= 4.0 / np.sqrt(neff)
    assert abs(F.work()["q"] - m._calc_ke_qg()) <= 1e-9 * m._calc_ke_qg()      # nothing else changes ke_qg here (advection conserves it)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_injection_rate_of_a_phi_ring(seed):
    from niwqg_amd import forcing
    nx, dt, eps, nsteps = 128, 100.0, 8e-11, 64
    m = quiet_model("ybj", nx, dt)
    dk = m.dk
    A = forcing.ring(m, 16 * dk, 2 * dk, eps, field="phi")
    e = A ** 2
    neff = e.sum() ** 2 / (e ** 2).sum()
    F = forcing.attach(m, phi=A, seed=seed)
    m._ctx.step(nsteps)
    m._after_steps()
    ratio = m._calc_ke_niw() / (nsteps * eps * dt)
    print("injection phi seed %d: ratio %.4f, N_eff %.1f, bound %.3f" % (seed, ratio, neff, 4 / np.sqrt(neff)))
    assert abs(ratio - 1.0) <= 4.0 / np.sqrt(neff)
    assert abs(F.work()["phi"] - m._calc_ke_niw()) <= 1e-10 * m._calc_ke_niw()


# ---- off means off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mask", [("coupled", "filter"), ("coupled", "mask"), ("uncoupled", "filter"), ("ybj", "filter"), ("qg", "filter")])
def test_off_means_off(kind, mask):
    from niwqg_amd import forcing
    nx = 128
    Aq, Aphi = amplitudes(nx, "q" if kind == "qg" else ("phi" if kind == "ybj" else "q+phi"))
    A, B, C = (make(kind, nx, mask, tdiags=3) for _ in range(3))
    for m in (A, B, C):
        m.twrite = 5
        set_tmax(m, 12)
    b0 = A._ctx.device_bytes()
    F = forcing.attach(A, q=Aq, phi=Aphi, seed=1)
    assert A._ctx.device_bytes() > b0
    F.detach()
    assert A._ctx.device_bytes() == b0
    forcing.attach(B, q=None if Aq is None else 0 * Aq, phi=None if Aphi is None else 0 * Aphi, seed=1)
    for m in (A, B, C):
        m.run()
    assert_same(outputs(A, kind), outputs(C, kind), kind)
    for name in ("qh", "ph") + (("phih",) if kind != "qg" else ()):
        assert np.array_equal(np.array(getattr(B, name)), np.array(getattr(C, name))), name
    assert A._ctx.device_bytes() == C._ctx.device_bytes()


# ---- with particles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "uncoupled", "qg"])
def test_particles_beside_forcing(kind):
    from niwqg_amd import forcing, particles
    nx = 128
    Aq, Aphi = amplitudes(nx, "q" if kind == "qg" else "q+phi")
    A, B = make(kind, nx), make(kind, nx)
    x, y = particle_set(A, 500)
    P = particles.attach(A, x, y)
    for m in (A, B):
        forcing.attach(m, q=Aq, phi=Aphi, seed=4)
        m._ctx.step(6)
        m._after_steps()
    for name in ("qh", "ph") + (("phih",) if kind != "qg" else ()):
        assert np.array_equal(np.array(getattr(A, name)), np.array(getattr(B, name))), name
    from test_particles_host import interp
    xa, ya = P.positions()
    s = P.sample(("u", "v"))
    u, v = velocity(A)                      # of the forced, re-inverted state the model holds
    for got, plane in ((s["u"], u), (s["v"], v)):
        assert np.max(np.abs(got - interp(plane, xa, ya, A.L))) <= 1e-12 * max(np.abs(u).max(), np.abs(v).max())
    assert np.max(np.hypot(xa - x, ya - y)) > 1e-5 * A.L


# ---- refusals, restart, determinism ----------------------------------------------------------------------------------------------
def test_slab_ranks_refuse():
    import niwqg_amd
    from niwqg_amd import forcing, _lib
    m = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    Aq, Aphi = amplitudes(64, "q+phi")
    with pytest.raises(NotImplementedError, match="slab"):
        forcing.attach(m, q=Aq, phi=Aphi)
    lib = _lib.lib()
    h = m._ctx.sim.ranks[0].h
    out = np.zeros(64 * 64 * 2)
    assert lib.nq_forcing_attach(h, _lib._dptr(np.ascontiguousarray(Aq)), None, 0, 0) == -4
    assert lib.nq_forcing_detach(h) == -4
    assert lib.nq_forcing_apply(h) == -4
    assert lib.nq_forcing_increment(h, 0, 0, _lib._dptr(out)) == -4
    assert lib.nq_forcing_state(h, _lib._dptr(out)) == -4


def test_class_scope_and_second_attach():
    from niwqg_amd import forcing
    Aq, Aphi = amplitudes(64, "q+phi")
    with pytest.raises(ValueError, match="YBJModel"):
        forcing.attach(make("ybj", 64), q=Aq)
    with pytest.raises(ValueError, match="QGModel"):
        forcing.attach(make("qg", 64), phi=Aphi)
    m = make("coupled", 64)
    F = forcing.attach(m, q=Aq)
    with pytest.raises(ValueError, match="attached already"):
        forcing.attach(m, phi=Aphi)
    with pytest.raises(ValueError, match="not forced"):
        F.increment("phi", 0)
    F.detach()
    F2 = forcing.attach(m, phi=Aphi)
    F2.detach()
    with pytest.raises(RuntimeError, match="detached"):
        F2.work()


@pytest.mark.parametrize("kind", ["coupled", "ybj", "qg"])
def test_restart_and_determinism(kind):
    from niwqg_amd import forcing
    nx = 128
    Aq, Aphi = amplitudes(nx, "q" if kind == "qg" else ("phi" if kind == "ybj" else "q+phi"))
    res = []
    for split in (False, False, True):
        m = make(kind, nx)
        F = forcing.attach(m, q=Aq, phi=Aphi, seed=2 ** 40 + 17)
        if split:
            m._ctx.step(5)
            st = F.state()
            assert st == {"seed": 2 ** 40 + 17, "step": 5}
            F.detach()
            F = forcing.attach(m, q=Aq, phi=Aphi, seed=st["seed"], step0=st["step"])
            m._ctx.step(5)
        else:
            m._ctx.step(10)
        m._after_steps()
        res.append(([np.array(m.qh), np.array(m.ph)] + ([np.array(m.phih)] if kind != "qg" else []), F.work(), F.state()["step"]))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    assert res[0][1] == res[1][1] and res[0][1] != {"q": 0.0, "phi": 0.0}
    for x, y in zip(res[0][0], res[2][0]):                       # 5 + 5 steps with a re-attach at step0 = 5
        assert np.array_equal(x, y)
    assert res[0][2] == res[2][2] == 10
