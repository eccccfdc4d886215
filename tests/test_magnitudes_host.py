"""Field magnitudes on the CPU: the helpers of tests/test_gpu_magnitudes.py, and every property those tests rely on pinned on
the oracle (oracle/niwqg_oracle.py, itself pinned to the reference by tests/test_oracle_golden.py).

A. Exact symmetries.  A change of units by powers of two (length x 2^a, time x 2^b) and a rescaling of a linearly evolving
   field (the passive scalar of QGModel; phi of UnCoupledModel and YBJModel, where q does not see the waves) multiply every
   operand of the step by a power of two or leave the dimensionless c dt alone, so the mantissas of the results must not
   change.  `same_bits` is the comparison rule of both modules.
B. Weak potential vorticity under strong waves: the oracle's own sensitivity to one ulp of its inputs on exactly the states
   of the GPU tests (so that their 1e-11 is a statement about the device, not about the reference), and the premise of the
   zero-PV case (q stays identically zero in the oracle).
"""
import numpy as np
import pytest

from oracle import niwqg_oracle as O
from test_oracle_golden import notebook_kwargs, rel, L, K0, U0, MZ, NB, F0

TINY = 2.0 ** -960                                     # below it only the absolute difference is looked at (filter tail, denormals)
UNIT_EXPONENTS = [(0, 3), (4, 0), (-7, 5), (20, -33)]      # (a, b): length x 2^a, time x 2^b
KINDS = ["coupled", "uncoupled", "ybj", "qg"]
WAVE_MIXED = ("Ke", "cfl")                              # see assert_linear_scaling
WEAK_PV = [(1.0, 1.0), (1e-4, 1.0), (1e-8, 1.0), (1e-8, 3.0), (1.0, 1e-6)]      # (sq, amp)

# how every constructor keyword scales with (sL, sT); keywords not listed are dimensionless
_UNITS = dict(L=(1, 0), dt=(0, 1), f=(0, -1), N=(0, -1), m=(-1, 0), U=(1, -1), nu=(2, -1), nuw=(2, -1), nuc=(2, -1),
              nu4=(4, -1), nu4w=(4, -1), nu4c=(4, -1), mu=(0, -1), muw=(0, -1), muc=(0, -1), beta=(-1, -1))
# ... and every output: name -> (power of sL, power of sT)
_OUT_UNITS = dict(q=(0, -1), qh=(0, -1), phi=(1, -1), phih=(1, -1), c=(0, 0), ch=(0, 0), cvar=(0, 0), Ke=(2, -2), Kw=(2, -2),
                  Pw=(2, -2), ke_qg=(2, -2), ke_niw=(2, -2), pe_niw=(2, -2), cfl=(0, 0))


def same_bits(got, base, factor=1.0):
    """The rule of section A for `got` against `base * factor` (factor a power of two): equal bits wherever the expected
    magnitude is >= 2^-960, |difference| <= 2^-960 elsewhere (real and imaginary parts separately).  Underflow can have happened
    in either run (the filter's tail reaches the denormals), so "expected magnitude" is that of the entry in BOTH frames: an entry
    whose base value is below 2^-960 has lost mantissa bits there already and is compared absolutely, at 2^-960 in the base's frame
    (2^-960 * factor, never less than 2^-960).  Returns (number of entries that break the rule, largest difference among them)."""
    g = np.ascontiguousarray(np.asarray(got)).ravel()
    b = np.ascontiguousarray(np.asarray(base)).ravel()
    assert g.shape == b.shape and g.dtype == b.dtype, (g.shape, b.shape, g.dtype, b.dtype)
    if np.iscomplexobj(g):
        g, b = g.view(np.float64), b.view(np.float64)
    g, b = g.astype(np.float64, copy=False), b.astype(np.float64, copy=False)
    e = b * factor
    big = (np.abs(e) >= TINY) & (np.abs(b) >= TINY)
    with np.errstate(invalid="ignore", over="ignore"):
        bad = np.where(big, g.view(np.uint64) != e.view(np.uint64), ~(np.abs(g - e) <= TINY * max(1.0, factor)))
        worst = float(np.abs(g - e)[bad].max()) if bad.any() else 0.0
    return int(bad.sum()), worst


def assert_same_bits(got, base, tag, factor=1.0):
    n, worst = same_bits(got, base, factor)
    assert n == 0, "%s: %d entries differ, largest difference %.3e" % (tag, n, worst)


def base_kwargs(kind, nx, tdiags=10 ** 9):
    """The unscaled configuration of each model class: notebook parameters, filter on, every dissipation coefficient that the
    class has non-zero (mu, beta and the scalar's own for QGModel included), a mean flow."""
    kw = notebook_kwargs(nx, True, tdiags=tdiags)
    kw.update(mu=1e-8)
    if kind == "qg":
        for k in ("m", "N", "f", "nuw", "nu4w", "muw"):
            kw.pop(k)
        kw.update(beta=2e-11, passive_scalar=True, nu4c=0.5 * kw["nu4"], nuc=2.0, muc=1e-8)
    else:
        kw.update(nu4w=0.1 * kw["nu4"], muw=2e-8)
    return kw


def scale_kwargs(kw, a, b):
    """kw in units of length x 2^a and time x 2^b (exact: every factor is a power of two)"""
    out = dict(kw)
    for k, (pl, pt) in _UNITS.items():
        if k in out:
            out[k] = float(np.ldexp(float(out[k]), pl * a + pt * b))
    return out


def out_factor(name, a, b):
    pl, pt = _OUT_UNITS[name]
    return float(np.ldexp(1.0, pl * a + pt * b))


def initial_fields(kind, nx, seed=0):
    """q0, phi0, c0 of the suite's usual amplitudes, built ONCE on the unscaled grid (the callers multiply them)"""
    rng = np.random.default_rng(7000 + seed)
    g = O.SpectralGrid(nx, L, half=False)
    out = dict(q=O.lamb_dipole(g, U=U0, R=2 * np.pi / K0) + 2e-6 * rng.standard_normal((nx, nx)))
    if kind == "qg":
        out["c"] = 1.0 + 0.3 * rng.standard_normal((nx, nx))
    else:
        out["phi"] = 0.1 * O.wave_packet(g, k=2 * K0, l=K0, R=L / 6, x0=L / 2, y0=L / 2) + 0.02 * (
            rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx)))
    return out


def make_oracle(kind, kw):
    return O.QGOracle(**kw) if kind == "qg" else O.NIWQGOracle(kind, **kw)


def make_device(kind, kw, **extra):
    import niwqg_amd
    cls = dict(coupled=niwqg_amd.CoupledModel, uncoupled=niwqg_amd.UnCoupledModel, ybj=niwqg_amd.YBJModel, qg=niwqg_amd.QGModel)[kind]
    return cls.Model(**kw, **extra)


def start(x, fields):
    x.set_q(fields["q"])
    if "phi" in fields:
        x.set_phi(fields["phi"])
    if "c" in fields:
        x.set_c(fields["c"])
    return x


def observe(x, kind, spectra=True, scalars=True):
    """copies of everything sections A compares; spectra=False, scalars=False: the physical fields only (8192^2)"""
    names = dict(coupled=["q", "phi"], uncoupled=["q", "phi"], ybj=["phi"], qg=["q", "c"])[kind]
    if spectra:
        names = names + [n + "h" for n in names]
    out = {n: np.array(getattr(x, n)) for n in names}
    if scalars:
        if kind == "qg":
            out.update(Ke=x.Ke, cvar=x.cvar, ke_qg=x._calc_ke_qg(), cfl=x._calc_cfl())
        else:
            out.update(Kw=x.Kw, Pw=x.Pw, ke_niw=x._calc_ke_niw(), pe_niw=x._calc_pe_niw())
            if kind != "ybj":
                out.update(Ke=x.Ke, ke_qg=x._calc_ke_qg(), cfl=x._calc_cfl())
        out = {k: (v if isinstance(v, np.ndarray) else np.float64(v)) for k, v in out.items()}
    return out


def run(make, kind, kw, fields, nsteps, **obs):
    x = start(make(kind, kw), fields)
    for _ in range(nsteps):
        x._step_forward()
    return observe(x, kind, **obs)


def scale_fields(fields, a, b):
    out = dict(fields)
    out["q"] = np.ldexp(fields["q"], -b)
    if "phi" in fields:
        out["phi"] = fields["phi"] * float(np.ldexp(1.0, a - b))
    return out


def assert_unit_scaling(base, scaled, a, b, tag):
    assert set(base) == set(scaled)
    for name in base:
        assert_same_bits(scaled[name], base[name], "%s (a, b) = (%d, %d) %s" % (tag, a, b, name), out_factor(name, a, b))


def assert_linear_scaling(base, scaled, s, moved, squared, tag, mixed=()):
    """`moved` scale by 2^s, `squared` by 4^s, everything else must not change by one bit; `mixed` are sums of terms of
    different degree in the scaled field (Ke's budget holds the wave-to-flow conversion, the CFL number max |phi|): not compared"""
    for name in base:
        if name in mixed:
            continue
        f = float(np.ldexp(1.0, s if name in moved else (2 * s if name in squared else 0)))
        assert_same_bits(scaled[name], base[name], "%s s = %d %s" % (tag, s, name), f)


# ---- B: states of weak potential vorticity under strong waves ---------------------------------------------------------------
def weak_pv_state(nx, sq, amp, seed=0):
    """CoupledModel, notebook parameters, filter on: q0 = sq (dipole + 2e-6 randn), phi0 = amp (0.1 packet + 0.02 randn)"""
    f = initial_fields("coupled", nx, seed)
    return notebook_kwargs(nx, True), dict(q=sq * f["q"], phi=amp * f["phi"])


def degenerate_states(nx=64):
    """name -> (kind, kw, fields): the rows where one operand of a packed pair is exactly zero or constant (section B3)"""
    f, g = initial_fields("coupled", nx, 1), initial_fields("qg", nx, 1)
    kw, kq = notebook_kwargs(nx, True), base_kwargs("qg", nx)
    mask = np.ones((nx, 1))
    mask[nx // 2:] = 0.0                                                # exactly zero on the upper half of the y rows
    zero = np.zeros((nx, nx))
    return {
        "phi_zero": ("coupled", kw, dict(q=f["q"], phi=zero + 0j)),
        "phi_uniform": ("coupled", kw, dict(q=f["q"], phi=np.full((nx, nx), 0.2 + 0.1j))),
        "phi_half_masked": ("coupled", kw, dict(q=f["q"], phi=f["phi"] * mask)),
        "q_zero": ("coupled", kw, dict(q=zero, phi=f["phi"])),
        "c_zero": ("qg", kq, dict(q=g["q"], c=zero)),
        "c_one": ("qg", kq, dict(q=g["q"], c=np.ones((nx, nx)))),
        # c0 = (-1)^i g(y), filter off, the scalar undamped (its hyperviscosity would remove the grid mode within the four
        # steps): every row of c-hat holds the self-mirrored element kx = N/2 and nothing else
        "c_nyquist": ("qg", dict(kq, use_filter=False, nu4c=0.0, nuc=0.0, muc=0.0), dict(q=g["q"], c=_nyquist_only(nx))),
    }


def _nyquist_only(nx):
    y = (np.arange(nx) + 0.5) / nx
    return np.cos(np.pi * np.arange(nx))[None, :] * (1.0 + 0.5 * np.sin(2 * np.pi * y) + 0.25 * np.cos(6 * np.pi * y))[:, None]


def jacobian_psi_q_reference(m, q0, phi0, workers=1):
    """ik F[u q] + il F[v q] of a CoupledModel state set as set_phi(phi0); set_q(q0) (psi contains the wave part), from the
    reference's formulas on the host with pocketfft (Kernel.py:471-486, CoupledModel.py:59-97): the expressions of
    tests/test_gpu_at_size.py::test_row_kernels_8192_on_a_full_spectrum_against_numpy."""
    import scipy.fft

    def F(a):
        return scipy.fft.fft2(a, workers=workers)

    def Fi(a):
        return scipy.fft.ifft2(a, workers=workers)

    ik, il = 1j * m.kk[None, :], 1j * m.ll[:, None]
    wv2 = m.kk[None, :] ** 2 + m.ll[:, None] ** 2
    wv2i = np.zeros_like(wv2)
    wv2i[wv2 != 0] = 1.0 / wv2[wv2 != 0]
    phih = F(phi0)
    phix, phiy = Fi(ik * phih), Fi(il * phih)
    jw = F((1j * (np.conj(phix) * phiy - np.conj(phiy) * phix)).real)
    jw[0, 0] = 0
    del phix, phiy
    qwh = 0.5 * (0.5 * (-wv2 * F(np.abs(phi0) ** 2)) + jw) / m.f * m.filtr
    del jw, phih
    qh = F(q0)
    ph = F(Fi(-(wv2i * qh)).real + Fi(wv2i * qwh).real)
    del qwh
    u, v = Fi(-il * ph).real, Fi(ik * ph).real
    del ph
    q = Fi(qh).real
    jq = ik * F(u * q) + il * F(v * q)
    jq[0, 0] = 0
    return jq


# ---- the oracle itself --------------------------------------------------------------------------------------------------------
_BASE = {}


def oracle_base(kind, nsteps=3, tdiags=10 ** 9):
    key = (kind, nsteps, tdiags)
    if key not in _BASE:
        _BASE[key] = run(make_oracle, kind, base_kwargs(kind, 64, tdiags), initial_fields(kind, 64), nsteps)
    return _BASE[key]


@pytest.mark.parametrize("a,b", UNIT_EXPONENTS)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_is_exact_under_a_change_of_units(kind, a, b):
    """Section A1 on the reference's arithmetic: coupled, uncoupled, ybj and QGModel with beta, the passive scalar and
    mu != 0, 64^2, 3 steps.  Forcing is absent (its amplitude takes a square root of dt)."""
    kw, f = base_kwargs(kind, 64), initial_fields(kind, 64)
    scaled = run(make_oracle, kind, scale_kwargs(kw, a, b), scale_fields(f, a, b), 3)
    assert_unit_scaling(oracle_base(kind), scaled, a, b, "oracle " + kind)


@pytest.mark.parametrize("s", [-64, 40, 300])
def test_oracle_scalar_is_linear_bit_for_bit(s):
    """Section A2: c0 -> 2^s c0 returns c 2^s, ch 2^s, the scalar's variance budget 4^s; q and Ke do not change by one bit."""
    kw, f = base_kwargs("qg", 64, tdiags=2), initial_fields("qg", 64)
    scaled = run(make_oracle, "qg", kw, dict(f, c=np.ldexp(f["c"], s)), 4)
    assert_linear_scaling(oracle_base("qg", 4, 2), scaled, s, ("c", "ch"), ("cvar",), "oracle qg")


@pytest.mark.parametrize("s", [-64, 40, 200])
@pytest.mark.parametrize("kind", ["uncoupled", "ybj"])
def test_oracle_passive_waves_are_linear_bit_for_bit(kind, s):
    """Section A2: phi0 -> 2^s phi0 returns phi 2^s, phih 2^s, Kw and Pw 4^s; q unchanged.  4 steps with a tick every second
    one, so that UnCoupledModel's stale gradients (quirk Q1) are part of it."""
    kw, f = base_kwargs(kind, 64, tdiags=2), initial_fields(kind, 64)
    scaled = run(make_oracle, kind, kw, dict(f, phi=f["phi"] * float(np.ldexp(1.0, s))), 4)
    assert_linear_scaling(oracle_base(kind, 4, 2), scaled, s, ("phi", "phih"), ("Kw", "Pw", "ke_niw", "pe_niw"), "oracle " + kind,
                          mixed=WAVE_MIXED)


def test_same_bits_rule_itself():
    e = np.array([1.0, -3.0, 2.0 ** -970, 0.0, -0.0, 1e-310])
    assert same_bits(e.copy(), e) == (0, 0.0)
    assert same_bits(np.array([1.0, -3.0, 0.0, -0.0, 0.0, 0.0]), e) == (0, 0.0)               # below 2^-960: absolute
    assert same_bits(np.nextafter(e, 4.0), e)[0] == 2                                          # one ulp above it: caught
    assert same_bits(np.array([1.0, -3.0, 2.0 ** -950, 0.0, 0.0, 0.0]), e)[0] == 1
    assert same_bits(np.array([1.0, np.nan, 0.0, np.nan, 0.0, 0.0]), e)[0] == 2
    assert same_bits(np.array([2.0 ** -600]), np.array([2.0 ** -1000]), 2.0 ** 400) == (0, 0.0)
    assert same_bits(np.array([2.0 ** -600]), np.array([2.0 ** -1070]), 2.0 ** 400)[0] == 0          # the base had underflowed
    assert same_bits(np.array([2.0 ** -500]), np.array([2.0 ** -1000]), 2.0 ** 400)[0] == 1
    z = np.array([1.0 + 2.0j])
    assert same_bits(z, z)[0] == 0 and same_bits(z + 1j * 2.0 ** -51, z)[0] == 1


@pytest.mark.parametrize("sq,amp", WEAK_PV)
def test_oracle_sensitivity_on_the_weak_pv_states(sq, amp):
    """Section B1's reference: 6 steps at 128^2 from inputs moved by one ulp in a random direction.  The GPU test asserts 1e-11;
    the reference must sit well inside that on these very states (measured: q 2.6e-16, phi 4.4e-16), here 1e-14."""
    kw, f = weak_pv_state(128, sq, amp)
    rng = np.random.default_rng(5)

    def ulp(x):
        return np.nextafter(x, np.where(rng.integers(0, 2, x.shape) == 1, np.inf, -np.inf))

    g = dict(q=ulp(f["q"]), phi=ulp(f["phi"].real) + 1j * ulp(f["phi"].imag))
    a = run(make_oracle, "coupled", kw, f, 6, scalars=False)
    b = run(make_oracle, "coupled", kw, g, 6, scalars=False)
    errs = {n: rel(b[n], a[n]) for n in ("q", "qh", "phi", "phih")}
    print("sq %g amp %g: one-ulp sensitivity of the oracle" % (sq, amp), {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < 1e-14, errs
    assert np.isfinite(a["q"]).all() and np.isfinite(a["phi"]).all()


def test_oracle_keeps_zero_pv_identically_zero():
    """Premise of the q0 = 0 case of section B3: with q = 0 every product u q, v q is zero, so the reference's q stays exactly
    zero under any waves, while q_w does not -- the device's q can only be judged against ||q_w||."""
    kind, kw, f = degenerate_states()["q_zero"]
    o = start(make_oracle(kind, kw), f)
    for _ in range(4):
        o._step_forward()
    assert not o.q.any() and not o.qh.any()
    assert np.linalg.norm(o.qw) > 0


def test_oracle_on_the_degenerate_states():
    """What section B3 asserts of the device holds in the oracle: phi = 0 and c = 0 stay exactly zero; a uniform phi has no
    wave Jacobian."""
    st = degenerate_states()
    o = start(make_oracle(*st["phi_zero"][:2]), st["phi_zero"][2])
    for _ in range(4):
        o._step_forward()
    assert not o.phi.any() and not o.phih.any()
    o = start(make_oracle(*st["phi_uniform"][:2]), st["phi_uniform"][2])
    assert not o.jacobian_phic_phi().any()
    o = start(make_oracle(*st["c_zero"][:2]), st["c_zero"][2])
    for _ in range(4):
        o._step_forward()
    assert not o.c.any() and not o.ch.any()
    kind, kw, f = st["phi_half_masked"]
    assert not f["phi"][32:].any() and f["phi"][:32].all()
    kind, kw, f = st["c_nyquist"]
    ch = np.fft.rfft(f["c"], axis=1)                      # the rows as the row kernels see them: only kx = N/2 is populated
    assert np.abs(ch[:, :-1]).max() < 1e-13 * np.abs(ch[:, -1]).min()
    o = start(make_oracle(kind, kw), f)
    for _ in range(4):
        o._step_forward()
    assert np.linalg.norm(o.c) > 0.1 * np.linalg.norm(f["c"]) and np.isfinite(o.c).all()
