"""GPU parity across field magnitudes ("Field magnitudes").

Real fields travel in pairs through one complex transform, so the size of one field against another
decides the arithmetic of the row kernels.  Every other parity test starts from the same physical amplitudes; these do not.

A. Exact symmetries, bit for bit, no oracle: a change of units by powers of two and the linearity of the passively carried
   fields, at every row-kernel variant (64^2: single-pass columns and k_x_wavepv, 1024^2: two-pass tiles, 4096^2: k_x_wavepv2
   and the dual-stream step, 8192^2: the even/odd kernels).
B. Weak and zero potential vorticity under strong waves, and rows where one operand of a pair is exactly zero, against the
   oracle (tests/test_magnitudes_host.py pins the oracle's own sensitivity on these states and shares the helpers).
"""
import gc
import time

import numpy as np
import pytest

from oracle import niwqg_oracle as O
from test_oracle_golden import notebook_kwargs, rel, L
from test_magnitudes_host import (UNIT_EXPONENTS, WEAK_PV, WAVE_MIXED, base_kwargs, scale_kwargs, scale_fields, initial_fields,
                                  make_device, make_oracle, start, run, assert_unit_scaling, assert_linear_scaling,
                                  assert_same_bits, weak_pv_state, degenerate_states, jacobian_psi_q_reference)
from test_gpu_at_size import rough_kwargs, NW

pytestmark = pytest.mark.gpu


def device_run(kind, kw, fields, nsteps, **obs):
    """one context at a time: the model is gone before the next one is created"""
    out = run(make_device, kind, kw, fields, nsteps, **obs)
    gc.collect()
    return out


# ---- A1: change of units ------------------------------------------------------------------------------------------------------
UNIT_CASES = ([(kind, 64, 3, UNIT_EXPONENTS, True) for kind in ("coupled", "uncoupled", "ybj", "qg")]
              + [(kind, 1024, 3, UNIT_EXPONENTS, True) for kind in ("coupled", "qg")]
              + [("coupled", 4096, 1, [(-7, 5), (20, -33)], True)]
              + [(kind, 8192, 1, [(-7, 5), (20, -33)], False) for kind in ("coupled", "qg")])


@pytest.mark.parametrize("kind,nx,nsteps,exps,everything", UNIT_CASES, ids=["%s-%d" % c[:2] for c in UNIT_CASES])
def test_change_of_units_is_exact(kind, nx, nsteps, exps, everything):
    """L x 2^a, dt x 2^b and every parameter and field with its own units (the table of test_magnitudes_host._UNITS): q, qh
    x 2^-b, phi, phih x 2^(a-b), c unchanged, the budgets and energies x 4^(a-b), the CFL number unchanged -- the same mantissas.
    8192^2: q, phi, c only.  Forcing is out of scope (its amplitude takes a square root of dt)."""
    t0 = time.time()
    kw, f = base_kwargs(kind, nx), initial_fields(kind, nx)
    obs = {} if everything else dict(spectra=False, scalars=False)
    base = device_run(kind, kw, f, nsteps, **obs)
    for a, b in exps:
        scaled = device_run(kind, scale_kwargs(kw, a, b), scale_fields(f, a, b), nsteps, **obs)
        assert_unit_scaling(base, scaled, a, b, "%s %d" % (kind, nx))
    print("change of units %s %d^2, %d step(s), %d exponent pairs: %.1f s" % (kind, nx, nsteps, len(exps), time.time() - t0))


def test_change_of_units_moves_particles_exactly():
    """CoupledModel 64^2 with particles attached: the positions come back x 2^a, bit for bit."""
    from niwqg_amd import particles
    kw, f = base_kwargs("coupled", 64), initial_fields("coupled", 64)
    rng = np.random.default_rng(3)
    x0, y0 = rng.uniform(0, L, 200), rng.uniform(0, L, 200)

    def positions(kw, f, sL):
        m = start(make_device("coupled", kw), f)
        p = particles.attach(m, x0 * sL, y0 * sL)
        for _ in range(3):
            m._step_forward()
        x, y = p.positions()
        return np.array(x), np.array(y)

    bx, by = positions(kw, f, 1.0)
    assert np.abs(bx - x0).max() > 0
    for a, b in UNIT_EXPONENTS:
        gc.collect()
        sx, sy = positions(scale_kwargs(kw, a, b), scale_fields(f, a, b), 2.0 ** a)
        assert_same_bits(sx, bx, "particle x (a, b) = (%d, %d)" % (a, b), 2.0 ** a)
        assert_same_bits(sy, by, "particle y (a, b) = (%d, %d)" % (a, b), 2.0 ** a)


# ---- A2: linearity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nsteps", [(64, 4), (1024, 4), (8192, 1)])
def test_passive_scalar_is_linear_bit_for_bit(nx, nsteps):
    """c0 -> 2^s c0: c and ch x 2^s, the scalar's variance budget x 4^s, q (and Ke, the CFL number) unchanged in every bit.
    This is the exact undo of the per-row rescale of c in the MODE_QGC branches of k_x_products / k_x_products_eo; its +-900
    clamp cannot be reached without overflowing the products u c and stays untested."""
    t0 = time.time()
    kw, f = base_kwargs("qg", nx, tdiags=2), initial_fields("qg", nx)
    obs = dict(spectra=nx < 8192)
    base = device_run("qg", kw, f, nsteps, **obs)
    for s in (-64, 40, 300):
        scaled = device_run("qg", kw, dict(f, c=np.ldexp(f["c"], s)), nsteps, **obs)
        assert_linear_scaling(base, scaled, s, ("c", "ch"), ("cvar",), "qg %d" % nx)
    print("scalar linearity %d^2, %d step(s): %.1f s" % (nx, nsteps, time.time() - t0))


@pytest.mark.parametrize("nx", [64, 1024])
@pytest.mark.parametrize("kind", ["uncoupled", "ybj"])
def test_passive_waves_are_linear_bit_for_bit(kind, nx):
    """phi0 -> 2^s phi0 where q does not see the waves: phi, phih x 2^s, Kw, Pw x 4^s, q unchanged.  4 steps, a tick every
    second one (UnCoupledModel's stale gradients, quirk Q1)."""
    kw, f = base_kwargs(kind, nx, tdiags=2), initial_fields(kind, nx)
    base = device_run(kind, kw, f, 4)
    for s in (-64, 40, 200):
        scaled = device_run(kind, kw, dict(f, phi=f["phi"] * float(np.ldexp(1.0, s))), 4)
        assert_linear_scaling(base, scaled, s, ("phi", "phih"), ("Kw", "Pw", "ke_niw", "pe_niw"), "%s %d" % (kind, nx), mixed=WAVE_MIXED)


# ---- B1: weak PV under strong waves, steps against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("sq,amp", WEAK_PV)
@pytest.mark.parametrize("nx,nsteps", [(128, 6), (512, 2)])
def test_weak_pv_under_strong_waves_against_the_oracle(nx, nsteps, sq, amp):
    """CoupledModel, notebook parameters, filter on, q0 = sq (dipole + 2e-6 randn), phi0 = amp (0.1 packet + 0.02 randn):
    q, qh, phi, phih at 1e-11 of their OWN norms (the tolerance of random_configuration_against_the_oracle; the oracle moves
    by 2.6e-16 / 4.4e-16 under one ulp of these inputs, test_magnitudes_host), budgets at rtol 1e-8.

    Before q_w was rescaled per row in the (q, q_w) pair of k_x_products / k_x_products_eo / k_x_diag the roundoff of q_w's
    transform landed in q: measured errors in DESIGN.md section 6."""
    kw, f = weak_pv_state(nx, sq, amp)
    m, o = start(make_device("coupled", kw), f), start(make_oracle("coupled", kw), f)
    for _ in range(nsteps):
        m._step_forward()
        o._step_forward()
    errs = {n: rel(getattr(m, n), getattr(o, n)) for n in ("q", "qh", "phi", "phih")}
    print("weak PV %d^2 sq %g amp %g, %d steps:" % (nx, sq, amp, nsteps), {k: "%.2e" % v for k, v in errs.items()},
          "||qw||/||q|| %.1e" % (np.linalg.norm(o.qw) / np.linalg.norm(o.q)))
    for n, e in errs.items():
        assert e < 1e-11, (n, e)
    assert np.allclose([m.Ke, m.Pw, m.Kw], [o.Ke, o.Pw, o.Kw], rtol=1e-8, atol=0.0), ([m.Ke, m.Pw, m.Kw], [o.Ke, o.Pw, o.Kw])


# ---- B2: one call, at every row-kernel variant ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [64, 4096, 8192])
def test_jacobian_psi_q_of_weak_pv_against_numpy(nx):
    """jacobian_psi_q() on the white-noise state of test_gpu_at_size.test_row_kernels_8192_on_a_full_spectrum_against_numpy
    (its parameters, its seed, phi set before q) with q0 scaled by sq = 1 and 1e-8, against the same numpy expressions
    (test_magnitudes_host.jacobian_psi_q_reference), relative to the Jacobian's own norm.  The bound is that test's 1e-12 at
    both sq: the relative error of a correct kernel does not depend on sq."""
    t0 = time.time()
    rng = np.random.default_rng(21)
    q0 = 1e-5 * rng.standard_normal((nx, nx))
    phi0 = 0.05 * (rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx)))
    m = make_device("coupled", rough_kwargs(nx))
    m.set_phi(phi0)
    errs = {}
    for sq in (1.0, 1e-8):
        m.set_q(sq * q0)
        got = m.jacobian_psi_q()
        errs[sq] = rel(got, jacobian_psi_q_reference(m, sq * q0, phi0, workers=NW))
        del got
        print("%d^2 jacobian_psi_q, q0 x %g: %.2e" % (nx, sq, errs[sq]))
    print("jacobian_psi_q %d^2: %.1f s" % (nx, time.time() - t0))
    for sq, e in errs.items():
        assert e < 1e-12, (sq, e)


# ---- B3: zero and degenerate rows ---------------------------------------------------------------------------------------------------
def _four_steps(name):
    kind, kw, f = degenerate_states()[name]
    m, o = start(make_device(kind, kw), f), start(make_oracle(kind, kw), f)
    at_start = (m.jacobian_phic_phi(), o.jacobian_phic_phi()) if name == "phi_uniform" else None
    for _ in range(4):
        m._step_forward()
        o._step_forward()
    return m, o, at_start


def test_zero_waves_stay_exactly_zero():
    m, o, _ = _four_steps("phi_zero")
    assert not np.asarray(m.phi).any() and not np.asarray(m.phih).any()
    assert rel(m.q, o.q) < 1e-11 and rel(m.qh, o.qh) < 1e-11


def test_uniform_waves_have_no_jacobian():
    """phi0 uniform: J(phi*, phi) is identically zero (the mb = 0 side of the rescale in k_x_wavepv), in the device as in the oracle"""
    m, o, (jd, jo) = _four_steps("phi_uniform")
    assert not jo.any() and not np.asarray(jd).any()
    for n in ("q", "qh", "phi", "phih"):
        assert rel(getattr(m, n), getattr(o, n)) < 1e-11, n


def test_waves_that_vanish_on_half_of_the_rows():
    """phi0 exactly zero on the upper half of the y rows: rows with ma = mb = 0 next to ordinary ones in the first inversion"""
    m, o, _ = _four_steps("phi_half_masked")
    for n in ("q", "qh", "phi", "phih"):
        assert rel(getattr(m, n), getattr(o, n)) < 1e-11, n
    assert np.allclose([m.Ke, m.Pw, m.Kw], [o.Ke, o.Pw, o.Kw], rtol=1e-8, atol=0.0)


def test_zero_pv_under_waves():
    """q0 = 0: the oracle's q stays identically zero (test_magnitudes_host), so the device's is judged against ||q_w||, the
    absolute scale of the transform that q shares with q_w."""
    m, o, _ = _four_steps("q_zero")
    assert not o.q.any()
    qd, qw = np.linalg.norm(np.asarray(m.q)), np.linalg.norm(o.qw)
    print("zero PV: ||q_dev|| %.2e, ||qw|| %.2e" % (qd, qw))
    assert qd <= 1e-11 * qw
    assert rel(m.phi, o.phi) < 1e-11 and rel(m.phih, o.phih) < 1e-11


def test_zero_scalar_stays_exactly_zero():
    m, o, _ = _four_steps("c_zero")
    assert not np.asarray(m.c).any() and not np.asarray(m.ch).any()
    assert rel(m.q, o.q) < 1e-11 and rel(m.qh, o.qh) < 1e-11


def test_uniform_scalar():
    m, o, _ = _four_steps("c_one")
    assert rel(m.c, o.c) < 1e-11 and rel(m.ch, o.ch) < 1e-11
    assert rel(m.q, o.q) < 1e-11 and rel(m.qh, o.qh) < 1e-11


def test_scalar_that_lives_on_the_nyquist_column_alone():
    """c0 = (-1)^i g(y), filter off: every row of c-hat holds the self-mirrored element kx = N/2 and nothing else.  The row
    maxima of the rescale must see that element: a row that carries only it does not vanish."""
    m, o, _ = _four_steps("c_nyquist")
    assert np.linalg.norm(o.c) > 0
    assert rel(m.c, o.c) < 1e-11 and rel(m.ch, o.ch) < 1e-11
    assert rel(m.q, o.q) < 1e-11 and rel(m.qh, o.qh) < 1e-11
