"""Time-mean spectra, transfer and flux accumulated in the step (niwqg_amd/timespectra.py, nq_tspec_*).

Model A carries the attachment, model B has the same initial state and none: B is driven by ``B._ctx.step(1)`` and the two raw
binned host calls after each step (the context directly: no Python status line refreshes UnCoupledModel's gradients between the
step and the call), and its results are accumulated with ``timespectra.accumulate``.  Both binned calls are deterministic, so the
first-moment tables of A must equal B's bit for bit; the second moments may differ by the one rounding per sample the device's
fused multiply-add saves.

Shapes: 64 is the smallest fused plan (single-pass columns), every family once; 64 with dealias=True is a dual-copy context (the
mean of the two q-hat copies goes through the scratch plane the two bodies share); 1024 has two-pass columns; 4096 (two steps,
the only large case here) runs the q update on a second stream, which the sample must come after; 128, 256, 512, 2048, 8192 and
the two-pass tiles at 64 ... 512 are in tests/test_gpu_plan_ladder_analysis.py and the children of tests/test_gpu_plan_ladder.py,
through ``check_bit_identity`` of this module."""
import ctypes

import numpy as np
import pytest

from test_gpu_spectra import make, MASKS
from test_gpu_attachments import attached, batched
from test_oracle_golden import notebook_kwargs, K0, U0, L

pytestmark = pytest.mark.gpu

NSTEPS = 8
U = 2.0 ** -52
KERNEL = ("coupled", "uncoupled", "ybj")


def big_twin(nx):
    """two CoupledModels at nx with one cheap, smooth initial state (outer products: no host transform at this size)"""
    import niwqg_amd
    kw = notebook_kwargs(nx, False)
    kw.update(MASKS["filter"])
    kw.update(nu4w=3e9 * (128.0 / nx) ** 4, muw=1e-7, mu=2e-8)
    x = np.arange(nx) * (L / nx)
    q0 = U0 * K0 * (np.outer(np.cos(2 * K0 * x), np.sin(K0 * x)) + 0.3 * np.outer(np.sin(3 * K0 * x), np.sin(5 * K0 * x + 1.0)))
    phi0 = 0.2 * (1 + 0.5j) / np.sqrt(2) + 0.05 * np.outer(np.cos(K0 * x), np.exp(2j * K0 * x))
    out = []
    for _ in range(2):
        m = niwqg_amd.CoupledModel.Model(**kw)
        m.set_q(q0)
        m.set_phi(phi0)
        out.append(m)
    return out


def twin(kind, nx, mask="filter"):
    if nx >= 4096:
        return big_twin(nx)
    return make(kind, nx, mask), make(kind, nx, mask)


def state(m, kind):
    from niwqg_amd import _lib
    ids = [_lib.F_QH, _lib.F_PH] + ([_lib.F_PHIH] if kind in KERNEL else []) + ([_lib.F_CH] if kind == "qgc" else [])
    return [m._ctx.field(i) for i in ids]


def same_state(a, b, kind):
    for x, y in zip(state(a, kind), state(b, kind)):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)


def drive(B, n, spectra=True, transfer=True, every=1):
    """B's side: single steps of the context, the raw binned host calls after every `every`-th, accumulated in numpy"""
    from niwqg_amd import timespectra, _lib
    from niwqg_amd.spectra import shell_count
    sums = timespectra.tables(32, _lib.TRANSFER_ROWS, shell_count(B.nx))
    taken = 0
    for i in range(n):
        B._ctx.step(1)
        if every and (i + 1) % every == 0:
            s = B._ctx.diagnostic_sums_binned() if spectra else None
            t = B._ctx.transfer_sums_binned() if transfer else None
            timespectra.accumulate(sums, s, t)
            taken += 1
    return sums, taken


def assert_tables(R, sums, n, spectra=True, transfer=True):
    """R (A's result) against B's accumulated tables: first moments bit for bit, second moments within n roundings"""
    assert R.n == n
    first = (["S1"] if spectra else []) + (["T1", "P1"] if transfer else [])
    second = (["S2"] if spectra else []) + (["T2", "P2"] if transfer else [])
    for k in first:
        assert np.all(np.isfinite(sums[k])) and sums[k].any(), k
        assert np.array_equal(R.sums[k], sums[k]), (k, np.abs(R.sums[k] - sums[k]).max())
    for k in second:
        err = np.abs(R.sums[k] - sums[k])
        print("%s: max second-moment difference %.3e of %.3e" % (k, err.max(), sums[k].max()))
        assert np.all(err <= n * U * sums[k]), k
    for k in set(R.sums) - set(first) - set(second):
        assert not R.sums[k].any(), k
    if spectra:
        assert R.raw_spectra is R.sums["S1"]
    if transfer:
        assert R.raw_transfer is R.sums["T1"] and R.raw_cumulative is R.sums["P1"]


def assert_named(R, m, sums, n, spectra=True, transfer=True):
    from niwqg_amd import spectra as sp, transfer as tr
    M2 = (float(m.nx) * m.ny) ** 2
    if spectra:
        want = sp._named(m, sums["S1"] / n, sp.available(m))
        for name in sp.available(m):
            assert np.array_equal(R.mean(name), want[name]), name
    if transfer:
        for name in tr.available(m):
            row, factor = tr.ROWS[name]
            assert np.array_equal(R.mean_transfer(name), factor * (sums["T1"][row] / n) / M2), name
            assert np.array_equal(R.mean_flux(name), -factor * (sums["P1"][row] / n) / M2), name
            assert np.all(np.isfinite(R.variance_flux(name))) and np.all(np.isfinite(R.variance_transfer(name))), name


# ---- 5. bit identity, batched ----------------------------------------------------------------------------------------------------
CASES5 = [("coupled", 64, "filter", NSTEPS), ("uncoupled", 64, "filter", NSTEPS), ("ybj", 64, "filter", NSTEPS), ("qg", 64, "filter", NSTEPS),
          ("qgc", 64, "filter", NSTEPS), ("coupled", 64, "mask", NSTEPS), ("coupled", 1024, "filter", NSTEPS), ("coupled", 4096, "filter", 2)]


@pytest.mark.parametrize("kind, nx, mask, n", CASES5)
def test_bit_identity_batched(kind, nx, mask, n):
    A, B = twin(kind, nx, mask)
    check_bit_identity(A, B, kind, n, mask)


def check_bit_identity(A, B, kind, n, mask="filter"):
    """A with both bodies attached and two batched nq_step calls, B driven by single steps and the two host calls"""
    from niwqg_amd import timespectra
    if mask == "mask":
        assert A._ctx.dual_q
    T = timespectra.attach(A, spectra=True, transfer=True, every=1)
    assert T.info() == {"n": 0, "steps": 0}                      # attach takes no sample
    first = n // 2 - 1 if n > 2 else n
    A._ctx.step(first)                                           # batched calls: the samples are taken inside nq_step(n)
    if n > first:
        A._ctx.step(n - first)
    assert T.info() == {"n": n, "steps": n}
    sums, taken = drive(B, n)
    assert taken == n
    R = T.result()
    assert R.steps == n
    assert_tables(R, sums, n)
    assert_named(R, A, sums, n)
    same_state(A, B, kind)
    T.detach()


# ---- 6. each body alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectra, transfer", [(True, False), (False, True)])
def test_each_body_alone(spectra, transfer):
    from niwqg_amd import timespectra
    A, B = twin("coupled", 64)
    T = timespectra.attach(A, spectra=spectra, transfer=transfer, every=1)
    A._ctx.step(5)
    A._ctx.step(3)
    sums, _ = drive(B, NSTEPS, spectra, transfer)
    R = T.result()
    assert_tables(R, sums, NSTEPS, spectra, transfer)
    assert_named(R, A, sums, NSTEPS, spectra, transfer)
    assert (R.raw_spectra is None) == (not spectra) and (R.raw_transfer is None) == (not transfer)
    with pytest.raises(KeyError):
        (R.mean_flux if spectra else R.mean)("ens")
    same_state(A, B, "coupled")


# ---- 7. the run is left alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, mask", [("coupled", "filter"), ("coupled", "mask"), ("uncoupled", "filter"), ("qgc", "filter")])
def test_the_run_is_left_alone(kind, mask):
    """B takes the same steps with no attachment and no host call at all"""
    from niwqg_amd import timespectra
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    A, B = twin(kind, 64, mask)
    T = timespectra.attach(A, every=1)
    A._ctx.step(3)
    A._ctx.step(5)
    B._ctx.step(NSTEPS)
    assert T.info()["n"] == NSTEPS
    same_state(A, B, kind)
    for m in (A, B):
        m._after_steps()
    sa, sb = isotropic_spectra(A), isotropic_spectra(B)
    for name in sb.values:
        assert sb.values[name].any() and np.array_equal(sa.values[name], sb.values[name]), name
    ta, tb = spectral_transfer(A), spectral_transfer(B)
    for name in tb.transfer:
        assert tb.transfer[name].any() and np.array_equal(ta.transfer[name], tb.transfer[name]), name
        assert np.array_equal(ta.flux[name], tb.flux[name]), name
    A._ctx.step(2)                                               # and after the host calls the two still step alike
    B._ctx.step(2)
    same_state(A, B, kind)


# ---- 8. every order and cadence --------------------------------------------------------------------------------------------------
def test_cadence_sample_reset_and_batched_against_single_steps():
    from niwqg_amd import timespectra
    A, B = twin("coupled", 64)
    TA, TB = timespectra.attach(A, every=3), timespectra.attach(B, every=3)
    assert batched(A, NSTEPS) == NSTEPS - 2                      # (the first step ends with the tick of tc = 0)
    for _ in range(NSTEPS):
        B._step_forward()
    assert TA.info() == TB.info() == {"n": 2, "steps": NSTEPS}
    RA, RB = TA.result(), TB.result()
    for k in timespectra.TABLES:
        assert RA.sums[k].any() and np.array_equal(RA.sums[k], RB.sums[k]), k
    # against the host calls at steps 3 and 6 of a third run
    C = make("coupled", 64)
    C._step_forward()                                            # (the tick of tc = 0, as A and B had it)
    sums = timespectra.tables(32, 6, len(RA.k))
    for i in range(2, NSTEPS + 1):
        C._ctx.step(1)
        if i % 3 == 0:
            timespectra.accumulate(sums, C._ctx.diagnostic_sums_binned(), C._ctx.transfer_sums_binned())
    assert_tables(RA, sums, 2)
    # sample() adds the current state, reset() zeroes
    now = timespectra.accumulate(timespectra.tables(32, 6, len(RA.k)), A._ctx.diagnostic_sums_binned(), A._ctx.transfer_sums_binned())
    TA.sample()
    R3 = TA.result()
    assert R3.n == 3 and R3.steps == NSTEPS
    for k in ("S1", "T1", "P1"):
        assert np.array_equal(R3.sums[k], RA.sums[k] + now[k]), k
    TA.reset()
    assert TA.info() == {"n": 0, "steps": NSTEPS}
    with pytest.raises(RuntimeError, match="no sample"):
        TA.result()
    TA.sample()
    R1 = TA.result()
    for k in ("S1", "T1", "P1"):
        assert np.array_equal(R1.sums[k], now[k]), k
    A._step_forward()                                            # step 9: the phase of `every` survived the reset
    assert TA.info() == {"n": 2, "steps": NSTEPS + 1}


def test_every_zero_samples_only_on_request():
    from niwqg_amd import timespectra
    A = make("qg", 64)
    T = timespectra.attach(A, every=0)
    A._ctx.step(4)
    assert T.info() == {"n": 0, "steps": 4}
    T.sample()
    R = T.result()
    assert np.array_equal(R.raw_spectra, A._ctx.diagnostic_sums_binned()) and np.array_equal(R.raw_transfer, A._ctx.transfer_sums_binned())
    assert np.array_equal(R.raw_cumulative, np.cumsum(R.raw_transfer, axis=1))


# ---- 9. with the others ----------------------------------------------------------------------------------------------------------
def everything():
    """forcing, particles and the recorder of test_gpu_attachments, averages and the time-mean spectra on one 64^2 CoupledModel"""
    from niwqg_amd import averages, timespectra
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    m, F, P, R, b0 = attached("coupled", 64)
    Av = averages.attach(m, ["q", "phi2"], [("q", "phi2")], every=2)
    before = m._ctx.device_bytes()
    isotropic_spectra(m)                                         # the context-owned planes of the two calls exist from here on
    spectral_transfer(m)
    base = m._ctx.device_bytes()
    T = timespectra.attach(m, every=2)
    assert m._ctx.device_bytes() > base
    return m, T, [F, P, R, Av], base, b0 + (base - before)


@pytest.mark.parametrize("ts_first", [True, False])
def test_with_the_other_attachments(ts_first):
    from niwqg_amd import timespectra
    A, TA, othersA, baseA, bareA = everything()
    B, TB, othersB, _, _ = everything()
    assert batched(A, NSTEPS) == NSTEPS - 1
    for _ in range(NSTEPS):
        B._step_forward()
    assert TA.info() == TB.info() == {"n": NSTEPS // 2, "steps": NSTEPS}
    RA, RB = TA.result(), TB.result()
    for k in timespectra.TABLES:
        assert np.all(np.isfinite(RA.sums[k])) and RA.sums[k].any() and np.array_equal(RA.sums[k], RB.sums[k]), k
    same_state(A, B, "coupled")
    sa, sb = othersA[3].result(), othersB[3].result()
    for k in sa.sums:
        assert np.array_equal(sa.sums[k], sb.sums[k]), k
    # the forced state is what was sampled: the last sample is the host calls' view of the state now
    TA.reset()
    TA.sample()
    R1 = TA.result()
    assert np.array_equal(R1.raw_spectra, A._ctx.diagnostic_sums_binned()) and np.array_equal(R1.raw_transfer, A._ctx.transfer_sums_binned())
    # detach: the tables go back, the context-owned planes stay; either order
    c = A._ctx
    if ts_first:
        TA.detach()
        assert c.device_bytes() == baseA                         # the value before its attach, the four others still there
        for att in othersA:
            att.detach()
    else:
        for att in othersA:
            att.detach()
        held = c.device_bytes()
        TA.detach()
        assert c.device_bytes() < held
    assert c.device_bytes() == bareA                             # the context and the planes its own two calls allocated
    assert "_timespectra" not in A.__dict__
    with pytest.raises(RuntimeError, match="nq_tspec_info"):
        c.tspec_info()
    A._step_forward()
    assert np.all(np.isfinite(np.array(A.qh)))


def test_device_bytes_return_at_detach_and_close_leaves_the_device_usable():
    from niwqg_amd import timespectra
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    # attach on a context that has not made the two calls yet: their planes are allocated at attach and stay at detach
    m = make("coupled", 64)
    fresh = m._ctx.device_bytes()
    T = timespectra.attach(m)
    with_tables = m._ctx.device_bytes()
    nb = len(isotropic_spectra(m).shell)
    spectral_transfer(m)
    assert m._ctx.device_bytes() == with_tables                  # nothing left for the two calls to allocate
    assert with_tables - fresh >= (2 * 32 + 4 * 6) * nb * 8
    T.detach()
    owned = m._ctx.device_bytes()
    assert with_tables - owned == (2 * 32 + 4 * 6) * nb * 8      # exactly the tables
    for order in (0, 1):                                         # from here attach / detach return to `owned`, around the others too
        from niwqg_amd import averages
        first = timespectra.attach(m, every=1) if order == 0 else averages.attach(m, ["q"])
        second = averages.attach(m, ["q"]) if order == 0 else timespectra.attach(m, every=1)
        assert m._ctx.device_bytes() > owned
        m._ctx.step(2)
        first.detach()
        assert owned < m._ctx.device_bytes()
        second.detach()
        assert m._ctx.device_bytes() == owned
    C = everything()[0]
    batched(C, 3)
    C._ctx.close()                                               # nq_destroy releases the attachment itself
    assert C._ctx.h is None
    D, TD = everything()[:2]
    batched(D, 2)
    assert TD.result().n == 1 and np.all(np.isfinite(np.array(D.qh)))


# ---- 10. any-size ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupled", "qg"])
def test_any_size_means(kind):
    from niwqg_amd import timespectra
    from niwqg_amd.spectra import isotropic_spectra
    from niwqg_amd.transfer import spectral_transfer
    n = 4
    A, B = twin(kind, 96)
    assert A._any_size
    T = timespectra.attach(A, every=1)
    sp, tr, fl = [], [], []
    for _ in range(n):
        A._step_forward()
        B._step_forward()
        sp.append(isotropic_spectra(B).values)
        t = spectral_transfer(B)
        tr.append(t.transfer)
        fl.append(t.flux)
    R = T.result()
    assert R.n == n and R.raw_spectra is None and R.raw_transfer is None

    def close(got, stack, what):
        want, scale = np.mean(stack, axis=0), np.mean(np.abs(stack), axis=0)
        err = np.abs(got - want)
        print("%s: max err %.3e, bound %.3e" % (what, err.max(), ((n + 8) * U * scale).max()))
        assert scale.any() and np.all(err <= (n + 8) * U * scale), what

    for name in sp[0]:
        close(R.mean(name), np.array([s[name] for s in sp]), name)
    for name in tr[0]:
        close(R.mean_transfer(name), np.array([t[name] for t in tr]), "T " + name)
        close(R.mean_flux(name), np.array([f[name] for f in fl]), "Pi " + name)
    T.detach()
    A._step_forward()


# ---- 11. refusals ----------------------------------------------------------------------------------------------------------------
def test_slab_ranks_refuse():
    import niwqg_amd
    from niwqg_amd import timespectra, _lib
    m = niwqg_amd.CoupledModel.Model(slab=2, **notebook_kwargs(64, True))
    with pytest.raises(NotImplementedError, match="slab"):
        timespectra.attach(m)
    L_ = _lib.lib()
    h = m._ctx.sim.ranks[0].h
    i3 = (ctypes.c_longlong * 3)()
    d = np.zeros(4)
    assert L_.nq_tspec_attach(h, 3, 1) == -4
    assert L_.nq_tspec_detach(h) == -4
    assert L_.nq_tspec_sample(h) == -4
    assert L_.nq_tspec_reset(h) == -4
    assert L_.nq_tspec_info(h, i3) == -4
    assert L_.nq_tspec_read(h, 0, _lib._dptr(d)) == -4


def test_library_refusals_and_missing_transfers():
    from niwqg_amd import timespectra, _lib
    m = make("ybj", 64)
    c, L_ = m._ctx, _lib.lib()
    d = np.zeros(4)
    assert L_.nq_tspec_read(c.h, 0, _lib._dptr(d)) == -4 and b"no time-mean spectra attached" in L_.nq_last_error(c.h)
    assert L_.nq_tspec_sample(c.h) == -4 and L_.nq_tspec_detach(c.h) == -4 and L_.nq_tspec_reset(c.h) == -4
    for mask, every in ((0, 1), (4, 1), (-1, 1), (3, -1)):
        assert L_.nq_tspec_attach(c.h, mask, every) == -1, (mask, every)
    assert L_.nq_tspec_sample(c.h) == -4                         # nothing got attached
    T = timespectra.attach(m, every=1)
    assert L_.nq_tspec_attach(c.h, 3, 1) == -4                   # a second attach
    with pytest.raises(RuntimeError, match="already"):
        timespectra.attach(m)
    with pytest.raises(RuntimeError, match="table 6"):
        c.tspec_read(6)
    c.step(3)
    assert c.tspec_info() == (3, 3, 3)
    R = T.result()
    # YBJModel does not step q: no ke_qg or ens transfer, the error spectral_transfer raises
    from niwqg_amd.transfer import spectral_transfer
    with pytest.raises(ValueError, match="not available") as e0:
        spectral_transfer(m, ["ens"])
    for call in (R.mean_transfer, R.mean_flux, R.variance_flux):
        for name in ("ke_qg", "ens"):
            with pytest.raises(ValueError, match="spectral_transfer: '%s' not available" % name):
                call(name)
    assert "valid names: ke_niw_adv, ke_niw_ref" in str(e0.value)
    assert R.mean_flux("ke_niw_adv").any() and not R.raw_transfer[:2].any()
    with pytest.raises(ValueError, match="several raw rows"):
        R.variance("ep_psi")
    assert np.all(np.isfinite(R.variance("ke_niw")))
    T.detach()
