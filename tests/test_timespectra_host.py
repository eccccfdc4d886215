"""Time-mean spectra, transfer and flux, host side (niwqg_amd/timespectra.py): the C ABI's names in the header and in the built
library, every refusal of the contract before any device call, the accumulation rule's numpy restatement against a hand-written
loop, and the any-size flavour on a fake model whose spectra are known arrays."""
import ctypes
import os
import re

import numpy as np
import pytest

from niwqg_amd import _attach, _lib, spectra, timespectra, transfer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = 16
NB = spectra.shell_count(NX)


class Touchy(object):
    """a stub context: any use of it is recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        self.calls.append(name)
        raise AssertionError("the context was touched: %s" % name)


class FakeKernelModel(object):
    """enough of a CoupledModel for the argument checks and for the formulas of ``result()``"""
    nx = ny = NX
    dk = 0.25
    f, kappa2, hslash = 1e-4, 3.0, 0.7
    nu4, nu, mu, nu4w, nuw, muw = 5.0, 2.0, 0.5, 7.0, 3.0, 0.25
    model_id = _lib.COUPLED

    def __init__(self, ctx=None):
        self._ctx = ctx


class FakeAnySizeModel(FakeKernelModel):
    """the any-size path as the attachment sees it: _spectra / _transfer return known arrays, different at every call"""
    _any_size = True

    def __init__(self):
        FakeKernelModel.__init__(self)
        self.rng = np.random.default_rng(4)
        self.step = 0
        self.spectra_log, self.transfer_log = [], []          # (step, {name: values}) of every call

    def _spectra(self, names):
        v = {n: self.rng.standard_normal(NB) + 2.0 for n in names}
        self.spectra_log.append((self.step, v))
        return v

    def _transfer(self, names):
        v = {n: self.rng.standard_normal(NB) for n in names}
        self.transfer_log.append((self.step, v))
        return v

    def one_step(self):
        self.step += 1
        _attach.after_step(self)


# ---- 1. the binding ----------------------------------------------------------------------------------------------------------
def test_abi_names_in_header_and_library():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "niwqg_amd.h")).read()
    I, LLP, DP, CTX = ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    want = {"nq_tspec_attach": [CTX, I, I], "nq_tspec_detach": [CTX], "nq_tspec_sample": [CTX], "nq_tspec_reset": [CTX],
            "nq_tspec_info": [CTX, LLP], "nq_tspec_read": [CTX, I, DP]}
    for name, argtypes in want.items():
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint %s\(" % name, header), name
        fn = getattr(L, name)
        assert list(fn.argtypes) == argtypes and fn.restype is I, name
    for i, n in enumerate(("NQ_TSPEC_S1", "NQ_TSPEC_S2", "NQ_TSPEC_T1", "NQ_TSPEC_T2", "NQ_TSPEC_P1", "NQ_TSPEC_P2")):
        assert re.search(r"\b%s = %d\b" % (n, i), header) and getattr(_lib, n[3:]) == i
    assert _lib.TSPEC_SPECTRA == 1 and _lib.TSPEC_TRANSFER == 2
    # null contexts are refused without a device
    i3 = (ctypes.c_longlong * 3)()
    d = (ctypes.c_double * 4)()
    assert L.nq_tspec_attach(None, 3, 1) != 0
    assert L.nq_tspec_detach(None) != 0
    assert L.nq_tspec_sample(None) != 0
    assert L.nq_tspec_reset(None) != 0
    assert L.nq_tspec_info(None, i3) != 0
    assert L.nq_tspec_read(None, 0, d) != 0


# ---- 2. argument checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(spectra=False, transfer=False), dict(spectra=1), dict(transfer="yes"), dict(spectra=None), dict(every=-1), dict(every=1.0),
    dict(every=True), dict(every="3"), dict(every=None),
])
def test_value_errors_before_any_device_call(kw):
    ctx = Touchy()
    with pytest.raises(ValueError, match="valid"):
        timespectra.attach(FakeKernelModel(ctx), **kw)
    assert ctx.calls == []
    with pytest.raises(ValueError, match="timespectra.attach"):
        timespectra.check(**kw)


def test_check_normalises():
    assert timespectra.check() == (True, True, 1)
    assert timespectra.check(np.bool_(True), False, np.int64(0)) == (True, False, 0)


def test_slab_refusal_second_attach_and_detached_use():
    m = FakeKernelModel()
    # a model whose context is not the single-GPU one (a slab-decomposed simulation's facade) is refused, after the argument checks
    with pytest.raises(NotImplementedError, match="slab"):
        timespectra.attach(m)
    with pytest.raises(ValueError):
        timespectra.attach(m, every=-1)
    m.__dict__["_timespectra"] = object()
    with pytest.raises(RuntimeError, match="already"):
        timespectra.attach(m)
    A = timespectra.Accumulator(None, True, True, 1)
    for call in (A.sample, A.reset, A.result, A.info):
        with pytest.raises(RuntimeError, match="^timespectra: detached$"):
            call()
    A.detach()                                        # idempotent


def random_tables(n=7, seed=2):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((32, NB)) * 10.0 ** rng.integers(-3, 4, (32, 1)), rng.standard_normal((_lib.TRANSFER_ROWS, NB)))
            for _ in range(n)]


def fused_result(samples, m=None):
    sums = timespectra.tables(32, _lib.TRANSFER_ROWS, NB)
    for s, t in samples:
        assert timespectra.accumulate(sums, s, t) is sums
    m = m or FakeKernelModel()
    return timespectra.TimeSpectra(m, len(samples), 3 * len(samples), sums, spectra.available(m), transfer.available(m), True), sums


def test_variance_of_multi_row_spectra_raises_and_says_why():
    R, _ = fused_result(random_tables())
    for name in ("ep_psi", "ep_phi", "chi_phi"):
        with pytest.raises(ValueError, match="several raw rows"):
            R.variance(name)
    assert set(timespectra.MULTI_ROW) == {"ep_psi", "ep_phi", "chi_phi", "ep_c", "chi_c"}
    assert R.variance("ens").shape == (NB,) and np.all(np.isfinite(R.variance("ens")))
    for name in spectra.KERNEL_NAMES + spectra.QG_SCALAR_NAMES:
        assert (name in timespectra.MULTI_ROW) != (name in timespectra.SINGLE_ROW), name
    # names the model does not have: the errors of isotropic_spectra / spectral_transfer
    with pytest.raises(ValueError, match="isotropic_spectra: 'C2' not available"):
        R.mean("C2")
    with pytest.raises(ValueError, match="spectral_transfer: 'gradC2' not available"):
        R.mean_flux("gradC2")
    ybj = FakeKernelModel()
    ybj.model_id = _lib.YBJ
    Ry, _ = fused_result(random_tables(2), ybj)
    for call in (Ry.mean_transfer, Ry.mean_flux, Ry.variance_transfer, Ry.variance_flux):
        with pytest.raises(ValueError, match="spectral_transfer: 'ens' not available"):
            call("ens")
    assert Ry.mean_transfer("ke_niw_adv").shape == (NB,)


# ---- 3. the accumulation rule ------------------------------------------------------------------------------------------------
def test_accumulate_against_a_hand_written_loop():
    samples = random_tables()
    n = len(samples)
    R, sums = fused_result(samples)
    S1, S2 = np.zeros((32, NB)), np.zeros((32, NB))
    T1, P1, P2 = (np.zeros((_lib.TRANSFER_ROWS, NB)) for _ in range(3))
    for s, t in samples:
        S1 = np.add(S1, s)
        S2 = S2 + s * s
        T1 = np.add(T1, t)
        for r in range(_lib.TRANSFER_ROWS):
            c = 0.0
            for b in range(NB):                        # one shell after the other
                c = c + t[r, b]
                P1[r, b] = P1[r, b] + c
                P2[r, b] = P2[r, b] + c * c
    assert np.array_equal(sums["S1"], S1) and np.array_equal(sums["S2"], S2) and np.array_equal(sums["T1"], T1)
    assert np.array_equal(sums["P1"], P1) and np.array_equal(sums["P2"], P2)
    assert R.raw_spectra is sums["S1"] and R.raw_transfer is sums["T1"] and R.raw_cumulative is sums["P1"]
    assert R.n == n and R.steps == 3 * n
    assert np.array_equal(R.k, np.arange(NB) * 0.25) and np.array_equal(R.k_edge, (np.arange(NB) + 0.5) * 0.25)
    m = FakeKernelModel()
    M2 = float(NX * NX) ** 2
    # the named results: the tree's formulas applied to S1 / n
    named = spectra._named(m, S1 / n, spectra.available(m))
    for name in spectra.available(m):
        assert np.array_equal(R.mean(name), named[name]), name
    stack = np.array([t for _, t in samples])
    for name in transfer.available(m):
        row, factor = transfer.ROWS[name]
        assert np.array_equal(R.mean_transfer(name), factor * (T1[row] / n) / M2), name
        assert np.array_equal(R.mean_flux(name), -factor * (P1[row] / n) / M2), name
        # the flux of the mean transfer: the two differ by the rounding of n sequential additions per running sum.  Every
        # partial sum is bounded by A = sum_samples sum_b |x|; an addition rounds by at most 2^-53 of that, there are NB of
        # them in a cumsum and n in the sum over the samples, on each side
        want = -factor * np.cumsum(T1[row] / n) / M2
        A = np.abs(stack[:, row]).sum() / n
        bound = 2.0 * (n + NB + 2) * 2.0 ** -53 * A * abs(factor) / M2
        assert np.abs(R.mean_flux(name) - want).max() <= bound, name
        assert np.abs(R.mean_flux(name)).max() > 1e3 * bound
    # variances against numpy's, to the digits the raw-moment formula keeps: 1e-12 of the second moment
    for name, row in (("ke_qg", 11), ("ens", 6), ("gamma_a", 24)):
        c = float(spectra._named(m, np.eye(32)[row], [name])[name])
        x = np.array([s[row] for s, _ in samples]) * c
        assert np.abs(R.variance(name) - x.var(axis=0)).max() <= 1e-12 * (x * x).mean(axis=0).max(), name
    for name in transfer.available(m):
        row, factor = transfer.ROWS[name]
        x = stack[:, row] * factor / M2
        assert np.abs(R.variance_transfer(name) - x.var(axis=0)).max() <= 1e-12 * (x * x).mean(axis=0).max(), name
        c = np.cumsum(x, axis=1)
        assert np.abs(R.variance_flux(name) - c.var(axis=0)).max() <= 1e-12 * (c * c).mean(axis=0).max(), name


def test_one_body_alone():
    s, t = random_tables(1)[0]
    sums = timespectra.accumulate(timespectra.tables(32, 6, NB), spectra=s)
    assert np.array_equal(sums["S1"], s) and not any(sums[k].any() for k in ("T1", "T2", "P1", "P2"))
    sums = timespectra.accumulate(timespectra.tables(32, 6, NB), transfer=t)
    assert np.array_equal(sums["P1"], np.cumsum(t, axis=1)) and not sums["S1"].any() and not sums["S2"].any()
    m = FakeKernelModel()
    R = timespectra.TimeSpectra(m, 1, 1, sums, [], transfer.available(m), True)
    assert R.raw_spectra is None and R.raw_transfer is sums["T1"]
    with pytest.raises(KeyError, match="spectra=True"):
        R.mean("ens")


# ---- 4. the any-size flavour -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every, due", [(0, []), (1, [1, 2, 3, 4, 5, 6, 7]), (3, [3, 6])])
def test_any_size_sampling_steps_and_results(every, due):
    m = FakeAnySizeModel()
    T = timespectra.attach(m, every=every)
    assert m.__dict__["_timespectra"] is T and T.info() == {"n": 0, "steps": 0}          # attach takes no sample
    assert m.spectra_log == [] and m.transfer_log == []
    for _ in range(7):
        m.one_step()
    assert [s for s, _ in m.spectra_log] == due and [s for s, _ in m.transfer_log] == due
    assert T.info() == {"n": len(due), "steps": 7}
    if not due:
        with pytest.raises(RuntimeError, match="no sample"):
            T.result()
    T.sample()                                            # one more, now
    n = len(due) + 1
    R = T.result()
    assert R.n == n and R.steps == 7 and R.raw_spectra is None and R.raw_transfer is None and R.raw_cumulative is None
    for name in spectra.available(m):
        x = np.array([v[name] for _, v in m.spectra_log])
        S = np.zeros(NB)
        for row in x:
            S = S + row
        assert np.array_equal(R.mean(name), S / n), name
        if name in timespectra.MULTI_ROW:
            with pytest.raises(ValueError, match="several raw rows"):
                R.variance(name)
        else:
            assert np.abs(R.variance(name) - x.var(axis=0)).max() <= 1e-12 * (x * x).mean(axis=0).max(), name
    for name in transfer.available(m):
        x = np.array([v[name] for _, v in m.transfer_log])
        S, P = np.zeros(NB), np.zeros(NB)
        for row in x:
            S = S + row
            P = P + np.cumsum(row)
        assert np.array_equal(R.mean_transfer(name), S / n) and np.array_equal(R.mean_flux(name), -(P / n)), name
        f = np.array([transfer.flux_of(row) for row in x])
        assert np.abs(R.variance_flux(name) - f.var(axis=0)).max() <= 1e-12 * (f * f).mean(axis=0).max(), name
    # reset zeroes the sums and n, not the step counter (so the phase of `every` stays)
    T.reset()
    assert T.info() == {"n": 0, "steps": 7}
    m.one_step()
    m.one_step()
    assert T.info() == {"n": {0: 0, 1: 2, 3: 1}[every], "steps": 9}
    if every:
        want = np.zeros(NB)
        for _, v in m.spectra_log[n:]:
            want = want + v["ens"]
        assert np.array_equal(T.result().sums["S1"][spectra.available(m).index("ens")], want)
    T.detach()
    assert "_timespectra" not in m.__dict__ and T.m is None
    m.one_step()                                          # the model steps on without it


def test_any_size_one_body_takes_only_its_own_pass():
    m = FakeAnySizeModel()
    T = timespectra.attach(m, spectra=False, every=1)
    m.one_step()
    assert m.spectra_log == [] and len(m.transfer_log) == 1
    R = T.result()
    assert R.spectra_names == [] and R.mean_flux("ens").shape == (NB,)
    with pytest.raises(KeyError):
        R.mean("ens")


def test_the_slot_is_last_in_after_step():
    order = []

    class Probe(object):
        def __init__(self, slot):
            self.slot = slot

        def _after_step(self):
            order.append(self.slot)

    m = FakeAnySizeModel()
    slots = ("_timespectra", "_averages", "_frequency", "_particles", "_forcing")
    for s in slots:
        m.__dict__[s] = Probe(s)
    _attach.after_step(m)
    assert order == ["_forcing", "_particles", "_frequency", "_averages", "_timespectra"]
    assert timespectra.Accumulator.SLOT == "_timespectra"
