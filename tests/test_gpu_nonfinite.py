"""Non-finite model states: the CFL maxima of the device and the status line that stops a run.

The reference stops a run at the first status line whose CFL is not below cflmax (ref niwqg/Kernel.py:598, QGModel.py:578).  Its
CFL is numpy's max over |u|, |v| (and |phi|), which is NaN as soon as one element is, and `nan < cflmax` is False: a state that
blew up raises AssertionError there.  Every device maximum behind a status line has to propagate NaN the same way (an fmax tree
drops it, and an all-NaN plane would reduce to 0).  Expected values: the numpy oracle (oracle/niwqg_oracle.py).
"""
import warnings

import numpy as np
import pytest

from oracle import niwqg_oracle as O
from test_oracle_golden import notebook_kwargs, L, U0

pytestmark = pytest.mark.gpu

KINDS = {"coupled": "CoupledModel", "uncoupled": "UnCoupledModel", "ybj": "YBJModel", "qg": "QGModel"}


def _kw(kind, nx, **over):
    kw = notebook_kwargs(nx, True)
    if kind == "qg":
        kw = dict(L=L, nx=nx, tmax=kw["tmax"], dt=kw["dt"], twrite=kw["twrite"], nu4=kw["nu4"], use_filter=True, U=-U0,
                  tdiags=kw["tdiags"])
    kw.update(over)
    return kw


def _device(kind, **kw):
    import niwqg_amd
    return getattr(niwqg_amd, KINDS[kind]).Model(**kw)


def _oracle(kind, **kw):
    kw = dict(kw)
    kw.pop("slab", None)
    return O.QGOracle(**kw) if kind == "qg" else O.NIWQGOracle(kind, **kw)


def _state(nx):
    """a smooth finite q and phi of the notebook's magnitudes"""
    k = 2 * np.pi / L
    x = np.arange(nx) * L / nx
    X, Y = np.meshgrid(x, x)
    q = 1e-5 * (np.sin(3 * k * X) * np.cos(2 * k * Y) + 0.5 * np.cos(5 * k * X + 1.0) * np.sin(4 * k * Y))
    phi = (2 * U0 / np.sqrt(2)) * ((1 + 1j) + 0.3 * np.exp(1j * (2 * k * X - k * Y)))
    return q, phi


def _set(mods, q, phi):
    for m in mods:
        m.set_q(q)
        if phi is not None:
            m.set_phi(phi)


def _same(got, want, rtol):
    """NaN-ness preserved; finite values equal (to the transforms' rounding: the device forms u, v, phi by its own FFTs)"""
    assert np.isnan(got) == np.isnan(want), (got, want)
    if not np.isnan(want):
        assert np.isinf(got) == np.isinf(want), (got, want)
        if np.isfinite(want):
            assert abs(got - want) <= rtol * abs(want), (got, want)


def _nan_at(a, idx):
    a = a.copy()
    a.flat[idx] = np.nan
    return a


# ---- A1: the device maxima at the value level --------------------------------------------------------------------------
def _a1_cases(nx):
    n2 = nx * nx
    mid = 1024 * 256 + 3 if n2 > 1024 * 256 + 3 else n2 // 2 + 5      # past one pass of the 1024 x 256 grid-stride reduction
    return [("finite", None), ("phi_nan_first", 0), ("phi_nan_last", n2 - 1), ("phi_nan_strided", mid), ("all_nan", None),
            ("q_inf", None)]


def _a1_state(case, idx, nx):
    q, phi = _state(nx)
    if case.startswith("phi_nan"):
        phi = _nan_at(phi, idx)
    elif case == "all_nan":
        q, phi = np.full_like(q, np.nan), np.full_like(phi, np.nan)
    elif case == "q_inf":
        q = q.copy()
        q.flat[nx * nx // 3] = np.inf
    return q, phi


@pytest.mark.parametrize("kind,nx", [("coupled", 64), ("uncoupled", 64), ("qg", 64), ("coupled", 1024), ("qg", 1024)])
def test_cfl_maxima_of_the_device_against_numpy(kind, nx):
    """NQ_S_CFL and NQ_S_MAX_PHI through Context.scalar, and Context.status_cfl_max after a step with request_stage4_max, equal
    the oracle's _calc_cfl() (max |phi|) with NaN preserved: one NaN in phi at the first, the last and a grid-strided element
    (set_phi does not re-invert: only the |phi| reduction sees it), an all-NaN state, one +inf in q, and a finite state.  At
    1024^2 the 1024-block reductions stride (one thread visits several elements); there the (slow) oracle step is taken for the
    finite state and the strided NaN only."""
    from niwqg_amd import _lib
    kw = _kw(kind, nx)
    m, o = _device(kind, **kw), _oracle(kind, **kw)          # one of each: set_q / set_phi start every case afresh
    for case, idx in _a1_cases(nx):
        if kind == "qg" and case.startswith("phi_"):
            continue
        q, phi = _a1_state(case, idx, nx)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _set((m, o), q, None if kind == "qg" else phi)
            scale = m.dt / m.dx
            want = o._calc_cfl()
            got = m._ctx.scalar(_lib.S_CFL) * scale
            print("%s %d %s: CFL device %r oracle %r" % (kind, nx, case, got, want))
            _same(got, want, 1e-12)
            if kind != "qg":
                got_phi = m._ctx.scalar(_lib.S_MAX_PHI)
                want_phi = np.abs(o.phi).max()
                print("%s %d %s: max |phi| device %r oracle %r" % (kind, nx, case, got_phi, want_phi))
                _same(got_phi, want_phi, 1e-12)
            if kind != "qg" and (nx < 1024 or case in ("finite", "phi_nan_strided")):
                # the status line after a step without a tick: the fourth stage's max |u|, |v| and the new state's max |phi|
                m._ctx.request_stage4_max()
                m._ctx.step(1)
                o._step_etdrk4()
                got4 = m._ctx.status_cfl_max() * scale
                want4 = o._calc_cfl()
                print("%s %d %s: stage-4 CFL device %r oracle %r" % (kind, nx, case, got4, want4))
                _same(got4, want4, 1e-9)


# ---- A2: the status line raises where the reference's does ----------------------------------------------------------------
PATHS = {"fused": dict(nx=64), "slab": dict(nx=64, slab=2), "anysize": dict(nx=96)}


@pytest.mark.parametrize("tdiags", [1, 10 ** 9])
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_status_line_of_a_nan_state_raises_as_the_reference(kind, path, tdiags):
    """One NaN in q, twrite = 1: the first status line raises AssertionError on the device exactly where the oracle raises, and
    m.cfl is NaN as the oracle's is.  tdiags = 1: the CFL of _calc_cfl after a tick; tdiags = 10^9: the fourth stage's maxima
    recorded during the step (Kernel.py:440-442)."""
    spec = dict(PATHS[path])
    nx = spec.pop("nx")
    kw = _kw(kind, nx, twrite=1, tdiags=tdiags)
    m = _device(kind, **dict(kw, **spec))
    o = _oracle(kind, **kw)
    q, phi = _state(nx)
    q = _nan_at(q, nx * nx // 2 + 7)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _set((m, o), q, None if kind == "qg" else phi)
        with pytest.raises(AssertionError):
            o._step_forward()
        with pytest.raises(AssertionError):
            m._step_forward()
    assert m.tc == o.tc == 1
    assert np.isnan(o.cfl) and np.isnan(m.cfl), (o.cfl, m.cfl)


# ---- A3: a blow-up between two status lines -------------------------------------------------------------------------------
A3_DT_FACTOR = 1000.0       # picked with the oracle: every field is NaN at the first status line (tc = 4), not merely large


def test_blow_up_between_status_lines_stops_the_run_where_the_oracle_stops():
    """run() with twrite = 4 and a dt 1000 times the notebook's: the oracle's fields are all NaN at tc = 4 (asserted), so its CFL
    is NaN and the run stops there; the device run must stop at the same tc instead of carrying NaN fields on to tmax."""
    kw = notebook_kwargs(64, True)
    dt = kw["dt"] * A3_DT_FACTOR
    kw.update(dt=dt, twrite=4, tmax=12.5 * dt)
    m, o = _device("coupled", **kw), _oracle("coupled", **kw)
    q, phi = _state(64)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _set((m, o), q, phi)
        with pytest.raises(AssertionError):
            o.run()
        assert o.tc == 4 and np.isnan(o.q).all() and np.isnan(o.phi).all() and np.isnan(o.cfl), (o.tc, o.cfl)
        with pytest.raises(AssertionError):
            m.run()
    assert m.tc == o.tc, (m.tc, o.tc)
    assert np.isnan(m.cfl), m.cfl
