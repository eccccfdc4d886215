"""k_s_phi forms the phi-hat results of ETDRK4 stages 0 and 1 again where a later stage needs them instead of storing them and
reading them back (phi_stage_update).  NIWQG_AMD_PHI_STAGE_STORE=1 keeps the stored data flow; both do the
same arithmetic through one helper, so every result is equal bit for bit, and the default context is smaller by the plane that
held the stage-0 result.  The switch is read when a context is created."""
import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

SWITCH = "NIWQG_AMD_PHI_STAGE_STORE"
STEPS = 3
#        id                 class            bench workload  nx    extra keywords        ranks
CASES = [("coupled128", "CoupledModel", "coupled", 128, {}, 0),                    # single-pass columns, S2 = 1
         ("coupled1024", "CoupledModel", "coupled", 1024, {}, 0),                  # smallest two-pass plan: mirrored rows, pair_order
         ("coupled1024_dealias", "CoupledModel", "coupled", 1024, {"dealias": True}, 0),     # cmirror off: full coefficient planes
         ("uncoupled1024", "UnCoupledModel", "uncoupled", 1024, {}, 0),
         ("ybj1024", "YBJModel", "uncoupled", 1024, {}, 0),                        # no budgets in the step
         ("coupled1024_slab2", "CoupledModel", "coupled", 1024, {}, 2)]

_fields = {}


def initial_fields(workload, nx, grid):
    """bench.py's LambDipole q and uniform phi, formed once per grid"""
    if nx not in _fields:
        _fields[nx] = bench.initial_fields(workload, nx, grid)
    return _fields[nx]


def device_bytes(ctx):
    if hasattr(ctx, "sim"):
        return sum(int(r.L.nq_device_bytes(r.h)) for r in ctx.sim.ranks)
    return ctx.device_bytes()


def run(monkeypatch, store, cls, workload, nx, extra, ranks):
    import niwqg_amd
    from niwqg_amd import _lib
    if store:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    kw = bench.c3_kwargs(nx, workload)
    kw.update(extra)
    m = getattr(niwqg_amd, cls).Model(device=0, slab=ranks if ranks else False, **kw)
    q, phi = initial_fields(workload, nx, m)
    m.set_q(q)
    m.set_phi(phi)
    ctx = m._ctx
    if ctx.budgets_enabled:
        ctx.take_budget_increments()
    ctx.step(STEPS)
    out = {"phih": np.array(ctx.field(_lib.F_PHIH)), "qh": np.array(ctx.field(_lib.F_QH)),
           "phih_stage4": np.array(ctx.field(_lib.F_PHIH_STAGE4))}
    if ctx.budgets_enabled:
        out["budget_increments"] = np.array(ctx.take_budget_increments())
    return out, device_bytes(ctx)


@pytest.mark.parametrize("cls,workload,nx,extra,ranks", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_recomputed_stage_results_equal_the_stored_ones_bit_for_bit(monkeypatch, cls, workload, nx, extra, ranks):
    a, bytes_default = run(monkeypatch, False, cls, workload, nx, extra, ranks)
    b, bytes_stored = run(monkeypatch, True, cls, workload, nx, extra, ranks)
    assert sorted(a) == sorted(b) and ("budget_increments" in a) == (cls != "YBJModel")
    for k in sorted(a):
        print(cls, nx, k, "max |default - stored| =", np.abs(a[k] - b[k]).max(), " max |default| =", np.abs(a[k]).max())
    for k in sorted(a):
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0, k
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["phih"], a["phih_stage4"])          # the stage-2 result, not the new state
    # the plane that held the stage-0 result is not there: one full complex plane (over all ranks of a slab model)
    assert bytes_stored - bytes_default == 16 * nx * nx, (bytes_stored, bytes_default)
