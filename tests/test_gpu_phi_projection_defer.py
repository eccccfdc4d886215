"""The Parseval sums of ETDRK4 stage 1 against the phi tendency (SG, SX: gamma1 + gamma2 and xi1 + xi2 of the budgets) are formed
by the stage-2 launch of k_s_phi, which holds both operands anyway, and land in slots 4, 5 of the stage-1 partial record; stage 1
no longer reads N1.  NIWQG_AMD_PHI_STAGE_STORE=1 keeps the flow in which every stage forms its own sums from
the stored stage results: same expressions, same tiles, same order of summation, so the state AND the budget increments are equal
bit for bit.  The increments are where a misplaced slot or another order of summation would show.

Every wave damping term is on (nu4w, nuw, muw): with muw != 0 the element [0,0] contributes to SX, and there the projection takes
the tendency as its transform gave it, not the stored N2 (which has the Jacobian's domain sum added back).

The switches are read when a context is created.  The dual-stream step exists at 4096^2 and 8192^2 only: at 1024^2 both settings
of NIWQG_AMD_OVERLAP_CUS give the serial step, so the case at 4096^2 is the one that runs the q branch on the second stream."""
import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

SWITCH = "NIWQG_AMD_PHI_STAGE_STORE"
OVERLAP = "NIWQG_AMD_OVERLAP_CUS"
STEPS = 3
#        id                      class             bench workload  nx    extra keywords    ranks  steps
CASES = [("coupled256", "CoupledModel", "coupled", 256, {}, 0, STEPS),                      # single-pass columns, S2 = 1
         ("coupled1024", "CoupledModel", "coupled", 1024, {}, 0, STEPS),                    # smallest two-pass plan: pair_order, mirrored rows
         # the 2/3 mask is not mirror-symmetric in l: full coefficient planes, no crow mirroring, both copies of q-hat.  The mask
         # is taken only without the exponential filter (Kernel._initialize_filter), hence use_filter=False
         ("coupled1024_dealias", "CoupledModel", "coupled", 1024, {"use_filter": False, "dealias": True}, 0, STEPS),
         ("uncoupled512", "UnCoupledModel", "uncoupled", 512, {}, 0, STEPS),
         ("ybj512", "YBJModel", "uncoupled", 512, {}, 0, STEPS),                            # budgets off: nothing touches the partials
         ("coupled1024_slab2", "CoupledModel", "coupled", 1024, {}, 2, STEPS)]

_fields = {}
_runs = {}


def initial_fields(workload, nx, grid):
    """bench.py's LambDipole q and uniform phi, formed once per grid"""
    if nx not in _fields:
        _fields[nx] = bench.initial_fields(workload, nx, grid)
    return _fields[nx]


def run(monkeypatch, store, cls, workload, nx, extra, ranks, steps, overlap=None, takes=1):
    """the state after `steps` steps and the budget increments of `takes` consecutive runs of `steps` steps; made once per
    setting and only read afterwards"""
    key = (store, cls, nx, tuple(sorted(extra.items())), ranks, steps, overlap, takes)
    if key in _runs:
        return _runs[key]
    import niwqg_amd
    from niwqg_amd import _lib
    if store:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    if overlap is None:
        monkeypatch.delenv(OVERLAP, raising=False)
    else:
        monkeypatch.setenv(OVERLAP, overlap)
    kw = bench.c3_kwargs(nx, workload)
    kw.update(nu4w=3e9 * (128.0 / nx) ** 4, muw=1e-7)
    kw.update(extra)
    m = getattr(niwqg_amd, cls).Model(device=0, slab=ranks if ranks else False, **kw)
    q, phi = initial_fields(workload, nx, m)
    m.set_q(q)
    m.set_phi(phi)
    ctx = m._ctx
    if not ranks:
        # the mask case must really run the full, un-mirrored planes (the context keeps both copies of q-hat exactly then)
        assert bool(ctx.dual_q) == bool(kw.get("dealias") and not kw["use_filter"]), (ctx.dual_q, kw)
    if ctx.budgets_enabled:
        ctx.take_budget_increments()
    bud = []
    for _ in range(takes):
        ctx.step(steps)
        if ctx.budgets_enabled:
            bud.append(ctx.take_budget_increments())
    out = {"phih": np.array(ctx.field(_lib.F_PHIH)), "qh": np.array(ctx.field(_lib.F_QH)),
           "phih_stage4": np.array(ctx.field(_lib.F_PHIH_STAGE4))}
    if ctx.budgets_enabled:
        out["budget_increments"] = np.array(bud)
    if not ranks and not store:
        info = np.zeros(3, np.int32)
        assert ctx.L.nq_overlap_info(ctx.h, _lib._iptr(info)) == 0
        out["overlap_cus"] = info[:1].copy()
    for v in out.values():
        v.setflags(write=False)
    _runs[key] = out
    return out


def compare(a, b, cls, what):
    names = sorted(k for k in a if k != "overlap_cus")
    assert names == sorted(k for k in b if k != "overlap_cus") and ("budget_increments" in a) == (cls != "YBJModel")
    for k in names:
        print(what, k, "max |default - stored| =", np.abs(a[k] - b[k]).max(), " max |default| =", np.abs(a[k]).max())
    for k in names:
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0, k
        assert np.array_equal(a[k], b[k]), k
    if "budget_increments" in a:
        assert np.all(a["budget_increments"] != 0), a["budget_increments"]      # Ke, Pw, Kw: each has moved in every take


@pytest.mark.parametrize("cls,workload,nx,extra,ranks,steps", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_deferred_stage1_projection_equals_the_stored_flow_bit_for_bit(monkeypatch, cls, workload, nx, extra, ranks, steps):
    a = run(monkeypatch, False, cls, workload, nx, extra, ranks, steps)
    b = run(monkeypatch, True, cls, workload, nx, extra, ranks, steps)
    compare(a, b, cls, "%s %d" % (cls, nx))
    assert not np.array_equal(a["phih"], a["phih_stage4"])          # the stage-2 result, not the new state


def test_serial_step_against_the_overlapped_step_1024(monkeypatch):
    """the partials do not depend on which stream ran the q branch (at this size both settings resolve to the serial step: see
    the module text and the case at 4096^2 below)"""
    a = run(monkeypatch, False, "CoupledModel", "coupled", 1024, {}, 0, STEPS)
    s = run(monkeypatch, False, "CoupledModel", "coupled", 1024, {}, 0, STEPS, overlap="0")
    b = run(monkeypatch, True, "CoupledModel", "coupled", 1024, {}, 0, STEPS, overlap="0")
    compare(a, s, "CoupledModel", "1024 default step / serial step")
    compare(a, b, "CoupledModel", "1024 default step / serial step, stored flow")


def test_serial_step_against_the_overlapped_step_4096(monkeypatch):
    """the default step at 4096^2 runs the q update on a second stream beside the wave-PV row kernel; the deferred projection and
    the serial step with the stored flow give the same bits"""
    from niwqg_amd import _lib
    a = run(monkeypatch, False, "CoupledModel", "coupled", 4096, {}, 0, 1)
    b = run(monkeypatch, True, "CoupledModel", "coupled", 4096, {}, 0, 1, overlap="0")
    if _lib.lib().nq_overlap_default_cus(4096) > 0:
        assert a["overlap_cus"][0] > 0, a["overlap_cus"]
    compare(a, b, "CoupledModel", "4096 overlapped / serial stored")


def test_stage1_slots_are_complete_at_every_step_boundary(monkeypatch):
    """one step, take the increments, one more, take them again: each take and their sum equal the stored flow's"""
    a = run(monkeypatch, False, "CoupledModel", "coupled", 1024, {}, 0, 1, takes=2)
    b = run(monkeypatch, True, "CoupledModel", "coupled", 1024, {}, 0, 1, takes=2)
    assert a["budget_increments"].shape == (2, 3)
    compare(a, b, "CoupledModel", "1024 two takes")
    assert np.array_equal(a["budget_increments"].sum(axis=0), b["budget_increments"].sum(axis=0))
    # and the two steps together are the first two of the three-step runs: nothing of step 1 was left for step 2 to finish
    c = run(monkeypatch, False, "CoupledModel", "coupled", 1024, {}, 0, 2)
    assert np.array_equal(a["phih"], c["phih"]) and np.array_equal(a["qh"], c["qh"])
