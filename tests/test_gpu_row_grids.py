"""The persistent row kernels on grids that do not divide their rows ("Row grids").

k_x_products<4096>, k_x_wavepv2<4096>, k_x_products_eo<8192> and k_x_wavepv_eo<8192> walk nb row blocks with a grid of g
workgroups in ceil(nb / g) rounds, g from the CU count of the device.  On a 256-CU device every launch of the rest of the suite
has full rounds (4096 / 256, 4096 / 128, 8192 / 256) or one round (slab chunks).  NIWQG_AMD_NUM_CU sizes the grids as if the
device had fewer CUs, so here the last round is partly empty: some workgroups leave the loop a round early, `more` differs
between the workgroups of one launch, and the last block's prefetch is skipped while its neighbour's is not.

The results of the four kernels are per row and hold no per-workgroup partial sums, so the expected answer on every grid is the
default grid's, bit for bit: each case builds twin models from the same inputs, one with the variable unset, and compares with
``np.array_equal``.  Each case first reads nq_row_grid_info -- filled by the arithmetic the launches use -- and asserts that the
second twin has more than one round and a partly empty last one; without that a case could pass without running the path.

The single-rank CoupledModel twin at 4096^2 is built with NIWQG_AMD_OVERLAP_CUS=0 beside the CU count: the default dual-stream
step would size the wave-PV grid from the CUs it leaves (its uneven grids are in tests/test_gpu_overlap_step.py), and with the
serial step BOTH row kernels run the grid of the table.  The default twin keeps the default step; the two steps are bit-identical.

States: a Lamb dipole plus white noise in q, a wave packet plus complex white noise in phi, white noise in c, so the Nyquist
lines, the filter band and the per-row rescale of the (q, q_w) and (q, c) pairs are live.  Two steps; with tdiags = 1 both are
followed by a diagnostics tick (UnCoupledModel: tdiags large, one tick after the first step, the second reads the frozen
gradients).  4096^2 is the smallest grid with a persistent loop, so nothing here is smaller; the 8192^2 case compares the
inversion and the Jacobian exports, which run its two kernels without the cost of a step."""
import contextlib
import ctypes
import os
import time

import numpy as np
import pytest

from test_oracle_golden import L, K0, U0
from test_gpu_at_size import rough_kwargs
from test_gpu_plan_ladder import record_budgets

pytestmark = pytest.mark.gpu

SWITCHES = ("NIWQG_AMD_NUM_CU", "NIWQG_AMD_OVERLAP_CUS", "NIWQG_AMD_SLAB_RESERVE_CUS")
NX = 4096
# CU count -> (rounds, busy workgroups of the last round) of nb = 4096 row blocks
ROUNDS_4096 = {255: (17, 16), 171: (24, 163), 97: (43, 22), 3: (1366, 1)}


@contextlib.contextmanager
def switches(**env):
    """the library reads its switches when a context is created: set exactly `env` of them around a construction"""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def row_grid_info(h):
    """nq_row_grid_info of one context handle: cus, reserve, (grid, nb) of the products and of the wave-PV row kernel"""
    from niwqg_amd import _lib
    out = (ctypes.c_int * 6)()
    assert _lib.lib().nq_row_grid_info(h, out) == 0
    cus, reserve, pg, pnb, wg, wnb = list(out)
    return dict(cus=cus, reserve=reserve, products=(pg, pnb), wavepv=(wg, wnb))


def handles(m):
    sim = getattr(m._ctx, "sim", None)
    return [r.h for r in sim.ranks] if sim is not None else [m._ctx.h]


def rounds_of(grid, nb):
    return -(-nb // grid), nb - (-(-nb // grid) - 1) * grid


def assert_helper_properties(info, nb):
    """what the host test states on nq_overlap_grid, on the launch arithmetic itself: 1 <= grid <= min(nb, cus - reserve) and
    rounds * grid >= nb > (rounds - 1) * grid"""
    for kernel in ("products", "wavepv"):
        grid, blocks = info[kernel]
        assert blocks == nb and 1 <= grid <= min(nb, info["cus"] - info["reserve"]), (kernel, info)
        rounds = -(-nb // grid)
        assert rounds * grid >= nb > (rounds - 1) * grid


def assert_uneven(info, kernels, nb, want_grid=None):
    """the grid the case is about: more than one round, and a last round that is partly empty"""
    assert_helper_properties(info, nb)
    for kernel in kernels:
        grid, blocks = info[kernel]
        assert blocks % grid != 0 and blocks > grid, (kernel, info)
        if want_grid is not None:
            assert grid == want_grid, (kernel, info)


def assert_full_rounds(info, kernels, nb):
    assert_helper_properties(info, nb)
    for kernel in kernels:
        grid, blocks = info[kernel]
        assert blocks % grid == 0, (kernel, info)


# ---- models and states ---------------------------------------------------------------------------------------------------------
def make(kind, nx, **over):
    import bench
    import niwqg_amd
    if kind in ("qg", "qgc"):
        kw = bench.c3_kwargs(nx, "qg")
        kw.update(nu=5.0, mu=1e-8, beta=2e-11, tdiags=1)
        if kind == "qgc":
            kw.update(passive_scalar=True, nu4c=kw["nu4"], nuc=2.0, muc=1e-8)
        cls = niwqg_amd.QGModel
    else:
        kw = rough_kwargs(nx)
        kw.update(tdiags=10 ** 9 if kind == "uncoupled" else 1)
        if kind == "dealias":                               # dual-copy q-hat and the 2/3 mask
            kw.update(use_filter=False, dealias=True)
        cls = {"coupled": niwqg_amd.CoupledModel, "dealias": niwqg_amd.CoupledModel, "uncoupled": niwqg_amd.UnCoupledModel,
               "ybj": niwqg_amd.YBJModel}[kind]
    kw.update(over)
    return cls.Model(**kw)


_STATE = {}


def state(m):
    """(q0, phi0, c0) of the grid of `m`, formed once per size and never written again"""
    from niwqg_amd import InitialConditions as ic
    nx = m.nx
    if nx not in _STATE:
        rng = np.random.default_rng(29 + nx)
        q = ic.LambDipole(m, U=U0, R=2 * np.pi / K0)
        q = q + 0.05 * np.abs(q).max() * rng.standard_normal((nx, nx))
        phi = 0.2 * ic.WavePacket(m, k=3 * K0, l=K0, R=L / 6, x0=L / 3, y0=L / 2)
        phi = phi + 0.01 * (rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx)))
        c = rng.standard_normal((nx, nx))
        for a in (q, phi, c):
            a.setflags(write=False)
        _STATE[nx] = (q, phi, c)
    return _STATE[nx]


def run(m, kind, nsteps=2):
    """the compared results of `nsteps` steps from the common state; nsteps = 0: of the inversion set_phi runs (the wave-PV row
    kernel) and of the two Jacobian exports (the products and the wave-PV row kernel once each).  The context is closed."""
    q0, phi0, c0 = state(m)
    m.set_q(q0)
    if kind in ("qg", "qgc"):
        if kind == "qgc":
            m.set_c(c0)
    else:
        m.set_phi(phi0)
    if nsteps == 0:
        res = dict(ph=np.array(m.ph), jacobian_psi_q=m.jacobian_psi_q(), jacobian_phic_phi=m.jacobian_phic_phi())
        m._ctx.close()
        return res
    log = record_budgets(m)
    for _ in range(nsteps):
        m._step_forward()
    res = dict(qh=np.array(m.qh), budgets=np.array(log, dtype=float), cfl=np.array(m._calc_cfl()))
    if kind == "qgc":
        res["ch"] = np.array(m.ch)
    elif kind != "qg":
        res["phih"] = np.array(m.phih)
    for name, d in m.diagnostics.items():
        if "value" in d:
            res["diag_" + name] = np.array(d["value"], dtype=float)
    m._ctx.close()
    return res


def check_run(res, kind, nsteps=2):
    """the run is one the comparison means something on: finite, moving, budgets and diagnostics present"""
    if nsteps == 0:
        assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in res.values()) and len(res) == 3
        return
    assert np.isfinite(res["qh"]).all() and np.abs(res["qh"]).max() > 0 and np.isfinite(res["cfl"]) and res["cfl"] > 0
    other = {"qg": None, "qgc": "ch"}.get(kind, "phih")
    if other:
        assert np.isfinite(res[other]).all() and np.abs(res[other]).max() > 0
    if kind != "ybj":                                       # (YBJModel's step accumulates no budgets)
        assert res["budgets"].size >= nsteps and np.isfinite(res["budgets"]).all() and np.abs(res["budgets"]).max() > 0
    assert sum(k.startswith("diag_") for k in res) >= 3


def compare(tag, a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        d = np.abs(a[k] - b[k]).max() if a[k].size and a[k].shape == b[k].shape else np.nan
        print("%s %s: max |default - uneven| = %g" % (tag, k, d))
    for k in sorted(a):
        assert np.array_equal(a[k], b[k]), (tag, k)


_DEFAULT = {}


def default_twin(kind, nx, kernels, keep=False, nsteps=2, **over):
    """results of the twin with every switch unset, after asserting that its row grids have full rounds"""
    key = (kind, nx, nsteps, tuple(sorted(over.items())))
    if key in _DEFAULT:
        return _DEFAULT[key]
    with switches():
        m = make(kind, nx, **over)
    for h in handles(m):
        info = row_grid_info(h)
        nb = info["products"][1]
        assert_full_rounds(info, kernels, nb)
    res = run(m, kind, nsteps)
    check_run(res, kind, nsteps)
    if keep:
        _DEFAULT[key] = res
    return res


def twins(tag, kind, nx, cus, kernels, nb, want_grid, nsteps=2, keep=False, env=None, **over):
    t0 = time.time()
    a = default_twin(kind, nx, kernels, keep=keep, nsteps=nsteps, **over)
    t1 = time.time()
    with switches(NIWQG_AMD_NUM_CU=cus, **(env or {})):
        m = make(kind, nx, **over)
    for h in handles(m):
        info = row_grid_info(h)
        assert info["cus"] == cus and info["reserve"] == 0
        assert_uneven(info, kernels, nb, want_grid)
    b = run(m, kind, nsteps)
    compare(tag, a, b)
    print("%s: wall time %.1f s (default twin and the state %.1f s)" % (tag, time.time() - t0, t1 - t0))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", sorted(ROUNDS_4096, reverse=True))
def test_coupled_4096_on_uneven_grids_equals_the_default_grid(cus):
    """k_x_products<4096, MODE_COUPLED> and k_x_wavepv2<4096>"""
    assert rounds_of(cus, NX) == ROUNDS_4096[cus]
    twins("coupled 4096 cus=%d" % cus, "coupled", NX, cus, ("products", "wavepv"), NX, cus, keep=True, env=dict(NIWQG_AMD_OVERLAP_CUS=0))


@pytest.mark.parametrize("kind, cus", [("uncoupled", 171), ("ybj", 97), ("qg", 255), ("qgc", 3)])
def test_other_product_modes_4096_on_uneven_grids_equal_the_default_grid(kind, cus):
    """MODE_UNCOUPLED (tdiags large: the second step reads the frozen gradients), YBJModel, MODE_QG and MODE_QGC"""
    assert rounds_of(cus, NX) == ROUNDS_4096[cus]
    twins("%s 4096 cus=%d" % (kind, cus), kind, NX, cus, ("products",), NX, cus)


def test_coupled_4096_dealias_on_an_uneven_grid_equals_the_default_grid():
    """dual-copy q-hat and the 2/3 mask (no dual-stream step on these contexts)"""
    twins("coupled 4096 dealias cus=97", "dealias", NX, 97, ("products", "wavepv"), NX, 97)


@pytest.mark.parametrize("kind", ["coupled", "qgc"])
def test_slab_ranks_4096_on_an_uneven_grid_equal_the_same_partition_on_the_default_grid(kind):
    """SLAB = true: two peer ranks, one chunk, nb = 2048 row blocks per rank on 171 workgroups (12 rounds, 167 in the last)
    against the same partition with the variable unset (256 workgroups, 8 full rounds)"""
    assert rounds_of(171, 2048) == (12, 167)
    twins("%s 4096 slab=2 cus=171" % kind, kind, NX, 171, ("products", "wavepv") if kind == "coupled" else ("products",), 2048, 171,
          slab=2, nchunks=1)


def test_coupled_8192_on_an_uneven_grid_equals_the_default_grid():
    """k_x_products_eo<8192> and k_x_wavepv_eo<8192>: 8192 rows on 171 workgroups, 48 rounds, 155 in the last.  The one slow case
    of this module: with one tick-free step it took 28.8 s on an MI355X, above the 25 s of the slowest 8192^2 case the suite had, so
    it compares the inversion and the Jacobian exports instead, which run the same two kernels (wave-PV twice, products once)."""
    assert rounds_of(171, 8192) == (48, 155)
    try:
        twins("coupled 8192 cus=171", "coupled", 8192, 171, ("products", "wavepv"), 8192, 171, nsteps=0)
    finally:
        _STATE.pop(8192, None)                              # 2.7 GB of host arrays no other case reads


def test_reserved_cus_shrink_the_grids_of_a_slab_rank():
    """NIWQG_AMD_SLAB_RESERVE_CUS on the null link (rank 0 of 8, nb = 512 row blocks; no step is taken): 37 CUs less in both
    grids; -1 and the device's own count are ignored, as nq_slab_set_null_link says"""
    from niwqg_amd import _lib, slab
    with switches():
        m = make("coupled", 64)                             # the device's CU count
        cus = row_grid_info(m._ctx.h)["cus"]
        m._ctx.close()
    dk = 2 * np.pi / L
    kk = dk * np.append(np.arange(0., NX // 2), np.arange(-NX // 2, 0.))
    kw = rough_kwargs(NX)

    def rank_info(setting):
        with switches(**({} if setting is None else {"NIWQG_AMD_SLAB_RESERVE_CUS": setting})):
            ranks = slab.make_ranks(_lib.COUPLED, NX, kk, kk, np.ones((NX, NX)), kw["dt"], 8, only_rank=0, nu4=kw["nu4"], nu4w=kw["nu4w"])
            sim = slab.SlabSimulation(ranks, "null", nchunks=1)
            info = row_grid_info(ranks[0].h)
            ranks[0].close()
            return info
    base = rank_info(None)
    assert cus > 37 + 1 and base == dict(cus=cus, reserve=0, products=(min(cus, 512), 512), wavepv=(min(cus, 512), 512))
    for setting in ("-1", str(cus)):
        assert rank_info(setting) == base, setting
    less = rank_info("37")
    assert less == dict(cus=cus, reserve=37, products=(cus - 37, 512), wavepv=(cus - 37, 512))
    assert_helper_properties(less, 512)


@pytest.mark.parametrize("setting", ["0", "-3", "100000", "abc"])
def test_cu_counts_outside_the_device_are_refused(setting):
    with switches(NIWQG_AMD_NUM_CU=setting):
        with pytest.raises(RuntimeError, match=r"NIWQG_AMD_NUM_CU=%s: an integer in 1\.\." % setting):
            make("coupled", 64)
    with switches():
        m = make("coupled", 64)                             # and the refusal left nothing behind
        info = row_grid_info(m._ctx.h)
        assert info["cus"] >= 1 and info["products"][0] == info["products"][1]
        m._ctx.close()
