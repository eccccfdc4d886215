"""The q update beside the wave-PV row kernel (do_step_overlap): the default step of CoupledModel at
4096^2 runs the same kernels in the same order inside each dependency chain as the serial step, so every result is the serial
step's bit for bit.  The switch (NIWQG_AMD_OVERLAP_CUS) is read when the context is created, hence child processes.

Other splits than the default leave the wave-PV kernel a grid that does not divide its 4096 row blocks (a partly empty last round,
tests/test_gpu_row_grids.py) and move the two branches against each other in time: a dependency missing between the streams would
not show at the even split.  At 8192^2 the variable opens the second stream as well; the default there is the serial step."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import ctypes
import bench
import niwqg_amd
case, out = sys.argv[1], sys.argv[2]
nx, nsteps = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 3 else (4096, 8)
kw = bench.c3_kwargs(nx, "coupled")                     # LambDipole, filter on; budgets are on by default
kw.update(twrite=4, tdiags=3 if case == "ticks" else 10 ** 9)   # status lines after steps 4 and 8: m.cfl from the 4th stage's u, v
m = niwqg_amd.CoupledModel.Model(device=0, slab=False, **kw)
q, phi = bench.initial_fields("coupled", nx, m)
m.set_q(q)
m.set_phi(phi)
info = (ctypes.c_int * 3)()
assert m._ctx.L.nq_overlap_info(m._ctx.h, info) == 0
res = {"info": np.array(list(info))}
P = None
if case == "particles":
    from niwqg_amd import particles
    rng = np.random.default_rng(5)
    P = particles.attach(m, rng.uniform(0, m.L, 1000), rng.uniform(0, m.L, 1000))
F = R = A = None
if case == "attachments":                               # the forcing tail, the recorder and the averages, in their hook order
    from niwqg_amd import forcing, frequency, averages
    F = forcing.attach(m, q=forcing.ring(m, 16 * m.dk, 2 * m.dk, 8e-11), phi=forcing.ring(m, 12 * m.dk, 2 * m.dk, 1e-9, field="phi"), seed=17)
    R = frequency.attach(m, 8, every=2, length=3)
    A = averages.attach(m, ("q_psi", "phi2"), (("q_psi", "phi2"),), every=2)
# the increments themselves: m.Ke, m.Pw, m.Kw start from set_q / set_phi's atomic device sums, whose last bits differ between
# any two runs
bud, cfl = [], []
take = m._ctx.take_budget_increments
def recording():
    d = take()
    bud.append(d)
    return d
m._ctx.take_budget_increments = recording
for i in range(nsteps):
    m._step_forward()
    cfl.append(m.__dict__.get("cfl", -1.0))
res.update(qh=np.array(m.qh), phih=np.array(m.phih), budgets=np.array(bud), cfl=np.array(cfl), cfl_now=np.array(m._calc_cfl()))
if P is not None:
    x, y = P.positions()
    res.update(px=np.array(x), py=np.array(y))
if F is not None:
    w = F.work()
    res.update(work=np.array([w["q"], w["phi"]]), forcing_step=np.array(F.state()["step"]))
    for n in R.fields:
        ts = R.series(n)
        res["series_" + n], res["series_step_" + n] = ts.values, ts.step
    S = A.result()
    res.update(avg_n=np.array(S.n), **{"avg_" + k.replace("*", "_"): v for k, v in S.sums.items() if k != "phi2*q_psi"})
np.savez(out, **res)
"""


def run_case(tmp_path, case, setting, size=()):
    script = tmp_path / "child.py"
    script.write_text(CHILD % {"root": ROOT})
    out = tmp_path / ("%s_%s.npz" % (case, "default" if setting is None else setting))
    env = dict(os.environ)
    env.pop("NIWQG_AMD_OVERLAP_CUS", None)
    env.pop("NIWQG_AMD_NUM_CU", None)
    if setting is not None:
        env["NIWQG_AMD_OVERLAP_CUS"] = setting
    r = subprocess.run([sys.executable, str(script), case, str(out)] + [str(v) for v in size], capture_output=True, text=True, timeout=900, env=env,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(str(out))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "particles", "ticks", "attachments"])
def test_default_step_equals_the_serial_step_bit_for_bit(tmp_path, case):
    a = run_case(tmp_path, case, None)
    b = run_case(tmp_path, case, "0")
    from niwqg_amd import _lib
    want = _lib.lib().nq_overlap_default_cus(4096)
    if want > 0:                                         # the default IS the dual-stream step, the other run is not
        assert a["info"][0] >= want and a["info"][1] == a["info"][2] - a["info"][0], a["info"]
    assert list(b["info"]) == [0, 0, 0]
    assert a["budgets"].shape == (8, 3) and np.isfinite(a["budgets"]).all() and np.abs(a["budgets"]).max() > 0 and np.abs(a["qh"]).max() > 0 and (a["cfl"][[3, 7]] > 0).all()
    names = ["qh", "phih", "budgets", "cfl", "cfl_now"] + (["px", "py"] if case == "particles" else [])
    if case == "attachments":
        # the forcing writes the q-hat the second stream has just produced and re-inverts; the recorder (records 4, 6, 8 after the
        # wrap) and the averages (four samples) read what that leaves
        assert np.all(a["work"] != 0) and a["forcing_step"] == 8 and a["avg_n"] == 4
        assert np.array_equal(a["series_step_phi"], [4, 6, 8]) and np.abs(a["series_q"]).max() > 0 and np.abs(a["avg_q_psi_phi2"]).max() > 0
        names += ["work", "forcing_step"] + sorted(k for k in a.files if k.startswith(("series_", "avg_")))
    for k in names:
        print(case, k, "max |default - serial| =", np.abs(a[k] - b[k]).max())
    for k in names:
        assert np.array_equal(a[k], b[k]), k


_SERIAL = {}


def serial_run(tmp_path, case):
    """the serial run of a case, made once for all splits and only read afterwards"""
    if case not in _SERIAL:
        with run_case(tmp_path, case, "0") as z:
            _SERIAL[case] = {k: z[k] for k in z.files}
        for v in _SERIAL[case].values():
            v.setflags(write=False)
    return _SERIAL[case]


@pytest.mark.gpu
@pytest.mark.parametrize("setting, grid", [("85", 171), ("96", 158), ("1", 241)])
@pytest.mark.parametrize("case", ["plain", "attachments"])
def test_other_splits_equal_the_serial_step_bit_for_bit(tmp_path, case, setting, grid):
    """NIWQG_AMD_OVERLAP_CUS = 85: wave-PV grid 171 (24 rounds, 163 workgroups in the last); 96: 160, which nq_overlap_grid snaps to
    158 (26 rounds, 146 in the last); 1: 255, snapped to 241, the smallest grid of 17 rounds (240 in the last; the q branch is left 15
    CUs, the fewest any setting gives it, and its join comes late)"""
    a = run_case(tmp_path, case, setting)
    b = serial_run(tmp_path, case)
    ncu = int(a["info"][2])
    assert ncu == 256 and list(a["info"]) == [ncu - grid, grid, ncu], a["info"]           # the second stream, and the grid of the table
    assert 4096 % grid != 0 and 4096 > grid
    assert list(b["info"]) == [0, 0, 0]
    assert a["budgets"].shape == (8, 3) and np.isfinite(a["budgets"]).all() and np.abs(a["budgets"]).max() > 0 and np.abs(a["qh"]).max() > 0 and (a["cfl"][[3, 7]] > 0).all()
    names = ["qh", "phih", "budgets", "cfl", "cfl_now"]
    if case == "attachments":
        assert np.all(a["work"] != 0) and a["forcing_step"] == 8 and a["avg_n"] == 4
        assert np.array_equal(a["series_step_phi"], [4, 6, 8]) and np.abs(a["series_q"]).max() > 0 and np.abs(a["avg_q_psi_phi2"]).max() > 0
        names += ["work", "forcing_step"] + sorted(k for k in a.files if k.startswith(("series_", "avg_")))
    for k in names:
        print(case, setting, k, "max |split - serial| =", np.abs(a[k] - b[k]).max())
    for k in names:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_dual_stream_step_at_8192_equals_the_serial_step_bit_for_bit(tmp_path):
    """8192^2: nq_create opens the second stream when the variable is set, and k_x_wavepv_eo runs on nq_overlap_grid(8192, 256 - 128)
    = 128 workgroups beside the q update.  do_step_overlap issues the same launches as at 4096^2 (nothing in it or in the column
    sub-passes it moves depends on the size), so two steps equal the serial 8192^2 run bit for bit."""
    a = run_case(tmp_path, "plain", "128", size=(8192, 2))
    b = run_case(tmp_path, "plain", "0", size=(8192, 2))
    ncu = int(a["info"][2])
    assert ncu > 128 and a["info"][1] > 0 and a["info"][0] == ncu - a["info"][1] and a["info"][0] >= 128, a["info"]
    assert list(b["info"]) == [0, 0, 0]
    assert a["phih"].shape == (8192, 8192) and a["budgets"].shape == (2, 3) and np.isfinite(a["budgets"]).all() and np.abs(a["budgets"]).max() > 0
    assert np.abs(a["qh"]).max() > 0 and a["cfl_now"] > 0
    names = ["qh", "phih", "budgets", "cfl", "cfl_now"]
    for k in names:
        print("8192", k, "max |dual-stream - serial| =", np.abs(a[k] - b[k]).max())
    for k in names:
        assert np.array_equal(a[k], b[k]), k


def test_row_grids_of_the_default_device_have_full_rounds():
    """The grids of the persistent row kernels come from the CU count (the launches: row_grid in csrc/nq_lib.hip, min(nb, CUs - reserved);
    the dual-stream step: nq_overlap_grid of what it leaves the wave-PV kernel).  For nb in {2048, 4096, 8192} row blocks, every CU
    count 1 ... 256 and 0 or 37 reserved CUs, nq_overlap_grid stays inside the clamp the launches apply and is a grid of
    ceil(nb / CUs) rounds; with the defaults (256 CUs, none reserved, 128 left to the q branch at 4096) every launch has full rounds --
    which is why the uneven last round needs tests of its own (tests/test_gpu_row_grids.py).  The launch arithmetic itself is
    reachable through a context only (nq_row_grid_info): the GPU module asserts the same properties on every context it builds."""
    from niwqg_amd import _lib
    L = _lib.lib()
    import ctypes
    assert L.nq_row_grid_info(None, (ctypes.c_int * 6)()) < 0          # no context, no grids: an error code
    uneven = 0
    for nb in (2048, 4096, 8192):
        for cus in range(1, 257):
            for reserve in (0, 37):
                n = cus - reserve
                if n < 1:
                    assert L.nq_overlap_grid(nb, n) == 0
                    continue
                g = L.nq_overlap_grid(nb, n)
                assert 1 <= g <= min(nb, n), (nb, cus, reserve, g)
                rounds = -(-nb // g)
                assert rounds * g >= nb > (rounds - 1) * g
                assert rounds == -(-nb // min(nb, n))                 # no more rounds than the launches' own clamp min(nb, n) needs
                uneven += nb % min(nb, n) != 0
        assert nb % 256 == 0 and L.nq_overlap_grid(nb, 256) == 256
    assert uneven > 1000                                             # ... and almost every other count has a partly empty last round
    d = L.nq_overlap_default_cus(4096)
    assert d == 0 or 4096 % L.nq_overlap_grid(4096, 256 - d) == 0
    assert L.nq_overlap_default_cus(8192) == 0 and L.nq_overlap_default_cus(2048) == 0


def test_wavepv_grid_wastes_at_most_half_a_percent_of_its_last_round():
    """A persistent grid of g workgroups walks the 4096 row blocks in ceil(4096 / g) rounds; rounds * g / 4096 - 1 of the kernel
    is the idle part of the last one.  The grid the default split gives wastes <= 0.5 %, nq_overlap_grid never needs more rounds
    than the CUs it was offered, never more CUs, and is the smallest such grid."""
    from niwqg_amd import _lib
    L = _lib.lib()
    nb, ncu = 4096, 256
    waste = {g: -(-nb // g) * g / nb - 1.0 for g in range(128, 241)}
    for cus in range(128, 241):
        g = L.nq_overlap_grid(nb, cus)
        assert 1 <= g <= cus and -(-nb // g) == -(-nb // cus)
        assert g == 1 or -(-nb // (g - 1)) > -(-nb // g)
        assert waste.get(g, 0.0) <= waste[cus] + 1e-15
    d = L.nq_overlap_default_cus(4096)
    assert 0 <= d < ncu
    if d:
        g = L.nq_overlap_grid(nb, ncu - d)
        assert waste[g] <= 0.005, (g, waste[g])
        assert g == min((h for h in waste if abs(h - g) <= 4), key=lambda h: (waste[h], h))     # the least waste near the target
    assert L.nq_overlap_grid(nb, 160) == 158 and L.nq_overlap_grid(nb, 171) == 171 and L.nq_overlap_grid(nb, 4096) == 4096
    assert L.nq_overlap_default_cus(2048) == 0 and L.nq_overlap_default_cus(8192) == 0
