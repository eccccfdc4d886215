"""The q update beside the wave-PV row kernel (do_step_overlap): the default step of CoupledModel at
4096^2 runs the same kernels in the same order inside each dependency chain as the serial step, so every result is the serial
step's bit for bit.  The switch (NIWQG_AMD_OVERLAP_CUS) is read when the context is created, hence child processes."""
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
nx = 4096
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
for i in range(8):
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


def run_case(tmp_path, case, setting):
    script = tmp_path / "child.py"
    script.write_text(CHILD % {"root": ROOT})
    out = tmp_path / ("%s_%s.npz" % (case, "default" if setting is None else setting))
    env = dict(os.environ)
    env.pop("NIWQG_AMD_OVERLAP_CUS", None)
    if setting is not None:
        env["NIWQG_AMD_OVERLAP_CUS"] = setting
    r = subprocess.run([sys.executable, str(script), case, str(out)], capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
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
