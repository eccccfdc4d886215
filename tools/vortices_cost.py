"""Cost of the vortex census.

    python tools/vortices_cost.py --cost 4096        # ms per call and per phase, one JSON line

--cost: CoupledModel at nx, advanced --steps steps so that the Okubo-Weiss field has structure, from --state bench (the default:
bench.py's configuration and initial fields, the Lamb dipole under a uniform wave) or --state broadband (band-limited random q:
many eddies, hundreds of times the components); the census of (ow, q_psi, phi2) at OW < -0.2 sigma.  The calls alternate --reps
times (at least five) in one run, each timed with device events after a warm-up call: the census without any download at both
connectivities, nq_vortex_profile (the same census with events between its phases: the store pass, range, rows, merge, flatten +
rank, sums), the range pass alone and a field_pdfs counting pass on the same names; on the host clock, downloads included, what
the Python calls cost (units="abs", "sigma", and with the label plane) and what a user does without the census: three planes to
the host and scipy.ndimage.label on one core (if scipy is there; the seams are not even united).  Medians, with every repetition
listed; the component count and set fraction the numbers belong to; the bytes each phase must move and the fraction of the 6.29 TB/s
copy rate that follows from its median."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

NAMES = ("ow", "q_psi", "phi2")
PHASES = ("store", "range", "rows", "merge", "flatten_rank", "sums")
COPY_RATE = 6.29e12


def model(nx, state="broadband"):
    import niwqg_amd
    if state == "bench":
        import bench
        return bench.build_model("coupled", nx, 0)
    L = 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    n = np.fft.fftfreq(nx, 1.0 / nx)
    kap = np.hypot(n[None, :nx // 2 + 1], n[:, None])
    w = kap * np.exp(-(kap / 24.0) ** 2)                       # eddies of a few hundredths of the domain
    q = np.fft.irfft2((rng.standard_normal(w.shape) + 1j * rng.standard_normal(w.shape)) * w, s=(nx, nx))
    m.set_q(q * (0.1 * k0) / q.std())
    m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))
    return m


def cost(nx, reps, steps, state):
    from niwqg_amd import _lib, averages, pdfs, vortices
    m = model(nx, state)
    c = m._ctx
    c.step(steps)
    m._after_steps()
    C = vortices.census(m, capacity=vortices.MAX_CAPACITY)
    codes = np.ascontiguousarray([vortices._CODES[n] for n in NAMES], np.int32)
    h = pdfs.field_pdfs(m, names=NAMES)
    ranges = {n: (h.edges[n][0], h.edges[n][-1]) for n in NAMES}
    cap = vortices.MAX_CAPACITY
    four = np.empty((3, 4))

    def census(conn):
        c._chk(c.L.nq_vortex_census(c.h, 3, _lib._iptr(codes), 0, _lib.VX_BELOW, C.threshold, conn, cap), "nq_vortex_census")
    calls = {"census_4_ms": lambda: census(4), "census_8_ms": lambda: census(8),
             "range_call_with_download_ms": lambda: c._chk(c.L.nq_vortex_range(c.h, 3, _lib._iptr(codes), _lib._dptr(four)), "nq_vortex_range"),
             "pdf_same_names_ms": lambda: pdfs._Fused(m).bin(list(NAMES), ranges, 256, None, 0, False)}

    def timed(f):
        f()
        c.timer_start()
        f()
        return c.timer_stop()

    def wall(f):
        f()
        c.sync()
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3
    user = {"python_census_abs_wall_ms": lambda: vortices.census(m, "ow", C.threshold, units="abs", sums=NAMES[1:]),
            "python_census_sigma_wall_ms": lambda: vortices.census(m),
            "python_census_sigma_labels_wall_ms": lambda: vortices.census(m, labels=True)}
    runs = {k: [] for k in list(calls) + list(user)}
    phases = {4: [], 8: []}
    ms = np.zeros(6)
    for _ in range(reps):
        for k, f in calls.items():
            runs[k].append(timed(f))
        for k, f in user.items():
            runs[k].append(wall(f))
        for conn in (4, 8):
            c._chk(c.L.nq_vortex_profile(c.h, 3, _lib._iptr(codes), 0, _lib.VX_BELOW, C.threshold, conn, cap, _lib._dptr(ms)), "nq_vortex_profile")
            phases[conn].append(ms.copy())
    C8 = vortices.census(m, connectivity=8, capacity=cap)
    out = dict(nx=nx, state=state, reps=reps, steps=steps, names=list(NAMES), threshold=C.threshold, set_fraction=round(C.points_in_set / float(nx * nx), 4),
               components_4=C.total, components_8=C8.total, capacity=cap, largest_area_4=int(C.area.max()), largest_area_8=int(C8.area.max()))
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_all"] = [round(x, 4) for x in v]
    plane, labels = nx * nx * 8.0, nx * nx * 4.0
    must = dict(store=3 * plane, range=3 * plane, rows=plane + labels, merge=labels, flatten_rank=2 * labels, sums=3 * plane + labels)
    for conn in (4, 8):
        med = np.median(np.array(phases[conn]), axis=0)
        for i, p in enumerate(PHASES):
            out["phase_%s_%d_ms" % (p, conn)] = round(float(med[i]), 4)
            out["phase_%s_%d_fraction_of_copy_rate" % (p, conn)] = round(must[p] / (med[i] * 1e-3) / COPY_RATE, 3) if med[i] > 0 else None
        out["phases_%d_all" % conn] = [[round(float(x), 4) for x in r] for r in phases[conn]]
    out["bytes_each_phase_must_move"] = must
    # the route without the census: three planes to the host, one core labels them
    t0 = time.perf_counter()
    A = averages.attach(m, NAMES, every=0)
    A.sample()
    R = A.result()
    host = {n: R.mean(n) for n in NAMES}
    A.detach()
    out["host_route_three_planes_s"] = round(time.perf_counter() - t0, 3)
    try:
        from scipy import ndimage
        t0 = time.perf_counter()
        _, n = ndimage.label(host["ow"] < C.threshold)
        out["host_route_scipy_label_s"] = round(time.perf_counter() - t0, 3)
        out["host_route_scipy_components_seams_not_united"] = int(n)
    except ImportError:
        out["host_route_scipy_label_s"] = None
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, metavar="NX", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--state", choices=("bench", "broadband"), default="bench")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5 (medians of fewer repetitions are not reported)")
    cost(a.cost, a.reps, a.steps, a.state)


if __name__ == "__main__":
    main()
