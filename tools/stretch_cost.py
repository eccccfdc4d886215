"""Cost of stretch mode inside the step, and of the stretching tables against the download they replace.

    python tools/stretch_cost.py --cost 4096            # the step
    python tools/stretch_cost.py --cost 4096 --ring     # lagrangian.stretching against P.trajectory()

CoupledModel at the given nx with a broadband state: steps/s of nq_step(--steps) without particles, and with 2^16, 2^18 and
2^20 uniformly placed particles attached with stretch=None, with stretch=True and with wave=1.0 and stretch=True, all in one process
and one run.  Each leg runs one warm-up call, then --steps steps timed with perf_counter around a synchronous call, --reps times
over, the legs of one count alternating; the medians are reported, with the ratio of the stretch step to the step without particles
and to the step with stretch=None, and the bytes the mode adds.

The new kernels alone, in the same run: with the particles of a count attached, the library's event pairs (nq_profile_enable, class
"pt_tangent" of niwqg_amd/_lib.py) bracket every launch of the step of stretch mode (k_pt_rk4_t, or k_pt_rk4_wt with the wave) over
--steps further steps; the mean per launch is reported in microseconds.

--ring: --particles (default 2^18) particles record f11, f12, f21, f22 after every step into a ring of --records (default 1024),
filled by stepping; then lagrangian.stretching with 8 groups, after a first call that allocates its tables, --reps times, and
P.trajectory(), the download of the same ring, in the same run.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model(nx):
    import niwqg_amd
    L = 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    m.set_q(q * 1e-5 / q.std())
    m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))
    return m, L, rng


def cost(a):
    from niwqg_amd import particles, _lib
    m, L, rng = model(a.cost)

    def rate():
        m._ctx.step(2)
        m._ctx.sync()
        t0 = time.perf_counter()
        m._ctx.step(a.steps)
        m._ctx.sync()
        return a.steps / (time.perf_counter() - t0)

    def alone():
        """mean microseconds per launch of the step of stretch mode over --steps steps"""
        m._ctx.profile_enable(_lib.Context.STRETCH_KERNEL_CLASSES["pt_tangent"])
        m._ctx.step(a.steps)
        n, ms = m._ctx.profile_read()
        m._ctx.profile_enable(-1)
        return 1e3 * ms / max(n, 1), n
    out = dict(nx=a.cost, steps=a.steps, reps=a.reps)
    for e in [int(v) for v in a.counts.split(",")]:
        n = 1 << e
        x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
        legs = {"none": [], "particles": [], "stretch": [], "wave_stretch": []}
        key = "2^%d" % e
        plain = 0
        for rep in range(a.reps):
            legs["none"].append(rate())
            for leg, kw in (("particles", {}), ("stretch", dict(stretch=True)), ("wave_stretch", dict(wave=1.0, stretch=True))):
                P = particles.attach(m, x, y, **kw)
                b = m._ctx.device_bytes()
                legs[leg].append(rate())
                if leg == "particles":
                    plain = b
                elif leg == "stretch":
                    out["bytes_added_by_stretch_" + key] = b - plain
                if leg != "particles" and rep == a.reps - 1:
                    us, launches = alone()
                    kernel = "k_pt_rk4_t" if leg == "stretch" else "k_pt_rk4_wt"
                    out["us_per_launch_%s_%s" % (kernel, key)] = round(us, 1)
                    out["launches_%s_%s" % (kernel, key)] = launches
                P.detach()
        med = {k: statistics.median(v) for k, v in legs.items()}
        for k, v in med.items():
            out["steps_per_s_%s_%s" % (k, key)] = round(v, 2)
        out["particles_over_none_" + key] = round(med["none"] / med["particles"], 4)
        out["stretch_over_none_" + key] = round(med["none"] / med["stretch"], 4)
        out["stretch_over_particles_" + key] = round(med["particles"] / med["stretch"], 4)
        out["wave_stretch_over_none_" + key] = round(med["none"] / med["wave_stretch"], 4)
    print(json.dumps(out))


def ring(a):
    from niwqg_amd import particles, lagrangian
    m, L, rng = model(a.cost)
    ctx = m._ctx
    n, T = a.particles, a.records
    b0 = ctx.device_bytes()
    P = particles.attach(m, rng.uniform(0, L, n), rng.uniform(0, L, n), record_every=1, capacity=T, record=("f11", "f12", "f21", "f22"),
                         stretch=True)
    t0 = time.perf_counter()
    ctx.step(T - 1)                                          # fill the ring
    ctx.sync()
    out = dict(nx=a.cost, particles=n, records=T, groups=a.groups, reps=a.reps, fill_ms_per_step=(time.perf_counter() - t0) / (T - 1) * 1e3,
               ring_bytes=8 * T * 6 * n, bytes_attached=ctx.device_bytes() - b0)
    groups = rng.integers(0, a.groups, n)
    t0 = time.perf_counter()
    S = lagrangian.stretching(P, groups)
    out["stretching_first_call_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for _ in range(a.reps):
        S = lagrangian.stretching(P, groups)
    out["stretching_ms"] = (time.perf_counter() - t0) / a.reps * 1e3
    out["finite"] = bool(np.all(np.isfinite(S.mean_lnsigma)) and np.all(np.isfinite(S.mean_det)))
    out["ftle_last"] = [float(v) for v in S.ftle()[-1]]
    out["max_abs_mean_det_minus_1"] = float(np.max(np.abs(S.mean_det - 1)))
    t0 = time.perf_counter()
    tr = P.trajectory()
    out["trajectory_download_ms"] = (time.perf_counter() - t0) * 1e3
    out["trajectory_host_bytes"] = int(tr.x.nbytes + tr.y.nbytes + sum(v.nbytes for v in tr.values.values()))
    P.detach()
    out["bytes_after_detach"] = ctx.device_bytes() - b0
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, default=4096, metavar="NX", help="the grid size")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--counts", default="16,18,20", help="log2 of the particle counts")
    ap.add_argument("--ring", action="store_true", help="time lagrangian.stretching against P.trajectory() instead")
    ap.add_argument("--particles", type=int, default=1 << 18)
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--groups", type=int, default=8)
    a = ap.parse_args()
    (ring if a.ring else cost)(a)


if __name__ == "__main__":
    main()
