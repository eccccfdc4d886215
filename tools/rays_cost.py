"""Cost of ray mode inside the step.

    python tools/rays_cost.py --cost 4096

CoupledModel at the given nx with a broadband state: steps/s of nq_step(--steps) without particles, and with 2^16, 2^18 and
2^20 uniformly placed particles attached with rays=None and with rays=(k0, l0), all in one process and one run.  Each leg runs one
warm-up call, then --steps steps timed with perf_counter around a synchronous call, --reps times over, the legs of one count
alternating; the medians are reported, with the ratio of the ray step to both other legs and the bytes the mode adds.

Each new kernel alone, in the same run: with the rays of a count attached, the library's event pairs (nq_profile_enable, classes
"pt_zeta" and "pt_rays" of niwqg_amd/_lib.py) bracket every launch of the zeta row pass (k_x_get_zeta) and of the ray step
(k_pt_rk4_r) over --steps further steps, one class at a time; the mean per launch is reported in microseconds.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, default=4096, metavar="NX", help="the grid size")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--counts", default="16,18,20", help="log2 of the particle counts")
    a = ap.parse_args()
    import niwqg_amd
    from niwqg_amd import particles, _lib
    nx, L = a.cost, 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    m.set_q(q * 1e-5 / q.std())
    m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))

    def rate():
        m._ctx.step(2)
        m._ctx.sync()
        t0 = time.perf_counter()
        m._ctx.step(a.steps)
        m._ctx.sync()
        return a.steps / (time.perf_counter() - t0)

    def alone(name):
        """mean microseconds per launch of one of ray mode's kernel classes over --steps steps"""
        m._ctx.profile_enable(_lib.Context.RAY_KERNEL_CLASSES[name])
        m._ctx.step(a.steps)
        n, ms = m._ctx.profile_read()
        m._ctx.profile_enable(-1)
        return 1e3 * ms / max(n, 1), n
    out = dict(nx=nx, steps=a.steps, reps=a.reps)
    for e in [int(v) for v in a.counts.split(",")]:
        n = 1 << e
        x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
        th = rng.uniform(0, 2 * np.pi, n)
        kl = (k0 * np.cos(th), k0 * np.sin(th))
        legs = {"none": [], "particles": [], "rays": []}
        added = 0
        key = "2^%d" % e
        for rep in range(a.reps):
            legs["none"].append(rate())
            for leg, rays in (("particles", None), ("rays", kl)):
                P = particles.attach(m, x, y, rays=rays)
                b = m._ctx.device_bytes()
                legs[leg].append(rate())
                if leg == "rays" and rep == a.reps - 1:
                    for name in ("pt_zeta", "pt_rays"):
                        us, launches = alone(name)
                        out["us_per_launch_%s_%s" % (name, key)] = round(us, 1)
                        out["launches_%s_%s" % (name, key)] = launches
                P.detach()
                added = b - added if leg == "rays" else b
        med = {k: statistics.median(v) for k, v in legs.items()}
        for k, v in med.items():
            out["steps_per_s_%s_%s" % (k, key)] = round(v, 2)
        out["particles_over_none_" + key] = round(med["none"] / med["particles"], 4)
        out["rays_over_none_" + key] = round(med["none"] / med["rays"], 4)
        out["rays_over_particles_" + key] = round(med["particles"] / med["rays"], 4)
        out["bytes_added_by_rays_" + key] = added
    print(json.dumps(out))


if __name__ == "__main__":
    main()
