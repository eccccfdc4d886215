"""Cost of drifter mode inside the step.

    python tools/drifters_cost.py --cost 4096

CoupledModel at the given nx with a broadband state: steps/s of nq_step(--steps) without particles, and with 2^16, 2^18 and
2^20 uniformly placed particles attached with wave=None and with wave=1, all in one process and one run.  Each leg runs one
warm-up call, then --steps steps timed with perf_counter around a synchronous call, --reps times over, the legs of one count
alternating; the medians are reported, with the ratio of the drifter step to both other legs and the bytes the mode adds.
Prints one JSON line.

Per-call times of the two things the mode adds to a step, k_pt_rk4_w and the phi row pass (k_x_c2c), come from a kernel trace of
this tool:  rocprofv3 --kernel-trace --stats -- python tools/drifters_cost.py --cost 4096 --counts 18 --reps 1"""
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
    from niwqg_amd import particles
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
    out = dict(nx=nx, steps=a.steps, reps=a.reps)
    for e in [int(v) for v in a.counts.split(",")]:
        n = 1 << e
        x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
        legs = {"none": [], "particles": [], "drifters": []}
        added = 0
        for _ in range(a.reps):
            legs["none"].append(rate())
            for leg, wave in (("particles", None), ("drifters", 1.0)):
                P = particles.attach(m, x, y, wave=wave)
                b = m._ctx.device_bytes()
                legs[leg].append(rate())
                P.detach()
                added = b - added if leg == "drifters" else b
        med = {k: statistics.median(v) for k, v in legs.items()}
        key = "2^%d" % e
        for k, v in med.items():
            out["steps_per_s_%s_%s" % (k, key)] = round(v, 2)
        out["particles_over_none_" + key] = round(med["none"] / med["particles"], 4)
        out["drifters_over_none_" + key] = round(med["none"] / med["drifters"], 4)
        out["drifters_over_particles_" + key] = round(med["particles"] / med["drifters"], 4)
        out["bytes_added_by_wave_" + key] = added
    print(json.dumps(out))


if __name__ == "__main__":
    main()
