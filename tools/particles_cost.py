"""Cost of Lagrangian particles inside the step.

CoupledModel at nx (default 4096) with a broadband state: steps/s of nq_step(--steps) with no particles, and with 2^16, 2^18,
2^20 and 2^22 uniformly placed particles, without records and with record=("phi",) at record_every=10.  Each leg runs one warm-up
call, then --steps steps timed with perf_counter around a synchronous call.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--counts", default="0,16,18,20,22", help="log2 of the particle counts (0: none)")
    a = ap.parse_args()
    import niwqg_amd
    from niwqg_amd import particles
    nx, L = a.nx, 2 * np.pi * 200e3
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
    out = dict(nx=nx, steps=a.steps)
    base = rate()
    out["steps_per_s_0"] = round(base, 2)
    for e in [int(v) for v in a.counts.split(",") if int(v) > 0]:
        n = 1 << e
        x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
        for rec in (False, True):
            b0 = m._ctx.device_bytes()
            P = particles.attach(m, x, y, record_every=10 if rec else 0, capacity=4, record=("phi",) if rec else ())
            key = "2^%d%s" % (e, "_phi" if rec else "")
            r = rate()
            out["steps_per_s_" + key] = round(r, 2)
            out["step_ratio_" + key] = round(base / r, 3)
            out["bytes_" + key] = m._ctx.device_bytes() - b0
            P.detach()
    out["steps_per_s_0_again"] = round(rate(), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
