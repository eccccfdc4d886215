"""Cost of one spectral_transfer call against one scalar diagnostics tick.

CoupledModel at nx (default 4096) with a broadband state; both calls are synchronous (the host waits for the result), timed
with perf_counter over --reps calls after two warm-up calls each.  Prints one JSON line."""
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
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import niwqg_amd
    from niwqg_amd.transfer import spectral_transfer
    nx, L = a.nx, 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    m.set_q(q * 1e-5 / q.std())
    m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))
    m._step_forward()

    def timed(fn):
        fn()
        fn()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return (time.perf_counter() - t0) / a.reps * 1e3
    tick = timed(lambda: m._ctx.diagnostic_sums())
    bytes0 = m._ctx.device_bytes()
    tr = timed(lambda: spectral_transfer(m))
    raw = timed(lambda: m._ctx.transfer_sums_binned())
    tick2 = timed(lambda: m._ctx.diagnostic_sums())
    print(json.dumps(dict(nx=nx, tick_ms=round(tick, 3), tick_again_ms=round(tick2, 3), transfer_ms=round(tr, 3),
                          raw_sums_ms=round(raw, 3), ratio=round(tr / min(tick, tick2), 2),
                          transfer_extra_bytes=m._ctx.device_bytes() - bytes0)))


if __name__ == "__main__":
    main()
