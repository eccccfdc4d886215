"""Cost of one field_pdfs call against one scalar diagnostics tick.

CoupledModel at nx (default 4096) with a broadband state; every call is synchronous (the host waits for the result), timed with
perf_counter over --reps calls after two warm-up calls each, all in the same run: explicit ranges (one device pass), default
ranges (the min/max pass first), and explicit ranges with the joint table.  Prints one JSON line."""
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
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--joint-bins", type=int, default=64)
    ap.add_argument("--state", choices=("broadband", "peaked"), default="broadband",
                    help="peaked: a bare Lamb dipole (q exactly zero outside r = R) under uniform waves: nearly every point of "
                         "every field falls into one bin, the worst case for the LDS atomics")
    a = ap.parse_args()
    import niwqg_amd
    from niwqg_amd.pdfs import field_pdfs
    nx, L = a.nx, 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    if a.state == "peaked":
        from niwqg_amd import InitialConditions as ic
        m.set_q(ic.LambDipole(m, U=0.1, R=2 * np.pi / k0))
        m.set_phi(np.full((nx, nx), 0.1 * (1 + 1j)))
    else:
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
    h = field_pdfs(m, bins=a.bins)
    r = {n: (float(e[0]), float(e[-1])) for n, e in h.edges.items()}
    two = timed(lambda: field_pdfs(m, bins=a.bins))
    one = timed(lambda: field_pdfs(m, bins=a.bins, ranges=r))
    joint = timed(lambda: field_pdfs(m, bins=a.bins, ranges=r, joint=("q_psi", "phi2"), joint_bins=a.joint_bins))
    tick2 = timed(lambda: m._ctx.diagnostic_sums())
    peak = {n: round(float(h.counts[n].max()) / (nx * nx), 4) for n in h.counts}
    print(json.dumps(dict(nx=nx, state=a.state, bins=a.bins, joint_bins=a.joint_bins, tick_ms=round(tick, 3), tick_again_ms=round(tick2, 3),
                          one_pass_ms=round(one, 3), two_pass_ms=round(two, 3), joint_ms=round(joint, 3),
                          ratio_one_pass=round(one / tick, 3), ratio_two_pass=round(two / tick, 3), ratio_joint=round(joint / tick, 3),
                          fullest_bin_share=peak, pdfs_extra_bytes=m._ctx.device_bytes() - bytes0)))


if __name__ == "__main__":
    main()
