"""Cost of the Lagrangian spectra, autocovariance and dispersion against downloading the ring they replace.

    python tools/lagrangian_cost.py --cost 4096

CoupledModel at the given nx with a broadband state, --particles (default 2^18) particles recording u, v and phi after every step
into a ring of --records (default 1024), filled by stepping.  Then, each after a first call that allocates its work memory and
builds the transform plan, and timed with perf_counter around the synchronous call, --reps times each: a phi spectrum (Hann, 8
groups), a uv autocovariance (8 groups), a dispersion with 8 groups and --pairs (default 2^18) pairs -- and, in the same run,
P.trajectory(), the download of the same ring, which is what one would do without them.  Prints one JSON line and writes it to
profiles/lagrangian_cost_<nx>.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, default=4096, metavar="NX")
    ap.add_argument("--particles", type=int, default=1 << 18)
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import niwqg_amd
    from niwqg_amd import particles, lagrangian
    nx, L = a.cost, 2 * np.pi * 200e3
    k0 = 10 * 2 * np.pi / L
    m = niwqg_amd.CoupledModel.Model(nx=nx, L=L, dt=0.025 / (0.1 * k0) * 128 / nx, tmax=1e30, twrite=10 ** 9, tdiags=10 ** 9,
                                     use_filter=True, U=-0.1, f=1e-4, N=0.01, m=2 * np.pi / 280.0, nu4=5e11 * (128.0 / nx) ** 4,
                                     nu=20, nuw=50.0, nu4w=1e9 * (128.0 / nx) ** 4, muw=1e-7)
    rng = np.random.default_rng(1)
    q = np.fft.irfft2((rng.standard_normal((nx, nx // 2 + 1)) + 1j * rng.standard_normal((nx, nx // 2 + 1))) * 1e-9, s=(nx, nx))
    m.set_q(q * 1e-5 / q.std())
    m.set_phi(0.1 * (1 + 1j) + 0.01 * rng.standard_normal((nx, nx)))
    ctx = m._ctx
    n, T = a.particles, a.records
    b0 = ctx.device_bytes()
    P = particles.attach(m, rng.uniform(0, L, n), rng.uniform(0, L, n), record_every=1, capacity=T, record=("u", "v", "phi"))
    t0 = time.perf_counter()
    ctx.step(T - 1)                                          # fill the ring
    ctx.sync()
    out = dict(nx=nx, particles=n, records=T, groups=a.groups, pairs=a.pairs, reps=a.reps,
               fill_ms_per_step=(time.perf_counter() - t0) / (T - 1) * 1e3, ring_bytes=8 * T * 6 * n)
    out["bytes_attached"] = ctx.device_bytes() - b0
    groups = rng.integers(0, a.groups, n)
    i = rng.integers(0, n, a.pairs)
    pairs = (i, (i + rng.integers(1, n, a.pairs)) % n)

    def timed(key, call):
        t0 = time.perf_counter()
        r = call()
        out[key + "_first_call_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for _ in range(a.reps):
            r = call()
        out[key + "_ms"] = (time.perf_counter() - t0) / a.reps * 1e3
        return r

    S = timed("phi_spectrum", lambda: lagrangian.spectrum(P, "phi", "hann", True, groups))
    R = timed("uv_autocovariance", lambda: lagrangian.autocovariance(P, "uv", groups=groups))
    D = timed("dispersion", lambda: lagrangian.dispersion(P, pairs, groups))
    out["spectrum_shape"] = list(S.values["phi"].shape)
    out["autocovariance_shape"] = list(R.values.shape)
    out["finite"] = bool(np.all(np.isfinite(S.values["phi"])) and np.all(np.isfinite(R.values)) and np.all(np.isfinite(D.A2)) and
                         np.all(np.isfinite(D.D2)))
    out["bytes_with_tables"] = ctx.device_bytes() - b0
    t0 = time.perf_counter()
    tr = P.trajectory()
    out["trajectory_download_ms"] = (time.perf_counter() - t0) * 1e3
    out["trajectory_host_bytes"] = int(tr.x.nbytes + tr.y.nbytes + sum(v.nbytes for v in tr.values.values()))
    P.detach()
    out["bytes_after_detach"] = ctx.device_bytes() - b0
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()})
    print(line)
    with open(os.path.join(ROOT, "profiles", "lagrangian_cost_%d.json" % nx), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
