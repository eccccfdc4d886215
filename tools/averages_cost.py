"""Cost of the averages' sample inside the step.

    python tools/averages_cost.py --cost 4096        # ms per sample for 2, 5 and 11 planes against the bare step, one JSON line
    python tools/averages_cost.py --check 8192       # one sample of q, q_psi, phi against the model's own reads, one JSON line

--cost: CoupledModel at nx with a broadband state; batched calls of --steps steps, timed with device events, alternating the bare
step (nothing attached) and the three configurations --reps times, each at every = 1; the medians are reported and ms per
sample is the difference to the bare step.  --check: the one grid whose rows run as two half-length problems."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {2: (("q_psi", "phi2"), ()),
           5: (("q_psi", "phi2"), (("q_psi", "phi2"), ("phi2", "phi2"), ("q_psi", "q_psi"))),
           11: (("q", "q_psi", "phi2", "phi"), (("q", "q"), ("q", "q_psi"), ("q", "phi2"), ("q_psi", "q_psi"), ("q_psi", "phi2"), ("phi2", "phi2")))}


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
    return m


def cost(nx, steps, reps):
    from niwqg_amd import averages
    m = model(nx)
    c = m._ctx
    c.step(2)

    def timed():
        c.timer_start()
        c.step(steps)
        return c.timer_stop() / steps
    runs = {k: [] for k in [0] + sorted(CONFIGS)}
    for _ in range(reps):
        for k in runs:
            A = averages.attach(m, *CONFIGS[k], every=1) if k else None
            timed()                                   # warm-up of this configuration
            runs[k].append(timed())
            if A:
                assert A.info()["n"] == 2 * steps
                A.detach()
    med = {k: float(np.median(v)) for k, v in runs.items()}
    out = dict(nx=nx, steps=steps, reps=reps, bare_step_ms=round(med[0], 4), bare_step_ms_all=[round(v, 4) for v in runs[0]])
    for k in sorted(CONFIGS):
        out["step_ms_%d_planes" % k] = round(med[k], 4)
        out["ms_per_sample_%d_planes" % k] = round(med[k] - med[0], 4)
        out["gb_per_s_%d_planes" % k] = round(2 * k * nx * nx * 8 / ((med[k] - med[0]) * 1e-3) / 1e9, 1) if med[k] > med[0] else None
    print(json.dumps(out))


def check(nx):
    from niwqg_amd import averages
    m = model(nx)
    m._ctx.step(1)
    m._after_steps()
    A = averages.attach(m, ("q", "q_psi", "phi"), every=0)
    A.sample()
    R = A.result()
    out = dict(nx=nx, n=R.n)
    for n in A.fields:
        want = np.array(getattr(m, n))
        out["rel_err_" + n] = float(np.abs(R.sums[n] - want).max() / np.abs(want).max())
    A.detach()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, metavar="NX")
    ap.add_argument("--check", type=int, metavar="NX")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.cost is None and a.check is None:
        ap.error("one of --cost NX, --check NX")
    if a.cost is not None:
        cost(a.cost, a.steps, a.reps)
    if a.check is not None:
        check(a.check)


if __name__ == "__main__":
    main()
