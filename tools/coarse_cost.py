"""Cost of the coarse-grained flux maps.

    python tools/coarse_cost.py --cost 4096        # ms per call: 1, 2, 3 scales without maps, a spectral_transfer call; one JSON line

CoupledModel at nx with a broadband state (tools/averages_cost.py), two steps in.  Before anything is timed the three identities
are asserted at that size: for the sharp cut at shell nx/8 the plane mean of each map equals the spectral flux through the cut at
1e-12 (mean |map| + sum |T|).  Then the calls alternate --reps times in one run, each timed with device events after a warm-up
call: all three maps, maps=False, with one, two and three scales, and nq_transfer_binned as the yardstick.  Medians, every
repetition, and the cost of each further scale (the slope between one and three scales) are reported."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from averages_cost import model          # noqa: E402


def identities(m):
    from niwqg_amd import coarse
    from niwqg_amd.transfer import spectral_transfer
    B = m.nx // 8
    R = coarse.flux_maps(m, [B])
    st = spectral_transfer(m)
    out = {}
    for name in R.names:
        scale = np.abs(R.maps[name][0]).mean() + np.abs(st.transfer[name]).sum()
        out[name] = float(abs(R.mean[name][0] - st.flux[name][B]) / scale)
        assert out[name] <= 1e-12, (name, out[name])
    return out


def cost(nx, reps):
    from niwqg_amd import coarse
    m = model(nx)
    c = m._ctx
    c.step(2)
    m._after_steps()
    out = dict(nx=nx, reps=reps, identity_rel_err=identities(m))
    shells = [nx // 64, nx // 16, nx // 8]
    tabs = np.array([coarse.sharp(m, B) for B in shells])

    def timed(f):
        f()
        c.timer_start()
        f()
        return c.timer_stop()
    calls = {"scales_%d_ms" % n: (lambda n=n: c.coarse_flux(7, tabs[:n], 0)) for n in (1, 2, 3)}
    calls["spectral_transfer_ms"] = lambda: c.transfer_sums_binned()
    runs = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            runs[k].append(timed(f))
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_all"] = [round(x, 4) for x in v]
    out["each_further_scale_ms"] = round((out["scales_3_ms"] - out["scales_1_ms"]) / 2, 4)
    out["device_bytes"] = c.device_bytes()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, metavar="NX", required=True)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    cost(a.cost, a.reps)


if __name__ == "__main__":
    main()
