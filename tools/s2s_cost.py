"""Cost of the shell-to-shell transfers.

    python tools/s2s_cost.py --cost 4096        # ms per call: 1, 2 and 8 donor bands, a spectral_transfer call; one JSON line

CoupledModel at nx with a broadband state (tools/averages_cost.py), two steps in, all four names.  Before anything is timed the
refraction's band-to-band matrix is asserted antisymmetric at that size (1e-12 sum |T|: it holds on any state).  Then the calls
alternate --reps times in one run, each timed with device events after a warm-up call: one, two and eight bands, and
nq_transfer_binned as the yardstick.  Medians, every repetition, the cost of the first band and of each further band (the slope
between one and eight bands), and the bytes per band of section 5p's count with the rate they would mean are reported."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from averages_cost import model          # noqa: E402


def bytes_per_band(nx):
    """DESIGN.md section 5p's count for CoupledModel with all names: planes of 16-byte values read or written per donor band,
    h = nx (nx/2 + 1) elements (half spectrum), f = nx^2 (full)"""
    h, f = nx * (nx // 2 + 1), nx * nx
    spectral = (h + f) + (h + 2 * f)                       # k_s_band: reads Q-hat, W; writes G Q, G W, il G W
    inverse = 2 * 2 * (h + 2 * f)                          # k_y_B and k_y_A, read and write, on the three planes
    rows = (2 * h + h + 2 * f) + (2 * h + f) + (2 * h + f) + f        # pass 0: reads mU, mP, gq, gw, wy, writes Muq, Mvq, Mw; pass 1: mQ, mQw, gw -> Mw
    forward = 2 * (2 * h + f) + 2 * f                      # k_y_A in place on Muq, Mvq, Mw; then on Mw again
    bins = 2 * 2 * h + 2 * 2 * f                           # k_y_B out of place: two half planes, twice one full plane
    binning = (2 * h + 2 * h) + 2 * 2 * f                  # BinTrQ: Fu, Fv, P, Q; BinTrW twice: W and the plane
    return 16 * (spectral + inverse + rows + forward + bins + binning)


def cost(nx, reps):
    from niwqg_amd import shelltoshell
    m = model(nx)
    c = m._ctx
    c.step(2)
    m._after_steps()
    edges = [0, 2, 4, 8, 16, 32, nx // 16, nx // 8, nx // 2]
    R = shelltoshell.shell_to_shell(m, edges)
    M = R.matrix("ke_niw_ref")
    anti = float(np.abs(M + M.T).max() / np.abs(R.rows["ke_niw_ref"]).sum())
    assert anti <= 1e-12, anti
    out = dict(nx=nx, reps=reps, ke_niw_ref_antisymmetry_rel_err=anti)
    tabs = R.table

    def timed(f):
        f()
        c.timer_start()
        f()
        return c.timer_stop()
    calls = {"bands_%d_ms" % n: (lambda n=n: c.shell_transfer(7, tabs[:n])) for n in (1, 2, 8)}
    calls["spectral_transfer_ms"] = lambda: c.transfer_sums_binned()
    runs = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            runs[k].append(timed(f))
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_all"] = [round(x, 4) for x in v]
    out["first_band_ms"] = out["bands_1_ms"]
    out["each_further_band_ms"] = round((out["bands_8_ms"] - out["bands_1_ms"]) / 7, 4)
    out["bytes_per_band"] = bytes_per_band(nx)
    out["per_band_tb_per_s"] = round(out["bytes_per_band"] / (out["each_further_band_ms"] * 1e-3) / 1e12, 3)
    out["per_band_over_spectral_transfer"] = round(out["each_further_band_ms"] / out["spectral_transfer_ms"], 3)
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
