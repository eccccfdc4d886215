#!/usr/bin/env python
"""Sweep of the CU split of the dual-stream step: CoupledModel 4096^2 (or --nx 8192), every setting of
NIWQG_AMD_OVERLAP_CUS measured right after a serial run (0) in the same process, so that drift of the box cancels in the pair.
    python tools/overlap_sweep.py [--nx 4096] [--steps 40] 28 40 51 60 69 85 92 104 128
The switch is read by nq_create, so each measurement builds its own model."""
import argparse, ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def measure(nx, setting, steps, reps=4):
    os.environ["NIWQG_AMD_OVERLAP_CUS"] = str(setting)
    m = bench.build_model("coupled", nx, 0)
    c = m._ctx
    info = (ctypes.c_int * 3)()
    c.L.nq_overlap_info(c.h, info)
    c.step(5); c.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); c.step(steps); c.sync(); t.append((time.perf_counter() - t0) / steps * 1e3)
    del c, m
    return sorted(t), list(info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("settings", type=int, nargs="+")
    a = ap.parse_args()
    nb = a.nx if a.nx == 8192 else 4096
    print("# nx=%d steps=%d x4; ms/step: median [min max]; waste = idle share of the wave-PV grid's last round" % (a.nx, a.steps))
    print("# asked  free  grid  rounds  waste    serial ms            overlap ms           gain(median)")
    for s in a.settings:
        t0, _ = measure(a.nx, 0, a.steps)
        t1, info = measure(a.nx, s, a.steps)
        g = info[1] or 256
        if a.nx == 8192 and not info[1]:
            g = 256
        r = -(-nb // g)
        med = lambda t: 0.5 * (t[len(t) // 2] + t[(len(t) - 1) // 2])
        print("%6d %5d %5d %6d  %.4f   %.3f [%.3f %.3f]   %.3f [%.3f %.3f]   %+.2f %%" % (
            s, info[0], g, r, r * g / nb - 1, med(t0), t0[0], t0[-1], med(t1), t1[0], t1[-1], (med(t0) / med(t1) - 1) * 100), flush=True)


if __name__ == "__main__":
    main()
