"""Cost and large-grid check of the flow fields in the PDFs and the averages.

    python tools/flow_cost.py --cost 4096        # ms per call: old-names PDFs, flow PDFs, a scalar tick; one JSON line
    python tools/flow_cost.py --check 2048       # one sample of every flow name against flow.reference; one JSON line

--cost: CoupledModel at nx with a broadband state; the three calls alternate --reps times in one run, each timed with device
events after a warm-up call, and the medians are reported.  --check: the instantiations the feature's own test does not reach, which tests/test_gpu_plan_ladder_analysis.py covers since (2048, 4096, and
8192, where every name runs in a launch of its own)."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from averages_cost import model          # noqa: E402  (tools/averages_cost.py: the broadband state of the averages' cost tool)

OLD = dict(names=("q", "q_psi", "phi2"), joint=("q_psi", "phi2"))
FLOW = dict(names=("q_psi", "ow", "gradphi2"), joint=("ow", "gradphi2"))


def cost(nx, reps):
    from niwqg_amd import pdfs
    m = model(nx)
    c = m._ctx
    c.step(2)
    ranges = {}
    for kw in (OLD, FLOW):
        h = pdfs.field_pdfs(m, **kw)
        ranges[kw["names"]] = {n: (h.edges[n][0], h.edges[n][-1]) for n in kw["names"]}

    def timed(f):
        f()
        c.timer_start()
        f()
        return c.timer_stop()
    calls = {"old_names_ms": lambda: pdfs._Fused(m).bin(list(OLD["names"]), ranges[OLD["names"]], 256, OLD["joint"], 64, False),
             "flow_names_ms": lambda: pdfs._Fused(m).bin(list(FLOW["names"]), ranges[FLOW["names"]], 256, FLOW["joint"], 64, False),
             "scalar_tick_ms": lambda: c.diagnostic_sums()}
    runs = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            runs[k].append(timed(f))
    out = dict(nx=nx, reps=reps, flow_names=list(FLOW["names"]))
    for k, v in runs.items():
        out[k] = round(float(np.median(v)), 4)
        out[k + "_all"] = [round(x, 4) for x in v]
    out["flow_over_old"] = round(out["flow_names_ms"] / out["old_names_ms"], 2)
    print(json.dumps(out))


def check(nx):
    from niwqg_amd import averages, flow
    m = model(nx)
    m._ctx.step(1)
    m._after_steps()
    ref = flow.reference(m)
    out = dict(nx=nx)
    for i in range(0, len(flow.NAMES), 3):
        A = averages.attach(m, flow.NAMES[i:i + 3], every=0)
        A.sample()
        R = A.result()
        for n in A.fields:
            out["rel_err_" + n] = float(np.abs(R.mean(n) - ref[n]).max() / np.abs(ref[n]).max())
        A.detach()
    out["ok"] = bool(all(v <= 1e-12 for k, v in out.items() if k.startswith("rel_err_")))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", type=int, metavar="NX")
    ap.add_argument("--check", type=int, metavar="NX")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.cost is None and a.check is None:
        ap.error("one of --cost NX, --check NX")
    if a.cost is not None:
        cost(a.cost, a.reps)
    if a.check is not None:
        check(a.check)


if __name__ == "__main__":
    main()
