#!/usr/bin/env python
"""How far apart are two runs of the SAME op-by-op `fused_tensorf` training step of a TensoRF model?

The factorised lookup's backward adds with fp32 atomics (csrc/ugrid_tensorf.hip): the same terms, summed in an order that differs from
run to run.  A native step over TensoRF grids (not built) has to be compared with this step under a bound that comes
from the spread two runs of THIS step show against each other.  For every configuration of tests/test_gpu_tensorf_step_spread.py the
tool runs the step `--reps` times on one model (forward + backward, nothing is updated) and records, per tensor kind (plane, vector,
f_vec, dense grid), the largest  max|dA - dB| / max|dB|  of a run against the first run and against the run before it, and whether
forward arrays, loss, mse, the rgbnet's gradients and the set of exactly-zero gradient entries were identical throughout.

    python tools/tensorf_step_spread.py [--reps 100] [--out profiles/tensorf/step_spread.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import board_state  # noqa: E402
import test_gpu_tensorf_step_spread as cases  # noqa: E402

KINDS = ("plane", "vector", "f_vec", "grid")


def compare(ga, gb, into):
    """per tensor kind, the largest max|ga - gb| / max|gb| into `into` -> (fixed-order gradients bit-identical?, zero sets identical?)"""
    fixed, zeros = True, True
    for k in gb:
        kind = cases.kind_of(k)
        if kind is None:
            fixed = fixed and bool(torch.equal(ga[k], gb[k]))
        else:
            into[kind] = max(into.get(kind, 0.0), float((ga[k] - gb[k]).abs().max()) / (float(gb[k].abs().max()) + 1e-30))
            zeros = zeros and bool(torch.equal(ga[k] == 0, gb[k] == 0))
    return fixed, zeros


def forward_equal(oa, ob):
    return all(bool(torch.equal(oa[k].detach(), ob[k].detach())) for k in ob if torch.is_tensor(ob[k]) and k in oa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensorf", "step_spread.json"))
    a = ap.parse_args()
    res = {"what": "two runs of the same op-by-op fused_tensorf step: max|dA - dB| / max|dB| per tensor kind", "reps": a.reps,
           "board_before": board_state.snapshot(), "cases": {}}
    worst = {}
    for name in cases.STEP_CASES:
        m, rays, kw = cases.setup_case(name)
        first_out, first = cases.run_step(m, rays, kw)
        prev = first
        case = {"samples": int(first_out["weights"].numel()), "vs_first": {}, "vs_previous": {}, "forward_always_equal": True,
                "rgbnet_grads_always_equal": True, "zero_entries_always_equal": True}
        for _ in range(a.reps):
            out, g = cases.run_step(m, rays, kw)
            case["forward_always_equal"] &= forward_equal(out, first_out)
            fixed, zeros = compare(g, first, case["vs_first"])
            case["rgbnet_grads_always_equal"] &= fixed
            case["zero_entries_always_equal"] &= zeros
            compare(g, prev, case["vs_previous"])
            prev = g
        for kind in KINDS:
            worst[kind] = max(worst.get(kind, 0.0), case["vs_first"].get(kind, 0.0), case["vs_previous"].get(kind, 0.0))
        res["cases"][name] = case
        print(name, json.dumps(case))
        del m
        torch.cuda.empty_cache()
    res["largest"] = worst
    res["times_4"] = {k: 4 * v for k, v in worst.items()}
    res["board_after"] = board_state.snapshot()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print("largest:", worst)


if __name__ == "__main__":
    main()
