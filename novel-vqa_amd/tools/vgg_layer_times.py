#!/usr/bin/env python3
"""vgg_layer_times.py -- per-layer times of the VGG-16 body's forward, d(input) and weight-gradient kernels from a rocprofv3
kernel trace (--kernel-trace, csv) of a fine-tuning run.  The convolutions share kernels, so a layer is told by its place in
the dispatch order: a forward pass launches its 13 convolutions bottom up (epilogue EpiBiasRelu), a backward pass the 13 weight
gradients (A_MC x B_NCTAP) and the 12 d(input) products (EpiGradMask) top down.  Prints / writes ONE JSON object: the median
microseconds per layer over all passes in the trace, and the step lines given with --step (ae_bench.py --finetune --out).

    python novel-vqa_amd/tools/vgg_layer_times.py TRACE.csv [--step STEP.json ...] [--out FILE]
"""
import argparse
import csv
import json

import numpy as np

NAMES = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1",
         "conv5_2", "conv5_3"]


def kind(name):
    if "gemm_f32_kernel" not in name:
        return None
    if "EpiBiasRelu" in name and "EpiBiasReluB16" not in name:
        return "forward"
    if "EpiGradMask" in name:
        return "dx"
    if ">, 1, 2, false, nvqa::EpiStore" in name:
        return "dw"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--step", action="append", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"]))
    seq = {"forward": [], "dx": [], "dw": []}
    for r in rows:
        k = kind(r["Kernel_Name"])
        if k:
            seq[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    per = {"forward": 13, "dx": 12, "dw": 13}
    layers, passes = {}, {}
    for k, v in seq.items():
        n = per[k]
        if not v or len(v) % n:
            raise SystemExit("%s: %d dispatches are not whole passes of %d" % (k, len(v), n))
        m = np.median(np.asarray(v).reshape(-1, n), axis=0)
        passes[k] = len(v) // n
        order = NAMES if k == "forward" else NAMES[::-1][:n]  # the backward runs top down; conv1_1 has no d(input)
        layers[k] = {name: round(float(x), 1) for name, x in zip(order, m)}
    out = {"unit": "us, median over the passes of the trace", "passes": passes,
           "layers": [{"layer": n, "forward": layers["forward"][n], "dx": layers["dx"].get(n), "dw": layers["dw"][n]} for n in NAMES],
           "totals_ms": {k: round(sum(v.values()) / 1e3, 3) for k, v in layers.items()},
           "steps": [json.loads(open(p).read()) for p in a.step]}
    s = json.dumps(out, indent=1)
    print(s if not a.out else json.dumps(out["totals_ms"]))
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
