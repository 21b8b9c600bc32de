"""Turns the rocprofv3 PMC passes of bench.py into per-launch HBM traffic per kernel group.

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d out/fetch -- python3 bench.py ...
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d out/write -- python3 bench.py ...
    python pmc_traffic.py out/fetch out/write profiles/traffic.json

FETCH_SIZE / WRITE_SIZE are in KiB.  On gfx950 FETCH_SIZE reports half the bytes of wide
coalesced reads (MI355X_MICROARCH.md, HBM section): it is doubled here, as the guide prescribes.
Kernel names are mapped to the group names of nvqa_profile_name().
"""
import collections
import csv
import glob
import json
import sys

GROUPS = [
    ("lstm_step_fwd", lambda n: "k_lstm_fwd_persist" in n or ("gemm_f32_multi_kernel" in n and "EpiLstmFwd" in n)),
    ("lstm_step_bwd", lambda n: "k_lstm_bwd_persist" in n),
    ("gemm_head", lambda n: ("gemm_f32_multi_kernel" in n and "EpiStore" in n) or "EpiHeadBwd" in n or "EpiResort" in n),
    ("gemm_wgrad", lambda n: "k_wgrad_bf16" in n or "k_wgrad_split" in n or ("gemm_f32_kernel" in n and "128, 128" in n and ", 1, 1, false" in n and "EpiStore" in n)),
    # i2h forward and the classifier's W_o product share a kernel (EpiBias2, K-contiguous x K-contiguous): the
    # time-batched one is the launch with more than a million threads
    ("gemm_i2h_fwd", lambda n, grid=0: "gemm_f32_kernel" in n and "EpiBias2" in n and grid > (1 << 20)),
    # d(input): the one K-contiguous x N-contiguous product with a plain store and a time-batched grid
    # (f32 mode by default: k_dx0_split, dx0_split.h)
    ("gemm_dgrad", lambda n, grid=0: "k_dx0_split" in n or ("gemm_f32_kernel" in n and ", 0, 1, false" in n and "EpiStore" in n and grid > 500000)),
    ("rmsprop", lambda n: "k_rmsprop" in n),
    ("emb_bwd", lambda n: "k_emb_bwd" in n),
    ("emb_fwd", lambda n: "k_emb_fwd" in n),
    ("softmax_ce", lambda n: "k_softmax_ce" in n),
]


def match(pred, row):
    """predicates take the kernel name, and optionally the launch's thread count as `grid`"""
    if pred.__code__.co_argcount > 1:
        return pred(row["Kernel_Name"], int(row.get("Grid_Size", 0) or 0))
    return pred(row["Kernel_Name"])


def collect(d, counter):
    f = glob.glob(d + "/*/*counter_collection.csv") + glob.glob(d + "/*counter_collection.csv")
    agg, cnt = collections.defaultdict(float), collections.Counter()
    for r in csv.DictReader(open(f[0])):
        if r["Counter_Name"] != counter:
            continue
        for g, pred in GROUPS:
            if match(pred, r):
                agg[g] += float(r["Counter_Value"])
                cnt[g] += 1
                break
    return {g: agg[g] / cnt[g] for g in agg}


def main():
    fetch = collect(sys.argv[1], "FETCH_SIZE")
    write = collect(sys.argv[2], "WRITE_SIZE")
    out = {}
    for g in sorted(set(fetch) | set(write)):
        fb = 2.0 * fetch.get(g, 0.0) * 1024  # gfx950: FETCH_SIZE counts 64 B per 128-B request
        wb = write.get(g, 0.0) * 1024
        out[g] = {"hbm_bytes_per_launch": round(fb + wb), "fetch_bytes_corrected": round(fb), "write_bytes": round(wb)}
    json.dump(out, open(sys.argv[3], "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
