#!/usr/bin/env python3
"""Condense a tools/profile_bench.sh output directory into profiles/<tag>_*.{csv,md,json} (tracked).

    profiles/<tag>_kernel_stats.csv      rocprofv3 --kernel-trace --stats of bench.py --full (both kernels)
    profiles/<tag>_bench.json            the un-profiled bench line of the same box
    profiles/<tag>_pmc_<precision>.json  PMC means per dispatch of that precision's kernel (+ HBM traffic)
    profiles/<tag>_summary.md            the table the DESIGN / VERDICT numbers are read from
"""
import collections
import csv
import glob
import json
import os
import shutil
import sys

tag = sys.argv[1] if len(sys.argv) > 1 else "r02"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(REPO, "gpurun_out", f"prof_{tag}")
dst = os.path.join(REPO, "profiles")
os.makedirs(dst, exist_ok=True)
KERNEL_OF = {"f32": "bk_leaf_eval_kernel<3, false>", "f16x2": "bk_leaf_eval_f16_kernel<3>"}
TAIL_OF = {"f32": "bk_leaf_eval_kernel<2, false>"}

stats = glob.glob(os.path.join(src, "trace", "*", "*_kernel_stats.csv"))[0]
shutil.copy(stats, os.path.join(dst, f"{tag}_kernel_stats.csv"))
bench = json.loads(open(os.path.join(src, "bench.json")).read().strip().splitlines()[-1])
json.dump(bench, open(os.path.join(dst, f"{tag}_bench.json"), "w"), indent=1)
rows = list(csv.DictReader(open(stats)))
B = bench["config"]["batch_per_gpu"]
# per-precision extracts of the same csv (the rows of that precision's kernels only)
for prec, pat in (("f32", "bk_leaf_eval_kernel<"), ("f16x2", "bk_leaf_eval_f16_kernel<")):
    with open(os.path.join(dst, f"{tag}_kernel_stats_{prec}.csv"), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows(r for r in rows if pat in r["Name"] or (prec == "f32" and "bk_leaf_eval_coop_kernel<" in r["Name"]))


# per-dispatch rows of the same trace: the profiled run also launches the kernels on other batch sizes (the in-run parity check's
# 536 positions, the small-batch latency leg), which the aggregated *_kernel_stats.csv averages in; durations below are those
# of each kernel's most frequent grid -- the timed batch
trace_files = glob.glob(os.path.join(src, "trace", "*", "*_kernel_trace.csv"))
per_dispatch = collections.defaultdict(list)
if trace_files:
    for r in csv.DictReader(open(trace_files[0])):
        per_dispatch[r["Kernel_Name"]].append((r["Grid_Size_X"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))


def full_size_ms(kernel_name):
    """(average ms, calls) over the dispatches of the kernel's most frequent grid; None without a per-dispatch trace"""
    rows_ = next((v for k, v in per_dispatch.items() if kernel_name in k), None)
    if not rows_:
        return None
    grid = collections.Counter(g for g, _ in rows_).most_common(1)[0][0]
    d = [ns for g, ns in rows_ if g == grid]
    return sum(d) / len(d) / 1e6, len(d)


def bench_block(prec):
    return bench if bench["config"]["precision"] == prec else bench.get(prec)


with open(os.path.join(dst, f"{tag}_summary.md"), "w") as o:
    o.write(f"# rocprofv3 summary {tag} (MI355X, `python3 bench.py --full`, batch {B})\n\n")
    o.write("## --kernel-trace --stats (one run: fp32 headline + nested f16x2 block)\n\n| kernel | calls | avg ms | min ms | max ms | % |\n|---|---|---|---|---|---|\n")
    for r in rows[:6]:
        o.write(f"| `{r['Name'][:80]}` | {r['Calls']} | {float(r['AverageNs'])/1e6:.4f} | {float(r['MinNs'])/1e6:.4f} | "
                f"{float(r['MaxNs'])/1e6:.4f} | {r['Percentage']} |\n")
    for prec, kname in KERNEL_OF.items():
        kern = [r for r in rows if kname in r["Name"]]
        blk = bench_block(prec)
        if not kern or not blk:
            continue
        kern = kern[0]
        avg_ms = own_ms = float(kern["AverageNs"]) / 1e6   # own_ms: this kernel alone (the PMC rows are per dispatch of it)
        fs = full_size_ms(kname)
        if fs:
            avg_ms = own_ms = fs[0]
            o.write(f"\n(`{kname}`: {fs[1]} dispatches of the timed batch, average {fs[0]:.4f} ms; the stats table above averages "
                    f"all {kern['Calls']} dispatches, smaller launches included)\n")
        # fp32 at B=4096 runs as 10 whole rounds of 3-board workgroups + a tail launch of 2-board ones (split launch):
        # bench.py's HIP events bracket both, so the per-step kernel time is the sum of the two rows
        tail = [r for r in rows if TAIL_OF.get(prec, "\0") in r["Name"]]
        fs_tail = full_size_ms(TAIL_OF[prec]) if tail else None
        # (the tail kernel also serves other legs of the bench -- 2-board rounds of the small-batch block: compare the counts of
        # the two kernels' timed-batch grids where the per-dispatch trace is there, else the aggregate call counts)
        same = (abs(fs_tail[1] - fs[1]) <= 0.1 * fs[1]) if (fs and fs_tail) else \
            (tail and abs(int(tail[0]["Calls"]) - int(kern["Calls"])) <= 0.1 * int(kern["Calls"]))
        if tail and same:
            tail_ms = (fs_tail or (float(tail[0]["AverageNs"]) / 1e6,))[0]
            o.write(f"\n(split launch: `{kname}` avg {avg_ms:.4f} ms + tail `{TAIL_OF[prec]}` avg {tail_ms:.4f} ms per step)\n")
            avg_ms += tail_ms
        rf = blk["roofline"]
        o.write(f"\n## {prec}: `{kname}`\n\nbench.py HIP-event kernel time (un-profiled run): {rf['kernel_ms']:.4f} ms "
                f"(sustained loop {rf.get('sustained_kernel_ms', float('nan')):.4f} ms); rocprofv3 average: {avg_ms:.4f} ms over {kern['Calls']} calls.\n"
                f"roofline.frac = {rf['frac']:.4f} of {rf['peak']} TFLOP/s (sustained {rf.get('sustained_frac', float('nan')):.4f}); "
                f"from the rocprofv3 average: {B * 266838272 / (avg_ms * 1e-3) / 1e12 / rf['peak']:.4f}.\n")
        pmc, meta = collections.OrderedDict(), {}
        for f in sorted(glob.glob(os.path.join(src, f"pmc_{prec}_*", "*", "*_counter_collection.csv"))):
            agg = collections.defaultdict(list)
            recs = [r for r in csv.DictReader(open(f)) if kname in r["Kernel_Name"]]
            # the profiled run also launches this kernel on other batch sizes (the in-run parity check's 536 positions):
            # keep the dispatches of the most frequent grid only, so that every mean is per launch of the timed batch
            grid = collections.Counter(r["Grid_Size"] for r in recs).most_common(1)[0][0] if recs else None
            for r in recs:
                if r["Grid_Size"] == grid:
                    agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
                    meta = {k: r[k] for k in ("Grid_Size", "Workgroup_Size", "LDS_Block_Size", "VGPR_Count", "Accum_VGPR_Count", "SGPR_Count")}
            for k, v in agg.items():
                pmc[k] = (sum(v) / len(v), len(v))
        if not pmc:
            continue
        o.write(f"\nDispatch: {meta}\n\n--pmc passes (mean per dispatch):\n\n| counter | mean | n |\n|---|---|---|\n")
        for k, (m, n) in pmc.items():
            o.write(f"| {k} | {m:.6g} | {n} |\n")
        g = pmc.get("GRBM_GUI_ACTIVE", (0, 0))[0]
        derived = {}
        if g:
            derived["effective_clock_ghz"] = g / 8 / (own_ms * 1e-3) / 1e9
            o.write(f"\nEffective clock = GRBM_GUI_ACTIVE / 8 XCDs / kernel time ({own_ms:.4f} ms) = {g/8/(own_ms*1e-3)/1e9:.3f} GHz\n")
        mf = pmc.get("SQ_VALU_MFMA_BUSY_CYCLES", (0, 0))[0]
        if mf and g:
            derived["mfma_busy"] = mf / 1024 / (g / 8)
            o.write(f"MFMA pipe busy = SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs / (GRBM_GUI_ACTIVE/8) = {mf/1024/(g/8)*100:.1f} %\n")
        mops, waves = pmc.get("SQ_INSTS_VALU_MFMA_MOPS_F32", (0, 0))[0], pmc.get("SQ_WAVES", (0, 0))[0]
        if mops and waves:
            wgs = waves / (int(meta["Workgroup_Size"]) / 64)
            derived["executed_mfma_flop_per_launch"] = mops * 512
            derived["executed_mfma_flop_per_workgroup"] = mops * 512 / wgs
            o.write(f"Executed fp32-MFMA work = SQ_INSTS_VALU_MFMA_MOPS_F32 x 512 = {mops*512/1e12:.4f} TFLOP per launch of {wgs:.0f} workgroups "
                    f"= {mops*512/wgs/1e6:.2f} MFLOP per workgroup (tile tables, bk_plan_flops: 435.36 per 3-board workgroup and net); "
                    f"algorithmic for the {wgs*3:.0f} boards of this launch {wgs*3*133419136/1e12:.4f} TFLOP: executed / algorithmic = {mops*512/(wgs*3*133419136):.4f}\n")
        fs, ws = pmc.get("FETCH_SIZE", (0, 0))[0], pmc.get("WRITE_SIZE", (0, 0))[0]
        traffic = (2 * fs + ws) * 1024 if fs else None
        if fs:
            o.write(f"Fabric-side traffic per launch = (2 x FETCH_SIZE + WRITE_SIZE) x 1024 = {traffic/1e6:.1f} MB "
                    f"(gfx950 FETCH_SIZE correction x2, MI355X_MICROARCH.md HBM section); algorithmic "
                    f"{rf['algorithmic_hbm_bytes_per_launch']/1e6:.1f} MB + 7.9 MB weights. "
                    f"= {traffic/(own_ms*1e-3)/1e9:.1f} GB/s vs 8000 GB/s peak.\n")
        h, m = pmc.get("TCC_HIT_sum", (0, 0))[0], pmc.get("TCC_MISS_sum", (0, 0))[0]
        if h:
            o.write(f"L2 hit rate = {h/(h+m)*100:.2f} %\n")
        c, a = pmc.get("SQ_LDS_BANK_CONFLICT", (0, 0))[0], pmc.get("SQ_LDS_IDX_ACTIVE", (0, 0))[0]
        if a and g:
            o.write(f"LDS: bank-conflict cycles / active cycles = {c/a*100:.1f} %; LDS active = {a/256/(g/8)*100:.1f} % of CU time\n")
        json.dump({"tag": tag, "precision": prec, "kernel": kern["Name"], "rocprof_avg_kernel_ms": avg_ms, "batch": B,
                   "own_kernel_ms": own_ms, "dispatch": meta, **derived,
                   "counters": {k: v[0] for k, v in pmc.items()}, "hbm_traffic_bytes_per_launch": traffic,
                   "traffic_formula": "(2*FETCH_SIZE + WRITE_SIZE)*1024, gfx950 FETCH_SIZE x2 correction"},
                  open(os.path.join(dst, f"{tag}_pmc_{prec}.json"), "w"), indent=1)
print(open(os.path.join(dst, f"{tag}_summary.md")).read())
