"""Kernel timeline of the last record verify in a rocprofv3 kernel trace
(`rocprofv3 --kernel-trace --output-format csv -- python3 bench.py ...`): every
hkv kernel from that call's prologue launch to its last verdict launch, with
its queue, grid and start / end relative to the first, then the call's span,
the sum of the kernels' durations and the time during which two or more of
them ran — the launches of a batch cut into parts (HKV_REC_PART) on two
streams show as overlapping intervals on two queues.
profiles/r13_rec_pipeline/timeline_*.txt.

    python tools/pipe_timeline.py prof_out/trace/t_kernel_trace.csv
"""
import csv
import sys


def main(path: str) -> None:
    rows = [r for r in csv.DictReader(open(path)) if "hkv" in r["Kernel_Name"] and "gen_" not in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    first = max(i for i, r in enumerate(rows) if "hkv_prologue_kernel" in r["Kernel_Name"])
    call = rows[first:]
    t0 = int(call[0]["Start_Timestamp"])
    edges = []
    for r in call:
        nm = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("hkv::", "")
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        edges += [(s, 1), (e, -1)]
        print(f"{nm[:34]:34s} queue {r.get('Queue_Id', '?'):>3s} grid {int(r['Grid_Size_X']):8d} "
              f"start {(s - t0) / 1e3:8.1f} end {(e - t0) / 1e3:8.1f} dur {(e - s) / 1e3:8.1f}")
    edges.sort()
    live, last, two, busy = 0, t0, 0, 0
    for t, d in edges:
        if live >= 1:
            busy += t - last
        if live >= 2:
            two += t - last
        live, last = live + d, t
    span = max(int(r["End_Timestamp"]) for r in call) - t0
    total = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in call)
    print(f"launches {len(call)} span {span / 1e3:.1f} us, sum of durations {total / 1e3:.1f} us, "
          f"a kernel running {busy / 1e3:.1f} us, two or more running {two / 1e3:.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
