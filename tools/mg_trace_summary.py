"""Per-level split of one multigrid-preconditioned solve from a `rocprofv3 --kernel-trace --output-format csv` run of
`tools/mg_probe.py --systems NAME --reps 1 --configs mg1 --applies 0`.

The kernel table of --stats adds a kernel's launches over all levels; a level is recognised here by the grid a launch was given
(the library's kernels size their grids by the level's rows), so the dispatches of the library's kernels (names with `hipk_`) are
grouped by (kernel, grid size): calls, average and total duration, and at the end the busy time against the span from the first
to the last of them -- the rest is launch gaps.

  python tools/mg_trace_summary.py DIR_OR_kernel_trace.csv [--from-last-solve]
"""
import csv
import glob
import os
import sys


def main():
    src = sys.argv[1]
    if os.path.isdir(src):
        src = sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))[-1]
    rows = []
    with open(src, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "hipk_" not in name:
                continue
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name.split("(")[0].replace("void ", ""),
                         int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)))
    rows.sort()
    # the timed solve is the last one: it starts at the last launch of the kernel that opens a callable-M CG (the <b,b> partials
    # follow the first residual), found as the last gap of more than 2 ms between library kernels
    start = 0
    if "--from-last-solve" in sys.argv:
        for i in range(1, len(rows)):
            if rows[i][0] - rows[i - 1][1] > 2_000_000:
                start = i
    rows = rows[start:]
    groups = {}
    for s, e, name, wgs in rows:
        g = groups.setdefault((name, wgs), [0, 0])
        g[0] += 1
        g[1] += e - s
    busy = sum(e - s for s, e, _, _ in rows)
    span = rows[-1][1] - rows[0][0]
    print(f"# {os.path.basename(src)}: {len(rows)} dispatches of library kernels, busy {busy / 1e6:.3f} ms of a span of {span / 1e6:.3f} ms "
          f"({100.0 * busy / span:.1f} %)")
    print(f"{'kernel':<64} {'workgroups':>10} {'calls':>7} {'avg_us':>9} {'total_ms':>9} {'% busy':>7}")
    for (name, wgs), (calls, ns) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        print(f"{name[:64]:<64} {wgs:>10} {calls:>7} {ns / calls / 1e3:>9.2f} {ns / 1e6:>9.3f} {100.0 * ns / busy:>7.2f}")


if __name__ == "__main__":
    main()
