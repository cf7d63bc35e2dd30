#!/usr/bin/env python3
"""condense_kernel_trace.py -- a rocprofv3 --kernel-trace CSV of
tools/pixel_sums_bench.py, tools/mask_bench.py, tools/pixel_times_bench.py,
tools/mask_components_bench.py or tools/background_bench.py as the compact table kept under profiles/: one row
per dispatch of the library's series kernels (name, ms, grid, VGPRs as the
profiler counts them); the torch reduce kernels that follow a map launch are
summed into one row per call, other kernels are dropped.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o pix -- python tools/pixel_sums_bench.py --reps 2 --inner 1 --warmup 1
    python tools/condense_kernel_trace.py DIR/pix_kernel_trace.csv profiles/pixel_sums/kernel_trace_4k_rgb8.csv
"""
import csv
import re
import sys

OURS = ("series_v2_kernel", "series_reduce_kernel", "series_pixels_kernel", "pixels_generic_kernel",
        "series_mask_kernel", "mask_generic_kernel", "series_times_kernel", "times_combine_kernel",
        "times_generic_kernel", "cc_rows_kernel", "cc_merge_kernel", "cc_stats_kernel", "cc_count_kernel",
        "cc_offsets_kernel", "cc_select_kernel", "cc_labels_kernel", "tr_overlap_kernel", "tr_link_kernel",
        "tr_scan_kernel", "tr_ids_kernel", "tr_keep_kernel", "series_background_kernel",
        "background_generic_kernel")


def main(src, dst):
    rows, torch_ms, torch_n, after_map = [], 0.0, 0, False

    def flush():
        nonlocal torch_ms, torch_n
        if torch_n:
            rows.append(('"torch sum of the map over t (%d reduce kernels)"' % torch_n, torch_ms, "", "", ""))
        torch_ms, torch_n = 0.0, 0

    for r in csv.DictReader(open(src)):
        k = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "at::native::reduce_kernel" in k:
            if after_map:  # the sum over t of a map leg, not the tool's own checks
                torch_ms, torch_n = torch_ms + ms, torch_n + 1
            continue
        if not any(s in k for s in OURS):
            continue
        flush()
        if "series_reduce_kernel" not in k:
            after_map = "series_v2_kernel" in k and re.search(r"series_v2_kernel<\d+, \d+, \d+, \w+, true", k) is not None
        k = re.sub(r"\(.*$", "", re.sub(r"^void ", "", k)).replace("dips::", "")
        rows.append(('"%s"' % k if "," in k else k, ms, r["Grid_Size_X"], r["Grid_Size_Y"], r["VGPR_Count"]))
    flush()
    with open(dst, "w") as f:
        f.write("kernel,duration_ms,grid_size_x,grid_size_y,vgpr_count\n")
        for row in rows:
            f.write("%s,%.3f,%s,%s,%s\n" % row)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
