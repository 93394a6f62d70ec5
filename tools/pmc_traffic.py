"""Turns rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over bench.py into profiles/<round>_pmc_hbm_traffic.json.

  python tools/pmc_traffic.py <fetch_dir> <write_dir> <steps_in_run> <out.json> [<launches.tsv of the same command>]

Each directory holds the *_counter_collection.csv of ONE pass (counters are collected in their own runs, never combined
with sys/hip/hsa tracing).  Corrections follow MI355X_MICROARCH.md (HBM section): gfx950 reports FETCH_SIZE (KiB) at half
of the bytes of coalesced 16-B streams -> x2; WRITE_SIZE (KiB) is taken as is.  Kernels are grouped into the same classes
the library's profiler uses (igemm_rows / igemm_conv / igemm_temporal / flash_attn / ...).
"""
import csv
import glob
import json
import os
import re
import sys


def kernel_class(name):
    m = re.search(r"igemm_kernel<\s*\d+,\s*\d+,\s*\d+,\s*\d+,\s*\d+,\s*\d+,\s*(\d+)", name) or \
        re.search(r"igemm_kernelILi\d+ELi\d+ELi\d+ELi\d+ELi\d+ELi\d+ELi(\d+)E", name)      # demangled or mangled
    if m:
        return {"0": "igemm_rows", "1": "igemm_conv", "2": "igemm_temporal"}[m.group(1)]
    m = re.search(r"igemm8_kernel<\s*\d+,\s*(\d+)>", name) or re.search(r"igemm8_kernelILi\d+ELi(\d+)E", name)      # round 4's wide tile: <NI, MODE>
    if m:
        return {"0": "igemm_rows", "1": "igemm_conv", "2": "igemm_temporal"}[m.group(1)]
    if "ffn512_kernel" in name:          # round 6: the fused GEGLU feed-forward (csrc/ffn.hip)
        return "ffn_fused"
    for key in ("splitk_finish", "flash_attn", "temporal_attn", "gn_stats", "gn_apply", "gn_fused", "layernorm", "conv3x3_direct", "conv3x3_small_mfma",
                "linear_small", "nchw_to_nhwc", "nhwc_to_nchw", "avgpool", "sincos", "blend", "add_rowvec", "merge", "fill_zero"):
        if key in name:
            return key
    return None


def symbol_of(name):
    """rocprofv3 kernel name (mangled or demangled) -> the symbol spelling the library's profiler / bench.py uses"""
    m = re.search(r"igemm_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E(?:Lb([01])E)?", name)
    if m:
        g = m.groups()
        tf = lambda v: "true" if v == "1" else "false"
        # (9th argument: round 2's last build = persistent-workgroup form, round 3 = fused GroupNorm partial sums; older traces lack it)
        return "igemm_kernel<%s, %s, %s, %s, %s, %s, %s, %s%s>" % (g[:7] + (tf(g[7]), ", " + tf(g[8]) if g[8] is not None else ""))
    m = re.search(r"igemm8_kernelILi(\d+)ELi(\d+)E", name)
    if m:
        return "igemm8_kernel<%s, %s>" % m.groups()
    m = re.search(r"flash_attn_d64_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name)
    if m:
        return "flash_attn_d64_kernel<%s, %s, %s, %s>" % m.groups()
    m = re.search(r"flash_attn_d64p_kernelILi(\d+)E", name)
    if m:
        return "flash_attn_d64p_kernel<%s>" % m.groups()
    m = re.search(r"flash_attn_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E", name)
    if m:
        tf = lambda v: "true" if v == "1" else "false"
        return "flash_attn_kernel<%s, %s, %s, %s>" % (m.group(1), m.group(2), tf(m.group(3)), tf(m.group(4)))
    if "ffn512_kernel" in name:
        return "ffn512_kernel"
    m = re.search(r"((?:igemm8|igemm|flash_attn|flash_attn_d64|flash_attn_d64p)_kernel<[^>]*>)", name)
    if m:
        return re.sub(r",\s*", ", ", m.group(1))
    m = re.search(r"_ZN12_GLOBAL__N_1\d+([a-z0-9_]+_kernel)", name) or re.search(r"([a-z0-9_]+_kernel)", name)
    return m.group(1) if m else name


def collect_kernels(directory, counter):
    """per (symbol, grid size): grid size tells the shapes of one template instantiation apart"""
    tot, launches = {}, {}
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] != counter or kernel_class(row["Kernel_Name"]) is None:
                    continue
                k = "%s|%s" % (symbol_of(row["Kernel_Name"]), row["Grid_Size"])
                tot[k] = tot.get(k, 0.0) + float(row["Counter_Value"])
                launches[k] = launches.get(k, 0) + 1
    return tot, launches


def step_sequences(directory, counter):
    """per denoise step (a step starts with the avgpool launch of bench.py's SDXL workload): the library's kernels in
    dispatch order as (symbol, counter value)"""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] == counter and kernel_class(row["Kernel_Name"]) is not None:
                    rows.append((int(row["Dispatch_Id"]), symbol_of(row["Kernel_Name"]), float(row["Counter_Value"])))
    rows.sort()
    steps = []
    for _, sym, val in rows:
        if sym == "avgpool_kernel":
            steps.append([])
        if steps:
            steps[-1].append((sym, val))
    return steps


def shapes_from_dump(tsv):
    """the library's per-launch dump (CTRL_PROF_DUMP) of the same command: per step the (symbol, shape note) sequence"""
    steps = []
    with open(tsv) as fh:
        for line in fh:
            f = line.rstrip("\n").split("\t")
            if len(f) < 6 or f[0] == "pack":
                continue
            if f[4] == "avgpool_kernel":
                steps.append([])
            if steps:
                steps[-1].append((f[4], f[3]))
    return steps


def collect_by_shape(fetch_dir, write_dir, tsv):
    """joins the counter rows with the per-launch dump by position inside a step: exact (symbol, shape) attribution --
    grid size alone cannot tell e.g. the self-attention from the cross-attention launch of one Lq"""
    ref = shapes_from_dump(tsv)
    if not ref:
        return None
    ref = ref[-1]
    out = {}
    for d, cname, scale in ((fetch_dir, "FETCH_SIZE", 2.0), (write_dir, "WRITE_SIZE", 1.0)):
        n_ok = 0
        for st in step_sequences(d, cname):
            if len(st) != len(ref) or any(a[0] != b[0] for a, b in zip(st, ref)):
                continue                       # a step with another launch sequence (first step: plan build) is skipped
            n_ok += 1
            for (sym, val), (_, det) in zip(st, ref):
                k = (sym + " " + det).strip()
                e = out.setdefault(k, {"FETCH_SIZE": 0.0, "WRITE_SIZE": 0.0, "n_FETCH_SIZE": 0, "n_WRITE_SIZE": 0})
                e[cname] += val
                e["n_" + cname] += 1
        if n_ok == 0:
            return None
    res = {}
    for k, e in out.items():
        if e["n_FETCH_SIZE"] and e["n_WRITE_SIZE"]:
            f, w = e["FETCH_SIZE"] / e["n_FETCH_SIZE"], e["WRITE_SIZE"] / e["n_WRITE_SIZE"]
            res[k] = {"fetch_kb_per_launch": round(f), "write_kb_per_launch": round(w),
                      "hbm_bytes_per_launch_corrected": round((2.0 * f + w) * 1024.0)}
    return res


def collect(directory, counter):
    tot, launches = {}, {}
    for path in glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] != counter:
                    continue
                cls = kernel_class(row["Kernel_Name"])
                if cls is None:
                    continue
                tot[cls] = tot.get(cls, 0.0) + float(row["Counter_Value"])
                launches[cls] = launches.get(cls, 0) + 1
    return tot, launches


def main():
    fetch_dir, write_dir, steps, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    tsv = sys.argv[5] if len(sys.argv) > 5 else None
    f, fl = collect(fetch_dir, "FETCH_SIZE")
    w, _ = collect(write_dir, "WRITE_SIZE")
    classes = {}
    for cls in sorted(f):
        lps = fl[cls] / steps
        fkb, wkb = f[cls] / steps, w.get(cls, 0.0) / steps
        tot = (2.0 * fkb + wkb) * 1024.0
        classes[cls] = {"launches_per_step": lps, "fetch_kb_per_step": round(fkb), "write_kb_per_step": round(wkb),
                        "hbm_bytes_per_step_corrected": round(tot), "hbm_bytes_per_launch_corrected": round(tot / lps)}
    fk, fkl = collect_kernels(fetch_dir, "FETCH_SIZE")
    wk, _ = collect_kernels(write_dir, "WRITE_SIZE")
    kernels = {}
    for k in sorted(fk):
        n = fkl[k]
        tot = (2.0 * fk[k] + wk.get(k, 0.0)) * 1024.0
        kernels[k] = {"launches_per_step": n / steps, "fetch_kb_per_launch": round(fk[k] / n), "write_kb_per_launch": round(wk.get(k, 0.0) / n),
                      "hbm_bytes_per_launch_corrected": round(tot / n)}
    doc = {"_note": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over `CTRL_ADAPTER_LANES=1 python bench.py "
                    "--full --no-graph --no-cpu-baseline --steps 2 --warmup 1` (%d steps in total, one stream so that counters "
                    "attribute to one kernel at a time); FETCH_SIZE doubled per MI355X_MICROARCH.md section HBM (gfx950 "
                    "reports 1/2 of coalesced 16-B streams); WRITE_SIZE taken as is" % steps,
           "classes": classes,
           "kernels": kernels,       # key = "<symbol>|<grid size in work-items>" (bench.py's per_kernel rows carry both)
           # key = bench.py's `kernel` string "<symbol> <shape>": counter rows joined with the library's per-launch dump of
           # the same command by position inside a step (null when the sequences did not line up)
           "kernels_by_shape": collect_by_shape(fetch_dir, write_dir, tsv) if tsv else None,
           "total_hbm_bytes_per_step_corrected": sum(c["hbm_bytes_per_step_corrected"] for c in classes.values())}
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps({k: v["hbm_bytes_per_launch_corrected"] for k, v in classes.items()}))


if __name__ == "__main__":
    main()
