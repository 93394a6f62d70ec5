"""The measurement tools that turn rocprofv3 output into the numbers bench.py quotes (`roofline.traffic`) -- run here on a
small synthetic counter dump: symbol spelling, the gfx950 FETCH_SIZE x2 correction, per-launch division, and the join of
counter rows with the library's per-launch dump by position inside a step.  CPU only."""
import csv
import importlib.util
import json
import os
import sys

from helpers import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_with_tools_path(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return _load(name)
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))


ATTN = "_ZN12_GLOBAL__N_121flash_attn_d64_kernelILi1ELi8ELi8ELi3EEEv14ctrl_attn_descPKDF16_"
GEMM = "_ZN12_GLOBAL__N_112igemm_kernelILi256ELi128ELi32ELi4ELi2ELi3ELi0ELb1EEEv15ctrl_igemm_desciiPKDF16_ii"
POOL = "_ZN12_GLOBAL__N_114avgpool_kernelEPKvPvii"


def test_symbol_spelling_matches_the_library_profiler():
    t = _load("pmc_traffic")
    assert t.symbol_of(ATTN) == "flash_attn_d64_kernel<1, 8, 8, 3>"
    assert t.symbol_of(GEMM) == "igemm_kernel<256, 128, 32, 4, 2, 3, 0, true>"
    assert t.symbol_of("void (anonymous namespace)::igemm_kernel<256,128,32,4,2,3,0,true>(ctrl_igemm_desc, int)") == \
        "igemm_kernel<256, 128, 32, 4, 2, 3, 0, true>"
    assert t.symbol_of(POOL) == "avgpool_kernel"
    assert t.kernel_class(GEMM) == "igemm_rows" and t.kernel_class(ATTN) == "flash_attn"
    assert t.kernel_class("some_torch_elementwise_kernel") is None        # torch's own kernels are not counted
    # round 6: the fused feed-forward kernel is a class of its own (left unclassified it silently dropped ~11 GB out of the step's HBM total)
    FFN = "void (anonymous namespace)::ffn512_kernel<0>((anonymous namespace)::FfnGroup, int, int)"
    assert t.kernel_class(FFN) == "ffn_fused" and t.symbol_of(FFN) == "ffn512_kernel"
    assert t.kernel_class("_ZN12_GLOBAL__N_113ffn512_kernelILi0EEEvNS_8FfnGroupEii") == "ffn_fused"


def _write_pass(directory, counter, steps):
    os.makedirs(os.path.join(directory, "host", "1"), exist_ok=True)
    with open(os.path.join(directory, "host", "1", "1_counter_collection.csv"), "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=["Dispatch_Id", "Kernel_Name", "Grid_Size", "Counter_Name", "Counter_Value"])
        wr.writeheader()
        did = 0
        for st in steps:
            for name, grid, val in st:
                did += 1
                wr.writerow(dict(Dispatch_Id=did, Kernel_Name=name, Grid_Size=grid, Counter_Name=counter, Counter_Value=val))
                wr.writerow(dict(Dispatch_Id=did, Kernel_Name=name, Grid_Size=grid, Counter_Name="OTHER", Counter_Value=1e9))


def test_traffic_json_from_a_synthetic_counter_dump(tmp_path, monkeypatch, capsys):
    t = _load("pmc_traffic")
    # two steps: avgpool, the self-attention (1000 KiB fetched as reported, 300 KiB written), the cross-attention launch of the
    # SAME symbol and grid (10 / 30 KiB), one GEMM; a torch kernel in between is ignored
    def step(f_or_w):
        a, c, g = ((1000.0, 10.0, 400.0) if f_or_w == "F" else (300.0, 30.0, 800.0))
        return [(POOL, 4096, 1.0), (ATTN, 1310720, a), ("at_native_copy_kernel", 64, 7777.0), (ATTN, 1310720, c), (GEMM, 524288, g)]
    fdir, wdir = str(tmp_path / "f"), str(tmp_path / "w")
    _write_pass(fdir, "FETCH_SIZE", [step("F"), step("F")])
    _write_pass(wdir, "WRITE_SIZE", [step("W"), step("W")])
    tsv = tmp_path / "launches.tsv"
    with open(tsv, "w") as fh:
        for _ in range(2):
            fh.write("0\t0\t0\t\tavgpool_kernel\t0.01\n")
            fh.write("0\t0\t0\tB8 h5 D64 Lq16384 Lk16384\tflash_attn_d64_kernel<1, 8, 8, 3>\t2.7\n")
            fh.write("0\t0\t0\tB8 h5 D64 Lq16384 Lk77\tflash_attn_d64_kernel<1, 8, 8, 3>\t0.06\n")
            fh.write("0\t0\t0\tM131072 N4096 K512 taps1 geglu\tigemm_kernel<256, 128, 32, 4, 2, 3, 0, true>\t0.77\n")
    out = tmp_path / "traffic.json"
    monkeypatch.setattr(sys, "argv", ["pmc_traffic.py", fdir, wdir, "2", str(out), str(tsv)])
    t.main()
    capsys.readouterr()
    doc = json.load(open(out))
    # per class: FETCH x2 + WRITE, KiB -> bytes, per step / per launch
    fa = doc["classes"]["flash_attn"]
    assert fa["launches_per_step"] == 2.0
    assert fa["hbm_bytes_per_step_corrected"] == round((2 * 1010.0 + 330.0) * 1024)
    assert doc["classes"]["igemm_rows"]["hbm_bytes_per_launch_corrected"] == round((2 * 400.0 + 800.0) * 1024)
    assert "avgpool" in doc["classes"] and len(doc["classes"]) == 3
    # per (symbol, grid): the two attention launches cannot be told apart ...
    k = doc["kernels"]["flash_attn_d64_kernel<1, 8, 8, 3>|1310720"]
    assert k["launches_per_step"] == 2.0 and k["hbm_bytes_per_launch_corrected"] == round((2 * 505.0 + 165.0) * 1024)
    # ... the join with the per-launch dump can: this is the entry bench.py's roofline.traffic looks up
    s = doc["kernels_by_shape"]["flash_attn_d64_kernel<1, 8, 8, 3> B8 h5 D64 Lq16384 Lk16384"]
    assert s["hbm_bytes_per_launch_corrected"] == round((2 * 1000.0 + 300.0) * 1024)
    x = doc["kernels_by_shape"]["flash_attn_d64_kernel<1, 8, 8, 3> B8 h5 D64 Lq16384 Lk77"]
    assert x["hbm_bytes_per_launch_corrected"] == round((2 * 10.0 + 30.0) * 1024)
    assert doc["total_hbm_bytes_per_step_corrected"] == sum(c["hbm_bytes_per_step_corrected"] for c in doc["classes"].values())


def test_committed_traffic_file_is_what_bench_reads():
    """the committed PMC summary resolves the headline kernel of the committed bench line (same spelling on both sides)"""
    import glob
    tf = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic*.json")))[-1]
    # (the bench line of the profile call itself precedes its PMC passes; the HEAD check taken afterwards carries the look-up)
    bf = os.path.join(ROOT, "profiles", os.path.basename(tf).split("_pmc_")[0] + "_bench_head_check.json")
    if not os.path.exists(bf):
        import pytest
        pytest.skip("no bench line taken after the PMC passes of " + os.path.basename(tf))
    doc = json.load(open(tf))
    line = json.loads(open(bf).read().strip().splitlines()[-1])
    roof = line["roofline"]
    ent = doc["kernels_by_shape"][roof["kernel"]]
    assert ent["hbm_bytes_per_launch_corrected"] == roof["traffic"]
    assert roof["traffic_source"] == os.path.basename(tf)
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3


def test_kernel_trace_summary_on_a_synthetic_trace(tmp_path, monkeypatch, capsys):
    """per (symbol, grid) durations of a rocprofv3 --kernel-trace run: the file the bench line's avg_launch_ms is checked against"""
    os.makedirs(tmp_path / "t" / "host", exist_ok=True)
    with open(tmp_path / "t" / "host" / "9_kernel_trace.csv", "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=["Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Start_Timestamp", "End_Timestamp"])
        wr.writeheader()
        t0 = 1000
        for _ in range(3):                     # three steps: two attention launches of 2.0 / 3.0 ms, one GEMM of 0.5 ms, a torch kernel
            for name, gx, ns in ((ATTN, 1310720, 2_000_000), (ATTN, 1310720, 3_000_000), (GEMM, 524288, 500_000), ("torch_fill", 64, 9_000_000)):
                wr.writerow(dict(Kernel_Name=name, Grid_Size_X=gx, Grid_Size_Y=1, Grid_Size_Z=1, Start_Timestamp=t0, End_Timestamp=t0 + ns))
                t0 += ns + 10
    out = tmp_path / "per_kernel.csv"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        k = _load("kernel_trace_summary")
        monkeypatch.setattr(sys, "argv", ["kernel_trace_summary.py", str(tmp_path / "t"), "3", str(out)])
        k.main()
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    capsys.readouterr()
    rows = list(csv.DictReader(open(out)))
    assert [r["symbol"] for r in rows] == ["flash_attn_d64_kernel<1, 8, 8, 3>", "igemm_kernel<256, 128, 32, 4, 2, 3, 0, true>"]   # by total time
    a = rows[0]
    assert int(a["calls"]) == 6 and float(a["calls_per_step"]) == 2.0
    assert float(a["avg_ms"]) == 2.5 and float(a["min_ms"]) == 2.0 and float(a["max_ms"]) == 3.0 and float(a["ms_per_step"]) == 5.0
    assert float(rows[1]["avg_ms"]) == 0.5 and int(rows[1]["grid_work_items"]) == 524288


def test_isa_mix_classifier_and_block_split():
    m = _load_with_tools_path("isa_mix")
    assert m.classify("v_mfma_f32_32x32x16_f16") == "mfma" and m.classify("v_exp_f32_e32") == "valu_trans"
    assert m.classify("v_cvt_pk_f16_f32") == "valu" and m.classify("ds_read_b128") == "lds"
    assert m.classify("global_load_lds_dwordx4") == "lds_dma" and m.classify("global_store_dwordx4") == "vmem"
    assert m.classify("scratch_load_dword") == "spill" and m.classify("s_waitcnt") == "s_waitcnt" and m.classify("s_add_i32") == "salu"
    asm = "\n_ZN12_GLOBAL__N_114avgpool_kernelEPKvPvii: ; @x\n\ts_load_dword s0, s[0:1], 0\n.LBB0_1:\n\tv_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]\n" \
          "\tv_add_f32_e32 v1, v2, v3\n\ts_cbranch_scc1 .LBB0_1\n.Lfunc_end0:\n\t.amdhsa_kernel x\namdhsa.kernels:\n  - .agpr_count: 0\n" \
          "    .group_segment_fixed_size: 0\n    .name: _ZN12_GLOBAL__N_114avgpool_kernelEPKvPvii\n    .private_segment_fixed_size: 0\n" \
          "    .sgpr_count: 10\n    .vgpr_count: 12\n"
    bodies, meta = m.kernels(asm)
    assert list(bodies) == ["_ZN12_GLOBAL__N_114avgpool_kernelEPKvPvii"] and "v_mfma" in bodies[list(bodies)[0]]
    assert meta["_ZN12_GLOBAL__N_114avgpool_kernelEPKvPvii"]["vgpr_count"] == 12


def _synthetic_device_asm(kernels, cuid):
    """a device assembly file in the shape hipcc leaves behind: kernels = [(symbol, instruction)] in emission order"""
    out = ["\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n"]
    for i, (sym, ins) in enumerate(kernels):
        out.append("\t.section\t.text.%s,\"axG\",@progbits,%s,comdat\n\t.globl\t%s\n%s:\n\t%s\n.LBB%d_1:%s; in Loop: Header=BB%d_1\n"
                   "\ts_cbranch_scc1 .LBB%d_1\n.Lfunc_end%d:\n\t.amdhsa_kernel %s\n" % (sym, sym, sym, sym, ins, i, " " * (3 + i), i, i, i, sym))
    out.append("\t.section\t.AMDGPU.gpr_maximums,\"\",@progbits\n__hip_cuid_%s:\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n" % cuid)
    for sym, _ in kernels:
        out.append("  - .agpr_count:    0\n    .name:           %s\n    .vgpr_count:     12\n" % sym)
    out.append("amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")
    return "".join(out)


def test_asm_compare_ignores_emission_order_and_sees_an_instruction(tmp_path, capsys):
    m = _load("igemm_asm_compare")
    a, b, c = ("k_a", "v_add_f32_e32 v1, v2, v3"), ("k_b", "v_mul_f32_e32 v1, v2, v3"), ("k_b", "v_mul_f32_e32 v1, v2, v4")
    files = {}
    for name, ks, cuid in (("parent", [a, b], "11aa"), ("moved", [b, a], "22bb"), ("changed", [a, c], "11aa"), ("fewer", [a], "11aa")):
        files[name] = str(tmp_path / (name + ".s"))
        with open(files[name], "w") as fh:
            fh.write(_synthetic_device_asm(ks, cuid))
    assert m.main(files["parent"], files["parent"]) == 0
    assert m.main(files["parent"], files["moved"]) == 0 and "same order: False" in capsys.readouterr().out
    assert m.main(files["parent"], files["changed"]) == 1 and "DIFFERS: k_b" in capsys.readouterr().out
    assert m.main(files["parent"], files["fewer"]) == 1
