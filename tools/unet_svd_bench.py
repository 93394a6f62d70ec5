"""Times SVD's backbone UNet on one GPU: the HIP plan (ctrl_adapter_amd.UNetSpatioTemporalConditionModel, fp16 module, fp32 streams)
against the restatement (tests/unet_svd_ref.py) in torch fp16 eager on the same GPU, same weights, same run.  The real SVD widths --
block_out_channels (320, 640, 1280, 1280), heads (5, 10, 20, 20), 2 layers per block, cross_attention_dim 1024 -- on seeded weights
(unit gain, fp16-representable, drawn on the device; distinct mix factors); B = 2 (the CFG pair) at F = 14 and F = 25, latents 72 x 128,
with and without the adapter's twelve + one residuals (fp16, `(b f) c h w`).  Device events, warm-up, runs alternated in rounds; prints
the median and the spread (min .. max over rounds) per case.  The first case also reports, on a reduced size (B = 1, F = 2, latents
16 x 16) where the fp32 restatement is affordable, the rel-inf error of the HIP plan and of torch fp16 against it, the HIP forward with
split ResNet operands (CTRL_UNET_SPLIT=1), and the HIP forward's time per kernel class (ctrl_prof_*, one kernel at a time).

No speed-up is asserted anywhere: the parent commit has no native UNet, the torch line is the only yardstick, and the number is
recorded whichever way it falls.  Every case runs in a process of its own under its own time limit, and a case is only started when the
one before it ended well:

    python tools/unet_svd_bench.py [--rounds 3] [--iters 1] [--out profiles/unet_svd_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SVD = dict(in_channels=8, out_channels=4, block_out_channels=(320, 640, 1280, 1280), num_attention_heads=(5, 10, 20, 20), layers_per_block=2,
           cross_attention_dim=1024, addition_time_embed_dim=256, projection_class_embeddings_input_dim=768)
# (frames, with residuals)
CASES = [(14, False), (14, True), (25, False), (25, True)]
LIMIT_S = [480, 300, 300, 300]
B, LAT_H, LAT_W = 2, 72, 128
HEADER = "%-26s %-30s %-30s %-9s %-8s" % ("case", "HIP", "torch fp16", "x fp16", "ws GiB")


def timed(fn, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def rel_inf(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def inputs(Fr, h, w, res, dev, batch=B):
    import torch
    from unet_svd_ref import seeded_inputs
    inp = seeded_inputs(SVD, batch, Fr, h, w, seed=5 * Fr + h, residuals="4d" if res else None)
    out = {}
    for k, v in inp.items():
        if isinstance(v, list):
            out[k] = [x.to(dev) for x in v]
        elif k in ("timestep", "added_time_ids"):
            out[k] = v.to(dev)
        else:
            out[k] = v.to(device=dev, dtype=torch.float16)
    return out


def run_case(i, rounds, iters):
    import time
    import torch
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from unet_svd_ref import seeded_unet_on_device
    t0 = time.time()

    def note(what):
        print("[case %d +%.0f s] %s" % (i, time.time() - t0, what), file=sys.stderr, flush=True)

    dev = torch.device("cuda:0")
    Fr, res = CASES[i]
    ref = seeded_unet_on_device(SVD, 2026, dev)

    def mirror(split=None):
        prev = ops.set_policy("CTRL_UNET_SPLIT", split) if split is not None else None
        m = P.UNetSpatioTemporalConditionModel(**SVD)
        m.load_state_dict(ref.state_dict())
        m = m.half().to(dev)
        m._ensure_plan()                      # (the policy is read when the plan is created)
        if split is not None:
            ops.set_policy("CTRL_UNET_SPLIT", prev)
        return m

    m = mirror()
    note("models built (%.2f G parameters); %s" % (sum(p.numel() for p in ref.parameters()) / 1e9, m.selection))
    extra = []
    with torch.no_grad():
        if i == 0:
            small = inputs(2, 16, 16, True, dev, batch=1)
            want = ref(**{k: ([x.float() for x in v] if isinstance(v, list) else v.float()) for k, v in small.items()}).sample
            e_hip = rel_inf(m(**small).sample, want)
            ms = mirror("1")
            e_split = rel_inf(ms(**small).sample, want)
            big = inputs(Fr, LAT_H, LAT_W, res, dev)
            ms(**big)
            torch.cuda.synchronize()
            t_split = [timed(lambda: ms(**big), iters) for _ in range(rounds)]
            del ms
            torch.cuda.empty_cache()
            note("reduced-size errors and the split-operand plan done")
        ref = ref.half()
        if i == 0:
            e_16 = rel_inf(ref(**small).sample, want)
            extra.append("# reduced size (B = 1, F = 2, latents 16 x 16, residuals): rel-inf vs the fp32 restatement  HIP %.2e  HIP split ResNet "
                         "operands %.2e  torch fp16 %.2e" % (e_hip, e_split, e_16))
            extra.append("# HIP with split ResNet operands (CTRL_UNET_SPLIT=1) at F = %d 576x1024: %.1f [%.1f .. %.1f] ms"
                         % (Fr, statistics.median(t_split), min(t_split), max(t_split)))
        inp = inputs(Fr, LAT_H, LAT_W, res, dev)
        runs = {"hip": lambda: m(**inp), "f16": lambda: ref(**inp)}
        free0 = torch.cuda.mem_get_info()[0]
        runs["hip"]()
        torch.cuda.synchronize()
        ws = (free0 - torch.cuda.mem_get_info()[0]) / 2.0 ** 30
        note("first HIP forward done")
        runs["f16"]()
        torch.cuda.synchronize()
        note("first torch fp16 pass done")
        t = {k: [] for k in runs}
        for _ in range(rounds):
            for k, f in runs.items():
                t[k].append(timed(f, iters))
        note("timed rounds done")
        if i == 0:
            with ops.Profiler() as prof:
                runs["hip"]()
            rows = sorted(prof.rows.items(), key=lambda kv: -kv[1][0])
            extra.append("# HIP forward per kernel class, one kernel at a time (ms, launches): " +
                         "  ".join("%s %.1f (%d)" % (k, v[0], v[1]) for k, v in rows))
    med = {k: statistics.median(v) for k, v in t.items()}
    fmt = lambda k: "%.1f [%.1f .. %.1f]" % (med[k], min(t[k]), max(t[k]))      # noqa: E731
    line = "%-26s %-30s %-30s %-9s %-8.2f" % ("F=%d 576x1024 %s" % (Fr, "residuals" if res else "plain"), fmt("hip"), fmt("f16"),
                                             "%.2fx" % (med["f16"] / med["hip"]), ws)
    return "\n".join([line] + extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, help="run this one case in this process and append its lines to --out")
    a = ap.parse_args()
    if a.case is not None:
        line = run_case(a.case, a.rounds, a.iters)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        return 0
    head = ["# SVD backbone UNet (block_out_channels 320/640/1280/1280, heads 5/10/20/20, 2 layers per block, cross 1024; seeded weights), "
            "B = 2 clips, latents 72 x 128, fp16 sample / states / residuals",
            "# ms per forward: median [min .. max] over %d rounds of %d calls, runs alternated; ws = device memory the first HIP forward took "
            "(the dry pass's workspace + the output)" % (a.rounds, a.iters), HEADER]
    print("\n".join(head), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(head) + "\n")
    for i in range(len(CASES)):
        cmd = ["timeout", "-k", "10", str(LIMIT_S[i]), sys.executable, os.path.abspath(__file__), "--case", str(i), "--rounds", str(a.rounds),
               "--iters", str(a.iters)] + (["--out", a.out] if a.out else [])
        rc = subprocess.call(cmd)
        if rc != 0:                         # a case that failed or ran out of time ends the run: nothing more is started on the GPU
            msg = "# case %d (F = %d, %s) ended with status %d: not measured, and nothing after it" % (i, CASES[i][0], "residuals" if CASES[i][1] else "plain", rc)
            print(msg)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(msg + "\n")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
