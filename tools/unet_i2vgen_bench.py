"""Times I2VGen-XL's backbone UNet on one GPU: the HIP plan (ctrl_adapter_amd.I2VGenXLUNet, fp16 module, fp32 streams) against the
restatement (tests/unet_i2vgen_ref.py) in torch fp16 eager on the same GPU, same weights, same run.  The real config --
block_out_channels (320, 640, 1280, 1280), heads of 64, 2 layers per block, cross_attention_dim 1024 -- on seeded weights (unit gain,
fp16-representable, drawn on the device); the CFG pair B = 2 of F = 16 frames at 64 x 64 latents (bench.py's i2vgen16 shape), 77 text
tokens, fp16 inputs, with the adapter's twelve + one residuals; the condition cache off and on (on: one KEEP forward, then REUSE
forwards are timed).  Device events, warm-up, runs alternated in rounds; prints the median and the spread (min .. max over rounds) per
case.  The first case also reports, on a reduced size (B = 1, F = 2, latents 16 x 16) where the fp32 restatement is affordable, the
rel-inf error of the HIP plan and of torch fp16 against it, and the HIP forward's time per kernel class (ctrl_prof_*, one kernel at a
time).

No speed-up is asserted anywhere: the parent commit has no native I2VGen-XL UNet, the torch line is the only yardstick, and the number
is recorded whichever way it falls.  Every case runs in a process of its own under its own time limit, and a case is only started when
the one before it ended well:

    python tools/unet_i2vgen_bench.py [--rounds 3] [--iters 1] [--out profiles/unet_i2vgen_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# condition cache
CASES = [False, True]
LIMIT_S = [420, 300]
B, FRAMES, LAT, TEXT = 2, 16, 64, 77
HEADER = "%-44s %-28s %-28s %-9s %-8s" % ("case", "HIP", "torch fp16", "x fp16", "ws GiB")


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


def inputs(batch, frames, lat, dev, dtype):
    """seeded_inputs on the device: tensors in `dtype`, the timestep and fps fp32"""
    import torch
    from unet_i2vgen_ref import I2VGEN, seeded_inputs
    inp = seeded_inputs(I2VGEN, batch, frames, lat, lat, seed=5 + lat, residuals="4d", text_len=TEXT)
    out = {}
    for k, v in inp.items():
        if isinstance(v, list):
            out[k] = [r.to(dev, dtype) for r in v]
        elif k in ("timestep", "fps"):
            out[k] = v.to(dev)
        else:
            out[k] = v.to(dev, dtype) if torch.is_tensor(v) else v
    return out


def run_case(i, rounds, iters):
    import time
    import torch
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from unet_i2vgen_ref import I2VGEN, seeded_unet_on_device
    t0 = time.time()

    def note(what):
        print("[case %d +%.0f s] %s" % (i, time.time() - t0, what), file=sys.stderr, flush=True)

    dev = torch.device("cuda:0")
    cache = CASES[i]
    ref = seeded_unet_on_device(I2VGEN, 2027, dev)
    with torch.device(dev):
        m = P.I2VGenXLUNet(**I2VGEN)
    m.load_state_dict(ref.state_dict())
    m = m.half()
    note("models built (%.3f G parameters)" % (sum(p.numel() for p in ref.parameters()) / 1e9))
    extra = []
    with torch.no_grad():
        if i == 0:
            small = inputs(1, 2, 16, dev, torch.float16)
            want = ref(**inputs(1, 2, 16, dev, torch.float32)).sample
            e_hip = rel_inf(m(**small).sample, want)
            note("reduced-size HIP forward done; %s" % m.selection)
        ref = ref.half()
        if i == 0:
            e_16 = rel_inf(ref(**small).sample, want)
            extra.append("# reduced size (B = 1, F = 2, latents 16 x 16, 77 text tokens, residuals): rel-inf vs the fp32 restatement  HIP %.2e  "
                         "torch fp16 %.2e" % (e_hip, e_16))
        inp = inputs(B, FRAMES, LAT, dev, torch.float16)
        m.cache_condition = cache
        runs = {"hip": lambda: m(**inp), "f16": lambda: ref(**inp)}
        runs["hip"]()                     # (with the cache on: the KEEP forward; every later one is a REUSE forward)
        torch.cuda.synchronize()
        ws = m.workspace_bytes() / 2.0 ** 30
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
    name = "B=%d F=%d %dx%d residuals, condition cache %s" % (B, FRAMES, LAT, LAT, "on" if cache else "off")
    line = "%-44s %-28s %-28s %-9s %-8.2f" % (name, fmt("hip"), fmt("f16"), "%.2fx" % (med["f16"] / med["hip"]), ws)
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
    head = ["# I2VGen-XL backbone UNet (block_out_channels 320/640/1280/1280, heads of 64, 2 layers per block, cross 1024; seeded weights), "
            "B = 2 clips of 16 frames, latents 64 x 64, 77 text tokens, fp16 module / sample / condition / residuals",
            "# ms per forward: median [min .. max] over %d rounds of %d calls, runs alternated; ws = the plan's forward workspace"
            % (a.rounds, a.iters), HEADER]
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
            msg = "# case %d (condition cache %s) ended with status %d: not measured, and nothing after it" % (i, CASES[i], rc)
            print(msg)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(msg + "\n")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
