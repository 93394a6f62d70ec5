"""Times SDXL's backbone UNet on one GPU: the HIP plan (ctrl_adapter_amd.UNet2DConditionModel, fp16 module, fp32 streams) against the
restatement (tests/unet_sdxl_ref.py) in torch fp16 eager on the same GPU, same weights, same run.  The real SDXL-base config --
block_out_channels (320, 640, 1280), heads (5, 10, 20), transformer depth (1, 2, 10), 2 layers per block, cross_attention_dim 2048,
text_time 1280 + 6 x 256 -- on seeded weights (unit gain, fp16-representable, drawn on the device); latents 128 x 128, 77 keys, fp16
inputs; B = 2 (the CFG pair) without and with the adapter's nine + one residuals, with the text K/V cache off and on, and B = 8.
Device events, warm-up, runs alternated in rounds; prints the median and the spread (min .. max over rounds) per case.  The first case
also reports, on a reduced size (B = 1, latents 16 x 16) where the fp32 restatement is affordable, the rel-inf error of the HIP plan
and of torch fp16 against it, and the HIP forward's time per kernel class (ctrl_prof_*, one kernel at a time).

No speed-up is asserted anywhere: the parent commit has no native SDXL UNet, the torch line is the only yardstick, and the number is
recorded whichever way it falls.  Every case runs in a process of its own under its own time limit, and a case is only started when the
one before it ended well:

    python tools/unet_sdxl_bench.py [--rounds 3] [--iters 1] [--out profiles/unet_sdxl_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# (batch, with residuals, text cache)
CASES = [(2, False, False), (2, True, False), (2, True, True), (8, True, False)]
LIMIT_S = [420, 300, 300, 300]
LAT, KEYS = 128, 77
HEADER = "%-34s %-28s %-28s %-9s %-8s" % ("case", "HIP", "torch fp16", "x fp16", "ws GiB")


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


def inputs(batch, lat, res, dev, dtype):
    """make_inputs on the device: the sample, states, text_embeds and residuals in `dtype`, the timestep and the time ids fp32"""
    from unet_sdxl_ref import SDXL, make_inputs
    inp = make_inputs(SDXL, batch, lat, lat, keys=KEYS, seed=5 + lat, residuals=res)
    out = dict(sample=inp["sample"].to(dev, dtype), timestep=inp["timestep"].to(dev), encoder_hidden_states=inp["encoder_hidden_states"].to(dev, dtype),
               added_cond_kwargs=dict(text_embeds=inp["added_cond_kwargs"]["text_embeds"].to(dev, dtype),
                                      time_ids=inp["added_cond_kwargs"]["time_ids"].to(dev)))
    if res:
        out["down_block_additional_residuals"] = [r.to(dev, dtype) for r in inp["down_block_additional_residuals"]]
        out["mid_block_additional_residual"] = inp["mid_block_additional_residual"].to(dev, dtype)
    return out


def run_case(i, rounds, iters):
    import time
    import torch
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from unet_sdxl_ref import SDXL, seeded_unet_on_device
    t0 = time.time()

    def note(what):
        print("[case %d +%.0f s] %s" % (i, time.time() - t0, what), file=sys.stderr, flush=True)

    dev = torch.device("cuda:0")
    batch, res, cache = CASES[i]
    ref = seeded_unet_on_device(SDXL, 2026, dev)
    with torch.device(dev):
        m = P.UNet2DConditionModel(**SDXL)
    m.load_state_dict(ref.state_dict())
    m = m.half()
    m.cache_text = cache
    note("models built (%.3f G parameters)" % (sum(p.numel() for p in ref.parameters()) / 1e9))
    extra = []
    with torch.no_grad():
        if i == 0:
            small = inputs(1, 16, True, dev, torch.float16)
            want = ref(**inputs(1, 16, True, dev, torch.float32)).sample
            e_hip = rel_inf(m(**small).sample, want)
            note("reduced-size HIP forward done; %s" % m.selection)
        ref = ref.half()
        if i == 0:
            e_16 = rel_inf(ref(**small).sample, want)
            extra.append("# reduced size (B = 1, latents 16 x 16, 77 keys, residuals): rel-inf vs the fp32 restatement  HIP %.2e  torch fp16 %.2e"
                         % (e_hip, e_16))
        inp = inputs(batch, LAT, res, dev, torch.float16)
        runs = {"hip": lambda: m(**inp), "f16": lambda: ref(**inp)}
        runs["hip"]()
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
    name = "B=%d 128x128 %s, text cache %s" % (batch, "residuals" if res else "plain", "on" if cache else "off")
    line = "%-34s %-28s %-28s %-9s %-8.2f" % (name, fmt("hip"), fmt("f16"), "%.2fx" % (med["f16"] / med["hip"]), ws)
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
    head = ["# SDXL backbone UNet (block_out_channels 320/640/1280, heads 5/10/20, transformer depth 1/2/10, 2 layers per block, cross 2048, "
            "text_time 2816; seeded weights), latents 128 x 128, 77 keys, fp16 module / sample / states / residuals",
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
            msg = "# case %d (%s) ended with status %d: not measured, and nothing after it" % (i, CASES[i], rc)
            print(msg)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(msg + "\n")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
