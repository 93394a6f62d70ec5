"""Times the CLIP ViT-H/14 image encoder of SVD / I2VGen-XL on one GPU: the HIP plan (ctrl_adapter_amd.CLIPVisionModelWithProjection,
fp16) with gemm_form 0 (pinned GEMM) and gemm_form 1 (the few-row split-K GEMM) against transformers' CLIPVisionModelWithProjection in
fp16 on torch-ROCm (eager), same weights, same GPU, same run.  Device events, warm-up, runs alternated in rounds; prints the median and
the spread (min .. max over rounds) per batch, the fp16 error of each against the fp32 restatement (tests/clip_vision_ref.py, B = 1),
and the HIP plan's per-class times from the kernel profiler (ctrl_prof_*).  Then the whole SVD image encoding from a 576 x 1024 PIL
image (host wall clock, synchronised): encode_svd_image on the mirror against the pipeline's CPU preprocessing (restated) plus the
transformers tower.

    python tools/vision_encoder_bench.py [--batches 1,2,8] [--rounds 7] [--iters 20] [--out profiles/vision_encoder_bench.txt]

Without transformers the baseline is skipped with a message."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from ctrl_adapter_amd.synthetic import seeded_init
    from clip_vision_ref import VIT_H, CLIPVisionRef, seeded_pixels, svd_preprocess
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ref = seeded_init(CLIPVisionRef(**VIT_H).eval(), seed=47)
    sd = ref.state_dict()
    hips = {}
    for form in (0, 1):
        m = P.CLIPVisionModelWithProjection(**VIT_H, gemm_form=form)
        m.load_state_dict(sd)
        hips["hip form %d" % form] = m.to(dev, torch.float16)
    hf = None
    try:
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
        c = CLIPVisionConfig(**{k: v for k, v in VIT_H.items()})
        hf = CLIPVisionModelWithProjection(c).eval()
        hf.load_state_dict(dict(sd, **{k: v for k, v in hf.state_dict().items() if k.endswith("position_ids")}))
        hf = hf.to(dev, torch.float16)
        say("baseline: transformers %s CLIPVisionModelWithProjection fp16, attention %s" % (
            __import__("transformers").__version__, getattr(hf.config, "_attn_implementation", "?")))
    except ImportError:
        say("baseline skipped: transformers is not installed")
    say("device: %s" % torch.cuda.get_device_name(0))

    px1 = seeded_pixels(1, 224, seed=3)
    want = ref.to(dev)(px1.to(dev))
    ref.cpu()
    err = lambda x, y: ((x.float() - y).abs().max() / y.abs().max()).item()      # noqa: E731
    for k, m in hips.items():
        o = m(px1.half().to(dev))
        say("fp16 error vs fp32 restatement (B = 1): %-12s image_embeds %.2e last %.2e" % (
            k, err(o.image_embeds, want.image_embeds), err(o.last_hidden_state, want.last_hidden_state)))
    if hf is not None:
        o = hf(px1.half().to(dev))
        say("fp16 error vs fp32 restatement (B = 1): %-12s image_embeds %.2e last %.2e" % (
            "transformers", err(o.image_embeds, want.image_embeds), err(o.last_hidden_state, want.last_hidden_state)))
    del want

    say("%-4s %-14s %10s %22s" % ("B", "path", "median ms", "spread (min..max) ms"))
    for B in [int(b) for b in a.batches.split(",")]:
        px = seeded_pixels(B, 224, seed=B).half().to(dev)
        runs = {k: (lambda m=m: m(px)) for k, m in hips.items()}
        if hf is not None:
            runs["transformers"] = lambda: hf(px)
        for f in runs.values():          # warm-up (plan creation, workspace, kernels loaded)
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for r in range(a.rounds):       # alternated rounds
            order = list(runs) if r % 2 == 0 else list(runs)[::-1]
            for k in order:
                t[k].append(timed(runs[k], a.iters))
        for k, v in t.items():
            say("%-4d %-14s %10.3f %12.3f .. %.3f" % (B, k, statistics.median(v), min(v), max(v)))
        if "transformers" in t:
            for k in hips:
                say("%-4d speed-up %-4s %10.2fx" % (B, k[-6:], statistics.median(t["transformers"]) / statistics.median(t[k])))
        for k, m in hips.items():
            with ops.Profiler() as p:
                m(px)
            torch.cuda.synchronize()
            tot = sum(v[0] for v in p.rows.values())
            say("     %s per class (profiled, serialised launches: %d launches, %.3f ms):" % (k, sum(v[1] for v in p.rows.values()), tot))
            for name, (ms, n, fl, by) in sorted(p.rows.items(), key=lambda kv: -kv[1][0]):
                say("       %-16s %3d launches %8.3f ms  %7.1f TFLOP/s  %7.1f GB/s" % (name, n, ms, fl / ms / 1e9 if ms else 0,
                                                                                    by / ms / 1e6 if ms else 0))

    # the whole SVD image encoding from a PIL image
    import PIL.Image
    arr = np.random.default_rng(1).integers(0, 256, (576, 1024, 3), dtype=np.uint8)
    img = PIL.Image.fromarray(arr)
    mirror = hips["hip form 0"]
    mean, std = P.vision_encoder.OPENAI_CLIP_MEAN, P.vision_encoder.OPENAI_CLIP_STD

    def hip_path():
        return P.encode_svd_image(mirror, None, img, dev, 1, True)

    def pipeline_path():
        pix = svd_preprocess(np.asarray(img)[None], mean, std)
        e = hf(pix.to(dev, torch.float16)).image_embeds.unsqueeze(1)
        return torch.cat([torch.zeros_like(e), e])

    paths = {"hip encode_svd_image": hip_path}
    if hf is not None:
        paths["cpu prep + transformers"] = pipeline_path
    for f in paths.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in paths}
    for r in range(a.rounds):
        order = list(paths) if r % 2 == 0 else list(paths)[::-1]
        for k in order:
            t0 = time.perf_counter()
            for _ in range(5):
                paths[k]()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3 / 5)
    say("SVD image encoding from a 576 x 1024 PIL image (host wall clock, B = 1, CFG):")
    for k, v in t.items():
        say("  %-24s %10.3f ms  %8.3f .. %.3f" % (k, statistics.median(v), min(v), max(v)))
    if hf is not None:
        e = (hip_path()[1].float() - pipeline_path()[1].float()).abs().max() / pipeline_path()[1].float().abs().max()
        say("  hip vs pipeline embedding: rel-inf %.2e" % e.item())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
