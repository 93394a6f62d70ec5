"""Times the CLIP text encoder (SD-1.5 shape, L = 77) on one GPU: the HIP plan (ctrl_adapter_amd.CLIPTextModel, fp16) against
transformers' CLIPTextModel in fp16 on torch-ROCm (eager), same weights, same GPU, same run.  Device events, warm-up, A/B runs
alternated in rounds; prints the median and the spread (min .. max over rounds) per batch, the fp16 error of both against the fp32
restatement (tests/clip_text_ref.py, at B = 2), and the HIP plan's per-class times from the kernel profiler (ctrl_prof_*).

    python tools/text_encoder_bench.py [--batches 1,2,16] [--rounds 7] [--iters 20] [--out profiles/text_encoder_bench.txt]

Without transformers the baseline is skipped with a message."""
import argparse
import os
import statistics
import sys

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
    ap.add_argument("--batches", default="1,2,16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from ctrl_adapter_amd.synthetic import seeded_init
    from clip_text_ref import CLIPTextRef, SD15, seeded_ids
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ref = seeded_init(CLIPTextRef(**SD15).eval(), seed=41)
    sd = ref.state_dict()
    hip = P.CLIPTextModel(**SD15)
    hip.load_state_dict(sd)
    hip = hip.to(dev, torch.float16)
    hf = None
    try:
        from transformers import CLIPTextConfig, CLIPTextModel
        c = CLIPTextConfig(vocab_size=SD15["vocab_size"], hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                           num_attention_heads=12, max_position_embeddings=77, eos_token_id=2, bos_token_id=0, pad_token_id=1)
        hf = CLIPTextModel(c).eval()
        prefixed = any(k.startswith("text_model.") for k in hf.state_dict())
        hf.load_state_dict({(k if prefixed else k[len("text_model."):]): v for k, v in sd.items()})
        hf = hf.to(dev, torch.float16)
        say("baseline: transformers %s CLIPTextModel fp16, attention %s" % (__import__("transformers").__version__,
                                                                             getattr(hf.config, "_attn_implementation", "?")))
    except ImportError:
        say("baseline skipped: transformers is not installed")
    say("device: %s" % torch.cuda.get_device_name(0))

    ids2 = seeded_ids(2, 77, SD15["vocab_size"], seed=3)
    want = ref(ids2)
    err = lambda x, y: ((x.float().cpu() - y).abs().max() / y.abs().max()).item()      # noqa: E731
    o = hip(ids2.to(dev))
    say("fp16 error vs fp32 restatement (B = 2): HIP last %.2e pooled %.2e" % (err(o[0], want[0]), err(o[1], want[1])))
    if hf is not None:
        o = hf(ids2.to(dev))
        say("                                     transformers last %.2e pooled %.2e" % (err(o.last_hidden_state, want[0]),
                                                                                          err(o.pooler_output, want[1])))

    say("%-4s %-14s %10s %22s" % ("B", "path", "median ms", "spread (min..max) ms"))
    for B in [int(b) for b in a.batches.split(",")]:
        ids = seeded_ids(B, 77, SD15["vocab_size"], seed=B).to(dev)
        runs = {"hip": lambda: hip(ids)}
        if hf is not None:
            runs["transformers"] = lambda: hf(ids)
        for f in runs.values():          # warm-up (plan creation, workspace, kernels loaded)
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for r in range(a.rounds):       # alternated A / B rounds
            order = list(runs) if r % 2 == 0 else list(runs)[::-1]
            for k in order:
                t[k].append(timed(runs[k], a.iters))
        for k, v in t.items():
            say("%-4d %-14s %10.3f %12.3f .. %.3f" % (B, k, statistics.median(v), min(v), max(v)))
        if "transformers" in t:
            say("%-4d speed-up       %10.2fx" % (B, statistics.median(t["transformers"]) / statistics.median(t["hip"])))
        with ops.Profiler() as p:
            hip(ids)
        torch.cuda.synchronize()
        tot = sum(v[0] for v in p.rows.values())
        say("     HIP per class (profiled, serialised launches: %d launches, %.3f ms):" % (sum(v[1] for v in p.rows.values()), tot))
        for name, (ms, n, fl, by) in sorted(p.rows.items(), key=lambda kv: -kv[1][0]):
            say("       %-14s %3d launches %8.3f ms  %7.1f TFLOP/s  %7.1f GB/s" % (name, n, ms, fl / ms / 1e9 if ms else 0, by / ms / 1e6 if ms else 0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
