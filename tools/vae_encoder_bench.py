"""Times the KL-VAE encoder of the SVD / I2VGen-XL image latents on one GPU: the HIP plan (ctrl_adapter_amd.AutoencoderKLEncoder, fp16
operands, fp32 stream) against the fp32 restatement (tests/vae_encoder_ref.py) in fp32 -- what the SVD pipeline runs under force_upcast --
and in fp16, on torch-ROCm (eager), same weights (synthetic.seeded_init), same GPU, same run.  Device events, warm-up, runs alternated in
rounds; prints the median and the spread (min .. max over rounds) per case, the rel-inf error of latent_dist.mode() against the fp32
restatement, and the HIP plan's per-class times from the kernel profiler (ctrl_prof_*) with the achieved TFLOP/s against the encoder's
FLOP count (1.117 TFLOP per 512^2 image, 2.609 at 576 x 1024).

    python tools/vae_encoder_bench.py [--rounds 5] [--iters 5] [--out profiles/vae_encoder_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CASES = [(1, 512, 512), (2, 512, 512), (8, 512, 512), (1, 576, 1024)]
TFLOP_PER_IMAGE = {(512, 512): 1.117, (576, 1024): 2.609}


def timed(fn, iters):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from ctrl_adapter_amd.synthetic import seeded_init
    from vae_encoder_ref import SD_VAE, VaeEncoderRef, seeded_pixels
    dev = torch.device("cuda:0")
    ref32 = seeded_init(VaeEncoderRef(**SD_VAE), seed=2024).eval()
    m = P.AutoencoderKLEncoder(**SD_VAE)
    m.load_state_dict(ref32.state_dict())
    m = m.to(torch.float16).to(dev)
    ref32 = ref32.to(dev)
    ref16 = VaeEncoderRef(**SD_VAE).eval()
    ref16.load_state_dict(ref32.state_dict())
    ref16 = ref16.to(dev).half()
    lines = ["# KL-VAE encoder (SD / SVD VAE: block_out_channels 128/256/512/512, 2 layers, 4 latent channels) on %s" % torch.cuda.get_device_name(0),
             "# ms per call: median [min .. max] over %d rounds of %d calls, runs alternated; err = rel-inf of latent_dist.mode() vs the fp32 "
             "restatement" % (a.rounds, a.iters),
             "%-14s %-26s %-26s %-26s %-10s %-10s %-9s %-9s" % ("case", "HIP", "torch fp32", "torch fp16", "x fp32", "x fp16", "err HIP",
                                                                "err fp16")]
    with torch.no_grad():
        for N, H, W in CASES:
            x = seeded_pixels(N, H, W, seed=N * 7 + H, device=dev)
            x16 = x.half()
            runs = {"hip": lambda: m.run(x16), "f32": lambda: ref32.encode(x).latent_dist.mode(),
                    "f16": lambda: ref16.encode(x16).latent_dist.mode()}
            for f in runs.values():
                f()
            torch.cuda.synchronize()
            t = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, f in runs.items():
                    t[k].append(timed(f, a.iters))
            want = ref32.encode(x).latent_dist.mode()
            e_hip, e_16 = rel_inf(m.run(x16), want), rel_inf(ref16.encode(x16).latent_dist.mode(), want)
            med = {k: statistics.median(v) for k, v in t.items()}
            fmt = lambda k: "%.3f [%.3f .. %.3f]" % (med[k], min(t[k]), max(t[k]))
            lines.append("%-14s %-26s %-26s %-26s %-10s %-10s %-9.2e %-9.2e" % (
                "B=%d %dx%d" % (N, H, W), fmt("hip"), fmt("f32"), fmt("f16"), "%.2fx" % (med["f32"] / med["hip"]),
                "%.2fx" % (med["f16"] / med["hip"]), e_hip, e_16))
            torch.cuda.empty_cache()
        for N, H, W in [(1, 512, 512), (1, 576, 1024)]:
            x16 = seeded_pixels(N, H, W, seed=1, device=dev).half()
            m.run(x16)
            torch.cuda.synchronize()
            with ops.Profiler() as p:
                m.run(x16)
            torch.cuda.synchronize()
            rows = sorted(((k, v[0], v[1], v[2]) for k, v in p.rows.items()), key=lambda r: -r[1])
            total = sum(r[1] for r in rows)
            tf = TFLOP_PER_IMAGE[(H, W)] * N
            lines.append("")
            lines.append("# per-class kernel time, B=%d %dx%d (profiled launches, one at a time): total %.3f ms = %.1f TFLOP/s on %.3f TFLOP"
                         % (N, H, W, total, tf / total * 1e3, tf))
            lines.append("%-18s %10s %8s %10s %10s" % ("class", "ms", "launches", "TFLOP/s", "share"))
            for name, ms, n, flops in rows:
                lines.append("%-18s %10.3f %8d %10.1f %9.1f%%" % (name, ms, n, flops / ms * 1e-9 if ms > 0 else 0.0, 100.0 * ms / total))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
