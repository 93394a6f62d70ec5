"""Times the KL-VAE decoder of the SDXL images and the I2VGen-XL frames on one GPU: the HIP plan (ctrl_adapter_amd.AutoencoderKLDecoder,
fp16 weights, fp32 stream) against the fp32 restatement (tests/vae_decoder_ref.py) in fp32 -- what the SDXL pipeline runs under
force_upcast -- and in fp16, on torch-ROCm (eager), same weights (synthetic.seeded_init), same GPU, same run.  Device events, warm-up,
runs alternated in rounds; prints the median and the spread (min .. max over rounds) per case, and the rel-inf error of decode(z).sample
against the fp32 restatement for the HIP plan and for torch fp16 on the same input.  A last step times the two new kernels alone (the head
at 128 x 128 latents, the tail at 1024^2 with each epilogue) through their ctrl_op_* entries, and the table ends with the shapes at which
the plan is slower than torch fp16.

Every case runs in a process of its own under its own time limit, and a case is only started when the one before it ended well:

    python tools/vae_decoder_bench.py [--rounds 3] [--iters 2] [--out profiles/vae_decoder_bench.txt]

is `timeout -k 10 T python tools/vae_decoder_bench.py --case 0 --out F && timeout -k 10 T python ... --case 1 --out F && ...`."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# (images, latent h, latent w): B = 1 / 2 at 512^2, B = 1 at 1024^2, 16 frames at 704 x 1280 (I2VGen-XL's default clip)
CASES = [(1, 64, 64), (2, 64, 64), (1, 128, 128), (16, 88, 160)]
LIMIT_S = [240, 240, 300, 600]
HEADER = "%-16s %-26s %-26s %-26s %-10s %-10s %-9s %-9s %-9s" % ("case", "HIP", "torch fp32", "torch fp16", "x fp32", "x fp16", "err HIP",
                                                                 "err fp16", "ws GiB")


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


def run_case(i, rounds, iters):
    import torch
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    from vae_decoder_ref import SD_VAE, VaeDecoderRef, seeded_latents
    dev = torch.device("cuda:0")
    ref32 = seeded_init(VaeDecoderRef(**SD_VAE), seed=2024).eval()
    m = P.AutoencoderKLDecoder(**SD_VAE)
    m.load_state_dict(ref32.state_dict())
    m = m.to(torch.float16).to(dev)
    ref32 = ref32.to(dev)
    ref16 = VaeDecoderRef(**SD_VAE).eval()
    ref16.load_state_dict(ref32.state_dict())
    ref16 = ref16.to(dev).half()
    N, h, w = CASES[i]
    chunk = 4 if N > 4 else N              # torch decodes the clip four frames at a time (the activations of 16 would not pay)

    def torch_decode(ref, z):
        return torch.cat([ref.decode(z[k:k + chunk]).sample for k in range(0, N, chunk)])

    with torch.no_grad():
        z = seeded_latents(N, h, w, seed=N * 7 + h, device=dev)
        z16 = z.half()
        runs = {"hip": lambda: m.run(z16, out_dtype=torch.float32), "f32": lambda: torch_decode(ref32, z), "f16": lambda: torch_decode(ref16, z16)}
        free0 = torch.cuda.mem_get_info()[0]
        runs["hip"]()
        torch.cuda.synchronize()
        ws = (free0 - torch.cuda.mem_get_info()[0]) / 2.0 ** 30          # the plan's workspace + the output, as the driver sees it
        for k in ("f32", "f16"):
            runs[k]()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(rounds):
            for k, f in runs.items():
                t[k].append(timed(f, iters))
        want = torch_decode(ref32, z16.float())
        e_hip, e_16 = rel_inf(runs["hip"](), want), rel_inf(runs["f16"](), want)
    med = {k: statistics.median(v) for k, v in t.items()}
    fmt = lambda k: "%.2f [%.2f .. %.2f]" % (med[k], min(t[k]), max(t[k]))
    return "%-16s %-26s %-26s %-26s %-10s %-10s %-9.2e %-9.2e %-9.2f" % (
        "N=%d %dx%d" % (N, 8 * h, 8 * w), fmt("hip"), fmt("f32"), fmt("f16"), "%.2fx" % (med["f32"] / med["hip"]),
        "%.2fx" % (med["f16"] / med["hip"]), e_hip, e_16, ws)


def run_kernels(iters=20):
    """the head and the tail kernel alone at the 1024^2 shapes of the SD VAE: ms per launch and the stream bytes they move per second"""
    import torch
    from ctrl_adapter_amd import _lib as L, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    lat, h, w, Ct, C0, H, W = 4, 128, 128, 512, 128, 1024, 1024
    z = torch.randn(1, lat, h, w, generator=g).half().to(dev)
    wpq, bpq = torch.randn(lat, lat, generator=g).to(dev), torch.randn(lat, generator=g).to(dev)
    win, b_in = ops.pack_conv_w_direct((torch.randn(Ct, lat, 3, 3, generator=g) / 6).to(dev)), torch.randn(Ct, generator=g).to(dev)
    head_out = torch.empty(h * w, Ct, device=dev)
    x = torch.randn(H * W, C0, generator=g).to(dev)
    gamma, beta = torch.ones(C0, device=dev), torch.zeros(C0, device=dev)
    wout, b_out = ops.pack_conv_w_direct((torch.randn(3, C0, 3, 3, generator=g) / 34).to(dev)), torch.zeros(3, device=dev)
    st = torch.zeros(int(L.lib().ctrl_op_gn_stats_floats(1, H * W, C0, 32)), device=dev)
    L.check(L.lib().ctrl_op_gn_stats(L.ptr(x), L.F32, L.ptr(st), 1, H * W, C0, 32, L.cur_stream()))
    out = torch.empty(3 * H * W, device=dev)

    def head():
        L.check(L.lib().ctrl_op_vae_dec_head(L.ptr(z), L.dtype_code(z.dtype), 1.0, L.ptr(wpq), L.ptr(bpq), L.ptr(win), L.ptr(b_in),
                                             L.ptr(head_out), lat, h, w, h * w, Ct, L.cur_stream()))

    def tail(kind):
        L.check(L.lib().ctrl_op_vae_dec_tail(L.ptr(x), L.ptr(st), L.ptr(gamma), L.ptr(beta), 1e-6, L.ptr(wout), L.ptr(b_out), H, W, C0, 3,
                                             kind, L.ptr(out), L.dtype_code(torch.float16), L.cur_stream()))

    lines = ["# the new kernels alone (ctrl_op_vae_dec_head / _tail), ms per launch over %d launches and the fp32 stream bytes per second" % iters]
    cases = [("head 128x128 lat 4 -> 512 (writes 32 MiB)", head, h * w * Ct * 4.0)]
    cases += [("tail 1024x1024 128 -> 3 %s (reads 512 MiB)" % n, (lambda k=k: tail(k)), H * W * C0 * 4.0)
              for n, k in (("sample fp16", L.VAE_DEC_SAMPLE), ("unit", L.VAE_DEC_UNIT), ("u8", L.VAE_DEC_U8))]
    for name, fn, nbytes in cases:
        fn()
        torch.cuda.synchronize()
        ms = min(timed(fn, iters) for _ in range(3))
        lines.append("%-50s %.3f ms  %.2f TB/s" % (name, ms, nbytes / ms * 1e-9))
    return "\n".join(lines)


def slower_than_fp16(table):
    """the closing line of the table: the cases whose `x fp16` column is below 1"""
    import re
    slow = [ln.split("  ")[0].strip() for ln in table.splitlines()
            for m in [re.search(r"(\d+\.\d+)x\s+(\d+\.\d+)x", ln)] if m and float(m.group(2)) < 1.0]
    return "# slower than torch fp16: %s" % (", ".join(slow) if slow else "none of these shapes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, help="run this one case in this process and append its line to --out "
                                                           "(%d: the two new kernels alone)" % len(CASES))
    a = ap.parse_args()
    if a.case is not None:
        line = run_kernels() if a.case == len(CASES) else run_case(a.case, a.rounds, a.iters)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        return 0
    head = ["# KL-VAE decoder (SD / SDXL VAE: block_out_channels 128/256/512/512, 2 layers per block, 4 latent channels), fp16 latents",
            "# ms per call: median [min .. max] over %d rounds of %d calls, runs alternated; err = rel-inf of decode(z).sample vs the fp32 "
            "restatement on the same (fp16-rounded) latents; ws = device memory the first HIP forward took" % (a.rounds, a.iters), HEADER]
    print("\n".join(head), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(head) + "\n")
    for i in range(len(CASES) + 1):
        cmd = ["timeout", "-k", "10", str((LIMIT_S + [120])[i]), sys.executable, os.path.abspath(__file__), "--case", str(i), "--rounds", str(a.rounds),
               "--iters", str(a.iters)] + (["--out", a.out] if a.out else [])
        rc = subprocess.call(cmd)
        if rc != 0:                         # a case that failed or ran out of time ends the run: nothing more is started on the GPU
            print("case %d ended with status %d: stopping" % (i, rc))
            return rc
    if a.out:
        note = slower_than_fp16(open(a.out).read())
        print(note)
        with open(a.out, "a") as fh:
            fh.write(note + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
