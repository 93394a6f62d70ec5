"""Times the temporal KL-VAE decoder of SVD's decode_latents on one GPU: the HIP plan (ctrl_adapter_amd.AutoencoderKLTemporalDecoder, fp16
weights, fp32 stream) against the fp32 restatement (tests/vae_tdecoder_ref.py) in fp32 and in fp16 on torch-ROCm (eager), same weights
(synthetic.seeded_init, distinct mix factors), same GPU, same run.  A case is one clip of 14 frames decoded in chunks (decode_chunk_size),
every chunk as one clip, as the pipeline does.  Device events, warm-up, runs alternated in rounds; prints the median and the spread (min ..
max over rounds) per case, the rel-inf error of the frames against the fp32 restatement for the HIP plan and for torch fp16 on the same
input, and the device memory the first HIP forward took (the workspace its dry pass asked for + the output).  The first step times the
time-conv kernel alone through ctrl_op_vae_time_conv as bytes over time.

Every case runs in a process of its own under its own time limit, and a case is only started when the one before it ended well:

    python tools/vae_tdecoder_bench.py [--rounds 3] [--iters 1] [--out profiles/vae_tdecoder_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# (frames, latent h, latent w, decode_chunk_size): 14 frames at 320 x 512 and at 576 x 1024 (SVD's default clip), chunks of 14 and 8
CASES = [(14, 40, 64, 14), (14, 40, 64, 8), (14, 72, 128, 14), (14, 72, 128, 8)]
# (a fresh machine has no MIOpen kernel cache: torch's first pass over the restatement's conv shapes, fp32 and fp16, builds it and takes
# minutes in EVERY process, 150 .. 165 s per dtype at 320 x 512 -- run_case reports where its time goes on stderr; at 576 x 1024 that pass
# has not finished inside these limits on an MI355X: profiles/vae_tdecoder_bench.txt)
LIMIT_S = [900, 420, 600, 420]
HEADER = "%-22s %-28s %-28s %-28s %-9s %-9s %-9s %-9s %-8s" % ("case", "HIP", "torch fp32", "torch fp16", "x fp32", "x fp16", "err HIP",
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
    import time
    import torch
    import ctrl_adapter_amd as P
    t0 = time.time()

    def note(what):
        print("[case %d +%.0f s] %s" % (i, time.time() - t0, what), file=sys.stderr, flush=True)

    from vae_decoder_ref import seeded_latents
    from vae_tdecoder_ref import SD_VAE, VaeTemporalRef, seeded_tdecoder
    dev = torch.device("cuda:0")
    ref32 = seeded_tdecoder(VaeTemporalRef, SD_VAE, 2025)
    m = P.AutoencoderKLTemporalDecoder(**SD_VAE)
    m.load_state_dict(ref32.state_dict())
    m = m.to(torch.float16).to(dev)
    ref32 = ref32.to(dev)
    ref16 = VaeTemporalRef(**SD_VAE).eval()
    ref16.load_state_dict(ref32.state_dict())
    ref16 = ref16.to(dev).half()
    Fr, h, w, chunk = CASES[i]
    note("models built")

    def torch_decode(ref, z):
        return torch.cat([ref.decode(z[k:k + chunk], z[k:k + chunk].shape[0]).sample for k in range(0, Fr, chunk)])

    def hip_decode(z):
        out = torch.empty((Fr, 3, 8 * h, 8 * w), dtype=torch.float32, device=dev)
        for k in range(0, Fr, chunk):
            n = min(chunk, Fr - k)
            m.run_decoder(z[k:k + n], n, out_dtype=torch.float32, out=out[k:k + n])
        return out

    with torch.no_grad():
        z = seeded_latents(Fr, h, w, seed=Fr * 7 + h, device=dev)
        z16 = z.half()
        runs = {"hip": lambda: hip_decode(z16), "f32": lambda: torch_decode(ref32, z), "f16": lambda: torch_decode(ref16, z16)}
        free0 = torch.cuda.mem_get_info()[0]
        runs["hip"]()
        torch.cuda.synchronize()
        ws = (free0 - torch.cuda.mem_get_info()[0]) / 2.0 ** 30          # the plan's workspace + the output, as the driver sees it
        note("first HIP forward done")
        for k in ("f32", "f16"):
            runs[k]()
            torch.cuda.synchronize()
            note("first torch %s pass done" % k)
        t = {k: [] for k in runs}
        for _ in range(rounds):
            for k, f in runs.items():
                t[k].append(timed(f, iters))
        note("timed rounds done")
        want = torch_decode(ref32, z16.float())
        e_hip, e_16 = rel_inf(runs["hip"](), want), rel_inf(runs["f16"](), want)
    med = {k: statistics.median(v) for k, v in t.items()}
    fmt = lambda k: "%.1f [%.1f .. %.1f]" % (med[k], min(t[k]), max(t[k]))      # noqa: E731
    return "%-22s %-28s %-28s %-28s %-9s %-9s %-9.2e %-9.2e %-8.2f" % (
        "F=%d %dx%d chunk %d" % (Fr, 8 * h, 8 * w, chunk), fmt("hip"), fmt("f32"), fmt("f16"), "%.2fx" % (med["f32"] / med["hip"]),
        "%.2fx" % (med["f16"] / med["hip"]), e_hip, e_16, ws)


def run_kernel(iters=20):
    """the time-conv kernel alone on 14 frames at 576 x 1024: ms per launch and the bytes it has to move (every input plane once, every
    output element once) per second"""
    import torch
    from ctrl_adapter_amd import _lib as L
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    Fr, H, W, oc = 14, 576, 1024, 3
    x = torch.randn(Fr, oc, H, W, generator=g).to(dev)
    w = (torch.randn(oc, oc, 3, generator=g) * 0.5).to(dev)
    b = torch.zeros(oc, device=dev)
    out = torch.empty(Fr * oc * H * W, device=dev)

    def run(kind, odt):
        L.check(L.lib().ctrl_op_vae_time_conv(L.ptr(x), L.ptr(w), L.ptr(b), Fr, H, W, oc, kind, L.ptr(out), L.dtype_code(odt), L.cur_stream()))

    lines = ["# the time-conv kernel alone (ctrl_op_vae_time_conv), 14 frames of 3 x 576 x 1024 fp32: ms per launch (best of 3 x %d launches) and "
             "(input bytes + output bytes) per second" % iters]
    n = Fr * oc * H * W
    for name, kind, odt, osz in (("sample fp32", L.VAE_DEC_SAMPLE, torch.float32, 4), ("sample fp16", L.VAE_DEC_SAMPLE, torch.float16, 2),
                                 ("unit", L.VAE_DEC_UNIT, torch.float16, 4), ("u8", L.VAE_DEC_U8, torch.float16, 1)):
        run(kind, odt)
        torch.cuda.synchronize()
        ms = min(timed(lambda: run(kind, odt), iters) for _ in range(3))
        lines.append("%-14s %.3f ms  %.2f TB/s  (%d MiB)" % (name, ms, n * (4.0 + osz) / ms * 1e-9, n * (4 + osz) >> 20))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, help="run this one case in this process and append its line to --out "
                                                           "(%d: the time-conv kernel alone)" % len(CASES))
    a = ap.parse_args()
    if a.case is not None:
        line = run_kernel() if a.case == len(CASES) else run_case(a.case, a.rounds, a.iters)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        return 0
    head = ["# temporal KL-VAE decoder (SVD VAE config: block_out_channels 128/256/512/512, 2 layers per block, 4 latent channels), fp16 latents, "
            "one clip of 14 frames decoded in chunks, every chunk as one clip (SVD's decode_latents)",
            "# ms per clip: median [min .. max] over %d rounds of %d calls, runs alternated; err = rel-inf of the frames vs the fp32 restatement on "
            "the same (fp16-rounded) latents; ws = device memory the first HIP forward took (the dry pass's workspace + the output)"
            % (a.rounds, a.iters), HEADER]
    print("\n".join(head), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(head) + "\n")
    for i in [len(CASES)] + list(range(len(CASES))):          # the kernel alone first: it needs none of torch's warm-up
        cmd = ["timeout", "-k", "10", str((LIMIT_S + [120])[i]), sys.executable, os.path.abspath(__file__), "--case", str(i), "--rounds", str(a.rounds),
               "--iters", str(a.iters)] + (["--out", a.out] if a.out else [])
        rc = subprocess.call(cmd)
        if rc != 0:                         # a case that failed or ran out of time ends the run: nothing more is started on the GPU
            print("case %d ended with status %d: stopping" % (i, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
