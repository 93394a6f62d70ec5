"""Times the PiDiNet annotator (ctrl_adapter_amd.PidiNetDetector, csrc/pidinet.hip) on one GPU: 16 frames of 512 x 512, soft edge and
scribble, frames already on the device, against the restatement's torch module (tests/pidinet_ref.py: PiDiNetRef, which computes every
pixel-difference convolution on the fly, as controlnet_aux does) cast to fp16 and run by PyTorch on the same GPU in the same run, all
frames in one batch, the two sides alternated (no scribble tail on the baseline: cv2 does that on the host in the reference, and cv2 is
not installed here).  Weights are the seeded calibrated ones (no PiDiNet checkpoint exists here): time does not depend on them.

Per row: median ms over rounds, device synchronised around the host clock (a library forward ends in a stream synchronisation of its own).
Then one profiled forward (the library's HIP-event profiler, a run of its own): per kernel class and shape the time, the bytes the kernel
must move by the traffic model kept with each launch (its input and output maps once) and those bytes over the time,
beside the copy rate of the card (6.29 TB/s, a float4 copy).

    python tools/pidinet_bench.py [--frames 16] [--rounds 5] [--iters 3] [--out profiles/pidinet_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

COPY_RATE = 6.29e12


def host_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pidinet_bench.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "pidinet_bench needs a GPU: there is no fallback and no number without one"
    import ctrl_adapter_amd as P
    import pidinet_ref as R
    from ctrl_adapter_amd import ops
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    sd = R.make_state_dict(3, "calibrated")
    det = P.PidiNetDetector.from_state_dict(sd, device=dev)
    ref = R.PiDiNetRef()
    ref.load_state_dict(sd)
    ref = ref.to(dev).half()
    H = W = 512
    N = a.frames

    def baseline(frames):
        edge = ref(frames.permute(0, 3, 1, 2).flip(1).half() / 255.0)[-1]
        return (edge.float() * 255).clamp(0, 255).to(torch.uint8)[:, 0]

    frames = R.make_frames(N, N, H, W).to(dev)
    soft = det.run(frames, channels=1)
    base = baseline(frames)
    diff = (soft.int() - base.int()).abs()
    lines = ["PiDiNet annotator, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "%d frames of 512 x 512 on the device; median ms [min .. max] over %d rounds of %d calls, the two sides alternated" % (
                 N, a.rounds, a.iters),
             "baseline: tests/pidinet_ref.py PiDiNetRef .half() (PDC on the fly), one batch, no scribble tail", "",
             "library vs baseline soft map: max |diff| %d, mean %.3f levels; workspace of one group of frames %.0f MB" % (
                 int(diff.max()), float(diff.float().mean()), det.workspace_bytes(N, H, W) / 2 ** 20)]
    for scribble in (False, True):
        lib_t, base_t = [], []
        for _ in range(a.rounds):
            lib_t.append(host_ms(lambda: det.run(frames, scribble=scribble), a.iters))
            base_t.append(host_ms(lambda: baseline(frames), a.iters))
        lm, bm = statistics.median(lib_t), statistics.median(base_t)
        lines.append("%-9s library %8.3f [%.3f .. %.3f] ms   baseline %8.3f [%.3f .. %.3f] ms   library / baseline %.2f   %.3f ms per frame" % (
            "scribble" if scribble else "softedge", lm, min(lib_t), max(lib_t), bm, min(base_t), max(base_t), lm / bm, lm / N))
    lines += ["", "one profiled soft-edge forward (HIP events around every launch; a run of its own, slower than the rows above):",
              "%-62s %3s %9s %10s %9s %7s" % ("kernel | shape", "n", "ms", "model MB", "GB/s", "% copy")]
    with ops.Profiler() as prof:
        det.run(frames)
    torch.cuda.synchronize()
    tot_ms = tot_b = 0.0
    for key, r in prof.per_kernel().items():
        ms, by = r["ms_per_step"], r["bytes_per_launch"] * r["launches_per_step"]
        tot_ms += ms
        tot_b += by
        name = key.replace("(anonymous namespace)::", "")
        lines.append("%-62s %3d %9.3f %10.1f %9.0f %6.1f%%" % (name[:62], r["launches_per_step"], ms, by / 1e6, by / (ms * 1e-3) / 1e9 if ms > 0 else 0,
                                                               100 * by / (ms * 1e-3) / COPY_RATE if ms > 0 else 0))
    lines.append("%-62s %3s %9.3f %10.1f %9.0f %6.1f%%" % ("sum of the kernels", "", tot_ms, tot_b / 1e6, tot_b / (tot_ms * 1e-3) / 1e9,
                                                           100 * tot_b / (tot_ms * 1e-3) / COPY_RATE))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
