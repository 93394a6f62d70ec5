"""Times the lineart annotator (ctrl_adapter_amd.LineartDetector, csrc/lineart.hip, csrc/plan_lineart.cpp) on one GPU: 16 frames of
512 x 512, fine and coarse, frames already on the device, against the restatement's torch module (tests/lineart_ref.py: GeneratorRef,
torch's own ReflectionPad2d / Conv2d / InstanceNorm2d / ConvTranspose2d) cast to fp16 and run by PyTorch on the same GPU in the same run,
all frames in one batch, the two sides alternated.  Weights are the seeded calibrated ones (no lineart checkpoint exists here): time does
not depend on them.

Per row: every shape warmed up, then the median ms over rounds with min and max, device synchronised around the host clock (a library
forward ends in a stream synchronisation of its own).  Then one profiled fine forward (the library's HIP-event profiler, a run of its own):
per kernel class and shape the time, the algorithmic work kept with each launch and the rates it gives; the six residual convolutions'
achieved rate (about 116 of the 160 GFLOP of a frame), and the share of the time the kernels that are not GEMMs take.

    python tools/lineart_bench.py [--frames 16] [--rounds 5] [--iters 3] [--out profiles/lineart_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lineart_bench.txt"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "lineart_bench needs a GPU: there is no fallback and no number without one"
    import ctrl_adapter_amd as P
    import lineart_ref as R
    from ctrl_adapter_amd import ops
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    sds = [R.make_state_dict(3, "calibrated"), R.make_state_dict(4, "calibrated")]
    det = P.LineartDetector.from_state_dict(sds[0], sds[1], device=dev)
    refs = []
    for sd in sds:
        m = R.GeneratorRef()
        m.load_state_dict(sd)
        refs.append(m.to(dev).half().eval())
    H = W = a.size
    N = a.frames

    def baseline(frames, coarse):
        line = refs[int(coarse)](frames.permute(0, 3, 1, 2).half() / 255.0)[:, 0]
        return 255 - (line.float() * 255).clamp(0, 255).to(torch.uint8)

    frames = R.make_frames(N, N, H, W).to(dev)
    lines = ["lineart annotator, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "%d frames of %d x %d on the device; median ms [min .. max] over %d rounds of %d calls after a warm-up of both sides, the two sides "
             "alternated" % (N, H, W, a.rounds, a.iters),
             "baseline: tests/lineart_ref.py GeneratorRef .half() (torch's own layers), one batch", ""]
    for coarse in (False, True):
        got = det.run(frames, coarse=coarse, channels=1)           # (warm-up of both sides, and the comparison)
        base = baseline(frames, coarse)
        diff = (got.int() - base.int()).abs()
        lib_t, base_t = [], []
        for _ in range(a.rounds):
            lib_t.append(host_ms(lambda: det.run(frames, coarse=coarse), a.iters))
            base_t.append(host_ms(lambda: baseline(frames, coarse), a.iters))
        lm, bm = statistics.median(lib_t), statistics.median(base_t)
        lines.append("%-7s library %8.3f [%.3f .. %.3f] ms   baseline %8.3f [%.3f .. %.3f] ms   library / baseline %.2f   %.3f ms per frame   "
                     "maps: max |diff| %d, mean %.3f levels" % ("coarse" if coarse else "fine", lm, min(lib_t), max(lib_t), bm, min(base_t),
                                                              max(base_t), lm / bm, lm / N, int(diff.max()), float(diff.float().mean())))
    lines += ["workspace of one group of frames %.0f MB (one frame alone: %.0f MB)" % (
        det.workspace_bytes(N, H, W) / 2 ** 20, det.workspace_bytes(1, H, W) / 2 ** 20), "",
        "one profiled fine forward (HIP events around every launch; a run of its own, slower than the rows above):",
        "(GFLOP: the work each launch is booked with -- a transposed convolution in phase form counts its 16 taps, 16/9 of the layer's own)",
        "%-66s %3s %9s %9s %9s %9s" % ("kernel | shape", "n", "ms", "GFLOP", "TFLOP/s", "GB/s")]
    with ops.Profiler() as prof:
        det.run(frames)
    torch.cuda.synchronize()
    tot_ms = gemm_ms = res_ms = res_fl = 0.0
    h = H // 4
    for key, r in prof.per_kernel().items():
        ms, n = r["ms_per_step"], r["launches_per_step"]
        fl, by = r["flops_per_launch"] * n, r["bytes_per_launch"] * n
        tot_ms += ms
        if r["tag"].startswith("igemm"):
            gemm_ms += ms
            if " N256 K2304 " in r["shape"] + " ":          # 256 -> 256, nine taps: only the residual blocks' convolutions have this shape
                res_ms += ms
                res_fl += fl
        name = key.replace("(anonymous namespace)::", "")
        lines.append("%-66s %3d %9.3f %9.1f %9.1f %9.0f" % (name[:66], n, ms, fl / 1e9, fl / (ms * 1e-3) / 1e12 if ms > 0 else 0,
                                                          by / (ms * 1e-3) / 1e9 if ms > 0 else 0))
    lines += ["%-66s %3s %9.3f" % ("sum of the kernels", "", tot_ms),
              "implicit GEMMs %.3f ms (%.1f %%), the other kernels (stem, InstanceNorm statistics and apply, head) %.3f ms (%.1f %%)" % (
                  gemm_ms, 100 * gemm_ms / tot_ms, tot_ms - gemm_ms, 100 * (tot_ms - gemm_ms) / tot_ms)]
    if res_ms > 0:
        lines.append("the residual blocks' 3x3 convolutions (256 -> 256 at %d x %d): %.1f GFLOP in %.3f ms = %.1f TFLOP/s" % (
            h, h, res_fl / 1e9, res_ms, res_fl / (res_ms * 1e-3) / 1e12))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
