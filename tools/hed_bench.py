"""Times the HED annotator (ctrl_adapter_amd.HEDdetector, csrc/hed.hip + the implicit GEMM) on one GPU: 1, 8 and 16 frames of 512 x 512,
soft-edge and scribble, frames already on the device, against the baseline the other towers use -- the fp32 restatement module
(tests/hed_ref.py: ControlNetHEDRef) cast to fp16 and run by PyTorch on the same GPU, all frames in one batch, followed by torch's
bilinear fuse (no scribble tail: cv2 does that on the host in the reference, and cv2 is not installed here; the baseline's scribble rows
are therefore its soft-edge rows).  Weights are seeded He-initialised ones (no HED checkpoint exists here): time does not depend on them.

Per row: median ms over rounds (the two sides alternated), device synchronised around the host clock (a library forward ends in a stream
synchronisation of its own); the library's attained share of the trunk's FLOPs: 2 * 9 * Cin * Cout * pixels over the twelve GEMM
convolutions, divided by the forward's time and by the dense fp16 matrix peak of the card (2.5 PFLOP/s).

    python tools/hed_bench.py [--rounds 5] [--iters 5] [--out profiles/hed_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PEAK_FP16 = 2.5e15


def trunk_flops(H, W):
    import hed_ref as R
    total, cin, hw = 0.0, 3, H * W
    for k, (c, n) in enumerate(zip(R.CHANNELS, R.LAYERS)):
        if k:
            hw //= 4
        for j in range(n):
            if k + j:
                total += 2.0 * 9 * cin * c * hw
            cin = c
    return total


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hed_bench.txt"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "hed_bench needs a GPU: there is no fallback and no number without one"
    import ctrl_adapter_amd as P
    import hed_ref as R
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    sd = R.make_state_dict(1, "he")
    det = P.HEDdetector.from_state_dict(sd, device=dev)
    ref = R.ControlNetHEDRef()
    ref.load_state_dict(sd)
    ref = ref.to(dev).half()
    H = W = 512

    def baseline(frames):
        maps = ref(frames.permute(0, 3, 1, 2).half())
        edge = sum(F.interpolate(m.float(), size=(H, W), mode="bilinear", align_corners=False) for m in maps) / 5
        return (torch.sigmoid(edge) * 255).clamp(0, 255).to(torch.uint8)

    lines = ["HED annotator, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "frames 512 x 512 on the device; median ms [min .. max] over %d rounds of %d calls; trunk = %.1f GFLOP per frame" % (
                 a.rounds, a.iters, trunk_flops(H, W) / 1e9),
             "baseline: tests/hed_ref.py ControlNetHEDRef .half() + torch bilinear fuse, one batch (no scribble tail)", ""]
    fl = trunk_flops(H, W)
    for N in (1, 8, 16):
        frames = R.make_frames(N, N, H, W).to(dev)
        soft = det.run(frames, channels=1)
        base = baseline(frames)[:, 0]
        diff = (soft.int() - base.int()).abs()
        lines.append("N = %2d: library vs baseline soft map: max |diff| %d, mean %.3f levels; workspace of one group of frames %.0f MB" % (
            N, int(diff.max()), float(diff.float().mean()), det.workspace_bytes(N, H, W) / 2 ** 20))
        for scribble in (False, True):
            lib_t, base_t = [], []
            for _ in range(a.rounds):
                lib_t.append(host_ms(lambda: det.run(frames, scribble=scribble), a.iters))
                base_t.append(host_ms(lambda: baseline(frames), a.iters))
            lm, bm = statistics.median(lib_t), statistics.median(base_t)
            lines.append("N = %2d %-9s library %8.3f [%.3f .. %.3f] ms   baseline %8.3f [%.3f .. %.3f] ms   library / baseline %.2f   "
                         "trunk %.1f TFLOP/s = %.1f %% of the fp16 peak" % (
                             N, "scribble" if scribble else "softedge", lm, min(lib_t), max(lib_t), bm, min(base_t), max(base_t), lm / bm,
                             N * fl / (lm * 1e-3) / 1e12, 100 * N * fl / (lm * 1e-3) / PEAK_FP16))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
