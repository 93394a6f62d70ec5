"""Times the canny extractor (ctrl_adapter_amd.canny, csrc/canny.hip) on one GPU, on the two loads of the reference's scripts: a clip of
16 frames of 512 x 512 and one image of 1024 x 1024 (the golden inputs of tests/golden/canny/, shifted per frame so that no two frames
are equal; the 1024 x 1024 image is a golden input enlarged with Pillow).  Per load and per number of hysteresis passes enqueued per
flag readback (CTRL_CANNY_BATCH = 1, 2, 4, 8, alternated in rounds):

  * median ms of a call end to end, upload included (host uint8 arrays in) and excluded (device tensors in); a call ends in a stream
    synchronisation of its own (the flag readback), the host clock is read after a device synchronise
  * the passes and readbacks of the hysteresis loop
  * the three ops alone (device events, median): map, hysteresis, finish
  * the output is compared with the numpy restatement (tests/canny_ref.py) before anything is timed
  * cv2.Canny on the host, one frame after the other as the reference calls it, if cv2 can be imported; otherwise the file says it cannot

    python tools/canny_bench.py [--rounds 5] [--iters 20] [--out profiles/canny_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BATCHES = (1, 2, 4, 8)


def loads():
    import numpy as np
    from PIL import Image
    import canny_forms as F
    base = [F.load_pair(i)[0] for i in range(3)]
    clip = [np.ascontiguousarray(np.roll(base[k % 3], (7 * k, 11 * k), axis=(0, 1))) for k in range(16)]
    big = np.array(Image.fromarray(base[2]).resize((1024, 1024)))
    return {"16 x 512 x 512": clip, "1 x 1024 x 1024": [big]}


def host_ms(fn, iters):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def event_ms(fn, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def med(v):
    return "%.3f [%.3f .. %.3f]" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canny_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "canny_bench needs a GPU: there is no fallback and no number without one"
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import _lib, ops
    import canny_ref as R
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["# canny extractor on %s; median [min .. max] over %d rounds of %d calls; ms" % (torch.cuda.get_device_name(0), a.rounds, a.iters)]
    try:
        import cv2
    except Exception as e:                                   # noqa: BLE001 -- absent is an answer, not an error
        cv2 = None
        lines.append("# cv2 cannot be imported here (%s): no host cv2.Canny time" % type(e).__name__)
    prev = ops.set_policy("CTRL_CANNY_BATCH", None)
    try:
        for name, frames in loads().items():
            N, (H, W) = len(frames), frames[0].shape[:2]
            want = np.stack([np.stack([R.canny(f)] * 3, axis=2) for f in frames])
            devf = [torch.from_numpy(f).to(dev) for f in frames]
            lines.append("")
            lines.append("## %s" % name)
            t_up = {b: [] for b in BATCHES}
            t_dev = {b: [] for b in BATCHES}
            stats = {}
            for b in BATCHES:                                    # correctness and warm-up of every form first
                ops.set_policy("CTRL_CANNY_BATCH", b)
                got, stats[b] = P.canny(frames, channels=3, device=dev, return_stats=True)
                bad = int((got.cpu().numpy() != want).sum())
                assert bad == 0, "%s, batch %d: %d bytes differ from the restatement" % (name, b, bad)
                P.canny(devf, channels=3)
            for _ in range(a.rounds):
                for b in BATCHES:                                # alternated: drift of the machine lands on every form alike
                    ops.set_policy("CTRL_CANNY_BATCH", b)
                    t_up[b].append(host_ms(lambda: P.canny(frames, channels=3, device=dev), a.iters))
                    t_dev[b].append(host_ms(lambda: P.canny(devf, channels=3), a.iters))
            lines.append("output equals the numpy restatement of cv2.Canny: 0 differing bytes of %d, every form below" % want.size)
            lines.append("%-22s %-30s %-30s %-7s %-9s" % ("passes per readback", "end to end, upload included", "end to end, frames on device", "passes",
                                                          "readbacks"))
            for b in BATCHES:
                lines.append("%-22d %-30s %-30s %-7d %-9d" % (b, med(t_up[b]), med(t_dev[b]), stats[b]["passes"], stats[b]["readbacks"]))
            # the three ops alone
            ops.set_policy("CTRL_CANNY_BATCH", None)
            src = torch.stack(devf).contiguous()
            mp = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
            mp0 = torch.empty_like(mp)
            out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
            ws = torch.empty(int(lib.ctrl_canny_ws_bytes(N, H, W)), dtype=torch.uint8, device=dev)
            p, r = C.c_int(0), C.c_int(0)
            f_map = lambda: _lib.check(lib.ctrl_op_canny_map(src.data_ptr(), N, H, W, 3, 100.0, 200.0, mp0.data_ptr(), stream()))
            f_fin = lambda: _lib.check(lib.ctrl_op_canny_finish(mp.data_ptr(), N, H, W, 3, out.data_ptr(), stream()))

            def f_hyst():                                        # from the candidate map every time: the copy is inside the window
                mp.copy_(mp0)
                _lib.check(lib.ctrl_op_canny_hysteresis(mp.data_ptr(), N, H, W, ws.data_ptr(), ws.numel(), C.byref(p), C.byref(r), stream()))
            f_copy = lambda: mp.copy_(mp0)
            for f in (f_map, f_hyst, f_fin):
                f()
            t = {k: [event_ms(f, a.iters) for _ in range(a.rounds)] for k, f in (("map", f_map), ("copy", f_copy), ("hyst", f_hyst), ("finish", f_fin))}
            lines.append("ops alone (device events): map %s   hysteresis + a map copy %s (the copy alone %s; default passes per readback, "
                         "%d passes, %d readbacks)   finish %s" % (med(t["map"]), med(t["hyst"]), med(t["copy"]), p.value, r.value, med(t["finish"])))
            if cv2 is not None:
                def host():
                    for f in frames:
                        e = cv2.Canny(f, 100, 200)
                        np.concatenate([e[:, :, None]] * 3, axis=2)
                host()
                tc = []
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        host()
                    tc.append((time.perf_counter() - t0) * 1e3 / a.iters)
                lines.append("cv2.Canny on the host (%s, frame by frame, %d threads): %s" % (cv2.__version__, cv2.getNumThreads(), med(tc)))
    finally:
        ops.set_policy("CTRL_CANNY_BATCH", prev)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
