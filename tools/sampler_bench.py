"""Times the sampler launches (csrc/sampler.hip) against what they replace, on the GPU this runs on, and writes profiles/sampler_bench.txt.

(a) the per-step glue at SVD's shape (B = 1, F = 25, 4 + 4 channels, 72 x 128 latents, fp16, CFG): ONE fused launch
    (guided_step(prepare_next=True)) against the same arithmetic as the reference pipeline's torch-op sequence
    (svd/pipelines/svd_controlnet_adapter_pipeline.py:646-647, :755, :769-774 with diffusers' EulerDiscreteScheduler ops), the two
    alternated in the same process.  The torch sequence is given python floats for sigma (no device indexing, no host read).
(b) DenoiseLoop over a miniature SVD UNet, eager steps against the recorded step, in steps per second.

Timing: device events around a window of calls that ends in a synchronise, every shape warmed first, windows repeated and alternated;
the median window and the spread (min .. max) are reported.  There is no CPU path: without a GPU this fails."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SVD_SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="v_prediction", sigma_max=700.0,
                 sigma_min=0.002, steps_offset=1, timestep_spacing="leading", timestep_type="continuous", use_karras_sigmas=True)
MINI_UNET = dict(in_channels=8, out_channels=4, block_out_channels=(64, 128, 256, 256), num_attention_heads=(1, 2, 4, 4), layers_per_block=1,
                 cross_attention_dim=64, addition_time_embed_dim=32, projection_class_embeddings_input_dim=96)


def window_us(fn, iters):
    """microseconds per call over one window of `iters` calls (device events; ends in a synchronise)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def alternate(fns, iters, rounds):
    """{name: [us per call of every window]}: the candidates take turns, window by window"""
    for fn in fns.values():
        for _ in range(max(iters // 10, 10)):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window_us(fn, iters))
    return out


def fmt(name, v, unit="us"):
    return "%-44s median %9.2f %s   (min %.2f .. max %.2f over %d windows)" % (name, statistics.median(v), unit, min(v), max(v), len(v))


def glue(P, dev, lines, iters, rounds):
    B, Fr, C, h, w = 1, 25, 4, 72, 128
    sch = P.EulerDiscreteScheduler(**SVD_SCHED)
    sch.set_timesteps(25, device=dev)
    i = 12
    g = torch.Generator().manual_seed(1)
    latents0 = (torch.randn(B, Fr, C, h, w, generator=g) * 30).half().to(dev)
    noise_pred = torch.randn(2 * B, Fr, C, h, w, generator=g).half().to(dev)
    image_latents = torch.randn(2 * B, Fr, C, h, w, generator=g).half().to(dev)
    guidance = torch.linspace(1.0, 3.0, Fr).to(device=dev, dtype=torch.float16)
    g32 = guidance.float().contiguous()
    g5 = guidance.reshape(1, Fr, 1, 1, 1)
    sigma, sigma_next, sigma_in = float(sch.sigmas[i]), float(sch.sigmas[i + 1]), float(sch.sigmas[i + 1])
    unet_in = torch.empty(2 * B, Fr, 2 * C, h, w, dtype=torch.float16, device=dev)
    cn_in = torch.empty(2 * B, Fr, C, h, w, dtype=torch.float16, device=dev)
    lat_a, lat_b = latents0.clone(), latents0.clone()

    def fused():
        sch.guided_step(noise_pred, lat_a, g32, prepare_next=True, concat=image_latents, out=(unet_in, cn_in), step_index=i)

    state = {}

    def torch_sequence():
        # :769-771 the CFG combine
        u, c = noise_pred.chunk(2)
        m = u + g5 * (c - u)
        # EulerDiscreteScheduler.step, v_prediction, gamma = 0 (diffusers upcasts the sample to fp32 and casts the result back)
        sample = lat_b.to(torch.float32)
        x0 = m * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        derivative = (sample - x0) / sigma
        prev = (sample + derivative * (sigma_next - sigma)).to(m.dtype)
        # the next iteration's :646-647 (CFG duplication, scale_model_input), :660 (a view) and :755 (the concat)
        lmi = torch.cat([prev] * 2)
        lmi = lmi / ((sigma_in ** 2 + 1) ** 0.5)
        state["cn"] = lmi.reshape(-1, C, h, w)
        state["unet"] = torch.cat([lmi, image_latents], dim=2)
        state["prev"] = prev

    # the two compute the same thing (one application each from the same latents)
    fused()
    torch_sequence()
    torch.cuda.synchronize()
    d_prev = (lat_a.float() - state["prev"].float()).abs().max().item()
    d_in = (unet_in.float() - state["unet"].float()).abs().max().item()
    scale = state["prev"].float().abs().max().item()
    res = alternate({"fused": fused, "torch": torch_sequence}, iters, rounds)
    nbytes = latents0.numel() * 2 * (1 + 2 + 1 + 2 + 2) + image_latents.numel() * 2 * 2      # x, [u ; c], prev, 2 replicas twice; concat in + out
    mf, mt = statistics.median(res["fused"]), statistics.median(res["torch"])
    lines += ["(a) per-step glue, SVD shape: B=1 F=25 4+4 ch 72x128 fp16, CFG, per-frame guidance, Euler v-prediction (row %d of 25)" % i,
              "    " + fmt("fused sampler launch (1 launch)", res["fused"]),
              "    " + fmt("torch-op sequence of the reference's glue", res["torch"]),
              "    fused / torch = %.3f   (fused moves %.1f MB: %.0f GB/s at the median)" % (mf / mt, nbytes / 1e6, nbytes / mf / 1e3),
              "    agreement after one application: max |prev - prev_torch| = %.3e (max |prev| = %.1f), max |unet_in - torch| = %.3e"
              % (d_prev, scale, d_in),
              "    (the torch sequence rounds the guided output and the scaled input to fp16 on the way; the launch rounds once each)"]
    return mf, mt


def loop(P, dev, lines, steps, rounds):
    from ctrl_adapter_amd.synthetic import seeded_init, seeded_tensor
    B, Fr, h, w = 1, 8, 16, 24
    unet = seeded_init(P.UNetSpatioTemporalConditionModel(**MINI_UNET), seed=5).to(dev)
    ehs = seeded_tensor((2 * B, 1, 64), 2).half().to(dev)
    ids = torch.tensor([[6.0, 127.0, 0.02]] * (2 * B)).to(dev)
    image_latents = seeded_tensor((2 * B, Fr, 4, h, w), 3).half().to(dev)
    guidance = torch.linspace(1.0, 3.0, Fr).to(dev)

    def model_fn(unet_in, cn_in, t, t0, t1):
        return unet(unet_in, t, encoder_hidden_states=ehs, added_time_ids=ids, return_dict=False)[0]

    sch = P.EulerDiscreteScheduler(**SVD_SCHED)
    latents = (seeded_tensor((B, Fr, 4, h, w), 4) * sch.init_noise_sigma).half().to(dev)
    out, rates = {}, {"eager": [], "graph": []}
    for warm in (True, False):
        for _ in range(1 if warm else rounds):
            for name in ("eager", "graph"):
                lp = P.DenoiseLoop(sch, model_fn, guidance, cfg=True, concat=image_latents, graph=name == "graph")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[name] = lp.run(latents, steps)
                torch.cuda.synchronize()
                if not warm:
                    rates[name].append(steps / (time.perf_counter() - t0))
    same = torch.equal(out["eager"], out["graph"])
    me, mg = statistics.median(rates["eager"]), statistics.median(rates["graph"])
    lines += ["(b) DenoiseLoop, %d steps, miniature SVD UNet (block_out_channels 64/128/256/256), B=1 F=%d %dx%d fp16, CFG; host clock around"
              % (steps, Fr, h, w),
              "    run() ending in a synchronise -- the graph figure includes step 0 (eager) and the recording of step 1",
              "    " + fmt("eager: every step launched from Python", rates["eager"], "steps/s"),
              "    " + fmt("graph: step 1 recorded, replayed", rates["graph"], "steps/s"),
              "    graph / eager = %.2fx   results bit-identical: %s" % (mg / me, same)]
    return me, mg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_bench.txt"))
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench needs a GPU: a timing taken anywhere else says nothing")
    import ctrl_adapter_amd as P
    dev = torch.device("cuda:0")
    lines = ["sampler_bench on %s (torch %s)" % (torch.cuda.get_device_name(0), torch.__version__),
             "windows of %d calls, %d windows per candidate, candidates alternated; device events" % (a.iters, a.rounds), ""]
    with torch.no_grad():
        glue(P, dev, lines, a.iters, a.rounds)
        lines.append("")
        loop(P, dev, lines, a.steps, max(a.rounds // 2, 3))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
