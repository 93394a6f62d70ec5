"""DenoiseLoop and denoise_svd on the GPU: a recorded step replays bit-identically to eager steps, every step's glue stays within the
op-level bounds (tests/test_gpu_sampler.py) of its fp64 evaluation, and the modules are told the right timesteps.

How the loop is compared with "a torch loop that calls the same UNet and does the glue in fp64": the UNet is not a contraction, so a
bound on the FINAL latents cannot be derived from the formats; what can be is every step on its own.  The eager run records, at each
call of model_fn, the latents the step starts from, the inputs the model was given and its output.  Then for every step k
    * the recorded output equals the same UNet called again, outside the loop, on the recorded input with row k's timestep (bit for bit),
    * latents_{k+1} is within the step bound of the fp64 glue applied to (latents_k, that output), and
    * the recorded input of step k + 1 is within the model-input bound of c_{k+1} * latents_{k+1},
which by induction bounds the whole run, and graph = True equals that run bit for bit."""
import pytest
import torch

import helpers  # noqa: F401
import unet_svd_ref as R
from sampler_check import assert_within, input_bound, step_bound

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
SVD_SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="v_prediction", sigma_max=700.0,
                 sigma_min=0.002, steps_offset=1, timestep_spacing="leading", timestep_type="continuous", use_karras_sigmas=True)
DDIM_SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="v_prediction", clip_sample=False,
                  rescale_betas_zero_snr=True, timestep_spacing="trailing", set_alpha_to_one=False, steps_offset=1)
_CACHE = {}


def _narrow_unet(gpu):
    if "unet" not in _CACHE:
        import ctrl_adapter_amd as P
        from ctrl_adapter_amd.synthetic import seeded_init
        _CACHE["unet"] = seeded_init(P.UNetSpatioTemporalConditionModel(**R.NARROW), seed=2027).to(gpu)
    return _CACHE["unet"]


def _narrow_setup(gpu, B=1, Fr=3, h=8, w=8):
    """the miniature SVD UNet (NARROW), fixed synthetic residuals, CFG operands for B clips of Fr frames, fp16"""
    unet = _narrow_unet(gpu)
    inp = R.seeded_inputs(R.NARROW, 2 * B, Fr, h, w, seed=11, residuals="4d")
    ehs, ids = inp["encoder_hidden_states"].half().to(gpu), inp["added_time_ids"].to(gpu)
    down = [r.to(gpu) for r in inp["down_block_additional_residuals"]]
    mid = inp["mid_block_additional_residual"].to(gpu)
    g = torch.Generator().manual_seed(4)
    image_latents = torch.randn(2 * B, Fr, 4, h, w, generator=g).half().to(gpu)
    noise = torch.randn(B, Fr, 4, h, w, generator=g)

    def unet_call(unet_in, t):
        return unet(unet_in, t, encoder_hidden_states=ehs, added_time_ids=ids, down_block_additional_residuals=down,
                    mid_block_additional_residual=mid, return_dict=False)[0]
    return unet_call, image_latents, noise


def _run_both_ways(P, sch, unet_call, image_latents, latents, guidance, n):
    """(graph result, eager result, the eager run's per-step records)"""
    rec = []
    holder = {}

    def model_fn(unet_in, cn_in, tm, ta0, ta1):
        out = unet_call(unet_in, tm)
        if holder.get("record"):
            rec.append(dict(x=holder["loop"].latents.clone(), unet_in=unet_in.clone(), cn_in=cn_in.clone(), t=(tm.clone(), ta0.clone(), ta1.clone()),
                            out=out.clone()))
        return out
    results = []
    for graph in (True, False):
        loop = P.DenoiseLoop(sch, model_fn, guidance, cfg=True, concat=image_latents, graph=graph)
        holder.update(loop=loop, record=not graph)
        results.append(loop.run(latents, n, aux0=[float(100 + i) for i in range(n)]))
        torch.cuda.synchronize()
        assert (loop.last_graph is not None) == (graph and n > 1)
    return results[0], results[1], rec


def _check_records(sch, rec, final, unet_call, image_latents, guidance, n):
    t64 = sch.table
    t32 = t64.float()
    Fr = final.shape[1]
    g = guidance.cpu().double().reshape(1, Fr, 1, 1, 1)
    assert len(rec) == n
    for k, r in enumerate(rec):
        # the modules were told row k's timesteps (fp32 roundings of the fp64 table)
        assert [float(v) for v in r["t"]] == [float(t32[k, 3]), float(t32[k, 4]), float(t32[k, 5])] and float(t32[k, 4]) == 100.0 + k
        # the same UNet, called outside the loop on the same input with that timestep
        again = unet_call(r["unet_in"], torch.tensor([float(t32[k, 3])], device=final.device))
        assert torch.equal(again, r["out"]), "step %d: the loop's UNet call is not the plain call" % k
        x = r["x"].cpu().double()
        # this step's input is c_k * latents_k (replicated, image_latents behind)
        ref_in = float(t64[k, 0]) * x
        ref_in = torch.cat([torch.cat([ref_in] * 2, 0), image_latents.cpu().double()], 2)
        b = input_bound(ref_in, F16)
        b[:, :, 4:] = 0
        assert_within(r["unet_in"], ref_in, b, "loop step %d unet_in" % k)
        assert torch.equal(r["cn_in"], r["unet_in"][:, :, :4])
        u, c = r["out"].cpu().double().chunk(2)
        A, B = float(t64[k, 1]), float(t64[k, 2])
        ref = A * x + B * (u + g * (c - u))
        nxt = rec[k + 1]["x"] if k + 1 < n else final
        assert_within(nxt, ref, step_bound(ref, nxt.dtype, A, B, x, u, c, g.expand(x.shape)), "loop step %d latents" % k)


def test_denoise_loop_graph_equals_eager_and_tracks_the_fp64_glue(gpu):
    """Euler with SVD's config over the miniature SVD UNet, 6 steps, fp16 latents, per-frame guidance"""
    import ctrl_adapter_amd as P
    unet_call, image_latents, noise = _narrow_setup(gpu)
    sch = P.EulerDiscreteScheduler(**SVD_SCHED)
    latents = (noise * sch.init_noise_sigma).half().to(gpu)
    guidance = torch.linspace(1.0, 3.0, 3).to(gpu)
    got_graph, got_eager, rec = _run_both_ways(P, sch, unet_call, image_latents, latents, guidance, 6)
    assert torch.equal(got_graph, got_eager), "graph replay differs from eager steps"
    assert bool(torch.isfinite(got_eager.float()).all()) and got_eager.dtype == F16 and got_eager.shape == latents.shape
    assert got_eager.data_ptr() != latents.data_ptr()
    _check_records(sch, rec, got_eager, unet_call, image_latents, guidance, 6)


def test_denoise_loop_ddim_v_prediction_zero_snr(gpu):
    """DDIM (v-prediction, zero terminal SNR, trailing: the first step starts at alpha_bar = 0), fp32 latents, 4 steps"""
    import ctrl_adapter_amd as P
    unet_call, image_latents, noise = _narrow_setup(gpu)
    sch = P.DDIMScheduler(**DDIM_SCHED)
    latents = noise.to(gpu)
    guidance = torch.linspace(1.0, 2.0, 3).to(gpu)
    got_graph, got_eager, rec = _run_both_ways(P, sch, unet_call, image_latents.float(), latents, guidance, 4)
    assert torch.equal(got_graph, got_eager) and got_eager.dtype == F32
    assert float(sch.table[0, 3]) == 999.0 and bool(torch.isfinite(got_eager).all())
    t64 = sch.table
    for k, r in enumerate(rec):
        x = r["x"].cpu().double()
        u, c = r["out"].cpu().double().chunk(2)
        g = guidance.cpu().double().reshape(1, 3, 1, 1, 1)
        A, B = float(t64[k, 1]), float(t64[k, 2])
        ref = A * x + B * (u + g * (c - u))
        nxt = rec[k + 1]["x"] if k + 1 < 4 else got_eager
        assert_within(nxt, ref, step_bound(ref, F32, A, B, x, u, c, g.expand(x.shape)), "ddim loop step %d latents" % k)


def test_one_step_loop_and_two_step_loop(gpu):
    """n = 1: only the eager step (nothing to record, no next input); n = 2: one replay"""
    import ctrl_adapter_amd as P
    unet_call, image_latents, noise = _narrow_setup(gpu)
    for n in (1, 2):
        sch = P.EulerDiscreteScheduler(**SVD_SCHED)
        latents = (noise * sch.init_noise_sigma).half().to(gpu)
        a, b, rec = _run_both_ways(P, sch, unet_call, image_latents, latents, torch.linspace(1.0, 3.0, 3).to(gpu), n)
        assert torch.equal(a, b) and len(rec) == n


def test_denoise_svd_miniature_graph_equals_eager(gpu):
    """ControlNet (SD-1.5) + Ctrl-Adapter (locations A and B of the video config) + a two-level SVD UNet whose first six skips are the
    adapter's first six outputs: 3 steps at 8 x 8 latents, F = 2, CFG.  Graph equals eager bit for bit, the result is finite, a
    window that switches the control off on the last step runs (eagerly) and differs, and the step-0 workspace rule holds."""
    import cases
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init, seeded_tensor
    B, Fr, h, w = 1, 2, 8, 8
    N = 2 * B * Fr
    cn = seeded_init(P.ControlNetModel(**cases.CONTROLNET_KW), seed=11).to(gpu)
    acfg = dict(cases.ADAPTER_VIDEO, backbone_model_name="svd", add_adapter_location_C=False, add_adapter_location_D=False, add_adapter_location_M=False)
    ad = seeded_init(P.ControlNetAdapter(**acfg), seed=22).to(gpu)
    unet = seeded_init(P.UNetSpatioTemporalConditionModel(**dict(R.WIDE2, layers_per_block=2)), seed=33).to(gpu)
    sch = P.EulerDiscreteScheduler(**SVD_SCHED)
    latents = (seeded_tensor((B, Fr, 4, h, w), 1) * sch.init_noise_sigma).half().to(gpu)
    kw = dict(image_latents=seeded_tensor((2 * B, Fr, 4, h, w), 2).half().to(gpu),
              image_embeddings=seeded_tensor((2 * B, 1, 1024), 3).half().to(gpu),
              added_time_ids=torch.tensor([[6.0, 127.0, 0.02]] * (2 * B)).to(gpu),
              controlnet_prompt_embeds=seeded_tensor((N, 77, 768), 4).half().to(gpu),
              images=seeded_tensor((N, 3, 8 * h, 8 * w), 5, kind="uniform").half().to(gpu),
              num_inference_steps=3, min_guidance_scale=1.0, max_guidance_scale=3.0)
    eager = P.denoise_svd(cn, ad, unet, sch, latents, graph=False, **kw)
    graph = P.denoise_svd(cn, ad, unet, sch, latents, graph=True, **kw)
    torch.cuda.synchronize()
    assert eager.shape == latents.shape and eager.dtype == F16 and bool(torch.isfinite(eager.float()).all())
    assert torch.equal(graph, eager), "denoise_svd: graph replay differs from eager steps"
    # the computed ControlNet timestep 1000 - (i + 1) (1000 // n) + 1, and the fixed one
    assert sch.table[:, 4].tolist() == [668.0, 335.0, 2.0] and sch.table[:, 5].tolist() == [668.0, 335.0, 2.0]
    fixed = P.denoise_svd(cn, ad, unet, sch, latents, graph=True, fixed_controlnet_timestep=50, **kw)
    assert sch.table[:, 4].tolist() == [50.0] * 3 and torch.equal(sch.table[:, 5], sch.table[:, 3])
    assert bool(torch.isfinite(fixed.float()).all()) and not torch.equal(fixed, eager)
    # a control window that ends before the last step: stepped eagerly, and the switched-off step changes the result
    windowed = P.denoise_svd(cn, ad, unet, sch, latents, graph=True, control_guidance_end=0.5, **kw)
    assert bool(torch.isfinite(windowed.float()).all()) and not torch.equal(windowed, eager)
    with pytest.raises(ValueError, match="sparse_frames"):
        P.denoise_svd(cn, ad, unet, sch, latents, sparse_frames=[0], **kw)
    # the step-0 rule: a first forward of a new size under capture is refused with a message (which is why step 0 runs eagerly)
    bigger = seeded_tensor((2 * B, Fr, 8, 16, 16), 6).half().to(gpu)
    t1 = torch.ones(1, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot run under stream capture"):
        with torch.cuda.graph(g):
            unet(bigger, t1, encoder_hidden_states=kw["image_embeddings"], added_time_ids=kw["added_time_ids"])
    torch.cuda.synchronize()
    del cn, ad, unet
    torch.cuda.empty_cache()
