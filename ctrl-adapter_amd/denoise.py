"""The denoise loop around the modules: DenoiseLoop drives a scheduler of schedulers.py with ONE sampler launch per step and, with
graph=True, records one whole step (the caller's models + that launch) as a graph and replays it; denoise_svd is the SVD pipeline's
loop (svd/pipelines/svd_controlnet_adapter_pipeline.py:640-785) built on it.

What makes a step recordable: nothing in it reads a host scalar.  The step index lives in a device counter (csrc/sampler.hip), the
coefficients in a device table, and the three per-step timesteps the modules need are rewritten by the sampler launch into a small
device buffer that the modules' `timestep` arguments point at."""
import torch

from .schedulers import check_guidance_rescale


class DenoiseLoop:
    """run(latents, n) -> the denoised latents.

    model_fn(unet_input, controlnet_input, t_model, t_aux0, t_aux1) -> noise_pred: the caller's closure over the modules of this
    package.  The five arguments are the SAME tensors at every call (the sampler launch rewrites them in place), the three timesteps
    1-element fp32 device tensors; model_fn must not read anything on the host (.item(), float(t), a python branch on a tensor).
    guidance: a number or an fp32 device tensor [frames]; cfg: the UNet's input holds [uncond ; cond] replicas of the latents and
    noise_pred both predictions; concat: [R b, ...] channels joined behind the latents' (SVD's image_latents); controlnet_layout:
    None (the ControlNet's sample is laid out as the latents) or "(b f) c h w" (the I2VGen-XL rearrange of b c f h w latents).

    Step 0 runs eagerly: the plans allocate their workspace on the first forward of a size and refuse that under capture.  With
    graph=True step 1 is then recorded with torch.cuda.graph and replayed for every remaining step; graph=False runs every step
    eagerly through the same launches.  The results are bit-identical."""

    def __init__(self, scheduler, model_fn, guidance=1.0, cfg=True, concat=None, controlnet_layout=None, graph=True, channel_dim=None,
                 guidance_rescale=0.0):
        check_guidance_rescale(guidance_rescale)
        self.scheduler, self.model_fn, self.guidance = scheduler, model_fn, guidance
        self.cfg, self.concat, self.controlnet_layout, self.graph, self.channel_dim = bool(cfg), concat, controlnet_layout, bool(graph), channel_dim
        self.last_graph = self.latents = None

    @torch.no_grad()
    def run(self, latents, num_inference_steps, aux0=None, aux1=None):
        """latents: the initial noise already multiplied by scheduler.init_noise_sigma (a private copy is stepped).  aux0 / aux1: per-step
        values (a number or a sequence of num_inference_steps) of the two extra timestep scalars; default: the model's timestep"""
        sch, n = self.scheduler, int(num_inference_steps)
        if not latents.is_cuda:
            raise RuntimeError("DenoiseLoop: the latents must live on the GPU; there is no CPU path")
        sch.set_timesteps(n, device=latents.device, aux0=aux0, aux1=aux1)
        x = latents.detach().clone(memory_format=torch.contiguous_format)
        self.latents = x                   # the tensor every step rewrites in place (a model_fn of a test or a preview may look at it)
        kw = dict(concat=self.concat, controlnet_layout=self.controlnet_layout, channel_dim=self.channel_dim)
        sch.reset()
        unet_in, cn_in = sch.model_input(x, cfg=self.cfg, **kw)
        bufs = (unet_in, cn_in)
        tm, ta0, ta1 = sch.timestep_tensors

        def one_step():
            noise_pred = self.model_fn(unet_in, cn_in, tm, ta0, ta1)
            sch.guided_step(noise_pred, x, self.guidance, prepare_next=True, out=bufs, **kw)

        one_step()
        self.last_graph = None
        if n > 1 and self.graph:
            torch.cuda.synchronize(latents.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                one_step()
            for _ in range(1, n):
                g.replay()
            self.last_graph = g
        else:
            for _ in range(1, n):
                one_step()
        return x


def controlnet_keep(n, control_guidance_start=0.0, control_guidance_end=1.0):
    """svd/pipelines/svd_controlnet_adapter_pipeline.py:624-628 for one ControlNet: 1.0 inside the guidance window, else 0.0"""
    return [1.0 - float(i / n < control_guidance_start or (i + 1) / n > control_guidance_end) for i in range(n)]


@torch.no_grad()
def denoise_svd(controlnet, adapter, unet, scheduler, latents, image_latents, image_embeddings, added_time_ids, controlnet_prompt_embeds,
                images, num_inference_steps=25, min_guidance_scale=1.0, max_guidance_scale=3.0, controlnet_conditioning_scale=1.0,
                control_guidance_start=0.0, control_guidance_end=1.0, fixed_controlnet_timestep=-1, skip_conv_in=False, skip_time_emb=False,
                guess_mode=False, sparse_frames=None, graph=True):
    """The SVD pipeline's denoising loop (:640-785), dense frames: per step ControlNet -> Ctrl-Adapter -> UNet -> per-frame CFG ->
    scheduler.step, with the glue in one sampler launch.

    latents [B, F, 4, h, w] (already scaled by scheduler.init_noise_sigma); with classifier-free guidance (image_latents holds 2 B
    clips) image_latents [2B, F, 4, h, w], image_embeddings [2B, 1, D], added_time_ids [2B, 3], controlnet_prompt_embeds [2B F, L, 768]
    and images [2B F, 3, H, W] hold the unconditional half first, as the pipeline concatenates them.  The ControlNet's timestep is
    fixed_controlnet_timestep (then the adapter gets the model's t), or the computed 1000 - (i + 1) (1000 // n) + 1 for both (:673-681).
    The adapter's residuals reach the UNet as the adapter writes them, (b f) c h w, which the UNet's skip join reads in place (the
    pipeline's rearrange to b c f h w is a layout change only).  guidance per frame: linspace(min, max, F) rounded to the latents'
    dtype as at :615-616.

    A conditioning scale that changes over the steps (control_guidance_start > 0 or control_guidance_end < 1) is a host decision per
    step (a step with scale 0 also drops the down residuals, :748): such a run is stepped eagerly, graph or not.
    Not built here (ValueError): sparse_frames inside the loop, the 64 x 64 pooling of use_size_512."""
    if sparse_frames is not None:
        raise ValueError("denoise_svd: sparse_frames inside the loop is not built (dense frames only)")
    if isinstance(controlnet_conditioning_scale, (list, tuple)):
        controlnet_conditioning_scale = controlnet_conditioning_scale[0]
    if latents.dim() != 5:
        raise ValueError("denoise_svd: latents must be [B, F, C, h, w] (got %s)" % (tuple(latents.shape),))
    B, F = latents.shape[0], latents.shape[1]
    if image_latents.shape[0] not in (B, 2 * B) or tuple(image_latents.shape[1:2]) != (F,):
        raise ValueError("denoise_svd: image_latents must be [B or 2B, F, C, h, w] (got %s)" % (tuple(image_latents.shape),))
    cfg = image_latents.shape[0] == 2 * B
    n = int(num_inference_steps)
    keep = controlnet_keep(n, control_guidance_start, control_guidance_end)
    scales = [float(controlnet_conditioning_scale) * k for k in keep]
    constant = len(set(scales)) == 1
    if fixed_controlnet_timestep >= 0:
        aux0, aux1 = float(int(fixed_controlnet_timestep)), None
    else:
        aux0 = [float(round(1000 - (i + 1) * (1000 // n) + 1)) for i in range(n)]
        aux1 = aux0
    guidance = torch.linspace(min_guidance_scale, max_guidance_scale, F).to(device=latents.device, dtype=latents.dtype).float().contiguous()
    adapter_ehs = image_embeddings[-1].unsqueeze(0)
    calls = [0]

    def model_fn(unet_in, cn_in, t_model, t_controlnet, t_adapter):
        i = min(calls[0], n - 1)          # read only when the scale varies (then every step is an eager call)
        calls[0] += 1
        scale = scales[0] if constant else scales[i]
        down, mid = controlnet(cn_in.reshape(-1, *cn_in.shape[2:]), t_controlnet, encoder_hidden_states=controlnet_prompt_embeds,
                               controlnet_cond=images, conditioning_scale=scale, guess_mode=guess_mode, return_dict=False,
                               skip_conv_in=skip_conv_in, skip_time_emb=skip_time_emb)
        a_down, a_mid = adapter(down_block_res_samples=[d.to(adapter.dtype) for d in down], mid_block_res_sample=mid.to(adapter.dtype),
                                sparsity_masking=None, num_frames=F, timestep=t_adapter, encoder_hidden_states=adapter_ehs)
        if scale == 0:
            a_down = None
        return unet(unet_in, t_model, encoder_hidden_states=image_embeddings, added_time_ids=added_time_ids,
                    down_block_additional_residuals=a_down, mid_block_additional_residual=a_mid, return_dict=False)[0]

    loop = DenoiseLoop(scheduler, model_fn, guidance if cfg else 1.0, cfg=cfg, concat=image_latents, controlnet_layout=None,
                       graph=graph and constant)
    return loop.run(latents, n, aux0=aux0, aux1=aux1)
