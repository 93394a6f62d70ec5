"""EulerDiscreteScheduler and DDIMScheduler -- drop-ins for `pipe.scheduler` with the surface the three reference pipelines touch
(set_timesteps, timesteps, init_noise_sigma, order, config, scale_model_input, step), whose arithmetic runs in libctrlhip
(csrc/sampler.hip).  For every configuration built here one step is linear in the sample x and the (guided) model output m,

    prev = A_i x + B_i m,        model input = c_i x,

so set_timesteps builds the schedule on the host in fp64, collapses every step to (c_i, A_i, B_i) and uploads one fp32 table; the
kernels multiply and add.  Beyond the reference: model_input() / guided_step() do the whole per-step glue of a pipeline's loop (CFG
replicas, channel concat, the ControlNet's rearranged sample, CFG combine, the step and the next step's input) in one launch each, with
the step index on the host or in a device counter (a loop recorded once as a graph: denoise.py).

The schedules restate diffusers v0.27 [DIFFUSERS v0.27, from knowledge: re-derive and cross-check] -- diffusers is not installed, so
every formula below was written from the published algorithm, re-derived, and is pinned by tests/test_scheduler_host.py against a
sequential fp64 restatement (tests/scheduler_ref.py) and an oracle-free invariant.  One deliberate difference: diffusers builds betas and
alphas_cumprod in fp32, this file in fp64 (the two agree to fp32 rounding).

Not built (ValueError): eta > 0, s_churn > 0, clip_sample, thresholding, interpolation_type != "linear", guidance_rescale > 0,
rescale_betas_zero_snr for Euler, any other scheduler class, stochastic / multi-step / second-order samplers."""
import ctypes as C
import json
import math
import os

import torch

from . import _lib as L
from ._plan import Config

_ROW = L.SAMPLER_ROW


class SchedulerOutput(tuple):
    """(prev_sample,) with attribute access, as diffusers' scheduler outputs"""

    def __new__(cls, prev_sample):
        self = super().__new__(cls, (prev_sample,))
        self.prev_sample = prev_sample
        return self


def make_betas(beta_schedule, beta_start, beta_end, T):
    """[DIFFUSERS v0.27, from knowledge: re-derive and cross-check] the three beta schedules, fp64 tensor [T]"""
    if beta_schedule == "linear":
        return torch.linspace(beta_start, beta_end, T, dtype=torch.float64)
    if beta_schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float64) ** 2
    if beta_schedule == "squaredcos_cap_v2":
        def bar(t):
            return math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
        return torch.tensor([min(1 - bar((i + 1) / T) / bar(i / T), 0.999) for i in range(T)], dtype=torch.float64)
    raise ValueError("beta_schedule %r is not built (linear, scaled_linear, squaredcos_cap_v2 are)" % (beta_schedule,))


def rescale_zero_terminal_snr(betas):
    """[DIFFUSERS v0.27, from knowledge: re-derive and cross-check] shift and scale sqrt(alphas_cumprod) so that its last value is 0 and
    its first is unchanged (Lin et al. 2023, algorithm 1)"""
    abar_sqrt = torch.cumprod(1.0 - betas, 0).sqrt()
    a0, aT = abar_sqrt[0].clone(), abar_sqrt[-1].clone()
    abar_sqrt = (abar_sqrt - aT) * (a0 / (a0 - aT))
    abar = abar_sqrt ** 2
    alphas = torch.cat([abar[0:1], abar[1:] / abar[:-1]])
    return 1.0 - alphas


def spaced_timesteps(spacing, T, n, steps_offset, integer):
    """[DIFFUSERS v0.27, from knowledge: re-derive and cross-check] descending fp64 timesteps of the three spacings.  integer: DDIM rounds
    the linspace positions, Euler keeps them fractional"""
    if spacing == "linspace":
        ts = torch.linspace(0, T - 1, n, dtype=torch.float64)
        ts = ts.round() if integer else ts
        return ts.flip(0)
    if spacing == "leading":
        ratio = T // n
        return (torch.arange(0, n, dtype=torch.float64) * ratio).round().flip(0) + steps_offset
    if spacing == "trailing":
        ratio = T / n
        return torch.tensor([T - k * ratio for k in range(n) if T - k * ratio > 0], dtype=torch.float64).round() - 1
    raise ValueError("timestep_spacing %r is not supported (linspace, leading, trailing)" % (spacing,))


def _interp(x, xp, fp):
    """numpy.interp on fp64 tensors (xp ascending; clamped at the ends)"""
    idx = torch.searchsorted(xp, x.clamp(xp[0], xp[-1]), right=True).clamp(1, len(xp) - 1)
    x0, x1, y0, y1 = xp[idx - 1], xp[idx], fp[idx - 1], fp[idx]
    return y0 + (x.clamp(xp[0], xp[-1]) - x0) * (y1 - y0) / (x1 - x0)


def _find_row(timesteps_host, t):
    """the first row whose timestep equals t (a python number or a 0-d / 1-element tensor, compared in the schedule's fp32 / int form)"""
    tv = float(t.detach().reshape(-1)[0].item()) if torch.is_tensor(t) else float(t)
    for i, v in enumerate(timesteps_host):
        if v == tv or (v != 0 and abs(v - tv) <= 1e-6 * abs(v)):
            return i
    raise ValueError("timestep %r is not in the schedule (set_timesteps first; pass an element of scheduler.timesteps)" % (tv,))


_RETIRED = []          # device objects of collected / re-scheduled schedulers, freed at the next creation (see _release)


class _DevPtr:
    """a raw device buffer as torch sees it (__cuda_array_interface__): the ctrl_sampler's three scalars become 1-element tensor views"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2, "strides": None}


class _SamplerScheduler:
    """what the two schedulers share: the config, the table and its device object, and the kernel calls"""
    order = 1
    _CLASS = None
    _DEFAULTS = {}
    # config keys of diffusers releases around v0.27 that change the schedule or the step: anything but the value built here is refused
    _REFUSED = dict(final_sigmas_type="zero", use_exponential_sigmas=False, use_beta_sigmas=False, variance_type="fixed_small")
    # keys of a saved config that no code here reads and that cannot change a result: bookkeeping, and switches of other schedulers
    _HARMLESS = ("_class_name", "_diffusers_version", "_use_default_values", "_name_or_path", "skip_prk_steps")

    def __init__(self, **kwargs):
        cfg = dict(self._DEFAULTS)
        cfg.update({k: v for k, v in kwargs.items() if k in self._DEFAULTS})
        self.config = Config(cfg)
        for k, ok in self._REFUSED.items():
            if k in kwargs and kwargs[k] != ok:
                raise ValueError("%s: %s = %r is not built (only %r is)" % (self._CLASS, k, kwargs[k], ok))
        # any other key is refused, not dropped: a key of a newer config that changes the schedule must not be ignored silently
        unknown = sorted(set(kwargs) - set(self._DEFAULTS) - set(self._REFUSED) - set(self._HARMLESS))
        if unknown:
            raise ValueError("%s: config key(s) %s are not known here -- refusing to guess whether they change the schedule"
                             % (self._CLASS, unknown))
        self._handle = None
        self._device = None
        self._table64 = None
        self._timesteps_host = None
        self.timesteps = None
        self.num_inference_steps = None
        self._step_index = None
        self._scalar_views = None
        self._check_config()

    # ---- config ----
    @classmethod
    def from_config(cls, config, **kwargs):
        cfg = dict(config)
        cfg.update(kwargs)
        name = cfg.get("_class_name", cls._CLASS)
        if name != cls._CLASS:
            raise ValueError("scheduler class %r is not built as %s: EulerDiscreteScheduler and DDIMScheduler run in libctrlhip, no other "
                             "scheduler does" % (name, cls._CLASS))
        return cls(**cfg)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **kwargs):
        d = os.path.join(path, subfolder) if subfolder else path
        fn = os.path.join(d, "scheduler_config.json")
        if not os.path.isfile(fn):
            raise FileNotFoundError("no scheduler_config.json in %s" % d)
        with open(fn) as fh:
            return cls.from_config(json.load(fh), **kwargs)

    def __del__(self):
        self._release()

    def _release(self):
        """retires the device object without freeing it: ctrl_sampler_destroy synchronises the device, which is not allowed while any
        stream captures, and this is reached from the garbage collector.  Retired objects (a few KB each) are freed by the next
        set_timesteps(..., device=) of any scheduler -- an explicit call that allocates and so cannot run under capture anyway."""
        h, self._handle = getattr(self, "_handle", None), None
        if h and _RETIRED is not None:          # (None: the interpreter is shutting down and has cleared the module)
            _RETIRED.append(h)

    def __len__(self):
        return self.config.num_train_timesteps

    # ---- the table ----
    def _install(self, rows, timesteps, device, aux0=None, aux1=None):
        """rows: [(c_in, A, B)] fp64 per step; timesteps: fp64 tensor [n] (what the model is told); aux0 / aux1: two more per-step
        scalars the loop's modules may read (default: the timestep itself)"""
        n = len(rows)
        t64 = torch.zeros(n, _ROW, dtype=torch.float64)
        t64[:, :3] = torch.tensor(rows, dtype=torch.float64)
        t64[:, 3] = timesteps
        for col, aux in ((4, aux0), (5, aux1)):
            t64[:, col] = timesteps if aux is None else torch.as_tensor(aux, dtype=torch.float64).reshape(-1).expand(n)
        if not bool(torch.isfinite(t64).all()):
            bad = int((~torch.isfinite(t64).all(1)).nonzero()[0])
            raise ValueError("%s: the step coefficients of step %d (timestep %s) are not finite -- this prediction type cannot step from "
                             "there (epsilon prediction at alpha_bar = 0: use v_prediction or sample with a zero-SNR schedule)"
                             % (self._CLASS, bad, float(timesteps[bad])))
        self._table64 = t64
        self.num_inference_steps = n
        self._step_index = None
        self._release()
        self._scalar_views = None
        self._device = torch.device(device) if device is not None else None
        if self._device is not None and self._device.type == "cuda":
            self._ensure(self._device)

    def _ensure(self, device):
        """the device object (created on the first GPU use: the table is uploaded once per set_timesteps)"""
        if self._table64 is None:
            raise RuntimeError("%s: call set_timesteps first" % self._CLASS)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("%s: the sample must live on the GPU; there is no CPU path" % self._CLASS)
        if self._handle is not None and device != self._device:
            raise ValueError("%s: the table lives on %s, the sample on %s" % (self._CLASS, self._device, device))
        if self._handle is None:
            while _RETIRED:
                L.lib().ctrl_sampler_destroy(_RETIRED.pop())
            t32 = self._table64.to(torch.float32).contiguous()
            h = C.c_void_p()
            with torch.cuda.device(device):
                L.check(L.lib().ctrl_sampler_create(t32.shape[0], C.c_void_p(t32.data_ptr()), C.byref(h)))
            self._handle, self._device = h, device
        return self._handle

    @property
    def table(self):
        """fp64 [n][8]: c_in, A, B, t_model, t_aux0, t_aux1, 0, 0 -- what the fp32 device table was rounded from"""
        return self._table64

    @property
    def timestep_tensors(self):
        """three 1-element fp32 device views (t_model, t_aux0, t_aux1) of the row the last model-input pass used: hand them to the
        modules as `timestep` and a recorded step reads the current values at every replay.  They belong to the current schedule:
        set_timesteps makes a new device object, so fetch them again after it (the old views then address a retired buffer)"""
        if self._scalar_views is None:
            if self._handle is None:
                raise RuntimeError("%s: set_timesteps(n, device='cuda') first" % self._CLASS)
            p = L.lib().ctrl_sampler_scalars(self._handle)
            with torch.cuda.device(self._device):
                self._scalar_views = tuple(torch.as_tensor(_DevPtr(p + 4 * i, 1), device=self._device) for i in range(3))
        return self._scalar_views

    def reset(self):
        """the device step counter back to 0 (a kernel: capturable)"""
        with torch.cuda.device(self._device):
            L.check(L.lib().ctrl_sampler_reset(self._ensure(self._device), L.cur_stream()))
        self._step_index = None

    # ---- the reference's surface ----
    def _row_for(self, t):
        return _find_row(self._timesteps_host, t)

    def scale_model_input(self, sample, timestep=None):
        """round(c_i * sample) in the sample's dtype (DDIM: c = 1, still one pass through the kernel: a copy)"""
        i = self._index_for_scale(timestep)
        if sample.dim() in (4, 5):
            return self.model_input(sample, cfg=False, step_index=i, controlnet_input=False)[0]
        flat = self._dense(sample, "sample").reshape(1, 1, -1, 1)         # any other rank, as step() takes it: one row of elements
        return self.model_input(flat, cfg=False, step_index=i, controlnet_input=False, channel_dim=1)[0].reshape(sample.shape)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None, variance_noise=None,
             return_dict=True, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0):
        if eta != 0.0:
            raise ValueError("%s: eta > 0 (the stochastic step) is not built" % self._CLASS)
        if s_churn != 0.0:
            raise ValueError("%s: s_churn > 0 (the stochastic step) is not built" % self._CLASS)
        if use_clipped_model_output or variance_noise is not None:
            raise ValueError("%s: use_clipped_model_output / variance_noise are not built" % self._CLASS)
        if tuple(model_output.shape) != tuple(sample.shape):
            raise ValueError("%s: model_output %s and sample %s differ in shape" % (self._CLASS, tuple(model_output.shape), tuple(sample.shape)))
        i = self._index_for_step(timestep)
        prev = torch.empty_like(model_output, memory_format=torch.contiguous_format)
        self._launch_step(model_output, sample, prev, None, 1, 1, i, None)
        self._advance()
        return SchedulerOutput(prev) if return_dict else (prev,)

    # ---- fused calls beyond the reference ----
    @staticmethod
    def _geometry(latents, channel_dim, controlnet_layout):
        """(channel_dim, outer, C, inner, cn_frames, frame_dim) of dense latents: 4-D b c h w; 5-D b f c h w (channel_dim 2, SVD) or b c f h w
        (channel_dim 1, I2VGen-XL, whose ControlNet sample is rearranged to (b f) c h w)"""
        if latents.dim() not in (4, 5):
            raise ValueError("latents must be [b, c, h, w], [b, f, c, h, w] or [b, c, f, h, w] (got %s)" % (tuple(latents.shape),))
        if controlnet_layout not in (None, "same", "(b f) c h w"):
            raise ValueError("controlnet_layout must be None / 'same' or '(b f) c h w' (got %r)" % (controlnet_layout,))
        if channel_dim is None:
            channel_dim = 1 if (latents.dim() == 4 or controlnet_layout == "(b f) c h w") else 2
        if channel_dim not in (1, 2) or channel_dim >= latents.dim() - 2:
            raise ValueError("channel_dim %r does not name the channel axis of %s" % (channel_dim, tuple(latents.shape)))
        sh = list(latents.shape)
        outer, Cc, inner = math.prod(sh[:channel_dim]), sh[channel_dim], math.prod(sh[channel_dim + 1:])
        frames, frame_dim = 0, None
        if latents.dim() == 5:
            frame_dim = 1 if channel_dim == 2 else 2
        if controlnet_layout == "(b f) c h w":
            if latents.dim() != 5 or channel_dim != 1:
                raise ValueError("controlnet_layout '(b f) c h w' rearranges [b, c, f, h, w] latents")
            frames = sh[2]
        return channel_dim, outer, Cc, inner, frames, frame_dim

    def model_input(self, latents, cfg=True, concat=None, controlnet_layout=None, step_index=None, out=None, channel_dim=None,
                    controlnet_input=True):
        """(unet_input, controlnet_input) of one step from the latents: c_i * latents, replicated twice along the batch when cfg, with
        `concat` ([R b, ...] with C2 channels on the latents' channel axis) behind the latents' channels of the UNet's input; the
        ControlNet's input is the same without the concat, in the latents' layout or rearranged `b c f h w -> (b f) c h w`.
        step_index None: the device counter's row.  out: (unet_input, controlnet_input) buffers to write into."""
        R = 2 if cfg else 1
        cd, outer, Cc, inner, frames, _ = self._geometry(latents, channel_dim, controlnet_layout)
        h = self._ensure(latents.device)
        latents = self._dense(latents, "latents")
        d = L.SamplerDesc()
        d.x, d.x_dtype = latents.data_ptr(), L.dtype_code(latents.dtype)
        want_cn = controlnet_input and (cfg or concat is not None or bool(frames))
        unet_in, cn_in = self._fill_inputs(d, latents, R, cd, Cc, frames, concat, out, want_cn)
        d.outer, d.C, d.inner, d.R = outer, Cc, inner, R
        d.g_count = d.g_inner = 1
        with torch.cuda.device(latents.device):
            L.check(L.lib().ctrl_sampler_model_input(h, C.byref(d), -1 if step_index is None else int(step_index), L.cur_stream()))
        return unet_in, (cn_in if cn_in is not None else unet_in)

    def guided_step(self, noise_pred, latents, guidance=1.0, prepare_next=True, concat=None, controlnet_layout=None, step_index=None,
                    out=None, channel_dim=None):
        """latents <- A_i latents + B_i (u + g (c - u)) in place, where noise_pred holds [u ; c] along the batch (or the single
        prediction: then guidance is not read).  guidance: a number, or an fp32 device tensor [frames] applied per frame of 5-D latents.
        prepare_next: the same launch writes the next step's model inputs (as model_input would, from the stepped latents) into `out` =
        (unet_input, controlnet_input) and returns (latents, unet_input, controlnet_input); on the last step that part is skipped.
        step_index None: the row of the device counter, which the launch advances."""
        if latents.shape[0] == 0 or noise_pred.shape[0] % latents.shape[0] or tuple(noise_pred.shape[1:]) != tuple(latents.shape[1:]):
            raise ValueError("noise_pred %s does not hold 1 or 2 predictions for latents %s" % (tuple(noise_pred.shape), tuple(latents.shape)))
        R = noise_pred.shape[0] // latents.shape[0]
        if R not in (1, 2):
            raise ValueError("noise_pred holds %d predictions per sample: 1 or 2 (classifier-free guidance) are built" % R)
        if not latents.is_contiguous():
            raise ValueError("guided_step writes the latents in place: they must be contiguous")
        g_vec = guidance if torch.is_tensor(guidance) else None
        g_scalar = 1.0 if g_vec is not None else float(guidance)
        prev_out = self._launch_step(noise_pred, latents, latents, g_vec, g_scalar, R, -1 if step_index is None else int(step_index),
                                     (concat, out) if prepare_next else None,
                                     layout=(channel_dim, controlnet_layout))
        if prepare_next:
            return (latents,) + prev_out
        return latents

    def _launch_step(self, model_output, sample, prev, g_vec, g_scalar, R, step_index, nxt, layout=(None, None)):
        h = self._ensure(sample.device)
        if model_output.device != sample.device:
            raise ValueError("%s: model_output on %s, the sample on %s" % (self._CLASS, model_output.device, sample.device))
        model_output, sample = self._dense(model_output, "model_output"), self._dense(sample, "sample")
        d = L.SamplerDesc()
        d.x, d.x_dtype = sample.data_ptr(), L.dtype_code(sample.dtype)
        d.prev, d.prev_dtype = prev.data_ptr(), L.dtype_code(prev.dtype)
        d.model_out, d.mo_dtype = model_output.data_ptr(), L.dtype_code(model_output.dtype)
        d.R, d.g_scalar, d.g_count, d.g_inner = R, g_scalar, 1, 1
        ret = ()
        if sample.dim() in (4, 5):
            cd, outer, Cc, inner, frames, frame_dim = self._geometry(sample, layout[0], layout[1])
        else:
            cd, outer, Cc, inner, frames, frame_dim = 0, 1, 1, sample.numel(), 0, None
        d.outer, d.C, d.inner = outer, Cc, inner
        if g_vec is not None and R == 2:
            if frame_dim is None or g_vec.dim() != 1 or g_vec.shape[0] != sample.shape[frame_dim]:
                raise ValueError("a guidance tensor must hold one fp32 value per frame of 5-D latents")
            if g_vec.dtype != torch.float32 or g_vec.device != sample.device or not g_vec.is_contiguous():
                raise ValueError("a guidance tensor must be contiguous fp32 on the latents' device")
            d.g, d.g_count, d.g_inner = g_vec.data_ptr(), g_vec.shape[0], math.prod(sample.shape[frame_dim + 1:])
        if nxt is not None:
            concat, out = nxt
            if out is None:
                raise ValueError("prepare_next writes the next step's inputs into out=(unet_input, controlnet_input)")
            unet_in, cn_in = self._fill_inputs(d, sample, R, cd, Cc, frames, concat, out, False)
            ret = (unet_in, cn_in if cn_in is not None else unet_in)
        with torch.cuda.device(sample.device):
            L.check(L.lib().ctrl_sampler_step(h, C.byref(d), step_index, 1 if nxt is not None else 0, L.cur_stream()))
        return ret

    def _fill_inputs(self, d, latents, R, cd, Cc, frames, concat, out, want_cn):
        """the model-input half of a descriptor: checks `concat` ([R b, ...], C2 channels on axis cd) and the `out` buffers (or
        allocates them), fills d; -> (unet_in, cn_in or None)"""
        C2 = 0
        if concat is not None:
            want = list(latents.shape)
            want[0] *= R
            C2 = concat.shape[cd] if concat.dim() == latents.dim() else -1
            want[cd] = C2
            if list(concat.shape) != want or concat.device != latents.device:
                raise ValueError("concat must be %s on %s (got %s on %s)" % (want, latents.device, tuple(concat.shape), concat.device))
            concat = self._dense(concat, "concat")
            d.concat, d.concat_dtype = concat.data_ptr(), L.dtype_code(concat.dtype)
        ush = list(latents.shape)
        ush[0] *= R
        csh = list(ush) if not frames else [ush[0] * frames, Cc] + ush[3:]
        ush[cd] = Cc + C2
        if out is not None:
            unet_in, cn_in = out
            if cn_in is unet_in:
                cn_in = None
            for t, sh in ((unet_in, ush), (cn_in, csh)):
                if t is not None and (list(t.shape) != sh or not t.is_contiguous() or t.device != latents.device):
                    raise ValueError("out buffers must be contiguous %s and %s on %s" % (ush, csh, latents.device))
        else:
            unet_in = torch.empty(ush, dtype=latents.dtype, device=latents.device)
            cn_in = torch.empty(csh, dtype=latents.dtype, device=latents.device) if want_cn else None
        d.unet_in, d.unet_dtype = unet_in.data_ptr(), L.dtype_code(unet_in.dtype)
        if cn_in is not None:
            d.cn_in, d.cn_dtype = cn_in.data_ptr(), L.dtype_code(cn_in.dtype)
        d.C2, d.cn_frames = C2, frames
        return unet_in, cn_in

    @staticmethod
    def _dense(t, what):
        if not t.is_cuda:
            raise RuntimeError("%s must live on the GPU; there is no CPU path" % what)
        L.dtype_code(t.dtype)
        return t if t.is_contiguous() else t.contiguous()


class EulerDiscreteScheduler(_SamplerScheduler):
    """diffusers.EulerDiscreteScheduler (v0.27 keyword names), the deterministic sampler: s_churn = 0"""
    _CLASS = "EulerDiscreteScheduler"
    _DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False, sigma_min=None, sigma_max=None,
                     timestep_spacing="linspace", timestep_type="discrete", steps_offset=0, rescale_betas_zero_snr=False)

    _REFUSED = dict(_SamplerScheduler._REFUSED, clip_sample=False, thresholding=False)
    _HARMLESS = _SamplerScheduler._HARMLESS + ("set_alpha_to_one", "clip_sample_range", "sample_max_value", "dynamic_thresholding_ratio")

    def _check_config(self):
        c = self.config
        if c.interpolation_type != "linear":
            raise ValueError("EulerDiscreteScheduler: interpolation_type %r is not built (linear is)" % (c.interpolation_type,))
        if c.prediction_type not in ("epsilon", "v_prediction", "sample"):
            raise ValueError("EulerDiscreteScheduler: prediction_type %r is not supported" % (c.prediction_type,))
        if c.timestep_type not in ("discrete", "continuous"):
            raise ValueError("EulerDiscreteScheduler: timestep_type %r is not supported" % (c.timestep_type,))
        if c.rescale_betas_zero_snr:
            raise ValueError("EulerDiscreteScheduler: rescale_betas_zero_snr is not built")
        betas = torch.tensor(c.trained_betas, dtype=torch.float64) if c.trained_betas is not None else \
            make_betas(c.beta_schedule, c.beta_start, c.beta_end, c.num_train_timesteps)
        abar = torch.cumprod(1.0 - betas, 0)
        self.alphas_cumprod = abar
        self._sigmas_train = ((1 - abar) / abar).sqrt()            # [DIFFUSERS v0.27, from knowledge: re-derive and cross-check]
        self.sigmas = None
        spaced_timesteps(c.timestep_spacing, c.num_train_timesteps, 1, c.steps_offset, False)      # refuses an unknown spacing now

    @property
    def init_noise_sigma(self):
        """[DIFFUSERS v0.27, from knowledge: re-derive and cross-check] sigma_max for linspace / trailing, else sqrt(sigma_max^2 + 1)"""
        s = self.sigmas if self.sigmas is not None else self._sigmas_train
        m = float(s.max())
        return m if self.config.timestep_spacing in ("linspace", "trailing") else math.sqrt(m * m + 1)

    def _sigma_to_t(self, sigma):
        """[DIFFUSERS v0.27, from knowledge: re-derive and cross-check] the fractional training index whose log sigma matches"""
        logs = self._sigmas_train.log()
        ls = sigma.clamp_min(1e-10).log()
        dists = ls[None, :] - logs[:, None]
        low = (dists >= 0).cumsum(0).argmax(0).clamp(max=len(logs) - 2)
        high = low + 1
        w = ((logs[low] - ls) / (logs[low] - logs[high])).clamp(0, 1)
        return (1 - w) * low + w * high

    def set_timesteps(self, num_inference_steps, device=None, aux0=None, aux1=None):
        """[DIFFUSERS v0.27, from knowledge: re-derive and cross-check] spacing -> linear interpolation of the training sigmas ->
        (optional) Karras rho = 7 -> timesteps -> a final zero sigma; then every step collapsed to (c_in, A, B) in fp64"""
        c, n = self.config, int(num_inference_steps)
        if n < 1:
            raise ValueError("num_inference_steps must be at least 1")
        T = c.num_train_timesteps
        ts = spaced_timesteps(c.timestep_spacing, T, n, c.steps_offset, False)
        sig = _interp(ts, torch.arange(T, dtype=torch.float64), self._sigmas_train)
        if c.use_karras_sigmas:
            smin = float(c.sigma_min) if c.sigma_min is not None else float(sig[-1])
            smax = float(c.sigma_max) if c.sigma_max is not None else float(sig[0])
            ramp = torch.linspace(0, 1, n, dtype=torch.float64)
            lo, hi = smin ** (1 / 7.0), smax ** (1 / 7.0)
            sig = (hi + ramp * (lo - hi)) ** 7.0
            if n > 1:
                sig[0], sig[-1] = smax, smin           # the ends exactly (the seventh power of a seventh root is not)
            ts = self._sigma_to_t(sig)
        if c.timestep_type == "continuous" and c.prediction_type == "v_prediction":
            ts = 0.25 * sig.log()
        sig = torch.cat([sig, torch.zeros(1, dtype=torch.float64)])
        rows = []
        for i in range(n):
            s, dt = float(sig[i]), float(sig[i + 1]) - float(sig[i])
            cin = 1.0 / math.sqrt(s * s + 1)
            if c.prediction_type == "epsilon":          # x0 = x - s m;  d = (x - x0) / s = m
                A, B = 1.0, dt
            elif c.prediction_type == "v_prediction":   # x0 = -s / sqrt(s^2 + 1) m + x / (s^2 + 1);  d = x s / (s^2 + 1) + m / sqrt(s^2 + 1)
                A, B = 1.0 + s * dt / (s * s + 1), dt / math.sqrt(s * s + 1)
            else:                                       # x0 = m;  d = (x - m) / s
                A, B = (1.0 + dt / s, -dt / s) if s != 0 else (float("nan"), float("nan"))
            rows.append((cin, A, B))
        self.sigmas = sig
        self._install(rows, ts, device, aux0, aux1)
        self._timesteps_host = [float(v) for v in ts.to(torch.float32)]
        self.timesteps = ts.to(torch.float32)
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    # the step index: found once from the first timestep seen (the first match), then incremented -- a repeated t does not rewind it
    def _index_for_scale(self, t):
        if self._step_index is None:
            if t is None:
                raise ValueError("EulerDiscreteScheduler: scale_model_input needs the timestep (an element of scheduler.timesteps)")
            self._step_index = self._row_for(t)
        return self._step_index

    def _index_for_step(self, t):
        if self._step_index is None:
            self._step_index = self._row_for(t)
        if self._step_index >= self.num_inference_steps:
            raise ValueError("EulerDiscreteScheduler: step() called more often than set_timesteps(%d) allows" % self.num_inference_steps)
        return self._step_index

    def _advance(self):
        self._step_index += 1

    @property
    def step_index(self):
        return self._step_index


class DDIMScheduler(_SamplerScheduler):
    """diffusers.DDIMScheduler (v0.27 keyword names), the deterministic sampler: eta = 0"""
    _CLASS = "DDIMScheduler"
    _DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading",
                     rescale_betas_zero_snr=False)
    init_noise_sigma = 1.0

    def _check_config(self):
        c = self.config
        if c.clip_sample:
            raise ValueError("DDIMScheduler: clip_sample is not built (a clipped x0 is not linear in the sample): set clip_sample=False")
        if c.thresholding:
            raise ValueError("DDIMScheduler: thresholding is not built")
        if c.prediction_type not in ("epsilon", "v_prediction", "sample"):
            raise ValueError("DDIMScheduler: prediction_type %r is not supported" % (c.prediction_type,))
        betas = torch.tensor(c.trained_betas, dtype=torch.float64) if c.trained_betas is not None else \
            make_betas(c.beta_schedule, c.beta_start, c.beta_end, c.num_train_timesteps)
        if c.rescale_betas_zero_snr:
            betas = rescale_zero_terminal_snr(betas)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0)
        self.final_alpha_cumprod = 1.0 if c.set_alpha_to_one else float(self.alphas_cumprod[0])
        spaced_timesteps(c.timestep_spacing, c.num_train_timesteps, 1, c.steps_offset, True)

    def set_timesteps(self, num_inference_steps, device=None, aux0=None, aux1=None):
        """[DIFFUSERS v0.27, from knowledge: re-derive and cross-check] integer timesteps of the spacing; step i goes from t_i to
        t_i - num_train_timesteps // n (below 0: final_alpha_cumprod), collapsed to (1, A, B) in fp64"""
        c, n = self.config, int(num_inference_steps)
        T = c.num_train_timesteps
        if n < 1 or n > T:
            raise ValueError("num_inference_steps must be in 1 .. num_train_timesteps (%d)" % T)
        ts = spaced_timesteps(c.timestep_spacing, T, n, c.steps_offset, True)
        if float(ts.max()) > T - 1 or float(ts.min()) < 0:
            raise ValueError("DDIMScheduler: timesteps %s leave the %d training steps (steps_offset too large)" % (ts.tolist(), T))
        rows = []
        for t in ts.tolist():
            t = int(t)
            p = t - T // n
            at = float(self.alphas_cumprod[t])
            ap = float(self.alphas_cumprod[p]) if p >= 0 else self.final_alpha_cumprod
            sa, sb, pa, pb = math.sqrt(at), math.sqrt(max(1 - at, 0.0)), math.sqrt(ap), math.sqrt(max(1 - ap, 0.0))
            if c.prediction_type == "epsilon":            # x0 = (x - sb m) / sa, e = m
                A, B = (pa / sa, pb - pa * sb / sa) if sa != 0 else (float("inf"), float("nan"))
            elif c.prediction_type == "sample":           # x0 = m, e = (x - sa m) / sb
                A, B = (pb / sb, pa - pb * sa / sb) if sb != 0 else (float("inf"), float("nan"))
            else:                                         # x0 = sa x - sb m, e = sa m + sb x
                A, B = pa * sa + pb * sb, pb * sa - pa * sb
            rows.append((1.0, A, B))
        self._install(rows, ts, device, aux0, aux1)
        self._timesteps_host = [float(v) for v in ts]
        self.timesteps = ts.to(torch.int64)
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    # DDIM keeps no index: the coefficients are a function of t alone, so every call finds its row (the first match of t)
    def _index_for_scale(self, t):
        return self._row_for(t) if t is not None else 0          # (c_in = 1 in every row: diffusers' DDIM ignores the timestep here)

    def _index_for_step(self, t):
        return self._row_for(t)

    def _advance(self):
        pass


def check_guidance_rescale(guidance_rescale):
    """the loops here combine u + g (c - u) only: guidance_rescale (a per-sample std ratio, not linear) is not built"""
    if guidance_rescale:
        raise ValueError("guidance_rescale > 0 is not built (the guided step is linear in the model output)")
