"""EulerDiscreteScheduler / DDIMScheduler on the host (no GPU): the fp64 schedules and the collapse of every step to (c_in, A, B)."""
import itertools
import json
import math

import pytest
import torch

import helpers  # noqa: F401
import scheduler_ref as R

import ctrl_adapter_amd as P
from ctrl_adapter_amd import schedulers as S

SVD_CFG = dict(_class_name="EulerDiscreteScheduler", beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
               interpolation_type="linear", num_train_timesteps=1000, prediction_type="v_prediction", set_alpha_to_one=False,
               sigma_max=700.0, sigma_min=0.002, skip_prk_steps=True, steps_offset=1, timestep_spacing="leading",
               timestep_type="continuous", trained_betas=None, use_karras_sigmas=True)
NS = (1, 2, 7, 25, 50)
SPACINGS = ("leading", "linspace", "trailing")
PRED = ("epsilon", "v_prediction", "sample")


def _rand(seed, n=64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, dtype=torch.float64, generator=g), torch.randn(n, dtype=torch.float64, generator=g)


def _euler(pred, spacing, karras, **kw):
    return P.EulerDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type=pred,
                                    timestep_spacing=spacing, use_karras_sigmas=karras, steps_offset=1 if spacing == "leading" else 0, **kw)


def _ddim(pred, spacing, zero_snr=False, **kw):
    return P.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type=pred, clip_sample=False,
                           timestep_spacing=spacing, rescale_betas_zero_snr=zero_snr, steps_offset=1 if spacing == "leading" else 0,
                           set_alpha_to_one=False, **kw)


def _assert_collapse(sch, seed):
    x, m = _rand(seed)
    t = sch.table
    for i in range(sch.num_inference_steps):
        want = R.sequential_step(sch, i, m, x)
        got = t[i, 1] * x + t[i, 2] * m
        scale = (t[i, 1].abs() * x.abs() + t[i, 2].abs() * m.abs()).max()
        assert float((got - want).abs().max()) <= 1e-12 * float(scale), (type(sch).__name__, dict(sch.config), i)
        ws = R.sequential_scale(sch, i, x)
        assert float((t[i, 0] * x - ws).abs().max()) <= 1e-12 * float(ws.abs().max())


@pytest.mark.parametrize("pred,spacing,karras", list(itertools.product(PRED, SPACINGS, (False, True))))
def test_euler_collapse_equals_the_sequential_restatement(pred, spacing, karras):
    for n in NS:
        sch = _euler(pred, spacing, karras)
        sch.set_timesteps(n)
        assert sch.table.shape == (n, 8) and len(sch.timesteps) == n and len(sch.sigmas) == n + 1 and float(sch.sigmas[n]) == 0.0
        assert bool((sch.sigmas[:-1] > sch.sigmas[1:]).all())
        _assert_collapse(sch, n)


@pytest.mark.parametrize("pred,spacing", list(itertools.product(PRED, SPACINGS)))
def test_ddim_collapse_equals_the_sequential_restatement(pred, spacing):
    for n in NS:
        for zero_snr in (False, True):
            if zero_snr and pred == "epsilon" and spacing != "leading":
                continue                      # alpha_bar = 0 at t = 999: refused (test_refusals)
            sch = _ddim(pred, spacing, zero_snr)
            sch.set_timesteps(n)
            assert sch.timesteps.dtype == torch.int64 and len(sch.timesteps) == n and bool((sch.table[:, 0] == 1).all())
            _assert_collapse(sch, n)


@pytest.mark.parametrize("pred,spacing,karras", list(itertools.product(("epsilon", "v_prediction", "sample"), SPACINGS, (False, True))))
def test_euler_invariant_exact_prediction_walks_down_the_sigmas(pred, spacing, karras):
    """oracle-free: with the exact prediction x stays x0 + sigma e along the whole schedule and ends at x0"""
    x0, e = _rand(5)
    for n in NS:
        sch = _euler(pred, spacing, karras)
        sch.set_timesteps(n)
        sig, t = sch.sigmas, sch.table
        x = x0 + float(sig[0]) * e
        scale = float((x0.abs() + float(sig[0]) * e.abs()).max())
        for i in range(n):
            m = R.exact_prediction("euler", pred, x0, e, float(sig[i]))
            x = t[i, 1] * x + t[i, 2] * m
            assert float((x - (x0 + float(sig[i + 1]) * e)).abs().max()) <= 1e-10 * scale, (pred, spacing, karras, n, i)
        assert float((x - x0).abs().max()) <= 1e-10 * scale


@pytest.mark.parametrize("pred,spacing", list(itertools.product(PRED, SPACINGS)))
def test_ddim_invariant_exact_prediction_follows_alpha_bar(pred, spacing):
    x0, e = _rand(6)
    for n in NS:
        sch = _ddim(pred, spacing)
        sch.set_timesteps(n)
        t = sch.table
        for i in range(n):
            a_t, a_prev = R.ddim_alphas(sch, i)
            m = R.exact_prediction("ddim", pred, x0, e, a_t)
            # the sample this step starts from is the exact one of ITS alpha_bar (consecutive timesteps need not chain: trailing / linspace)
            x = math.sqrt(a_t) * x0 + math.sqrt(1 - a_t) * e
            x = t[i, 1] * x + t[i, 2] * m
            want = math.sqrt(a_prev) * x0 + math.sqrt(1 - a_prev) * e
            assert float((x - want).abs().max()) <= 1e-10 * float((x0.abs() + e.abs()).max()), (pred, spacing, n, i)


def test_ddim_leading_steps_chain_down_to_the_final_alpha():
    """leading spacing: step i ends where step i + 1 starts, and the last one at final_alpha_cumprod"""
    x0, e = _rand(7)
    for pred in PRED:
        sch = _ddim(pred, "leading")
        sch.set_timesteps(25)
        a0 = R.ddim_alphas(sch, 0)[0]
        x = math.sqrt(a0) * x0 + math.sqrt(1 - a0) * e
        for i in range(25):
            a_t, a_prev = R.ddim_alphas(sch, i)
            x = sch.table[i, 1] * x + sch.table[i, 2] * R.exact_prediction("ddim", pred, x0, e, a_t)
            if i + 1 < 25:
                assert R.ddim_alphas(sch, i + 1)[0] == a_prev
        af = sch.final_alpha_cumprod
        assert float((x - (math.sqrt(af) * x0 + math.sqrt(1 - af) * e)).abs().max()) <= 1e-10 * float((x0.abs() + e.abs()).max())


@pytest.mark.parametrize("spacing", SPACINGS)
def test_euler_sigmas_match_a_numpy_restatement(spacing):
    cfg = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing=spacing,
               steps_offset=1 if spacing == "leading" else 0)
    for n in NS:
        sch = P.EulerDiscreteScheduler(**cfg)
        sch.set_timesteps(n)
        ts, sig = R.euler_sigmas_numpy(cfg, n)
        assert torch.allclose(sch.sigmas, torch.from_numpy(sig), rtol=1e-12, atol=0)
        assert torch.allclose(sch.timesteps.double(), torch.from_numpy(ts), rtol=1e-6, atol=0)
        want = float(sig.max()) if spacing != "leading" else math.sqrt(float(sig.max()) ** 2 + 1)
        assert abs(sch.init_noise_sigma - want) <= 1e-12 * want


def test_svd_config_anchors():
    for n in (2, 7, 25, 50):
        sch = P.EulerDiscreteScheduler.from_config(SVD_CFG)
        sch.set_timesteps(n)
        s = sch.sigmas
        assert float(s[0]) == 700.0 and float(s[n - 1]) == 0.002 and float(s[n]) == 0.0
        assert torch.equal(sch.timesteps, (0.25 * s[:n].log()).float())
        assert torch.equal(sch.table[:, 3], 0.25 * s[:n].log())
        assert sch.init_noise_sigma == math.sqrt(700.0 ** 2 + 1)
        assert bool((s[:-1] > s[1:]).all())
    # rho = 7: the middle of an odd schedule is the mean of the seventh roots
    sch.set_timesteps(3)
    assert abs(float(sch.sigmas[1]) - ((700.0 ** (1 / 7) + 0.002 ** (1 / 7)) / 2) ** 7) <= 1e-12 * float(sch.sigmas[1])


def test_step_index_advances_like_diffusers():
    """Euler finds its row once (the first match of t), then increments -- a repeated t does not rewind it; DDIM looks t up every call"""
    sch = _euler("epsilon", "leading", False)
    sch.set_timesteps(5)
    ts = [float(t) for t in sch.timesteps]
    assert sch.step_index is None
    assert sch._index_for_scale(sch.timesteps[1]) == 1 and sch._index_for_step(ts[1]) == 1
    sch._advance()
    assert sch._index_for_step(ts[1]) == 2            # the same t again: the index moved on
    sch._advance()
    assert sch.step_index == 3
    sch.set_timesteps(5)
    assert sch.step_index is None and sch._index_for_step(sch.timesteps[0]) == 0
    with pytest.raises(ValueError, match="not in the schedule"):
        S._find_row(ts, 12345.0)
    d = _ddim("epsilon", "leading")
    d.set_timesteps(4)
    for i, t in enumerate(d.timesteps):
        assert d._index_for_step(t) == i and d._index_for_step(int(t)) == i
        d._advance()
    assert d._index_for_step(d.timesteps[2]) == 2
    # a schedule with a repeated timestep: the first match
    assert S._find_row([9.0, 5.0, 5.0, 1.0], torch.tensor(5.0)) == 1


def test_refusals():
    with pytest.raises(ValueError, match="clip_sample"):
        P.DDIMScheduler()                                                       # diffusers' default clips
    with pytest.raises(ValueError, match="thresholding"):
        P.DDIMScheduler(clip_sample=False, thresholding=True)
    with pytest.raises(ValueError, match="interpolation_type"):
        P.EulerDiscreteScheduler(interpolation_type="log_linear")
    with pytest.raises(ValueError, match="prediction_type"):
        P.EulerDiscreteScheduler(prediction_type="flow")
    with pytest.raises(ValueError, match="timestep_spacing"):
        P.EulerDiscreteScheduler(timestep_spacing="sideways")
    with pytest.raises(ValueError, match="beta_schedule"):
        P.DDIMScheduler(clip_sample=False, beta_schedule="sigmoid")
    with pytest.raises(ValueError, match="not built as"):
        P.EulerDiscreteScheduler.from_config({"_class_name": "DPMSolverMultistepScheduler"})
    with pytest.raises(ValueError, match="not built as"):
        P.DDIMScheduler.from_config(SVD_CFG)
    with pytest.raises(ValueError, match="final_sigmas_type"):
        P.EulerDiscreteScheduler(final_sigmas_type="sigma_min")
    with pytest.raises(ValueError, match="not known here"):
        P.EulerDiscreteScheduler(use_flow_sigmas=True)                           # a key of a newer config: refused, not dropped
    with pytest.raises(ValueError, match="not known here"):
        P.DDIMScheduler(clip_sample=False, some_future_switch=1)
    with pytest.raises(ValueError, match="clip_sample"):
        P.EulerDiscreteScheduler(clip_sample=True)
    with pytest.raises(ValueError, match="needs the timestep"):
        _euler("epsilon", "leading", False).scale_model_input(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match="guidance_rescale"):
        P.DenoiseLoop(_euler("epsilon", "leading", False), lambda *a: None, guidance_rescale=0.7)
    x = torch.zeros(1, 4, 8, 8)
    e = _euler("epsilon", "leading", False)
    e.set_timesteps(3)
    with pytest.raises(ValueError, match="eta"):
        e.step(x, e.timesteps[0], x, eta=0.5)
    with pytest.raises(ValueError, match="s_churn"):
        e.step(x, e.timesteps[0], x, s_churn=0.1)
    d = _ddim("v_prediction", "trailing", zero_snr=True)
    d.set_timesteps(3)
    with pytest.raises(ValueError, match="eta"):
        d.step(x, d.timesteps[0], x, eta=1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        e.step(x, e.timesteps[0], x)                                           # there is no eager fall-back
    # epsilon prediction cannot leave alpha_bar = 0
    z = _ddim("epsilon", "trailing", zero_snr=True)
    with pytest.raises(ValueError, match="not finite"):
        z.set_timesteps(10)
    assert float(z.alphas_cumprod[-1]) == 0.0
    _ddim("v_prediction", "trailing", zero_snr=True).set_timesteps(10)


def test_from_pretrained_and_surface(tmp_path):
    d = tmp_path / "ckpt" / "scheduler"
    d.mkdir(parents=True)
    (d / "scheduler_config.json").write_text(json.dumps(dict(SVD_CFG, _diffusers_version="0.24.0.dev0")))
    sch = P.EulerDiscreteScheduler.from_pretrained(str(tmp_path / "ckpt"), subfolder="scheduler")
    assert sch.config.sigma_max == 700.0 and sch.config.use_karras_sigmas and sch.config.num_train_timesteps == 1000
    assert sch.order == 1 and sch.init_noise_sigma > 0
    sch.set_timesteps(4, device="cpu")
    assert sch.timesteps.dtype == torch.float32 and sch.timesteps.shape == (4,)
    for name in ("set_timesteps", "scale_model_input", "step", "from_config", "from_pretrained", "model_input", "guided_step", "reset"):
        assert callable(getattr(sch, name))
    with pytest.raises(FileNotFoundError):
        P.EulerDiscreteScheduler.from_pretrained(str(tmp_path / "ckpt"), subfolder="nothing")
    dd = P.DDIMScheduler.from_config(dict(_class_name="DDIMScheduler", clip_sample=False, prediction_type="v_prediction",
                                          rescale_betas_zero_snr=True, timestep_spacing="trailing", beta_schedule="scaled_linear",
                                          beta_start=0.00085, beta_end=0.012, set_alpha_to_one=False, steps_offset=1))
    assert dd.init_noise_sigma == 1.0 and dd.order == 1 and dd.config.num_train_timesteps == 1000
    dd.set_timesteps(50)
    assert dd.timesteps[0] == 999 and len(dd.timesteps) == 50
    # the aux columns: default the model's timestep, or what the caller hands over
    sch.set_timesteps(3, aux0=[5.0, 4.0, 3.0], aux1=20)
    assert sch.table[:, 4].tolist() == [5.0, 4.0, 3.0] and sch.table[:, 5].tolist() == [20.0] * 3


def test_controlnet_keep_window():
    from ctrl_adapter_amd.denoise import controlnet_keep
    assert controlnet_keep(5) == [1.0] * 5
    assert controlnet_keep(5, 0.0, 0.6) == [1.0, 1.0, 1.0, 0.0, 0.0]
    assert controlnet_keep(4, 0.5, 1.0) == [0.0, 0.0, 1.0, 1.0]


def test_sampler_launch_shape_and_descriptor_checks_on_the_host():
    """ctrl_op_sampler_launch_shape: the vector path needs inner, the frame plane, the guidance stride and every pointer to allow 16-byte
    accesses; the grid is capped; bad descriptors are refused with a message (host code: no device needed)"""
    import ctypes as C
    from ctrl_adapter_amd import _lib as L
    lib = L.lib()

    def shape(d, step, inp):
        b, v, cap = C.c_int(), C.c_int(), C.c_int()
        rc = lib.ctrl_op_sampler_launch_shape(C.byref(d), step, inp, C.byref(b), C.byref(v), C.byref(cap))
        return rc, b.value, v.value, cap.value

    def desc(inner=64, outer=2, off=0, **kw):
        d = L.SamplerDesc()
        d.x, d.prev, d.model_out, d.unet_in = 0x10000 + off, 0x10000 + off, 0x20000, 0x30000
        d.x_dtype = d.prev_dtype = d.mo_dtype = d.unet_dtype = d.cn_dtype = d.concat_dtype = L.F16
        d.outer, d.C, d.inner, d.R, d.g_count, d.g_inner = outer, 4, inner, 2, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert shape(desc(), 1, 1) == (0, 1, 8, 1024)                       # 512 elements: 64 chunks, one workgroup
    assert shape(desc(inner=30), 1, 1)[1:3] == (1, 1)
    assert shape(desc(off=2), 1, 1)[2] == 1                              # a base pointer one fp16 past the boundary
    # one pointer at a time, in the launches that read or write it: each alone must send the launch down the scalar path
    full = dict(cn_in=0x50000, concat=0x60000, C2=4, g=0x40000, g_count=1, g_inner=64)
    assert shape(desc(**full), 1, 1)[2] == 8 and shape(desc(**full), 0, 1)[2] == 8 and shape(desc(**full), 1, 0)[2] == 8
    for field, step, inp in (("x", 1, 1), ("x", 0, 1), ("x", 1, 0), ("prev", 1, 0), ("prev", 1, 1), ("model_out", 1, 0), ("model_out", 1, 1),
                             ("unet_in", 0, 1), ("unet_in", 1, 1), ("concat", 0, 1), ("concat", 1, 1), ("cn_in", 0, 1), ("cn_in", 1, 1)):
        d = desc(**full)
        if field in ("x", "prev"):
            d.prev = 0x70000                                              # out of place, so that x and prev move separately
        setattr(d, field, getattr(d, field) + 2)
        assert shape(d, step, inp)[:1] + shape(d, step, inp)[2:3] == (0, 1), (field, step, inp)
    # ... and a pointer the launch does not touch does not matter
    d = desc(**full)
    d.model_out += 2
    assert shape(d, 0, 1)[2] == 8
    d = desc(**full)
    d.unet_in += 2
    d.concat += 2
    d.cn_in += 2
    assert shape(d, 1, 0)[2] == 8
    assert shape(desc(g=0x40000, g_count=3, g_inner=36), 1, 0)[2] == 1 and shape(desc(g=0x40000, g_count=3, g_inner=64), 1, 0)[2] == 8
    assert shape(desc(inner=3 * 36, cn_in=0x50000, cn_frames=3), 0, 1)[2] == 1 and shape(desc(inner=3 * 64, cn_in=0x50000, cn_frames=3), 0, 1)[2] == 8
    rc, b, v, cap = shape(desc(inner=1 << 16, outer=16), 1, 0)
    assert (rc, b, v) == (0, cap, 8) and (16 * 4 << 16) // 8 > cap * 256
    for bad, word in ((desc(R=3), "R must be 1 or 2"), (desc(inner=0), "positive"), (desc(cn_in=0x50000, cn_frames=5), "cn_frames"),
                      (desc(C2=4), "concat and C2"), (desc(unet_in=0x10000), "alias"), (desc(prev_dtype=L.F32), "in place")):
        assert shape(bad, 1, 1)[0] == 1 and word in lib.ctrl_last_error().decode(), word
    assert shape(desc(), 0, 0)[0] == 1
