"""The op sequence of diffusers' EulerDiscreteScheduler.step / DDIMScheduler.step (v0.27, eta = 0, s_churn = 0) restated in torch fp64,
one operation after the other as the library performs them -- NOT collapsed to (A, B): the reference the collapsed coefficients of
ctrl_adapter_amd/schedulers.py are checked against (tests/test_scheduler_host.py) and the fp64 glue of the loop tests.
[DIFFUSERS v0.27, from knowledge: re-derive and cross-check]"""
import math

import torch


def euler_scale_model_input(sample, sigma):
    return sample / ((sigma ** 2 + 1) ** 0.5)


def euler_step(model_output, sample, sigma, sigma_next, prediction_type):
    """EulerDiscreteScheduler.step with gamma = 0 (sigma_hat = sigma, no noise)"""
    sigma_hat = sigma
    if prediction_type == "sample":
        pred_original_sample = model_output
    elif prediction_type == "epsilon":
        pred_original_sample = sample - sigma_hat * model_output
    elif prediction_type == "v_prediction":
        pred_original_sample = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
    else:
        raise ValueError(prediction_type)
    derivative = (sample - pred_original_sample) / sigma_hat
    dt = sigma_next - sigma_hat
    return sample + derivative * dt


def ddim_step(model_output, sample, alpha_prod_t, alpha_prod_t_prev, prediction_type):
    """DDIMScheduler.step with eta = 0, no clipping, no thresholding"""
    beta_prod_t = 1 - alpha_prod_t
    if prediction_type == "epsilon":
        pred_original_sample = (sample - beta_prod_t ** 0.5 * model_output) / alpha_prod_t ** 0.5
        pred_epsilon = model_output
    elif prediction_type == "sample":
        pred_original_sample = model_output
        pred_epsilon = (sample - alpha_prod_t ** 0.5 * pred_original_sample) / beta_prod_t ** 0.5
    elif prediction_type == "v_prediction":
        pred_original_sample = (alpha_prod_t ** 0.5) * sample - (beta_prod_t ** 0.5) * model_output
        pred_epsilon = (alpha_prod_t ** 0.5) * model_output + (beta_prod_t ** 0.5) * sample
    else:
        raise ValueError(prediction_type)
    std_dev_t = 0.0
    pred_sample_direction = (1 - alpha_prod_t_prev - std_dev_t ** 2) ** 0.5 * pred_epsilon
    return alpha_prod_t_prev ** 0.5 * pred_original_sample + pred_sample_direction


def ddim_alphas(sch, i):
    """(alpha_prod_t, alpha_prod_t_prev) of step i of a DDIMScheduler after set_timesteps, looked up as DDIMScheduler.step does"""
    t = int(sch.table[i, 3])
    prev_t = t - sch.config.num_train_timesteps // sch.num_inference_steps
    a_t = float(sch.alphas_cumprod[t])
    a_prev = float(sch.alphas_cumprod[prev_t]) if prev_t >= 0 else float(sch.final_alpha_cumprod)
    return a_t, a_prev


def sequential_step(sch, i, model_output, sample):
    """one step of either scheduler through the restated op sequence; fp64 tensors in, fp64 out"""
    if type(sch).__name__ == "EulerDiscreteScheduler":
        return euler_step(model_output, sample, float(sch.sigmas[i]), float(sch.sigmas[i + 1]), sch.config.prediction_type)
    a_t, a_prev = ddim_alphas(sch, i)
    return ddim_step(model_output, sample, a_t, a_prev, sch.config.prediction_type)


def sequential_scale(sch, i, sample):
    if type(sch).__name__ == "EulerDiscreteScheduler":
        return euler_scale_model_input(sample, float(sch.sigmas[i]))
    return sample


def cfg_combine(noise_pred, guidance):
    """noise_pred_uncond + guidance * (noise_pred_cond - noise_pred_uncond); guidance broadcastable"""
    u, c = noise_pred.chunk(2)
    return u + guidance * (c - u)


def euler_sigmas_numpy(cfg, n):
    """the non-Karras Euler sigmas with numpy's own interp, from fp64 betas: an independent restatement of set_timesteps' schedule"""
    import numpy as np
    T = cfg["num_train_timesteps"]
    if cfg["beta_schedule"] == "linear":
        betas = np.linspace(cfg["beta_start"], cfg["beta_end"], T, dtype=np.float64)
    else:
        betas = np.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, T, dtype=np.float64) ** 2
    ac = np.cumprod(1.0 - betas)
    sig = ((1 - ac) / ac) ** 0.5
    sp = cfg["timestep_spacing"]
    if sp == "linspace":
        ts = np.linspace(0, T - 1, n, dtype=np.float64)[::-1].copy()
    elif sp == "leading":
        ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float64) + cfg.get("steps_offset", 0)
    else:
        ts = np.round(np.arange(T, 0, -T / n)) - 1
    return ts, np.concatenate([np.interp(ts, np.arange(0, T), sig), [0.0]])


def exact_prediction(kind, prediction_type, x0, e, level):
    """the model output that is exactly right for a sample built from (x0, e): Euler at sigma = level (x = x0 + sigma e), DDIM at
    alpha_bar = level (x = sqrt(a) x0 + sqrt(1 - a) e)"""
    if prediction_type == "epsilon":
        return e
    if prediction_type == "sample":
        return x0
    if kind == "euler":
        s = level
        x = x0 + s * e
        return (x / (s * s + 1) - x0) * math.sqrt(s * s + 1) / s
    a = level
    return math.sqrt(a) * e - math.sqrt(1 - a) * x0
