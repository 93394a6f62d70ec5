"""Fingerprints of the libctrlhip plans, for comparing two builds of the library (a refactor against its parent): run it in both
trees and diff the output.  Every line must be identical.

  --spec   (no GPU) sha256 of the (name, shape) parameter inventory of each of the six plans, for the default configuration and the
           tiny one its GPU test uses.  The ControlNet, adapter, vision and VAE inventories come from the library (ctrl_*_param_spec,
           through the mirror that registers them); the text towers' from text_encoder_spec.
  default  (GPU) builds each stand-alone plan (text, vision, VAE encoder, VAE decoder, whole VAE) from seeded weights at the smallest
           shapes that reach every shared code path and prints the sha256 of every output tensor's bytes and of the ordered kernel
           symbols ops.Profiler records for the call.  The ControlNet and the SDXL adapter follow at 16 x 16 latents, N = 2: the plans
           whose convolutions split K (scratch and tickets carved per descriptor) and whose sibling blocks share grouped launches.

Only names both trees have are used: the mirrors, synthetic.seeded_init, ops.Profiler and text_encoder._forward_ext (the one entry
that reaches the text plan's hidden_index)."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import ctrl_adapter_amd as P  # noqa: E402
from ctrl_adapter_amd import _lib as L  # noqa: E402
from ctrl_adapter_amd import ops, text_encoder  # noqa: E402
from ctrl_adapter_amd.synthetic import seeded_init, seeded_tensor  # noqa: E402

# the configurations of tests/golden/cases.py and tests/*_ref.py (TINY), restated: tools do not import tests
ADAPTER_SDXL = dict(backbone_model_name="sdxl", num_blocks=1, num_frames=1, num_adapters_per_location=3, cross_attention_dim=2048,
                    add_spatial_resnet=True, add_temporal_resnet=False, add_spatial_transformer=True, add_temporal_transformer=False,
                    add_adapter_location_A=True, add_adapter_location_B=True, add_adapter_location_C=True,
                    add_adapter_location_D=False, add_adapter_location_M=False)
ADAPTER_VIDEO = dict(backbone_model_name="i2vgen-xl", num_blocks=1, num_frames=4, num_adapters_per_location=3, cross_attention_dim=1024,
                     add_spatial_resnet=True, add_temporal_resnet=True, add_spatial_transformer=True, add_temporal_transformer=True,
                     add_adapter_location_A=True, add_adapter_location_B=True, add_adapter_location_C=True,
                     add_adapter_location_D=True, add_adapter_location_M=True)
TEXT_TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=77)
VISION_TINY = dict(hidden_size=128, intermediate_size=256, projection_dim=96, num_hidden_layers=2, num_attention_heads=2, image_size=56,
                   patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5)
VAE_TINY = dict(block_out_channels=(32, 64), layers_per_block=1, latent_channels=4)
VAE_FLAT = dict(block_out_channels=(32, 32), layers_per_block=1, latent_channels=4)       # no shortcut convolution anywhere


def sha(data):
    return hashlib.sha256(data).hexdigest()


def spec_sha(spec):
    return sha(repr([(n, tuple(int(v) for v in s)) for n, s in spec]).encode())


def spec_mode():
    text_args = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "max_position_embeddings")
    text_default = P.CLIPTextModel().config
    plans = [
        ("controlnet", lambda kw: P.ControlNetModel(**kw)._spec, dict(), dict(cross_attention_dim=768)),
        ("adapter", lambda kw: P.ControlNetAdapter(**kw)._spec, dict(backbone_model_name="sdxl", cross_attention_dim=2048), ADAPTER_SDXL),
        ("text", lambda kw: text_encoder.text_encoder_spec(*[kw[a] for a in text_args]), {a: text_default[a] for a in text_args}, TEXT_TINY),
        ("vision", lambda kw: P.CLIPVisionModelWithProjection(**kw)._spec, dict(), VISION_TINY),
        ("vae_encoder", lambda kw: P.AutoencoderKLEncoder(**kw)._spec, dict(), VAE_TINY),
        ("vae_decoder", lambda kw: P.AutoencoderKLDecoder(**kw)._spec, dict(), VAE_TINY),
    ]
    for name, make, default, tiny in plans:
        # (the adapter's default enables no location and has no parameters: its video configuration stands beside it)
        for tag, kw in (("default", default), ("tiny", tiny)) + ((("video", ADAPTER_VIDEO),) if name == "adapter" else ()):
            spec = make(kw)
            print("spec %-12s %-8s entries %4d sha256 %s" % (name, tag, len(spec), spec_sha(spec)))


def tensor_sha(t):
    if t is None:
        return "-"
    t = t.detach().contiguous().cpu()
    return sha(t.view(torch.uint8).numpy().tobytes())[:32]


def case(tag, fn):
    """runs fn() plain and once more under the profiler; prints the outputs' digests and the launch list's"""
    outs = fn()
    torch.cuda.synchronize()
    with ops.Profiler() as prof:
        again = fn()
        torch.cuda.synchronize()
    same = all(tensor_sha(a) == tensor_sha(b) for a, b in zip(outs, again))
    syms = [sym for _, sym, _, _, _, _, _ in prof.launches]
    print("%-58s out %s | launches %3d %s%s" % (tag, " ".join(tensor_sha(o) for o in outs), len(syms),
                                                 sha("\n".join(syms).encode())[:16] if syms else "-", "" if same else " PROFILED-RUN-DIFFERS"))


def gpu_mode():
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    hidden_cases = [(-1, True), (-1, False), (1, True), (1, False)]         # (hidden_index, tail outputs asked for)

    # ---- text towers: hidden 64, 2 layers, N = 2, L = 5
    tkw = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, eos_token_id=2)
    ids = torch.randint(3, 100, (2, 5), generator=torch.Generator().manual_seed(7))
    ids[:, -1] = 2
    ids = ids.to(dev)
    m = seeded_init(P.CLIPTextModel(**tkw), seed=41).to(dev)
    for hs in (False, True):
        def run(hs=hs):
            o = m(ids, output_hidden_states=hs)
            return [o[0], o[1]] + (list(o[2]) if hs else [])
        case("text noproj form0 quick_gelu hidden_states=%d" % hs, run)
    for hi, tail in hidden_cases:
        case("text noproj form0 quick_gelu hidden_index=%d tail=%d" % (hi, tail),
             lambda hi=hi, tail=tail: text_encoder._forward_ext(m, ids, last=tail, pooled=tail, hidden_index=hi))
    for form in (0, 1):
        for act in ("quick_gelu", "gelu"):
            mp = seeded_init(P.CLIPTextModelWithProjection(**tkw, projection_dim=32, hidden_act=act, gemm_form=form), seed=41).to(dev)
            for hi, tail in hidden_cases:
                case("text proj form%d %s hidden_index=%d tail=%d" % (form, act, hi, tail),
                     lambda hi=hi, tail=tail: text_encoder._forward_ext(mp, ids, last=tail, pooled=tail, embeds=tail, hidden_index=hi))

    # ---- vision tower: image 28, patch 14 (L = 5), hidden 64, 2 layers, N = 2
    px = seeded_tensor((2, 3, 28, 28), 11).to(dev)
    for form in (0, 1):
        for act in ("quick_gelu", "gelu"):
            mv = seeded_init(P.CLIPVisionModelWithProjection(hidden_size=64, intermediate_size=128, projection_dim=32, num_hidden_layers=2,
                                                             num_attention_heads=1, image_size=28, patch_size=14, hidden_act=act,
                                                             gemm_form=form), seed=43).to(dev)
            for hi, tail in hidden_cases:
                case("vision form%d %s hidden_index=%d tail=%d" % (form, act, hi, tail),
                     lambda hi=hi, tail=tail: mv.run(px, last=tail, pooled=tail, embeds=tail, hidden_index=hi))

    # ---- KL-VAE: 16 x 16 images / 8 x 8 latents, N = 2
    x = seeded_tensor((2, 3, 16, 16), 13).to(dev)
    for name, kw in (("(32,64)", VAE_TINY), ("(32,32)", VAE_FLAT)):
        f = 2 ** (len(kw["block_out_channels"]) - 1)
        enc = seeded_init(P.AutoencoderKLEncoder(**kw), seed=45).to(dev)
        eps = seeded_tensor((2, 4, 16 // f, 16 // f), 17).to(dev)
        for kind, kname in ((L.VAE_MODE, "mode"), (L.VAE_SAMPLE, "sample"), (L.VAE_MOMENTS, "moments")):
            case("vae_encoder %s %s" % (name, kname),
                 lambda kind=kind: [enc.run(x, kind, eps=eps if kind == L.VAE_SAMPLE else None, scale=0.5)])
        dec = seeded_init(P.AutoencoderKLDecoder(**kw), seed=47).to(dev)
        z = seeded_tensor((2, 4, 8, 8), 19).to(dev)
        for kind, kname in ((L.VAE_DEC_SAMPLE, "sample"), (L.VAE_DEC_UNIT, "unit"), (L.VAE_DEC_U8, "u8")):
            case("vae_decoder %s %s" % (name, kname), lambda kind=kind: [dec.run(z, kind, scale=2.0)])
        clip = seeded_tensor((4, 3, 8, 8), 23).to(dev)            # [C, F, h, w]: its frames as the strided [F, C, h, w] view
        case("vae_decoder %s strided view" % name, lambda: [dec.run(clip.transpose(0, 1))])
    vae = seeded_init(P.AutoencoderKL(**VAE_TINY), seed=49).to(dev)

    def round_trip():
        dist = vae.encode(x).latent_dist
        return [dist.mean, dist.logvar, vae.decode(dist.mode()).sample]
    case("AutoencoderKL (32,64) encode -> mode -> decode", round_trip)

    # ---- ControlNet (SD-1.5 defaults, cross-attention 768) and the SDXL adapter over its pyramid: 16 x 16 latents, N = 2
    cn = seeded_init(P.ControlNetModel(cross_attention_dim=768), seed=11).to(dev)
    ad = seeded_init(P.ControlNetAdapter(**ADAPTER_SDXL), seed=22).to(dev)
    sample, cond = seeded_tensor((2, 4, 16, 16), 101).half().to(dev), seeded_tensor((2, 3, 128, 128), 103, kind="uniform").half().to(dev)
    ehs, ehs_a = seeded_tensor((2, 77, 768), 102).half().to(dev), seeded_tensor((2, 77, 2048), 7).half().to(dev)
    t = torch.tensor([999.0, 249.0]).to(dev)

    def controlnet():
        down, mid = cn(sample, t, ehs, cond, return_dict=False)
        return list(down) + [mid]
    case("controlnet 16x16 N=2", controlnet)
    down = controlnet()[:-1]
    case("adapter sdxl over the controlnet pyramid", lambda: [o for o in ad(down, num_frames=1, timestep=torch.tensor(499.0),
                                                                            encoder_hidden_states=ehs_a)[0] if o is not None])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--spec", action="store_true", help="parameter inventories only (no GPU)")
    if ap.parse_args().spec:
        spec_mode()
    else:
        gpu_mode()
