"""Which activations of the KL-VAE decoder may be plain fp16: the fp32 restatement (tests/vae_decoder_ref.py, seeded SD VAE weights, seeded
N(0, 1) latents) is run with ONE stage's activations rounded to fp16 and back (weights and everything else stay fp32), and the rel-inf
error of decode(z).sample against the unrounded run is printed per stage.  The stages are the candidates of the decoder plan's precision
selection:

  head       conv_in's output (the start of the residual stream)
  resnet     the GroupNorm + SiLU outputs that conv1 / conv2 of every ResNet read
  shortcut   the stream as the 1 x 1 conv_shortcut reads it
  upsample   the stream as Upsample2D's conv reads it
  attention  the mid-block attention's GroupNorm output, Q, K, V, P (the softmax's output) and O
  conv_out   conv_norm_out + SiLU as conv_out reads it
  all        all of the above

    python tools/vae_decoder_attribution.py [--device cpu|cuda] [--latent 32 32] [--out FILE]

Runs on the CPU at the default 32 x 32 latents (256^2 pixels); on a GPU 128 x 128 (1024^2, the attention's L = 16384) takes seconds."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STAGES = ("head", "resnet", "shortcut", "upsample", "attention", "conv_out", "all")


def rnd(t):
    return t.half().float()


def _pre(mod, args):
    return (rnd(args[0]),)


def _attention_fp16(att):
    """AttentionRef.forward with its GroupNorm output, Q, K, V, P and O rounded to fp16 (the softmax itself in fp32, as the plan's)"""
    def forward(x):
        B, C, H, W = x.shape
        h = rnd(att.group_norm(x).view(B, C, H * W).transpose(1, 2))
        q, k, v = rnd(att.to_q(h)), rnd(att.to_k(h)), rnd(att.to_v(h))
        p = rnd(torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=-1))
        o = att.to_out[0](rnd(p @ v))
        return o.transpose(1, 2).reshape(B, C, H, W) + x
    return forward


def arm(ref, stage):
    """hooks `stage` into the restatement; returns what undoes it"""
    d = ref.decoder
    handles, att = [], d.mid_block.attentions[0]
    resnets = list(d.mid_block.resnets) + [r for b in d.up_blocks for r in b.resnets]
    on = lambda s: stage in (s, "all")
    if on("head"):
        handles.append(d.conv_in.register_forward_hook(lambda m, a, out: rnd(out)))
    if on("resnet"):
        handles += [c.register_forward_pre_hook(_pre) for r in resnets for c in (r.conv1, r.conv2)]
    if on("shortcut"):
        handles += [r.conv_shortcut.register_forward_pre_hook(_pre) for r in resnets if r.conv_shortcut is not None]
    if on("upsample"):
        handles += [b.upsamplers[0].register_forward_pre_hook(_pre) for b in d.up_blocks if hasattr(b, "upsamplers")]
    if on("conv_out"):
        handles.append(d.conv_out.register_forward_pre_hook(_pre))
    if on("attention"):
        att.forward = _attention_fp16(att)

    def disarm():
        for h in handles:
            h.remove()
        att.__dict__.pop("forward", None)
    return disarm


def main():
    from ctrl_adapter_amd.synthetic import seeded_init
    from vae_decoder_ref import SD_VAE, VaeDecoderRef, seeded_latents
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--latent", type=int, nargs=2, default=(32, 32), metavar=("H", "W"))
    ap.add_argument("--out", default=None, help="append the table to this file")
    a = ap.parse_args()
    dev = torch.device(a.device)
    h, w = a.latent
    ref = seeded_init(VaeDecoderRef(**SD_VAE), seed=2024).eval().to(dev)
    lines = ["# one stage's activations rounded to fp16 in the fp32 restatement, SD VAE decoder, latents [1, 4, %d, %d] (%d x %d pixels, "
             "attention L = %d), torch on %s: rel-inf of decode(z).sample against the unrounded run" % (h, w, 8 * h, 8 * w, h * w, dev.type)]
    with torch.no_grad():
        z = seeded_latents(1, h, w, seed=7 + h, device=dev).half().float()
        want = ref.decode(z).sample
        for stage in STAGES:
            disarm = arm(ref, stage)
            got = ref.decode(z).sample
            disarm()
            lines.append("%-10s %.2e" % (stage, ((got - want).abs().max() / want.abs().max()).item()))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
