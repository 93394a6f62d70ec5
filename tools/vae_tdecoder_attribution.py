"""Which activations of the temporal KL-VAE decoder may be plain fp16: the fp32 restatement (tests/vae_tdecoder_ref.py, seeded SD-VAE-config
weights with distinct mix factors, seeded N(0, 1) latents, one clip) is run with ONE stage's activations rounded to fp16 and back
(weights and everything else stay fp32), and the rel-inf error of decode(z, F).sample against the unrounded run is printed per stage.
The stages of the image decoder's table (tools/vae_decoder_attribution.py) and the two the temporal plan adds:

  head        conv_in's output (the start of the residual stream)
  resnet      the GroupNorm + SiLU outputs that conv1 / conv2 of every spatial ResNet read
  shortcut    the stream as the 1 x 1 conv_shortcut reads it
  upsample    the stream as Upsample2D's conv reads it
  attention   the mid-block attention's GroupNorm output, Q, K, V, P and O
  t_norm1     the clip-wide GroupNorm + SiLU output that conv1 of every temporal ResNet reads
  t_norm2     the same for conv2 of every temporal ResNet
  conv_out    conv_norm_out + SiLU as conv_out reads it
  all         all of the above

    python tools/vae_tdecoder_attribution.py [--device cpu|cuda] [--latent 32 32] [--frames 3] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

STAGES = ("head", "resnet", "shortcut", "upsample", "attention", "t_norm1", "t_norm2", "conv_out", "all")


def arm(ref, stage):
    """hooks `stage` into the restatement; returns what undoes it"""
    from vae_decoder_attribution import _attention_fp16, _pre, rnd
    d = ref.decoder
    handles, att = [], d.mid_block.attentions[0]
    blocks = list(d.mid_block.resnets) + [r for b in d.up_blocks for r in b.resnets]
    spatial = [b.spatial_res_block for b in blocks]
    temporal = [b.temporal_res_block for b in blocks]
    on = lambda s: stage in (s, "all")      # noqa: E731
    if on("head"):
        handles.append(d.conv_in.register_forward_hook(lambda m, a, out: rnd(out)))
    if on("resnet"):
        handles += [c.register_forward_pre_hook(_pre) for r in spatial for c in (r.conv1, r.conv2)]
    if on("shortcut"):
        handles += [r.conv_shortcut.register_forward_pre_hook(_pre) for r in spatial if r.conv_shortcut is not None]
    if on("upsample"):
        handles += [b.upsamplers[0].register_forward_pre_hook(_pre) for b in d.up_blocks if hasattr(b, "upsamplers")]
    if on("t_norm1"):
        handles += [r.conv1.register_forward_pre_hook(_pre) for r in temporal]
    if on("t_norm2"):
        handles += [r.conv2.register_forward_pre_hook(_pre) for r in temporal]
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
    from vae_decoder_ref import seeded_latents
    from vae_tdecoder_ref import SD_VAE, VaeTemporalDecoderRef, seeded_tdecoder
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--latent", type=int, nargs=2, default=(32, 32), metavar=("H", "W"))
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the table to this file")
    a = ap.parse_args()
    dev = torch.device(a.device)
    h, w = a.latent
    ref = seeded_tdecoder(VaeTemporalDecoderRef, SD_VAE, 2025).to(dev)
    lines = ["# one stage's activations rounded to fp16 in the fp32 restatement, SD-VAE-config temporal decoder, mix factors -1.5 / 0.5 / 2.0, "
             "latents [%d, 4, %d, %d] as one clip (%d x %d pixels), torch on %s: rel-inf of decode(z, %d).sample against the unrounded run"
             % (a.frames, h, w, 8 * h, 8 * w, dev.type, a.frames)]
    with torch.no_grad():
        z = seeded_latents(a.frames, h, w, seed=7 + h, device=dev).half().float()
        want = ref.decode(z, a.frames).sample
        for stage in STAGES:
            disarm = arm(ref, stage)
            got = ref.decode(z, a.frames).sample
            disarm()
            lines.append("%-10s %.2e" % (stage, ((got - want).abs().max() / want.abs().max()).item()))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
