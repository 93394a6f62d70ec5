"""Times the CLIP text encoder (SD-1.5 shape, L = 77) on one GPU: the HIP plan (ctrl_adapter_amd.CLIPTextModel, fp16) against
transformers' CLIPTextModel in fp16 on torch-ROCm (eager), same weights, same GPU, same run.  Device events, warm-up, A/B runs
alternated in rounds; prints the median and the spread (min .. max over rounds) per batch, the fp16 error of both against the fp32
restatement (tests/clip_text_ref.py, at B = 2), and the HIP plan's per-class times from the kernel profiler (ctrl_prof_*).

    python tools/text_encoder_bench.py [--batches 1,2,16] [--rounds 7] [--iters 20] [--out profiles/text_encoder_bench.txt]
    python tools/text_encoder_bench.py --model sdxl [--out profiles/sdxl_text_encoder_bench.txt]

--model sdxl times SDXL's OpenCLIP bigG tower (ctrl_adapter_amd.CLIPTextModelWithProjection, fp16) with gemm_form 0 (pinned GEMM)
against gemm_form 1 (the few-row GEMM) and transformers' CLIPTextModelWithProjection(output_hidden_states=True), and the whole SDXL
prompt encoding from token ids: encode_sdxl_prompt on the mirrors against the pipeline's four transformers calls.

Without transformers the baseline is skipped with a message."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="sd15", choices=["sd15", "sdxl"])
    a = ap.parse_args()
    if a.model == "sdxl":
        return main_sdxl(a)
    torch.set_grad_enabled(False)
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from ctrl_adapter_amd.synthetic import seeded_init
    from clip_text_ref import CLIPTextRef, SD15, seeded_ids
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ref = seeded_init(CLIPTextRef(**SD15).eval(), seed=41)
    sd = ref.state_dict()
    hip = P.CLIPTextModel(**SD15)
    hip.load_state_dict(sd)
    hip = hip.to(dev, torch.float16)
    hf = None
    try:
        from transformers import CLIPTextConfig, CLIPTextModel
        c = CLIPTextConfig(vocab_size=SD15["vocab_size"], hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                           num_attention_heads=12, max_position_embeddings=77, eos_token_id=2, bos_token_id=0, pad_token_id=1)
        hf = CLIPTextModel(c).eval()
        prefixed = any(k.startswith("text_model.") for k in hf.state_dict())
        hf.load_state_dict({(k if prefixed else k[len("text_model."):]): v for k, v in sd.items()})
        hf = hf.to(dev, torch.float16)
        say("baseline: transformers %s CLIPTextModel fp16, attention %s" % (__import__("transformers").__version__,
                                                                             getattr(hf.config, "_attn_implementation", "?")))
    except ImportError:
        say("baseline skipped: transformers is not installed")
    say("device: %s" % torch.cuda.get_device_name(0))

    ids2 = seeded_ids(2, 77, SD15["vocab_size"], seed=3)
    want = ref(ids2)
    err = lambda x, y: ((x.float().cpu() - y).abs().max() / y.abs().max()).item()      # noqa: E731
    o = hip(ids2.to(dev))
    say("fp16 error vs fp32 restatement (B = 2): HIP last %.2e pooled %.2e" % (err(o[0], want[0]), err(o[1], want[1])))
    if hf is not None:
        o = hf(ids2.to(dev))
        say("                                     transformers last %.2e pooled %.2e" % (err(o.last_hidden_state, want[0]),
                                                                                          err(o.pooler_output, want[1])))

    say("%-4s %-14s %10s %22s" % ("B", "path", "median ms", "spread (min..max) ms"))
    for B in [int(b) for b in a.batches.split(",")]:
        ids = seeded_ids(B, 77, SD15["vocab_size"], seed=B).to(dev)
        runs = {"hip": lambda: hip(ids)}
        if hf is not None:
            runs["transformers"] = lambda: hf(ids)
        for f in runs.values():          # warm-up (plan creation, workspace, kernels loaded)
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for r in range(a.rounds):       # alternated A / B rounds
            order = list(runs) if r % 2 == 0 else list(runs)[::-1]
            for k in order:
                t[k].append(timed(runs[k], a.iters))
        for k, v in t.items():
            say("%-4d %-14s %10.3f %12.3f .. %.3f" % (B, k, statistics.median(v), min(v), max(v)))
        if "transformers" in t:
            say("%-4d speed-up       %10.2fx" % (B, statistics.median(t["transformers"]) / statistics.median(t["hip"])))
        with ops.Profiler() as p:
            hip(ids)
        torch.cuda.synchronize()
        tot = sum(v[0] for v in p.rows.values())
        say("     HIP per class (profiled, serialised launches: %d launches, %.3f ms):" % (sum(v[1] for v in p.rows.values()), tot))
        for name, (ms, n, fl, by) in sorted(p.rows.items(), key=lambda kv: -kv[1][0]):
            say("       %-14s %3d launches %8.3f ms  %7.1f TFLOP/s  %7.1f GB/s" % (name, n, ms, fl / ms / 1e9 if ms else 0, by / ms / 1e6 if ms else 0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def _ab(say, runs, rounds, iters):
    for f in runs.values():              # warm-up (plan creation, workspace, kernels loaded)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for r in range(rounds):              # alternated rounds
        order = list(runs) if r % 2 == 0 else list(runs)[::-1]
        for k in order:
            t[k].append(timed(runs[k], iters))
    for k, v in t.items():
        say("     %-22s %10.3f %12.3f .. %.3f" % (k, statistics.median(v), min(v), max(v)))
    return {k: statistics.median(v) for k, v in t.items()}


def _per_class(say, P, fn, weight_bytes):
    from ctrl_adapter_amd import ops
    with ops.Profiler() as p:
        fn()
    torch.cuda.synchronize()
    tot = sum(v[0] for v in p.rows.values())
    say("     per class (profiled, serialised launches: %d launches, %.3f ms):" % (sum(v[1] for v in p.rows.values()), tot))
    for name, (ms, n, fl, by) in sorted(p.rows.items(), key=lambda kv: -kv[1][0]):
        extra = ""
        if name in ("text_gemm", "igemm_rows") and ms:
            extra = "  %.2f TB/s of weight bytes" % (weight_bytes / ms / 1e9)
        say("       %-14s %4d launches %8.3f ms  %7.1f TFLOP/s  %7.1f GB/s%s" % (name, n, ms, fl / ms / 1e9 if ms else 0,
                                                                              by / ms / 1e6 if ms else 0, extra))


def main_sdxl(a):
    torch.set_grad_enabled(False)
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd.synthetic import seeded_init
    from clip_text_proj_ref import BIGG, CLIPTextProjRef
    from clip_text_ref import CLIPTextRef, SD15, seeded_ids
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    ref = seeded_init(CLIPTextProjRef(**BIGG).eval(), seed=47)
    sd = ref.state_dict()
    del ref
    hip = {}
    for form in (0, 1):
        m = P.CLIPTextModelWithProjection(**BIGG, gemm_form=form)
        m.load_state_dict(sd)
        hip[form] = m.to(dev, torch.float16)
    ref_l = seeded_init(CLIPTextRef(**SD15).eval(), seed=49)
    hip_l = P.CLIPTextModel(**SD15)
    hip_l.load_state_dict(ref_l.state_dict())
    hip_l = hip_l.to(dev, torch.float16)
    hf = hf_l = None
    try:
        import transformers as tr
        c = tr.CLIPTextConfig(**{k: BIGG[k] for k in ("vocab_size", "hidden_size", "intermediate_size", "projection_dim",
                                                       "num_hidden_layers", "num_attention_heads", "max_position_embeddings",
                                                       "hidden_act", "layer_norm_eps", "eos_token_id")}, bos_token_id=0, pad_token_id=1)
        hf = tr.CLIPTextModelWithProjection(c).eval()
        hf.load_state_dict(sd)
        hf = hf.to(dev, torch.float16)
        cl = tr.CLIPTextConfig(vocab_size=SD15["vocab_size"], hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                               num_attention_heads=12, max_position_embeddings=77, eos_token_id=2, bos_token_id=0, pad_token_id=1)
        hf_l = tr.CLIPTextModel(cl).eval()
        prefixed = any(k.startswith("text_model.") for k in hf_l.state_dict())
        hf_l.load_state_dict({(k if prefixed else k[len("text_model."):]): v for k, v in ref_l.state_dict().items()})
        hf_l = hf_l.to(dev, torch.float16)
        say("baseline: transformers %s fp16, attention %s" % (tr.__version__, getattr(hf.config, "_attn_implementation", "?")))
    except ImportError:
        say("baseline skipped: transformers is not installed")
    wbytes = sum(v.numel() * 2 for k, v in sd.items() if k.endswith(".weight") and v.dim() == 2 and "embedding" not in k)
    say("bigG GEMM weight bytes per forward (fp16): %.3f GB" % (wbytes / 1e9))

    say("bigG tower (L = 77), ms per forward: median, spread (min..max) over %d alternated rounds of %d" % (a.rounds, a.iters))
    res = {}
    for B in [int(b) for b in a.batches.split(",")]:
        ids = seeded_ids(B, 77, BIGG["vocab_size"], seed=B).to(dev)
        say("B = %d" % B)
        runs = {"hip gemm_form 0": lambda: hip[0](ids, output_hidden_states=True),
                "hip gemm_form 1": lambda: hip[1](ids, output_hidden_states=True)}
        if hf is not None:
            runs["transformers"] = lambda: hf(ids, output_hidden_states=True)
        res[B] = _ab(say, runs, a.rounds, a.iters)
        for form in (0, 1):
            say("   gemm_form %d:" % form)
            _per_class(say, P, lambda: hip[form](ids), wbytes)
    say("deciding A/B (gemm_form 1 faster at every B): %s" % all(r["hip gemm_form 1"] < r["hip gemm_form 0"] for r in res.values()))

    say("whole SDXL prompt encoding from token ids (B prompts + B negatives, both towers, tokenizers excluded)")
    for B in (1, 2):
        ids_l = seeded_ids(B, 77, SD15["vocab_size"], seed=B + 10).to(dev)
        ids_g = seeded_ids(B, 77, BIGG["vocab_size"], seed=B + 20).to(dev)
        nids_l = seeded_ids(B, 77, SD15["vocab_size"], seed=B + 30).to(dev)
        nids_g = seeded_ids(B, 77, BIGG["vocab_size"], seed=B + 40).to(dev)
        from ctrl_adapter_amd.text_encoder import _encode_states

        def hip_encode():
            pos_l, neg_l, _ = _encode_states(hip_l, torch.cat([ids_l, nids_l]), -2, -2, B, False)
            # (bigG on gemm_form 1, the B = 1 winner)
            pos_g, neg_g, pooled = _encode_states(hip[1], torch.cat([ids_g, nids_g]), -2, -2, B, True)
            return torch.cat([pos_l, pos_g], -1), torch.cat([neg_l, neg_g], -1), pooled

        runs = {"encode_sdxl_prompt": hip_encode}
        if hf is not None:
            def hf_encode():
                o = [hf_l(i, output_hidden_states=True) for i in (ids_l, nids_l)] + [hf(i, output_hidden_states=True) for i in (ids_g, nids_g)]
                return torch.cat([o[0].hidden_states[-2], o[2].hidden_states[-2]], -1), o[2][0]
            runs["transformers x4"] = hf_encode
        say("B = %d" % B)
        _ab(say, runs, a.rounds, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
