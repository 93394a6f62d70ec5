"""Randomised live comparison of the oracle with the REFERENCE'S OWN files (live: needs the reference checkout, REF below).

The goldens pin a fixed set of configurations; this script draws others -- adapter locations, adapters per location, number of
blocks, which of the four sub-modules exist, clips x frames, broadcast / per-sample / 2-D encoder states, scalar / per-sample
timesteps; ControlNet scale, guess mode, skip flags, global pooling -- and runs model/ctrl_adapter.py + model/adapter_spatial_temporal.py
+ model/resnet_block_2d.py + controlnet/controlnet.py (over oracle/_shim, like make_golden.py) against oracle/ on the same seeded
weights and inputs.  Prints one line per case and exits non-zero on the first mismatch > 2e-5 (fp32 vs fp32).

    python tests/golden/live_check.py [n_cases [first_seed]]
    python tests/golden/live_check.py 8 3000 --record tests/golden/live_random.pt     # live, and keeps the reference's outputs
    python tests/golden/live_check.py 8 3000 --stored tests/golden/live_random.pt     # the oracle against those: no reference needed

--record stores, per case, a SHA-1 of the reference's sorted state-dict keys and a digest of every output (the whole fp32 tensor up to
DIGEST_SAMPLES elements, else its shape, abs-sum, root-sum-of-squares, abs-max and DIGEST_SAMPLES strided samples: the
file stays small); --stored draws the same configurations from the same
seeds and holds the oracle to that file instead of running the reference (tests/test_oracle_golden.py does, on any machine).
"""
import hashlib
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"


def _take(flag):
    """removes `flag VALUE` from sys.argv and returns VALUE (None when absent)"""
    if flag not in sys.argv:
        return None
    i = sys.argv.index(flag)
    val = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return val


RECORD_PATH, STORED_PATH = _take("--record"), _take("--stored")
STORED = torch.load(STORED_PATH, weights_only=False) if STORED_PATH else None
RECORD = {"cases": {}} if RECORD_PATH else None
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import blocks_source  # noqa: E402
if STORED is None:
    sys.path.insert(0, REF)
    BLOCKS = blocks_source.select(require_real="--require-real-diffusers" in sys.argv)      # a real diffusers when there is one, else the shim
else:
    BLOCKS = "stored: " + STORED["__provenance__"]["blocks"]
sys.argv = [a for a in sys.argv if a != "--require-real-diffusers"]
torch.Tensor.cuda = lambda self, *a, **k: self

from oracle.init import seeded_init, seeded_tensor  # noqa: E402
import cases  # noqa: E402

TOL = 2e-5
DIGEST_SAMPLES = 256


def digest(t):
    """what --record keeps of one reference output: the whole tensor when small, else shape, sums and strided samples"""
    t = t.detach().float().contiguous()
    if t.numel() <= DIGEST_SAMPLES:
        return t.clone()
    flat = t.reshape(-1)
    step = max(1, flat.numel() // DIGEST_SAMPLES)
    return dict(shape=list(t.shape), abssum=float(flat.double().abs().sum()), rss=float(flat.double().square().sum().sqrt()),
                absmax=float(flat.abs().max()), step=step, samples=flat[::step][:DIGEST_SAMPLES].clone())


def keys_id(module):
    """the sorted state-dict keys of a module as (count, SHA-1): what --record keeps of them"""
    keys = sorted(module.state_dict())
    return len(keys), hashlib.sha1("\n".join(keys).encode()).hexdigest()


def reference(key, run):
    """the reference's outputs of case `key`: run() over its own files (kept as digests under --record), or what --stored holds"""
    if STORED is not None:
        return STORED["cases"][key]
    out = run()
    if RECORD is not None:
        RECORD["cases"][key] = _map(out, lambda t: digest(t) if torch.is_tensor(t) else t)
    return out


def _map(x, fn):
    if isinstance(x, (list, tuple)):
        return type(x)(_map(v, fn) for v in x)
    if isinstance(x, dict):
        return {k: _map(v, fn) for k, v in x.items()}
    return fn(x)


def rel(a, b):
    """rel-inf of the oracle's `a` against the reference's `b` (a tensor, or the digest --record stored of one)"""
    if torch.is_tensor(b):
        assert a.shape == b.shape, "shapes differ: %s vs %s" % (tuple(a.shape), tuple(b.shape))
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()
    assert list(a.shape) == b["shape"], "shapes differ: %s vs %s" % (tuple(a.shape), tuple(b["shape"]))
    flat = a.detach().float().reshape(-1)
    den = max(b["absmax"], 1e-12)
    e = ((flat[::b["step"]][:b["samples"].numel()] - b["samples"]).abs().max() / den).item()
    # the elements between the samples: whole-tensor abs-sum, root-sum-of-squares and abs-max
    e_sum = abs(float(flat.double().abs().sum()) - b["abssum"]) / max(b["abssum"], 1e-12)
    e_rss = abs(float(flat.double().square().sum().sqrt()) - b["rss"]) / max(b["rss"], 1e-12)
    return max(e, e_sum, e_rss, abs(float(flat.abs().max()) - b["absmax"]) / den)


def is_zero(b):
    return b.abs().max().item() == 0 if torch.is_tensor(b) else b["abssum"] == 0.0


def adapter_case(rng, seed):
    from oracle.adapter import ControlNetAdapterOracle
    video = rng.random() < 0.6
    cfg = dict(cases.ADAPTER_VIDEO if video else cases.ADAPTER_SDXL)
    locs = [l for l in "ABCD" if rng.random() < 0.5] or ["A"]
    for l in "ABCD":
        cfg["add_adapter_location_" + l] = l in locs
    cfg["add_adapter_location_M"] = video and rng.random() < 0.5
    cfg["num_adapters_per_location"] = rng.choice([1, 2, 3])
    cfg["num_blocks"] = rng.choice([1, 1, 2])
    if video:
        flags = [rng.random() < 0.7 for _ in range(4)]
        if not any(flags):
            flags[0] = True
        (cfg["add_spatial_resnet"], cfg["add_temporal_resnet"], cfg["add_spatial_transformer"], cfg["add_temporal_transformer"]) = flags
        clips, frames = rng.choice([(1, 3), (2, 2), (2, 3), (3, 2)])
    else:
        sr, st = rng.choice([(True, True), (True, False), (False, True)])
        cfg["add_spatial_resnet"], cfg["add_spatial_transformer"] = sr, st
        clips, frames = rng.choice([1, 2, 3]), 1
    N = clips * frames
    cross = cfg["cross_attention_dim"]
    kind = rng.choice(["broadcast", "per_sample"]) if video else rng.choice(["tokens", "tokens", "vector2d"])
    if kind == "broadcast":
        ehs = seeded_tensor((1, 1, cross), seed + 1)
    elif kind == "per_sample":
        ehs = seeded_tensor((N, 1, cross), seed + 1)
    elif kind == "tokens":
        ehs = seeded_tensor((N, rng.choice([5, 77]), cross), seed + 1)
    else:
        ehs = seeded_tensor((N, cross), seed + 1)
    ts = torch.tensor(float(rng.choice([1, 333, 961]))) if rng.random() < 0.5 else torch.tensor([float(rng.randrange(1, 999)) for _ in range(N)])
    downs, mid = cases.pyramid_inputs(N=N, h0=rng.choice([4, 8]), seed=seed + 2, with_mid=cfg["add_adapter_location_M"])

    def run():
        from model.ctrl_adapter import ControlNetAdapter
        ref = seeded_init(ControlNetAdapter(**cfg).eval(), seed=seed)
        ro, rm = ref(downs, mid_block_res_sample=mid, sparsity_masking=None, num_frames=frames, timestep=ts, encoder_hidden_states=ehs)
        return dict(keys=keys_id(ref), out=list(ro), mid=rm)
    r = reference("adapter%d" % seed, run)
    ro, rm = r["out"], r["mid"]
    ora = seeded_init(ControlNetAdapterOracle(**cfg).eval(), seed=seed)
    assert r["keys"] == keys_id(ora), "state-dict keys differ"
    oo, om = ora(downs, mid_block_res_sample=mid, num_frames=frames, timestep=ts, encoder_hidden_states=ehs)
    assert len(oo) == len(ro), "output counts differ"
    errs = [rel(a, b) for a, b in zip(oo, ro) if not is_zero(b)]
    assert all(list(a.shape) == list(b.shape if torch.is_tensor(b) else b["shape"]) and a.abs().max().item() == 0
               for a, b in zip(oo, ro) if is_zero(b)), "zero slots differ"
    if rm is not None:
        errs.append(rel(om, rm))
    else:
        assert om is None
    desc = "adapter %s loc %s%s x%d blocks %d sr/tr/st/tt %d%d%d%d clips %d frames %d ehs %s t %s" % (
        "video" if video else "sdxl", "".join(locs), "M" if cfg["add_adapter_location_M"] else "", cfg["num_adapters_per_location"],
        cfg["num_blocks"], cfg["add_spatial_resnet"], cfg.get("add_temporal_resnet", 0), cfg["add_spatial_transformer"],
        cfg.get("add_temporal_transformer", 0), clips, frames, kind, "scalar" if ts.dim() == 0 else "per-sample")
    return desc, max(errs)


_nets = {}


def _net(side, gp):
    """one ControlNet of each flavour and side ("ref": the reference's file, "ora": the oracle), built once: 360 M parameters"""
    if (side, gp) not in _nets:
        if side == "ref":
            from controlnet.controlnet import ControlNetModel as cls
        else:
            from oracle.controlnet import ControlNetOracle as cls
        _nets[side, gp] = seeded_init(cls(**dict(cases.CONTROLNET_KW, global_pool_conditions=gp)).eval(), seed=11)
    return _nets[side, gp]


def controlnet_case(rng, seed):
    gp = rng.random() < 0.3
    inp = cases.controlnet_inputs() if rng.random() < 0.5 else cases.controlnet_inputs_nonsquare()
    kw = dict(conditioning_scale=rng.choice([1.0, 0.5, 2.0]), guess_mode=rng.random() < 0.4, skip_conv_in=rng.random() < 0.4,
              skip_time_emb=rng.random() < 0.3)

    def run():
        rd, rm = _net("ref", gp)(inp["sample"], inp["timestep"], encoder_hidden_states=inp["encoder_hidden_states"],
                                 controlnet_cond=inp["controlnet_cond"], return_dict=False, **kw)
        return dict(out=list(rd) + [rm])
    ro = reference("controlnet%d" % seed, run)["out"]
    od, om = _net("ora", gp)(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["controlnet_cond"], **kw)
    assert len(ro) == len(od) + 1, "output counts differ"
    errs = [rel(a, b) for a, b in zip(list(od) + [om], ro)]
    return "controlnet N=%d pool %d %s" % (inp["sample"].shape[0], gp, " ".join("%s=%s" % kv for kv in sorted(kw.items()))), max(errs)


def multi_case(rng, seed):
    """controlnet/multicontrolnet.py:45-99 (per-net lists, no summation) against MultiControlNetOracle: two nets, two images, two scales"""
    from oracle.controlnet import MultiControlNetOracle
    inp = cases.controlnet_inputs()
    conds = [inp["controlnet_cond"], seeded_tensor(tuple(inp["controlnet_cond"].shape), seed + 5).abs()]
    scales = [rng.choice([1.0, 0.5]), rng.choice([1.0, 2.0])]
    skip = rng.random() < 0.5

    def run():
        from controlnet.multicontrolnet import MultiControlNetModel
        ref = MultiControlNetModel([_net("ref", False), _net("ref", True)])
        rd, rm = ref(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], conds, scales, return_dict=False, skip_conv_in=skip)
        return dict(down=[list(d) for d in rd], mid=list(rm))
    r = reference("multi%d" % seed, run)
    rd, rm = r["down"], r["mid"]
    ora = MultiControlNetOracle([_net("ora", False), _net("ora", True)])
    od, om = ora(inp["sample"], inp["timestep"], inp["encoder_hidden_states"], conds, scales, skip_conv_in=skip)
    assert len(rd) == len(od) == 2 and len(rm) == len(om) == 2
    errs = [rel(a, b) for k in range(2) for a, b in zip(list(od[k]) + [om[k]], list(rd[k]) + [rm[k]])]
    return "multi-controlnet 2 nets scales %s skip_conv_in %d" % (scales, skip), max(errs)


def router_case(rng, seed):
    """model/ctrl_router.py:49-112 against RouterOracle: expert count, router type, number of routers, random sparse masks"""
    from oracle.router import RouterOracle
    E, rt, nr = rng.choice([2, 3, 5]), rng.choice(["simple_weights", "equal_weights"]), rng.choice([9, 12])
    masks = []
    for _ in range(4):
        mask = [rng.randrange(2) for _ in range(E)]
        if not any(mask):
            mask[rng.randrange(E)] = 1
        masks.append(rng.choice([mask, None]))

    def run():
        from model.ctrl_router import ControlNetRouter
        ref = seeded_init(ControlNetRouter(num_experts=E, router_type=rt, num_routers=nr).eval(), seed=seed)
        return dict(keys=keys_id(ref), out=[ref(sparse_mask=m) for m in masks])
    r = reference("router%d" % seed, run)
    ora = seeded_init(RouterOracle(num_experts=E, router_type=rt, num_routers=nr).eval(), seed=seed)
    assert r["keys"] == keys_id(ora), "router state-dict keys differ"
    worst = 0.0
    for mask, (rd, rm) in zip(masks, r["out"]):
        od, om = ora(sparse_mask=mask)
        assert rd.shape == od.shape == (nr, E) and rm.shape == om.shape == (E,)
        worst = max(worst, (rd - od).abs().max().item(), (rm - om).abs().max().item())
    return "router E=%d %s routers %d, 4 masks" % (E, rt, nr), worst


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    torch.set_grad_enabled(False)
    if STORED is not None:
        assert (STORED["n"], STORED["first"]) == (n, first), "%s holds %d cases from seed %d" % (STORED_PATH, STORED["n"], STORED["first"])
    worst = 0.0
    for i in range(n):
        seed = first + 17 * i
        rng = random.Random(seed)
        desc, err = (multi_case if i % 8 == 7 else controlnet_case if i % 4 == 3 else router_case if i % 4 == 1 else adapter_case)(rng, seed)
        worst = max(worst, err)
        print("%-120s rel_inf %.2e%s" % (desc, err, "" if err <= TOL else "   MISMATCH"), flush=True)
        if not err <= TOL:
            raise SystemExit(1)
    if RECORD is not None:
        RECORD.update(n=n, first=first, __provenance__=dict(blocks_source.provenance(BLOCKS), generator="tests/golden/live_check.py"))
        torch.save(RECORD, RECORD_PATH)
    print("LIVE CHECK OK: %d cases, worst %.2e  (blocks: %s)" % (n, worst, BLOCKS))


if __name__ == "__main__":
    main()
