"""ops.merge_gather (ctrl_op_merge_gather_group, csrc/elementwise.hip): router merge + key-frame gather + cast of up to 13 slots in one
launch, at the edges of its work split -- the scalar and the 16-byte path, frames that end inside a chunk, slots of very different
size, the second trip of the grid-stride loop -- and for every dtype pair the loops use.

Asserted, per case:
  * where the output dtype is the input dtype: bit-identical to today's path, ops.router_merge per slot followed by index_select;
  * without weights: index_select(...).to(dtype), exactly;
  * always, element-wise against the fp64 sum over the same operands:
        |out - ref| <= (K + 1) 2^-24 sum_k |w_k x_k|  +  the output rounding
    (K products and K - 1 additions in fp32, contracted or not: at most K + 1 roundings of partial sums bounded by sum |w_k x_k|; the
    output rounding is 2^-11 |ref| + 2^-25 for fp16, 2^-8 |ref| for bf16, nothing for fp32).  Derived; no slack factor;
  * nothing outside the outputs is written, and the NaN around every input is not read into a result."""
import pytest
import torch

from helpers import Guarded

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DEV = "cuda"
# 13 unequal frame sizes, the largest 64 x the smallest as in the ControlNet's pyramid; all multiples of 8 / with odd ones
VEC13 = [4096, 64, 2056, 8, 512, 1024, 72, 16, 256, 128, 40, 24, 2048]
ODD13 = [4096, 64, 2056, 7, 512, 1024, 9, 16, 256, 128, 40, 24, 2047]

# name: (K, frame sizes, n_in, map, weights, in dtype, out dtype, elements in front of every buffer)
CASES = {
    "k3-1slot-7": (3, [7], 4, None, True, F16, F16, 64),
    "k3-1slot-8": (3, [8], 4, None, True, F16, F16, 64),
    "k3-1slot-9": (3, [9], 4, [3, 1], True, F16, F16, 64),
    "k3-1slot-2056-tail": (3, [2056], 4, [3, 1, 0], True, F16, F16, 64),
    "k1-1slot-2056-f32": (1, [2056], 3, None, True, F32, F32, 64),
    "k8-1slot-2056": (8, [2056], 3, [2, 0], True, F16, F16, 64),
    "k8-1slot-9-f32": (8, [9], 3, [2, 0], True, F32, F32, 3),
    "k3-13slots-vec": (3, VEC13, 5, [4, 2, 1], True, F16, F16, 64),
    "k3-13slots-vec-identity": (3, VEC13, 3, None, True, F16, F16, 64),
    "k3-13slots-scalar": (3, ODD13, 5, [4, 2, 1], True, F16, F16, 64),
    "k8-13slots-vec-f16-f32": (8, VEC13, 4, [3, 0], True, F16, F32, 64),
    "k3-13slots-bf16-f16": (3, VEC13, 4, [3, 0], True, BF16, F16, 64),
    "k3-13slots-scalar-bf16-f16": (3, ODD13, 4, [3, 0], True, BF16, F16, 5),
    "k3-13slots-f32-f32": (3, VEC13, 4, [3, 0], True, F32, F32, 64),
    "k3-misaligned-falls-to-scalar": (3, [2056, 64], 4, [3, 1], True, F16, F16, 4),
    "gather-13slots-vec": (1, VEC13, 5, [4, 2, 1], False, F16, F16, 64),
    "gather-13slots-f16-f32": (1, VEC13, 5, [4, 2, 1], False, F16, F32, 64),
    "gather-13slots-scalar-bf16-f16": (1, ODD13, 5, [0, 4], False, BF16, F16, 3),
    "gather-identity-cast-f32-f16": (1, [2056, 9], 3, None, False, F32, F16, 64),
}


def out_rounding(ref, dt):
    if dt == F16:
        return 2.0 ** -11 * ref.abs() + 2.0 ** -25
    if dt == BF16:
        return 2.0 ** -8 * ref.abs()
    return torch.zeros_like(ref)


def _operands(K, sizes, n_in, frame_map, weighted, in_dt, out_dt, front, seed):
    g = torch.Generator().manual_seed(seed)
    E, R = 9, len(sizes) + 2
    w = torch.softmax(torch.randn(R, E, generator=g), 1).float() if weighted else None
    rows = [(3 * s + 1) % R for s in range(len(sizes))]
    widx = [(2 * k + 1) % E for k in range(K)]
    n_out = len(frame_map) if frame_map is not None else n_in
    data, ins, outs = [], [], []
    for per in sizes:
        xs = [torch.randn(n_in, per, generator=g).to(in_dt) for _ in range(K)]
        data.append(xs)
        ins.append([Guarded.inp(x.reshape(-1), (front,), (37,), DEV) for x in xs])
        outs.append(Guarded.out((front + n_out * per + 37,), (slice(front, front + n_out * per),), out_dt, DEV))
    return w, rows, widx, n_out, data, ins, outs


def _check(name, K, sizes, n_in, frame_map, weighted, in_dt, out_dt, front, expect_vec=None, seed=5):
    from ctrl_adapter_amd import ops
    w, rows, widx, n_out, data, ins, outs = _operands(K, sizes, n_in, frame_map, weighted, in_dt, out_dt, front, seed)
    w_d = w.to(DEV) if weighted else None
    map_d = torch.tensor(frame_map, dtype=torch.int32, device=DEV) if frame_map is not None else None
    slots = [[gi.view.view(n_in, per) for gi in gs] for gs, per in zip(ins, sizes)]
    out_views = [go.view.view(n_out, per) for go, per in zip(outs, sizes)]
    blocks, vec, cap = ops.merge_gather_launch_shape(slots, out_views, w_d, rows if weighted else None, widx if weighted else None, map_d)
    if expect_vec is not None:
        assert vec == expect_vec, (name, vec)
    chunks = sum(-(-(per // vec * n_out) // 256) for per in sizes)
    assert blocks == min(chunks, cap) and cap == 8192
    got = ops.merge_gather(slots, w_d, rows if weighted else None, widx if weighted else None, frame_map=map_d, out=out_views)
    torch.cuda.synchronize()
    sel = torch.tensor(frame_map if frame_map is not None else list(range(n_in)))
    worst = 0.0
    for s, per in enumerate(sizes):
        o = got[s].cpu()
        assert o.dtype == out_dt and tuple(o.shape) == (n_out, per)
        x64 = torch.stack([x.double() for x in data[s]])[:, sel]                      # [K, n_out, per]
        wk = torch.stack([w[rows[s], widx[k]] for k in range(K)]).double() if weighted else torch.ones(1, dtype=torch.float64)
        terms = wk[:, None, None] * x64
        ref, mag = terms.sum(0), terms.abs().sum(0)
        bound = ((K + 1) * 2.0 ** -24 * mag if weighted else torch.zeros_like(ref)) + out_rounding(ref, out_dt)
        err = (o.double() - ref).abs()
        assert bool(torch.isfinite(o.float()).all()), "%s slot %d: non-finite (the NaN around an input was read)" % (name, s)
        assert bool((err <= bound).all()), "%s slot %d: %d beyond the bound" % (name, s, int((err > bound).sum()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()) if weighted or out_dt != in_dt else 0.0)
        if not weighted:
            assert torch.equal(o, data[s][0].index_select(0, sel).to(out_dt)), "%s slot %d: the gather is not exact" % (name, s)
        elif out_dt == in_dt:
            today = ops.router_merge([x.to(DEV) for x in data[s]], w_d[rows[s]].contiguous(), widx).index_select(0, sel.to(DEV))
            assert torch.equal(o, today.cpu()), "%s slot %d: differs from router_merge + index_select" % (name, s)
        outs[s].assert_untouched("%s out %d" % (name, s))
        for gi in ins[s]:
            gi.assert_untouched("%s in %d" % (name, s))
    print("PARITY merge_gather %-36s vec %d blocks %5d  worst err/bound %.3f" % (name, vec, blocks, worst))


@pytest.mark.parametrize("name", sorted(CASES))
def test_merge_gather_forms(gpu, name):
    K, sizes, n_in, frame_map, weighted, in_dt, out_dt, front = CASES[name]
    align = 16 // torch.empty(0, dtype=in_dt).element_size()
    align_out = 16 // torch.empty(0, dtype=out_dt).element_size()
    vec = 8 if all(p % 8 == 0 for p in sizes) and front % align == 0 and front % align_out == 0 else 1
    _check(name, K, sizes, n_in, frame_map, weighted, in_dt, out_dt, front, expect_vec=vec)


def test_merge_gather_second_trip_of_the_grid_stride_loop(gpu):
    """one slot whose chunks number one more than the grid cap: workgroup 0 takes a second trip"""
    from ctrl_adapter_amd import ops
    probe = [[torch.empty(2, 8, dtype=F16, device=DEV)]]
    _, vec, cap = ops.merge_gather_launch_shape(probe, [torch.empty(2, 8, dtype=F16, device=DEV)])
    assert (vec, cap) == (8, 8192)
    per = cap * 256 * vec // 2 + vec                    # two frames: cap * 256 * 8 elements and 16 more
    w = torch.tensor([[0.25, 0.625]], device=DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, per, generator=g).half()
    gi = Guarded.inp(x.reshape(-1), (64,), (64,), DEV)
    go = Guarded.out((64 + 2 * per + 64,), (slice(64, 64 + 2 * per),), F16, DEV)
    slots, outs = [[gi.view.view(2, per)]], [go.view.view(2, per)]
    map_d = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    blocks, vec, _ = ops.merge_gather_launch_shape(slots, outs, w, [0], [1], map_d)
    assert blocks == cap and -(-(2 * per // vec) // 256) == cap + 1
    got = ops.merge_gather(slots, w, [0], [1], frame_map=map_d, out=outs)[0]
    today = ops.router_merge([gi.view.view(2, per).contiguous()], w[0].contiguous(), [1]).index_select(0, map_d.long())
    torch.cuda.synchronize()
    assert torch.equal(got, today)
    ref = 0.625 * x.double()[[1, 0]]
    err = (got.cpu().double() - ref).abs()
    assert bool((err <= 2 * 2.0 ** -24 * ref.abs() + out_rounding(ref, F16)).all())
    go.assert_untouched("second trip out")
    gi.assert_untouched("second trip in")


def test_merge_gather_refuses_what_it_cannot_run(gpu):
    from ctrl_adapter_amd import ops
    x = torch.zeros(4, 8, dtype=F16, device=DEV)
    w = torch.ones(2, 2, device=DEV)
    with pytest.raises(RuntimeError, match="K == 1"):
        ops.merge_gather([[x, x.clone()]])
    with pytest.raises(RuntimeError, match="widx out of range"):
        ops.merge_gather([[x]], w, [0], [2])
    with pytest.raises(RuntimeError, match="row out of range"):
        ops.merge_gather([[x]], w, [2], [0])
    with pytest.raises(ValueError, match="1..13 slots"):
        ops.merge_gather([[x]] * 14)
    with pytest.raises(ValueError, match="int32"):
        ops.merge_gather([[x]], frame_map=torch.tensor([0], device=DEV))
    # a map entry outside the input frames reads nothing and shows as NaN
    got = ops.merge_gather([[x]], frame_map=torch.tensor([0, 7], dtype=torch.int32, device=DEV))[0]
    assert bool((got[0] == 0).all()) and bool(torch.isnan(got[1]).all())
