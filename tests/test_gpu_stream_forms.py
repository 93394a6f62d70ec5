"""The small streaming kernels of csrc/elementwise.hip that only a whole-model forward used to reach -- add_rowvec_clip_kernel,
upsample2x_nhwc_kernel, fill_zero_kernel, linear_small_group_kernel and the frame-index path of sincos_kernel -- each compared exactly
(or, for the linears, also to fp64) at the sizes where its index arithmetic can go wrong."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from helpers import _POISON, Guarded, _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import ops as o
    return o


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_add_rowvec_clip_reproduces_the_reference_reshape(ops, gpu, dt):
    """rows (clip b, frame f, pixel p) get v[(b L + p) % B]: the reference hands the temporal transformer a context ordered
    broadcast_to(L, B, 1, C).reshape(L * B, 1, C) while the block's rows are ordered (clip, pixel) -- block row b L + p meets context row
    b L + p of that reshape.  In place (as both plans call it), v at ldv = C + 4; exact: one fp32 add, one rounding"""
    n = 0
    for B, Fr, Lp, C in itertools.product((1, 2, 3), (1, 3), (1, 5), (8, 328)):
        g = _gen(1000 * B + 100 * Fr + 10 * Lp + C)
        x = torch.randn(B * Fr * Lp, C, generator=g).to(dt)
        v = torch.randn(B, C, generator=g)
        ctx = v.reshape(B, 1, C).broadcast_to(Lp, B, 1, C).reshape(Lp * B, 1, C)          # the reference expression, literally
        rows = torch.arange(B * Fr * Lp)
        b, p = rows // (Fr * Lp), rows % Lp
        want = (x.float() + ctx[b * Lp + p, 0]).to(dt)
        X = Guarded.inp(x, (2, 0), (3, 0), gpu, fill=_POISON[dt])
        V = Guarded.inp(v, (0, 0), (1, 4), gpu)
        ops.add_rowvec_clip(X.view, V.view, C + 4, X.view, B, Fr, Lp, C)
        torch.cuda.synchronize()
        X.is_input = False                                       # written in place: only the surroundings must be as they were
        X.assert_untouched("add_rowvec_clip B%d F%d L%d C%d: x" % (B, Fr, Lp, C))
        V.assert_untouched("add_rowvec_clip: v")
        assert torch.equal(_bits(X.view), _bits(want)), "add_rowvec_clip B%d F%d L%d C%d %s" % (B, Fr, Lp, C, dt)
        n += 1
    print("PARITY add_rowvec_clip %s: %d shapes bit-exact" % (dt, n))


@pytest.mark.parametrize("C", [8, 328])
def test_upsample2x_nhwc_is_nearest(ops, gpu, C):
    x = torch.randn(2, 3, 5, C, generator=_gen(C)).half()
    want = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).half()
    got = ops.upsample2x_nhwc(x.to(gpu))
    assert got.shape == (2, 6, 10, C) and torch.equal(_bits(got), _bits(want))


def _pattern(n, gpu):
    return ((torch.arange(n, dtype=torch.int64) * 37 + 11) % 251 + 1).to(torch.uint8).to(gpu)        # never zero


def test_fill_zero_head_and_tail_at_every_alignment(ops, gpu):
    """every pointer offset 0 .. 15 x sizes around one and two 16-byte vectors and a few thousand bytes, four fills per launch, each
    inside a patterned buffer whose other bytes must not change"""
    sizes = (1, 15, 16, 17, 31, 32, 33, 4101)
    jobs = [(off, sz) for off in range(16) for sz in sizes]
    span = 4101 + 64
    buf = _pattern(len(jobs) * span, gpu)
    want = buf.clone()
    assert buf.data_ptr() % 16 == 0 and span % 16 != 0
    starts = []
    for i, (off, sz) in enumerate(jobs):
        a = (i * span + 15) // 16 * 16 + off                        # 16-byte aligned + off
        starts.append(a)
        want[a:a + sz] = 0
    for i in range(0, len(jobs), 4):
        ops.fill_zero_group([buf.data_ptr() + a for a in starts[i:i + 4]], [sz for _, sz in jobs[i:i + 4]])
    torch.cuda.synchronize()
    bad = (buf != want).nonzero()
    assert bad.numel() == 0, "fill_zero: first wrong byte at %d (job %s)" % (int(bad[0]), jobs[int(bad[0]) // span])


@pytest.mark.parametrize("sizes", [(17,), (17, 1 << 20), (1 << 20, 17, 33), (5, 4101, 1 << 20, 17), (17, 0, 33), (0, 1 << 20)],
                         ids=["n1", "n2", "n3", "n4", "zero_member", "zero_first"])
def test_fill_zero_group_of_unequal_sizes(ops, gpu, sizes):
    """the grid is sized by the largest member: a 17-byte fill beside a 1 MB one, and a zero-byte member"""
    span = (1 << 20) + 64
    buf = _pattern(len(sizes) * span, gpu)
    want = buf.clone()
    starts = [i * span + 16 + (3 * i + 1) % 16 for i in range(len(sizes))]
    for a, sz in zip(starts, sizes):
        want[a:a + sz] = 0
    ops.fill_zero_group([buf.data_ptr() + a for a in starts], list(sizes))
    torch.cuda.synchronize()
    assert torch.equal(buf, want), "fill_zero_group %s: first wrong byte at %d" % (sizes, int((buf != want).nonzero()[0]))


@pytest.mark.parametrize("count", [41, 81])
def test_linear_small_group_across_the_launch_boundary(ops, gpu, count):
    """41 and 81 problems: two and three launches of at most kSmallGroup = 40.  Problem i takes the i-th combination of M, N, K and the
    SiLU flags, x at ldx = K + 4 and out at ldo = N + 3 inside guards; every result bit-identical to ctrl_op_linear_small alone and within
    1e-5 rel-inf of fp64"""
    Ms, Ns, Ks = (1, 8, 9, 16), (1, 3, 4, 5, 333), (8, 504, 512, 520, 1280)
    keep, descs, singles, probs = [], [], [], []
    for i in range(count):
        M, N, K = Ms[i % 4], Ns[(i // 2) % 5], Ks[(i // 3) % 5]
        in_silu, out_silu, bias = bool(i & 1), bool(i & 2), i % 5 != 0
        g = _gen(31 * i + count)
        x, w = torch.randn(M, K, generator=g), (0.05 * torch.randn(N, K, generator=g)).half()
        b = torch.randn(N, generator=g) if bias else None
        X = Guarded.inp(x, (1, 0), (1, 4), gpu)
        W = Guarded.inp(w, (1, 0), (1, 0), gpu)
        Bv = b.to(gpu) if bias else None
        O1 = Guarded.out((1 + M + 1, N + 3), (slice(1, 1 + M), slice(0, N)), torch.float32, gpu)
        O2 = Guarded.out((1 + M + 1, N + 3), (slice(1, 1 + M), slice(0, N)), torch.float32, gpu)
        ops.linear_small_into(X.view, K + 4, W.view, Bv, O1.view, N + 3, M, N, K, in_silu, out_silu)
        descs.append(ops.small_lin(X.view, K + 4, W.view, Bv, O2.view, N + 3, M, N, K, in_silu, out_silu))
        xx = x.double()
        ref = (F.silu(xx) if in_silu else xx) @ w.double().t() + (b.double() if bias else 0.0)
        probs.append((X, W, O1, O2, F.silu(ref) if out_silu else ref, (M, N, K, in_silu, out_silu)))
        keep.append(Bv)
    with ops.Profiler() as prof:
        ops.linear_small_group(descs)
    torch.cuda.synchronize()
    launches = [r for r in prof.launches if r[0] == "linear_small"]
    assert [r[2] for r in launches] == ["%d problems" % n for n in ([40, 1] if count == 41 else [40, 40, 1])], [r[2] for r in launches]
    worst = 0.0
    for i, (X, W, O1, O2, ref, shape) in enumerate(probs):
        what = "linear_small_group problem %d of %d %s" % (i, count, shape)
        for gd in (X, W, O1, O2):
            gd.assert_untouched(what)
        assert torch.equal(_bits(O1.view), _bits(O2.view)), what + ": differs from the single launch"
        rel = float((O2.view.cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-12))
        worst = max(worst, rel)
        assert rel <= 1e-5, (what, rel)
    print("PARITY linear_small_group %d problems: bit-identical to single launches, worst rel_inf %.2e" % (count, worst))


def test_frameidx_sincos_is_timestep_sincos_of_the_frame_index(ops, gpu):
    N, Fr = 7, 3
    for dim in (320, 1280):
        t = (torch.arange(N) % Fr).float().to(gpu)
        assert torch.equal(_bits(ops.frameidx_sincos(N, Fr, dim, device=gpu)), _bits(ops.timestep_sincos(t, N, dim)))
