"""The sampler launches of csrc/sampler.hip at op level (ctrl_op_sampler_*): the model-input pass, the guided step, the fused
step + next input, the device counter -- against the fp64 evaluation with the fp64 coefficients, every operand inside poisoned surroundings.

Element-wise bounds, derived (nothing measured, no slack factor):
    model input:  1/2 ulp_out(ref) + 2 * 2^-24 |ref|                       (the fp32 rounding of c_in, one fp32 product)
    step:         1/2 ulp_out(ref) + 8 * 2^-24 (|A x| + |B| (|u| + |g| (|c| + |u|)))
                  (c - u, the fma into u, B * mg, the fma with A x: five fp32 roundings at most, + the fp32 roundings of A, B, g)
The fused launch, the counter-driven launch and a reset + n counter-driven steps are compared bit for bit with their explicit forms."""
import ctypes as C
import math

import pytest
import torch

from helpers import Guarded, _bits
from sampler_check import assert_within, input_bound, step_bound

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
PAD = 16                       # elements in front of every operand: 16-byte aligned for every dtype; PAD + 1 breaks the alignment
N_STEPS = 5


@pytest.fixture(scope="module")
def L(gpu):
    import ctrl_adapter_amd  # noqa: F401
    from ctrl_adapter_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def table(gpu):
    """a table of N_STEPS rows with coefficients of both signs and magnitudes: fp64 (the reference's) and its fp32 device copy"""
    g = torch.Generator().manual_seed(99)
    t = torch.zeros(N_STEPS, 8, dtype=torch.float64)
    t[:, 0] = torch.rand(N_STEPS, generator=g, dtype=torch.float64) * 0.9 + 0.05
    t[:, 1] = torch.randn(N_STEPS, generator=g, dtype=torch.float64)
    t[:, 2] = torch.randn(N_STEPS, generator=g, dtype=torch.float64) * 3
    t[:, 3:6] = torch.randn(N_STEPS, 3, generator=g, dtype=torch.float64) * 100
    return t, t.float().to(gpu)


class Case:
    """one geometry: the latents, the model output, the concat operand, and the fp64 references of every output"""

    def __init__(self, L, gpu, layout, B, Fr, hw, R, lat_dt, mo_dt, concat, cn, g_mode, seed, misalign=False, Cc=4):
        self.L, self.gpu, self.R, self.lat_dt, self.mo_dt, self.layout, self.cn = L, gpu, R, lat_dt, mo_dt, layout, cn
        h, w = hw
        shape = {"bfchw": (B, Fr, Cc, h, w), "bcfhw": (B, Cc, Fr, h, w), "bchw": (B, Cc, h, w)}[layout]
        self.shape, self.cd = shape, {"bfchw": 2, "bcfhw": 1, "bchw": 1}[layout]
        self.outer, self.C, self.inner = math.prod(shape[:self.cd]), Cc, math.prod(shape[self.cd + 1:])
        self.frames = Fr if cn == "permuted" else 0
        gen = torch.Generator().manual_seed(seed)
        self.x = torch.randn(shape, generator=gen).to(lat_dt)
        self.mo = torch.randn((R * B,) + shape[1:], generator=gen).to(mo_dt)
        self.C2 = Cc if concat else 0
        self.cat = torch.randn((R * B,) + shape[1:], generator=gen).to(lat_dt) if concat else None
        self.g_scalar, self.g = 1.0, None
        if R == 2 and g_mode == "vector":
            self.g = (torch.linspace(1.0, 3.0, Fr) + 0.123).float()
        elif R == 2:
            self.g_scalar = 2.5
        self.pad = PAD + (1 if misalign else 0)
        n = self.x.numel()
        self.n = n
        self.ush = list(shape)
        self.ush[0] *= R
        self.csh = list(self.ush) if cn != "permuted" else [R * B * Fr, Cc, h, w]
        self.ush[self.cd] = Cc + self.C2

    # ---- device operands ----
    def _in(self, t):
        return Guarded.inp(t.reshape(-1), (self.pad,), (PAD,), self.gpu)

    def _out(self, numel, dt):
        return Guarded.out((self.pad + numel + PAD,), (slice(self.pad, self.pad + numel),), dt, self.gpu)

    def desc(self, X, MO=None, PREV=None, UN=None, CN=None, CAT=None, G=None, prev_dt=None):
        L, d = self.L, self.L.SamplerDesc()
        d.x, d.x_dtype = X.view.data_ptr(), L.dtype_code(self.lat_dt)
        if MO is not None:
            d.model_out, d.mo_dtype = MO.view.data_ptr(), L.dtype_code(self.mo_dt)
            d.prev, d.prev_dtype = PREV.view.data_ptr(), L.dtype_code(prev_dt or self.lat_dt)
        if UN is not None:
            d.unet_in, d.unet_dtype = UN.view.data_ptr(), L.dtype_code(self.lat_dt)
        if CN is not None:
            d.cn_in, d.cn_dtype = CN.view.data_ptr(), L.dtype_code(self.lat_dt)
        if CAT is not None:
            d.concat, d.concat_dtype = CAT.view.data_ptr(), L.dtype_code(self.lat_dt)
        d.outer, d.C, d.inner, d.C2, d.R, d.cn_frames = self.outer, self.C, self.inner, self.C2 if CAT is not None else 0, self.R, self.frames
        d.g_scalar, d.g_count, d.g_inner = self.g_scalar, 1, 1
        if G is not None:
            fd = 1 if self.layout == "bfchw" else 2
            d.g, d.g_count, d.g_inner = G.data_ptr(), self.shape[fd], math.prod(self.shape[fd + 1:])
        return d

    # ---- fp64 references ----
    def ref_inputs(self, lat, c_in):
        """(unet_in, cn_in) fp64 of latents `lat` (a tensor of the latents' dtype: what the kernel reads)"""
        s = c_in * lat.double().reshape(self.shape)
        rep = torch.cat([s] * self.R, 0)
        un = torch.cat([rep, self.cat.double()], self.cd) if self.cat is not None else rep
        cn = rep.permute(0, 2, 1, 3, 4).reshape(self.csh) if self.cn == "permuted" else rep
        return un, cn

    def ref_step(self, A, B):
        """(prev fp64, bound) of one step from self.x / self.mo"""
        x, mo = self.x.double(), self.mo.double()
        if self.R == 2:
            u, c = mo.chunk(2)
            if self.g is not None:
                gs = [1] * len(self.shape)
                gs[1 if self.layout == "bfchw" else 2] = -1
                g = self.g.double().reshape(gs).expand(self.shape)
            else:
                g = torch.full(self.shape, self.g_scalar, dtype=torch.float64)
            mg = u + g * (c - u)
        else:
            u, c, g, mg = mo, None, None, mo
        ref = A * x + B * mg
        return ref, lambda dt: step_bound(ref, dt, A, B, x, u, c, g)


def launch_shape(L, d, with_step, with_input):
    b, v, cap = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib().ctrl_op_sampler_launch_shape(C.byref(d), int(with_step), int(with_input), C.byref(b), C.byref(v), C.byref(cap)))
    return b.value, v.value, cap.value


def run_case(L, gpu, table, cs, i, inplace, expect_vec=None, what=""):
    """step i of `cs` three ways -- step then model input (explicit rows), fused (explicit row), fused (device counter) -- compared bit for
    bit with each other and, the first, element-wise with fp64"""
    t64, t32 = table
    lib, st = L.lib(), L.cur_stream()
    A, B = float(t64[i, 1]), float(t64[i, 2])
    last = i + 1 >= N_STEPS
    G = cs.g.to(gpu) if cs.g is not None else None
    counter = torch.zeros(2, dtype=torch.int32, device=gpu)
    results = []
    for mode in ("two launches", "fused", "fused, device counter"):
        X, MO = cs._in(cs.x), cs._in(cs.mo)
        CAT = cs._in(cs.cat) if cs.cat is not None else None
        PREV = X if inplace else cs._out(cs.n, cs.lat_dt)
        UN = cs._out(math.prod(cs.ush), cs.lat_dt)
        CN = cs._out(math.prod(cs.csh), cs.lat_dt)
        SC = Guarded.out((8,), (slice(2, 5),), F32, gpu)
        d = cs.desc(X, MO, PREV, UN, CN, CAT, G)
        if mode == "two launches":
            dstep = cs.desc(X, MO, PREV, G=G)
            blocks, vec, cap = launch_shape(L, dstep, True, False)
            if expect_vec is not None:
                assert vec == expect_vec, (what, vec)
            L.check(lib.ctrl_op_sampler_step(L.ptr(t32), N_STEPS, None, None, C.byref(dstep), i, 0, st))
            if not last:
                dpre = cs.desc(PREV, UN=UN, CN=CN, CAT=CAT)
                L.check(lib.ctrl_op_sampler_model_input(L.ptr(t32), N_STEPS, None, SC.view.data_ptr(), C.byref(dpre), i + 1, st))
        elif mode == "fused":
            L.check(lib.ctrl_op_sampler_step(L.ptr(t32), N_STEPS, None, SC.view.data_ptr(), C.byref(d), i, 1, st))
        else:
            counter.copy_(torch.tensor([i, 0], dtype=torch.int32))
            L.check(lib.ctrl_op_sampler_step(L.ptr(t32), N_STEPS, L.ptr(counter), SC.view.data_ptr(), C.byref(d), -1, 1, st))
        torch.cuda.synchronize()
        if mode.endswith("counter"):
            assert counter.tolist() == [i + 1, 0], (what, counter.tolist())
        if inplace:
            X.is_input = False
        for gd, nm in ((X, "x"), (MO, "model_out"), (PREV, "prev"), (UN, "unet_in"), (CN, "cn_in"), (SC, "scalars")) + (((CAT, "concat"),) if CAT else ()):
            gd.assert_untouched("%s [%s]: %s" % (what, mode, nm))
        results.append((PREV.view.clone(), UN.view.clone(), CN.view.clone(), SC.view.clone(), UN, CN, SC))
    prev, un, cn, sc, UNg, CNg, SCg = results[0]
    for k, mode in ((1, "fused"), (2, "fused, device counter")):
        for a, b, nm in zip(results[0][:4], results[k][:4], ("prev", "unet_in", "cn_in", "scalars")):
            assert torch.equal(_bits(a), _bits(b)), "%s: %s of the %s launch differs from the two explicit launches" % (what, nm, mode)
    ref, bound = cs.ref_step(A, B)
    assert_within(prev.reshape(cs.shape), ref, bound(cs.lat_dt), what + " step %d prev" % i)
    if last:
        for gd in (UNg, CNg, SCg):            # nothing of a next input exists past the table: the buffers are as they were
            assert torch.equal(_bits(gd.buf), gd._snap), what + ": the last step wrote a next input"
        return
    run, rcn = cs.ref_inputs(prev.cpu(), float(t64[i + 1, 0]))
    bu, bc = input_bound(run, cs.lat_dt), input_bound(rcn, cs.lat_dt)
    if cs.cat is not None:          # the concat channels are copies: exact
        sl = [slice(None)] * len(cs.ush)
        sl[cs.cd] = slice(cs.C, None)
        bu[tuple(sl)] = 0
    assert_within(un.reshape(cs.ush), run, bu, what + " next unet_in")
    assert_within(cn.reshape(cs.csh), rcn, bc, what + " next cn_in")
    assert torch.equal(sc.cpu(), t32[i + 1, 3:6].cpu()), what + ": the timestep scalars are not row %d's" % (i + 1)


DT_PAIRS = [(F16, F32), (F16, F16), (BF16, BF16), (F32, F32)]          # (model output, latents)


@pytest.mark.parametrize("mo_dt,lat_dt", DT_PAIRS, ids=["mo16-lat32", "f16", "bf16", "f32"])
def test_svd_layout_per_frame_guidance_concat(L, gpu, table, mo_dt, lat_dt):
    """[B, F, C, h, w] latents, R = 2, per-frame guidance, 4 + 4 concat, the ControlNet's sample in the same layout; in place"""
    for B, hw, vec in ((2, (6, 5), 1), (1, (8, 8), 8)):
        cs = Case(L, gpu, "bfchw", B, 3, hw, 2, lat_dt, mo_dt, True, "same", "vector", seed=B * 10 + hw[0])
        run_case(L, gpu, table, cs, 1, True, vec, "bfchw B%d %dx%d %s/%s" % (B, hw[0], hw[1], mo_dt, lat_dt))


@pytest.mark.parametrize("mo_dt,lat_dt", DT_PAIRS, ids=["mo16-lat32", "f16", "bf16", "f32"])
def test_i2vgen_layout_permuted_controlnet_sample(L, gpu, table, mo_dt, lat_dt):
    """[B, C, F, h, w] latents, R = 2, per-frame guidance, no concat, the ControlNet's sample as (b f) c h w; out of place"""
    for B, hw, vec in ((1, (6, 5), 1), (2, (8, 8), 8)):
        cs = Case(L, gpu, "bcfhw", B, 3, hw, 2, lat_dt, mo_dt, False, "permuted", "vector", seed=B * 11 + hw[0])
        run_case(L, gpu, table, cs, 2, False, vec, "bcfhw B%d %dx%d %s/%s" % (B, hw[0], hw[1], mo_dt, lat_dt))


@pytest.mark.parametrize("R", [1, 2])
def test_image_layout_scalar_guidance_first_and_last_rows(L, gpu, table, R):
    """[B, C, h, w] (fewer elements than one workgroup's threads at 8 x 8), scalar guidance or none, rows 0 and n - 1 of the table: the
    last step writes no next input"""
    for hw, vec in (((8, 8), 8), ((6, 5), 1)):
        for i in (0, N_STEPS - 1):
            for inplace in (True, False):
                cs = Case(L, gpu, "bchw", 1, 1, hw, R, F16, F16, False, "same", "scalar", seed=R * 100 + hw[0] + i)
                run_case(L, gpu, table, cs, i, inplace, vec, "bchw R%d %dx%d row %d %s" % (R, hw[0], hw[1], i, "in place" if inplace else "out of place"))


def test_misaligned_base_takes_the_scalar_path(L, gpu, table):
    """every operand one element past a 16-byte boundary: the geometry allows 16-byte accesses, the pointers do not"""
    cs = Case(L, gpu, "bfchw", 1, 3, (8, 8), 2, F16, F16, True, "same", "vector", seed=7, misalign=True)
    run_case(L, gpu, table, cs, 1, True, 1, "misaligned")
    cs = Case(L, gpu, "bfchw", 1, 3, (8, 8), 2, F16, F16, True, "same", "vector", seed=7)
    run_case(L, gpu, table, cs, 1, True, 8, "aligned twin")


@pytest.mark.parametrize("vec", [8, 1])
def test_grid_stride_loop_takes_a_second_trip(L, gpu, table, vec):
    """more chunks than grid cap x 256 threads: some threads work on two chunks (the cap is read from the library)"""
    hw = (256, 256) if vec == 8 else (211, 157)
    B = 9 if vec == 8 else 2
    cs = Case(L, gpu, "bchw", B, 1, hw, 2, F16, F16, False, "same", "scalar", seed=3)
    X, MO = cs._in(cs.x), cs._in(cs.mo)
    blocks, v, cap = launch_shape(L, cs.desc(X, MO, X), True, False)
    assert v == vec and blocks == cap and cs.n // vec > cap * 256, (blocks, v, cap, cs.n)
    run_case(L, gpu, table, cs, 3, True, vec, "second trip vec%d" % vec)


def test_model_input_alone_and_its_scalars(L, gpu, table):
    """the model-input pass on its own (step 0 of a loop), explicit row and counter row, against fp64"""
    t64, t32 = table
    lib, st = L.lib(), L.cur_stream()
    for layout, cn, hw in (("bfchw", "same", (6, 5)), ("bcfhw", "permuted", (8, 8))):
        cs = Case(L, gpu, layout, 2, 3, hw, 2, F16, F16, layout == "bfchw", cn, "vector", seed=21)
        outs = []
        for i, use_counter in ((0, False), (3, False), (3, True)):
            X = cs._in(cs.x)
            CAT = cs._in(cs.cat) if cs.cat is not None else None
            UN, CN = cs._out(math.prod(cs.ush), F16), cs._out(math.prod(cs.csh), F16)
            SC = Guarded.out((8,), (slice(2, 5),), F32, gpu)
            counter = torch.tensor([i, 0], dtype=torch.int32, device=gpu)
            L.check(lib.ctrl_op_sampler_model_input(L.ptr(t32), N_STEPS, L.ptr(counter), SC.view.data_ptr(),
                                                    C.byref(cs.desc(X, UN=UN, CN=CN, CAT=CAT)), -1 if use_counter else i, st))
            torch.cuda.synchronize()
            assert counter.tolist() == [i, 0]                      # the model-input pass does not advance the counter
            for gd in (X, UN, CN, SC) + ((CAT,) if CAT else ()):
                gd.assert_untouched("model input %s row %d" % (layout, i))
            run, rcn = cs.ref_inputs(cs.x, float(t64[i, 0]))
            bu = input_bound(run, F16)
            if cs.cat is not None:
                bu[:, :, cs.C:] = 0
            assert_within(UN.view.reshape(cs.ush), run, bu, "model input %s row %d unet_in" % (layout, i))
            assert_within(CN.view.reshape(cs.csh), rcn, input_bound(rcn, F16), "model input %s row %d cn_in" % (layout, i))
            assert torch.equal(SC.view.cpu(), t32[i, 3:6].cpu())
            outs.append((UN.view.clone(), CN.view.clone()))
        assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])


def test_reset_then_counter_steps_equal_explicit_steps(L, gpu, table):
    """reset + N_STEPS counter-driven fused steps == N_STEPS explicit ones, bit for bit; one more replay past the table is a no-op"""
    t64, t32 = table
    lib, st = L.lib(), L.cur_stream()
    cs = Case(L, gpu, "bfchw", 1, 3, (8, 8), 2, F16, F16, True, "same", "vector", seed=31)
    gen = torch.Generator().manual_seed(5)
    mos = [torch.randn(cs.mo.shape, generator=gen).half().to(gpu) for _ in range(N_STEPS)]
    G, cat = cs.g.to(gpu), cs.cat.to(gpu)
    finals = []
    for use_counter in (False, True):
        x = cs.x.to(gpu).clone()
        un = torch.zeros(cs.ush, dtype=F16, device=gpu)
        cn = torch.zeros(cs.csh, dtype=F16, device=gpu)
        sc = torch.zeros(3, device=gpu)
        counter = torch.tensor([3, 0], dtype=torch.int32, device=gpu)
        L.check(lib.ctrl_op_sampler_reset(L.ptr(counter), st))
        for i in range(N_STEPS + (1 if use_counter else 0)):
            d = L.SamplerDesc()
            d.x = d.prev = x.data_ptr()
            d.x_dtype = d.prev_dtype = d.mo_dtype = d.unet_dtype = d.cn_dtype = d.concat_dtype = L.F16
            d.model_out, d.unet_in, d.cn_in, d.concat, d.g = mos[min(i, N_STEPS - 1)].data_ptr(), un.data_ptr(), cn.data_ptr(), cat.data_ptr(), G.data_ptr()
            d.outer, d.C, d.inner, d.C2, d.R, d.cn_frames = cs.outer, cs.C, cs.inner, cs.C2, 2, 0
            d.g_count, d.g_inner, d.g_scalar = 3, cs.C * cs.inner, 1.0
            L.check(lib.ctrl_op_sampler_step(L.ptr(t32), N_STEPS, L.ptr(counter), L.ptr(sc), C.byref(d), -1 if use_counter else i, 1, st))
            if i == N_STEPS - 1:
                torch.cuda.synchronize()
                finals.append((x.clone(), un.clone(), cn.clone(), sc.clone()))
        torch.cuda.synchronize()
        if use_counter:
            assert counter.tolist() == [N_STEPS, 0]
            assert torch.equal(x, finals[-1][0]) and torch.equal(un, finals[-1][1])          # the sixth launch changed nothing
        else:
            assert counter.tolist() == [0, 0]
    for a, b in zip(finals[0], finals[1]):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(finals[0][0].float()).all())


def test_bad_descriptors_are_refused(L, gpu, table):
    t64, t32 = table
    lib, st = L.lib(), L.cur_stream()
    cs = Case(L, gpu, "bchw", 1, 1, (8, 8), 1, F16, F16, False, "same", "scalar", seed=1)
    X, MO = cs._in(cs.x), cs._in(cs.mo)
    d = cs.desc(X, MO, X)
    assert lib.ctrl_op_sampler_step(L.ptr(t32), N_STEPS, None, None, C.byref(d), N_STEPS, 0, st) == 1          # a row past the table
    assert lib.ctrl_op_sampler_step(L.ptr(t32), N_STEPS, None, None, C.byref(d), -1, 0, st) == 1               # no counter to read
    d.R = 3
    assert lib.ctrl_op_sampler_step(L.ptr(t32), N_STEPS, None, None, C.byref(d), 0, 0, st) == 1
    assert b"R must be 1 or 2" in lib.ctrl_last_error()
    torch.cuda.synchronize()
    X.assert_untouched("refused launches")


def test_scheduler_drop_in_step_and_scale(gpu):
    """pipe.scheduler's surface on the GPU: scale_model_input and step (prev in model_output.dtype, index advancing) against fp64"""
    import ctrl_adapter_amd as P
    for sch in (P.EulerDiscreteScheduler(prediction_type="v_prediction", use_karras_sigmas=True, sigma_min=0.002, sigma_max=700.0,
                                         timestep_type="continuous", timestep_spacing="leading", steps_offset=1),
                P.DDIMScheduler(clip_sample=False, prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")):
        sch.set_timesteps(4, device=gpu)
        assert sch.timesteps.device.type == "cuda"
        gen = torch.Generator().manual_seed(8)
        x = (torch.randn(1, 3, 4, 6, 5, generator=gen) * sch.init_noise_sigma)
        lat = x.to(gpu)
        for i, t in enumerate(sch.timesteps):
            m = torch.randn(x.shape, generator=gen).half()
            inp = sch.scale_model_input(lat, t)
            ref_in = float(sch.table[i, 0]) * lat.cpu().double()
            assert inp.dtype == lat.dtype
            assert_within(inp, ref_in, input_bound(ref_in, F32), "%s scale_model_input %d" % (type(sch).__name__, i))
            out = sch.step(m.to(gpu), t, lat)
            assert out.prev_sample.dtype == torch.float16 and out[0] is out.prev_sample
            A, B = float(sch.table[i, 1]), float(sch.table[i, 2])
            ref = A * lat.cpu().double() + B * m.double()
            assert_within(out.prev_sample, ref, step_bound(ref, F16, A, B, lat.cpu().double(), m.double(), None, None),
                          "%s step %d" % (type(sch).__name__, i))
            lat = out.prev_sample.float()
        tm, a0, a1 = sch.timestep_tensors
        assert tm.shape == (1,) and tm.dtype == torch.float32 and tm.is_cuda
        assert float(tm) == float(sch.table[3, 3].float())


def test_step_with_a_repeated_timestep(gpu):
    """step() itself, called twice with the SAME t: Euler found its row at the first call and moves on (rows 1, then 2), as diffusers'
    step index does; DDIM's coefficients are a function of t, so it takes row 1 both times.  Also a sample that is neither 4-D nor 5-D,
    which scale_model_input and step both take."""
    import ctrl_adapter_amd as P
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(2, 50, generator=gen)
    m = torch.randn(2, 50, generator=gen)
    for sch, rows in ((P.EulerDiscreteScheduler(prediction_type="epsilon", timestep_spacing="trailing"), (1, 2)),
                      (P.DDIMScheduler(clip_sample=False, prediction_type="epsilon"), (1, 1))):
        sch.set_timesteps(4, device=gpu)
        t = sch.timesteps[1]
        for call, row in enumerate(rows):
            out = sch.step(m.to(gpu), t, x.to(gpu), return_dict=False)[0]
            A, B = float(sch.table[row, 1]), float(sch.table[row, 2])
            ref = A * x.double() + B * m.double()
            assert_within(out, ref, step_bound(ref, F32, A, B, x.double(), m.double(), None, None),
                          "%s call %d with the same t: row %d" % (type(sch).__name__, call, row))
        if rows == (1, 2):
            assert sch.step_index == 3
            assert float(sch.table[1, 2]) != float(sch.table[2, 2])          # the two rows differ, so the check above tells them apart
        sch.set_timesteps(4, device=gpu)
        scaled = sch.scale_model_input(x.to(gpu), sch.timesteps[2])
        ref = float(sch.table[2, 0]) * x.double()
        assert scaled.shape == x.shape
        assert_within(scaled, ref, input_bound(ref, F32), "%s scale_model_input of a 2-D sample" % type(sch).__name__)
