"""conv1 of the SDXL adapter's up-sampling ResNets in the phase form (csrc/plan_common.cpp: run_resnet; CTRL_CONV_UP_PHASE), end to end
on a tiny adapter: the policy on and off against each other and against the CPU oracle, what the profiler saw, and a captured graph."""
import pytest
import torch

import cases
from conftest import rel_inf
from oracle.init import seeded_init, seeded_tensor

pytestmark = pytest.mark.gpu
TOL_ADAPTER = 1e-3      # the bound of the existing adapter and chain tests (tests/test_gpu_e2e.py)
TOL_ON_OFF = 2e-3       # the two forms against each other, per output tensor


def test_adapter_conv1_phase_form_on_off_oracle_and_graph(gpu):
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    from oracle.adapter import ControlNetAdapterOracle
    torch.set_grad_enabled(False)
    N = 2
    ad = seeded_init(P.ControlNetAdapter(**cases.ADAPTER_SDXL), seed=22).to(gpu)
    downs, _ = cases.pyramid_inputs(N=N, h0=8, seed=200, with_mid=False)
    ehs = seeded_tensor((N, 77, 2048), 290)
    ins = [d.half().to(gpu) for d in downs]
    kw = dict(sparsity_masking=None, num_frames=1, timestep=torch.tensor(749.0).to(gpu), encoder_hidden_states=ehs.half().to(gpu))
    ad(ins, **kw)                                     # builds the plan
    torch.cuda.synchronize()

    def run(value):
        prev = ops.set_policy("CTRL_CONV_UP_PHASE", value)
        try:
            with ops.Profiler() as prof:
                o, m = ad(ins, **kw)
            torch.cuda.synchronize()
        finally:
            ops.set_policy("CTRL_CONV_UP_PHASE", prev)
        assert m is None
        return [x.clone() for x in o], [rec[2] for rec in prof.launches if rec[1].startswith("igemm")]

    on, d_on = run(None)
    off, d_off = run("0")
    n_phase = sum("taps4 phase" in d for d in d_on)
    print("PHASE adapter: %d phase launches with the form on: %s" % (n_phase, sorted({d for d in d_on if "phase" in d})))
    assert n_phase >= 3, d_on                          # conv1 of locations A, B, C (grouped: one launch per location)
    assert not any("phase" in d for d in d_off), d_off
    assert len(d_on) == len(d_off)                     # the form replaces launches one for one

    oa = seeded_init(ControlNetAdapterOracle(**cases.ADAPTER_SDXL).eval(), seed=22)
    ro, _ = oa(downs, sparsity_masking=None, num_frames=1, timestep=torch.tensor(749.0), encoder_hidden_states=ehs)
    worst = {"on/off": 0.0, "on": 0.0, "off": 0.0}
    for i, (a, b, r) in enumerate(zip(on, off, ro)):
        if r.abs().max().item() == 0.0:
            assert a.abs().max().item() == 0.0 and b.abs().max().item() == 0.0
            continue
        e = (rel_inf(a, b), rel_inf(a, r), rel_inf(b, r))
        print("PHASE adapter out %2d: on vs off %.2e   on vs oracle %.2e   off vs oracle %.2e" % ((i,) + e))
        worst = {k: max(worst[k], v) for k, v in zip(("on/off", "on", "off"), e)}
        assert e[0] <= TOL_ON_OFF, "output %d: the two forms differ by %.3e" % (i, e[0])
        assert e[1] <= TOL_ADAPTER and e[2] <= TOL_ADAPTER, "output %d vs the oracle: on %.3e, off %.3e" % (i, e[1], e[2])
    print("PARITY adapter conv1 phase form: worst %s" % worst)

    # the form under a captured graph (the lanes are on there; the profiler above runs on one lane)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ad(ins, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o2, _ = ad(ins, **kw)
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(o2, on)):
            assert torch.equal(a, b), "graph replay %d: output %d differs from the eager forward" % (rep, i)
    del g
