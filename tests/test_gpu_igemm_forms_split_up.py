"""The implicit GEMM's paired split-operand walk (a_split = 2) TOGETHER with the nearest x2 gather (up = 2): the Upsample2D convolutions
of the KL-VAE decoder (csrc/plan_vae_decoder.cpp) read the fp32 stream's split [hi | lo] mirror through the up-sampling.
tests/test_gpu_igemm_forms.py has split forms and up-2 forms, none with both; these rows add them for every tile form the dispatcher
picks at the decoder's shapes (few tiles, the 128-wide ring tiles, the wide tiles forced and by default), with that file's runner:
the kernel symbol is pinned, every element is bounded against an fp64 reference (helpers.assert_igemm_close), and the surroundings of
every operand are poisoned (helpers.Guarded)."""
import pytest

from test_gpu_igemm_forms import CONV, F16, F32, C, ops, ring, run_case, wide8  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

FORMS = [
    (ring(64, 64, 64, 2, 2, 3, CONV), "a_split = 2, up = 2, few tiles",
     [C("paired up2 64x64x64 conv 5x7", mode=CONV, n=3, H=5, W=7, up=2, Cin=128, Nout=80, a_split=2, res=F32),
      C("paired up2 64x64x64 conv 1x3 split mirror", mode=CONV, n=2, H=1, W=3, up=2, Cin=128, Nout=64, a_split=2, res=F32, out=F32, mirror="split"),
      C("paired up2 64x64x64 conv 6x4 Cin/2=192", mode=CONV, n=2, H=6, W=4, up=2, Cin=384, Nout=80, a_split=2)]),
    (ring(128, 64, 64, 2, 2, 3, CONV), "a_split = 2, up = 2, >= 192 tiles of 128 x 64, eff(128) <= 0.8",
     [C("paired up2 128x64x64 conv 29x25", mode=CONV, n=3, H=29, W=25, up=2, Cin=128, Nout=192, a_split=2, res=F32)]),
    (ring(128, 128, 64, 2, 4, 4, CONV), "a_split = 2, up = 2, >= 192 tiles of 128^2",
     [C("paired up2 128x128x64 conv 24x22", mode=CONV, n=3, H=24, W=22, up=2, Cin=128, Nout=512, a_split=2, res=F16)]),
    (wide8(4, CONV), "a_split = 2, up = 2, set_igemm_wide(2)",
     [C("paired up2 wide4 conv 5x7", mode=CONV, n=5, H=5, W=7, up=2, Cin=128, Nout=256, a_split=2, wide=2, res=F32),
      C("paired up2 wide4 conv 9x3 split mirror", mode=CONV, n=3, H=9, W=3, up=2, Cin=256, Nout=256, a_split=2, wide=2, out=F32, mirror="split")]),
    (wide8(5, CONV), "a_split = 2, up = 2, set_igemm_wide(2)",
     [C("paired up2 wide5 conv 7x5", mode=CONV, n=5, H=7, W=5, up=2, Cin=128, Nout=320, a_split=2, wide=2)]),
    (wide8(4, CONV), "a_split = 2, up = 2, default: the grid fills the chip",
     [C("paired up2 wide4 conv default 113x113", mode=CONV, n=1, H=113, W=113, up=2, Cin=128, Nout=256, a_split=2, out=F32, mirror="split")]),
    (wide8(5, CONV), "a_split = 2, up = 2, default: the grid fills the chip",
     [C("paired up2 wide5 conv default 113x91", mode=CONV, n=1, H=113, W=91, up=2, Cin=128, Nout=320, a_split=2)]),
]

ALL = [(sym, how, c) for sym, how, cs in FORMS for c in cs]


@pytest.mark.parametrize("idx", range(len(ALL)), ids=[c.name.replace(" ", "_") for _, _, c in ALL])
def test_split_up_form(ops, gpu, idx):  # noqa: F811
    sym, how, c = ALL[idx]
    run_case(ops, gpu, sym, c, seed=500 + idx)
