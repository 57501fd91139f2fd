"""FlowNet2-SD on the HIP kernels, layer by layer: after ONE forward every layer of `ammcnet_aaai2021_amd/flownet.py` is
compared with an fp64 evaluation of that layer alone on the inputs it actually read, as they stand in the engine's
workspace (`net._engine.ws`: one buffer per layer output, nothing reused) - the descriptors and pointer arithmetic of
`_Engine._conv` / `_deconv` / `forward`, which tests/test_gpu_flownet.py sees only through 26 layers at 2e-5 of max|flow|.
References and readers: tests/aux_refs.py; their CPU half and the conditions on the inputs: tests/test_aux_refs_host.py.

Shapes: (2, 64, 64) - the 1/64 level is one pixel, every tap but the centre reads halo, deconv5 is all border;
(3, 64, 128) - odd batch, row stride != pixel stride at every level; (1, 128, 64) - transposed.

Gates (none fitted to the engine):
  S16 layers       max|got - want| / max|want| <= GATE_S16 = 2e-6 (tests/conv_gemm_cases.py), multi-part layers included: the
                   host file shows the S16 stores between parts cost a correct evaluation <= 0.14 gate
  fp32 layers      e_hip <= 3 e_witness, the witness torch's fp32 CPU evaluation of the same layer on the same operands
                   (tests/test_gpu_conv_gemm.py): the whole "fp32" form, and the 2 -> 2 up-convolutions in both forms
  prep, x4 resize  the element-wise bounds of tests/test_gpu_stream_kernels.py
`RATIO ...` lines print error / gate per layer.

Exact contracts: zero halos; zero pad channels of the flow estimates and of the prepared frame pair; `x0s` / `u*` are the
codec's encoding of `x0` / `uf*`; every slice of a concatenation buffer is checked against its own producer AFTER the whole
forward, so a neighbour that wrote into it shows; shape A, shape B, shape A again gives the first flow bit for bit."""
import os

import pytest
import torch

import aux_refs as X
from ammcnet_aaai2021_amd import synthetic as S
from ammcnet_aaai2021_amd.flownet import FlowNet2SD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ("s16", "fp32")


class _Run:
    pass


@pytest.fixture(scope="module")
def runs():
    """one network per precision and one forward per (shape, precision), shared by the tests of this file"""
    cache = dict(sd=S.make_flownet2sd_state(), nets={}, runs={})
    yield cache
    cache.clear()


def _net(cache, precision):
    if precision not in cache["nets"]:
        net = FlowNet2SD()
        net.load_state_dict(cache["sd"], strict=True)
        net.precision = precision
        cache["nets"][precision] = net.to(DEV).eval()
    return cache["nets"][precision]


def _forward(cache, shape, precision) -> _Run:
    key = (shape, precision)
    if key not in cache["runs"]:
        net = _net(cache, precision)
        r = _Run()
        r.x = X.flow_inputs(shape)
        out = net(r.x.to(DEV))
        torch.cuda.synchronize()
        assert getattr(net, "s16_fallbacks", 0) == 0, "the S16 range guard recomputed the batch on the fp32 engine"
        eng = net._engine
        assert eng.s16 == (precision == "s16")
        ws = [v for k, v in eng.ws.items() if tuple(k[:3]) == tuple(shape)]
        assert len(ws) == 1
        r.out, r.st, r.s16 = out.cpu(), X.flow_store(ws[0], eng.s16), eng.s16
        cache["runs"][key] = r
    return cache["runs"][key]


def _report(line: str):
    print(line)
    if os.environ.get("AMMC_AUX_RATIOS"):
        with open(os.environ["AMMC_AUX_RATIOS"], "a") as fp:
            fp.write(line + "\n")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", X.FLOW_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_every_layer_against_fp64_of_its_own_inputs(runs, shape, precision):
    r = _forward(runs, shape, precision)
    tag = f"flownet[{precision}] {shape}"
    res = X.flow_check(r.st, r.s16, r.x, r.out, runs["sd"])
    for name, ratio, text in res:
        _report(f"RATIO {tag} {name} {ratio:.3g} ({text})")
    bad = [x for x in res if not x[1] <= 1.0]
    assert not bad, f"{tag}: layers beyond their gate (name, error / gate, figures): {bad}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", X.FLOW_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_exact_contracts_of_the_workspace(runs, shape, precision):
    r = _forward(runs, shape, precision)
    bad = X.flow_contracts(r.st, r.s16)
    assert not bad, f"flownet[{precision}] {shape}: {bad}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_shape_a_then_b_then_a_again_gives_the_same_bits(runs, precision):
    """cached workspaces and packs: a forward at another size in between changes nothing"""
    a, b = X.FLOW_SHAPES[0], X.FLOW_SHAPES[2]
    first = _forward(runs, a, precision)
    net = _net(runs, precision)
    net(X.flow_inputs(b).to(DEV))
    third = net(first.x.to(DEV)).cpu()
    assert torch.equal(third.view(torch.int32), first.out.view(torch.int32))
    assert getattr(net, "s16_fallbacks", 0) == 0
