"""PixelDiscriminator on the HIP kernels, layer by layer and in both directions: after ONE forward and ONE backward every
launch group of `DiscEngine.forward` / `backward` (ammcnet_aaai2021_amd/discriminator.py) is compared with an fp64
evaluation of that layer alone on the operands it actually read, as they stand in the engine's retained buffers
(`slot.acts`, `slot.acts16`, the shared `eng._grads` / `eng._grads16`).  tests/test_gpu_discriminator.py sees the same
descriptors only end to end (1e-5 on the patch map, 1e-4 L2-relative per gradient tensor).  References and readers:
tests/aux_refs.py; their CPU half and the conditions on the inputs: tests/test_aux_refs_host.py.

Cases (B, H, W), filters (128, 256, 512, 512): (2, 8, 8) - 8 -> 5 -> 3 -> 2, head 3: odd levels, the two row parities of a
stride-2 input gradient have different extents; (3, 40, 72); (1, 5, 7); (2, 1, 9) - H = 1 at every level: the parity
py = 1 has no rows (the `hh <= 0` skip) and the head's 16-tap gradient window reads only halo above and below; and
(2, 9, 11) with filters (64, 128, 128).

Per layer i: the forward output from the input as read (its S16 twin in "s16"); `gs[i - 1]` = LeakyReLU-backward, by the
mask of `acts[i]`, of the fp64 input gradient of layer i from `gs[i]` as read (layer 0: `x.grad`); dW and db from
(`acts[i]`, `gs[i]`).  Gates (none fitted to the engine):
  S16 convolutions   max|got - want| / max|want| <= GATE_S16 = 2e-6 (tests/conv_gemm_cases.py)
  S16 dW             GATE = 3e-6 (tests/wgrad_cases.py)
  fp32 form          e_hip <= 3 e_witness, the witness torch's fp32 CPU evaluation of the same layer on the same operands
  db                 the bound of `ammc_chan_sum_f32` in tests/test_gpu_stream_kernels.py: 2 (n + 1) u sum|g| per channel
`RATIO ...` lines print error / gate per layer.

Exact contracts: every S16 twin - activations, packed filters, gradients after the engine's power of two - is the codec's
encoding of its fp32 tensor; halos of acts / acts16 / gs / gs16 are zero; the pad channels of the head's gradient and of the first input are zero;
with `deterministic` on the same gates hold and two runs give the same bits."""
import os

import pytest
import torch

import ammcnet_aaai2021_amd as A
import aux_refs as X
from ammcnet_aaai2021_amd import _lib, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ("s16", "fp32")


def _ids(case):
    return "%dx%dx%d-%d" % (*case[0], len(case[1]))


def _run(case, precision, det=False) -> X.DiscRun:
    shape, filters = case
    r = X.DiscRun()
    r.sd = S.make_discriminator_state(3, filters)
    net = A.PixelDiscriminator(3, list(filters), use_norm=False)
    net.load_state_dict(r.sd, strict=True)
    net.precision, net.deterministic = precision, det
    net = net.to(DEV).train()
    x, wgt = X.disc_inputs(shape, filters)
    xg = x.to(DEV).requires_grad_(True)
    y = net(xg)
    assert y.shape == wgt.shape
    (y * wgt.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    eng = net._engine
    assert eng.s16 == (precision == "s16") and eng.slots_created == 1
    pool = eng._pools[tuple(shape)]
    assert len(pool) == 1, "the backward gives the slot back"
    slot, cache = pool[0], {}
    r.s16, r.layers = eng.s16, [(L.cin, L.cout, L.stride, L.cin_p, L.gc) for L in eng.layers]
    r.acts = [X.store(a, cache) for a in slot.acts]
    r.acts16 = [X.store(a, cache) for a in slot.acts16] if eng.s16 else None
    r.gs = [X.store(g, cache) for g in eng._grads[tuple(shape)]]
    r.gs16 = [X.store(g, cache) for g in eng._grads16[tuple(shape)]] if eng.s16 else None
    r.twins = [(a.cpu(), b.cpu()) for a, b in zip(slot.wp + slot.wd, slot.w16 + slot.wd16)] if eng.s16 else []
    r.out, r.dx = y.detach().cpu(), xg.grad.cpu()
    r.grads = {k: p.grad.cpu() for k, p in net.named_parameters()}
    r.blocks = [int(_lib.load().ammc_chan_reduce_blocks(shape[0] * g.H * g.W)) for g in r.gs]
    return r


def _report(line: str):
    print(line)
    if os.environ.get("AMMC_AUX_RATIOS"):
        with open(os.environ["AMMC_AUX_RATIOS"], "a") as fp:
            fp.write(line + "\n")


def _check(r: X.DiscRun, tag: str):
    bad = X.disc_contracts(r)
    assert not bad, f"{tag}: {bad}"
    res = X.disc_check(r)
    for name, ratio, text in res:
        _report(f"RATIO {tag} {name} {ratio:.3g} ({text})")
    bad = [x for x in res if not x[1] <= 1.0]
    assert not bad, f"{tag}: layers beyond their gate (name, error / gate, figures): {bad}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", X.DISC_CASES, ids=_ids)
def test_every_layer_both_directions_against_fp64_of_its_own_operands(case, precision):
    _check(_run(case, precision), f"disc[{precision}] {_ids(case)}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", X.DISC_CASES, ids=_ids)
def test_deterministic_same_gates_and_the_same_bits_twice(case, precision):
    a = _run(case, precision, det=True)
    _check(a, f"disc[{precision}, det] {_ids(case)}")
    b = _run(case, precision, det=True)

    def same(p, q):
        return torch.equal(p.contiguous().view(torch.int32), q.contiguous().view(torch.int32))

    assert same(a.out, b.out) and same(a.dx, b.dx)
    diff = [k for k in a.grads if not same(a.grads[k], b.grads[k])]
    assert not diff, f"gradients that differ between two deterministic runs: {diff}"
