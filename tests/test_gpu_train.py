"""Training-mode parity of the HIP path: one optimisation step's forward outputs, every
parameter gradient and the in-place buffer updates (BatchNorm running statistics, EMA
codebook), against the CPU oracle with autograd and the vectors recorded from the reference.

Gradient gates (L2-relative per tensor) - there are exactly two kinds, and neither is fitted to a distance between two
fp32 evaluations:
  * ARITHMETIC, on fixtures where no ReLU mask can flip (`test_gradients_without_relu_flips_match_the_fp64_oracle`,
    every frame size the other tests use): 1e-4 per tensor against the oracle in float64 (measured: 3.6e-6 max for the
    default S16 training kernels);
  * SAME-BRANCH TRUTH (tests/truth.py), on the ordinary fixtures: the oracle in float64 taking the memory lookups the HIP
    evaluation made; per-tensor norms within SURVEY.md 8(d)'s 1e-3, entries within twice what the reference's own fp32
    arithmetic (recorded in the fixtures, or the oracle's fp32 evaluation on the host) is away from the truth on ITS
    branch.  Batch 32 (the timed batch): per tensor.  Batch 2 / 4: against the envelope of two fp32 witnesses - at these
    sizes a tensor's error is zero to three flipped ReLU masks, and the witnesses fail a per-tensor comparison against
    each other (truth.py's header has the measurement).
Outputs 1e-4 of max|ref|; buffers 1e-4."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import synthetic as S
from oracle import ammc_oracle as O
from conftest import GOLDEN, rel_err
import truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _l2rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _fixture_ref(d, names):
    """(dense samples, norms, lookups) the reference recorded for a generator-only step (make_golden.py `twostream_train`)"""
    return {n: d[f"gs4k.{n}"] for n in names}, {n: float(d[f"gn.{n}"]) for n in names}, T.fixture_idx(d)


def _truth_gate(net, sd, clips, mode="small_batch", ref=None, what=""):
    g_hip = {n: p.grad.detach() for n, p in net.named_parameters()}
    for n, g in g_hip.items():
        assert g is not None, n
    T.assert_ok(T.same_branch_verdict(T.g_stepper(sd, clips), g_hip, T.hip_lookups(net), DEV, mode, ref=ref, what=what))


def _train_step(net, sd, batch, hw, tag, k=2, train_precision="s16"):
    h, w = hw if isinstance(hw, tuple) else (hw, hw)
    rgb_x, op_x, rgb_t, op_t = S.make_clips(batch, h, w, tag=tag)
    net.train()
    net.train_precision = train_precision
    out = net(rgb_x.to(DEV), op_x.to(DEV))
    loss = O.generator_loss(out, rgb_t.to(DEV), op_t.to(DEV))
    loss.backward()
    msd = O.clone_state(sd, requires_grad=True)
    want = O.twostream_forward(msd, rgb_x, op_x, k, training=True)
    wloss = O.generator_loss(want, rgb_t, op_t)
    wloss.backward()
    return out, loss, want, wloss, msd


@pytest.mark.parametrize("train_precision", ["s16", "fp32"])
def test_twostream_train_step_vs_oracle_and_golden(train_precision):
    d = np.load(os.path.join(GOLDEN, "twostream_64_b2_train.npz"))
    cfg = json.loads(str(d["cfg"]))
    sd = S.make_twostream_state()
    net = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    net.load_state_dict(sd)
    net = net.to(DEV)
    out, loss, want, wloss, msd = _train_step(net, sd, cfg["batch"], cfg["hw"], cfg["tag"], train_precision=train_precision)
    assert net._train_engine.precision == train_precision
    assert rel_err(out[0].detach().cpu(), want[0]) <= 1e-4 and rel_err(out[1].detach().cpu(), want[1]) <= 1e-4
    assert rel_err(out[0].detach().cpu(), d["rgb"]) <= 1e-4 and rel_err(out[1].detach().cpu(), d["op"]) <= 1e-4
    assert rel_err(out[2][0].detach().cpu(), want[2][0]) <= 1e-4 and rel_err(out[2][1].detach().cpu(), want[2][1]) <= 1e-4
    assert abs(float(loss) - float(d["loss"])) <= 1e-4 * abs(float(d["loss"]))
    # gradients: the fp64 truth on this evaluation's branch, gated by the reference's own recorded fp32 gradients
    names = [n for n, _ in net.named_parameters()]
    _truth_gate(net, sd, S.make_clips(cfg["batch"], cfg["hw"], cfg["hw"], tag=cfg["tag"]), ref=_fixture_ref(d, names),
                what=f"64x64 batch 2, {train_precision}")
    # buffers updated inside forward: BN running stats, num_batches_tracked, EMA codebook
    nsd = net.state_dict()
    for key, v in msd.items():
        if key in dict(net.named_parameters()):
            continue
        assert rel_err(nsd[key].cpu().double(), v.double()) <= 1e-4, key
    for key in d.files:
        if key.startswith("buf."):
            assert rel_err(nsd[key[4:]].cpu().double(), d[key].astype(np.float64)) <= 1e-4, key


def _mask_free_state(tag="ammc"):
    """the synthetic parameters with every BatchNorm affine set to gamma = +-0.2, beta = 2: relu(gamma * xhat + beta)
    never clips, so no ReLU mask can flip between two evaluations of the step - what is left of the network (batch
    statistics, the memory block, max-pool, tanh, every conv / ConvTranspose) is a smooth function of the weights"""
    sd = S.make_twostream_state(tag=tag)
    out = {}
    for k, v in sd.items():
        leaf = k.rsplit(".", 1)[-1]
        if leaf in ("weight", "bias") and v.dim() == 1 and (k[:-len(leaf)] + "running_mean") in sd:
            out[k] = 0.2 * torch.sign(v) if leaf == "weight" else torch.full_like(v, 2.0)
        else:
            out[k] = v.clone()
    return out


def _oracle_grads(sd, clips, dtype, device="cpu"):
    rgb_x, op_x, rgb_t, op_t = (t.to(device=device, dtype=dtype) for t in clips)
    m = O.clone_state({k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)) for k, v in sd.items()},
                      requires_grad=True)
    out = O.twostream_forward(m, rgb_x, op_x, 2, training=True)
    loss = O.generator_loss(out, rgb_t, op_t)
    loss.backward()
    return float(loss.detach()), {k: v.grad.double().cpu() for k, v in m.items() if v.requires_grad}, [o.detach().cpu() for o in out[:2]]


@pytest.mark.parametrize("hw,batch", [((64, 64), 2), ((50, 36), 2), ((27, 21), 2), ((100, 100), 2), ((128, 128), 4), ((256, 256), 2)])
@pytest.mark.parametrize("train_precision", ["s16", "fp32"])
def test_gradients_without_relu_flips_match_the_fp64_oracle(train_precision, hw, batch):
    """The tight gradient gate.  On the ordinary fixtures a pre-activation within rounding noise of 0 flips its ReLU
    mask and moves whole gradient entries (the reference's own fp32 and fp64 gradients differ by 2e-3 there), so those
    gates cannot be tight.  Here no mask can flip (`_mask_free_state`), the truth is the oracle in FLOAT64, and every
    gradient tensor of both training precisions must agree with it to 1e-4 L2-relative - or, for the few tensors where
    the oracle's own fp32 evaluation is noisier than 3e-5 against fp64 (ill-conditioned sums), to 3x that noise.
    One discontinuity is left, max-pool near-ties: the exact-fp32 kernels (an fmaf chain over K up to 4608 per output)
    move forward values in the 6th digit, which re-routes ~0.01 % of the pooling windows (tools/train_fp32_debug.py:
    the inputs of `maxpool2x2_bwd` agree to 6e-6, its outputs to 1.7e-2); the S16 kernels' tree sums stay below the
    tie gaps of this fixture.  (Round 6: the pool routes of the evaluation under test are part of the branch the fp64
    truth takes - the S16 engine's recorded bytes, the first maxima of the fp32 engine's own skip tensors - so EVERY
    tensor of BOTH precisions is held to the tight gate; the 8e-3 allowance for `train_precision = "fp32"` is gone.)
    50x36 (-> 25x18 -> 12x9 -> 6x4) and 27x21 (-> 13x10 -> 6x5 -> 3x2): levels of odd size, which MaxPool2d floors and
    `up.forward` pads on the right / bottom (models/unet_parts.py).  Round 6: also 100x100, 128x128 (batch 4) and 256x256 -
    the sizes of the flip-prone fixtures whose gradient gates are the two-witness envelope of tests/truth.py: THIS is their
    per-tensor arithmetic gate (the halo-patch forward / input-gradient / weight-gradient instances of the 128- and
    256-pixel levels included)."""
    sd = _mask_free_state()
    clips = S.make_clips(batch, hw[0], hw[1], tag="maskfree")
    odev = DEV if hw[0] >= 100 else "cpu"            # (round 6: every frame size the flip-prone fixtures use; the larger ones on the device)
    net = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    net.train_precision = train_precision
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in clips)
    out = net(rgb_x, op_x)
    assert net._train_engine.precision == train_precision
    loss = O.generator_loss(out, rgb_t, op_t)
    loss.backward()
    # the truth on the branch this evaluation took: its memory lookups and - the default S16 engine records them, one byte
    # per pooled element - the routes of its max-pools (round 6: at 100x100 and above some 2x2 window of the ~1e6 always
    # ties inside rounding noise, and a re-routed element moves the gradients upstream of it by up to 5e-3)
    branch = T.branch_to(T.hip_lookups(net), odev)
    assert "pool" in branch                # (s16: the engine's recorded routes; fp32: the first maxima of its own skip tensors)
    loss64, g64, _, _ = T.g_step(sd, clips, torch.float64, odev, force_idx=branch)
    g64 = {k: v.double().cpu() for k, v in g64.items()}
    out64 = [o.cpu() for o in O.twostream_forward(T._cast(sd, torch.float64, odev, False), clips[0].to(odev).double(),
                                                  clips[1].to(odev).double(), 2, training=True, force_idx=branch)[:2]]
    _, g32, _ = _oracle_grads(sd, clips, torch.float32, odev)
    assert abs(float(loss) - loss64) <= 2e-6 * abs(loss64)
    assert rel_err(out[0].detach().cpu(), out64[0]) <= 1e-5 and rel_err(out[1].detach().cpu(), out64[1]) <= 1e-5
    bad, errs = [], []
    for name, p in net.named_parameters():
        e = _l2rel(p.grad.cpu(), g64[name])
        noise = _l2rel(g32[name], g64[name])
        errs.append(e)
        if e > max(1e-4, 3.0 * noise):
            bad.append((name, e, noise))
    assert not bad, bad
    assert float(np.median(errs)) <= 2e-5, float(np.median(errs))


def test_eval_after_train_uses_updated_buffers():
    """the eval plans must be re-packed after a training forward changed BN stats / codebook"""
    sd = S.make_twostream_state()
    net = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    net.load_state_dict(sd)
    net = net.to(DEV)
    rgb_x, op_x, _, _ = S.make_clips(2, 64, 64, tag="tr-ev")
    net.eval()
    before = net(rgb_x.to(DEV), op_x.to(DEV))[0].clone()
    net.train()
    with torch.no_grad():
        net(rgb_x.to(DEV), op_x.to(DEV))
    net.eval()
    after = net(rgb_x.to(DEV), op_x.to(DEV))[0]
    msd = O.clone_state(sd)
    with torch.no_grad():
        O.twostream_forward(msd, rgb_x, op_x, 2, training=True)
        want = O.twostream_forward(msd, rgb_x, op_x, 2)
    assert not torch.equal(before, after)
    assert rel_err(after.cpu(), want[0]) <= 1e-4


def test_unetmem_and_unet_train_step():
    """`UNetMem_v7` and the plain `UNet` (config 1's model) in training mode on their own, 32x48 at batch 2: forward,
    commit term, every gradient.  A 4x6 bottleneck is 48 values per channel - ONE flipped ReLU mask there is 3e-3 of a
    gradient tensor and two fp32 evaluations of the ordinary state disagree by that or by nothing at all - so the
    gradients are checked where no mask can flip (`_mask_free_state`: what remains is arithmetic): 1e-4 per tensor against
    the oracle in float64 on the HIP evaluation's own lookups."""
    full = _mask_free_state()
    sd = {k[4:]: v for k, v in full.items() if k.startswith("rgb.")}
    net = A.get_unet_vq_topk_res(12, 3, 64, 256, 2)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    x, _, t, _ = S.make_clips(2, 32, 48, tag="um")
    y, diff, q1 = net(x.to(DEV))
    loss = O.intensity_l2(y, t.to(DEV)) + diff.sum()
    loss.backward()
    idx_hip = net._train_engine._last["streams"][0].idx.reshape(-1, 2).long().cpu()
    m = O.clone_state({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, requires_grad=True)
    wy, wd, wq, widx = O.unetmem_forward(m, x.double(), 2, training=True, force_idx=idx_hip, want_idx=True)
    (O.intensity_l2(wy, t.double()) + wd.sum()).backward()
    own = O.unetmem_forward(O.clone_state({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}), x.double(), 2,
                            training=True, want_idx=True)[3]
    assert int((own != idx_hip).any(dim=1).sum()) <= 1                    # (the fp64 evaluation's own lookups: the same branch)
    assert rel_err(y.detach().cpu(), wy.detach()) <= 1e-5 and rel_err(diff.detach().cpu(), wd.detach()) <= 1e-5
    bad = [(n, _l2rel(p.grad.cpu(), m[n].grad)) for n, p in net.named_parameters() if _l2rel(p.grad.cpu(), m[n].grad) > 1e-4]
    assert not bad, bad
    # plain UNet (config 1 model) in training mode
    usd = {k: v for k, v in _mask_free_state(tag="ammc-unet").items() if k.startswith("rgb.") and ".vq_down3." not in k}
    usd = {k[4:]: v for k, v in usd.items()}
    u = A.get_unet(12, 3)
    u.load_state_dict(usd)
    u = u.to(DEV).train()
    yy = u(x.to(DEV))
    O.intensity_l2(yy, t.to(DEV)).backward()
    m2 = O.clone_state({k: (v.double() if v.is_floating_point() else v) for k, v in usd.items()}, requires_grad=True)
    wy2 = O.unet_forward(m2, x.double(), training=True)
    O.intensity_l2(wy2, t.double()).backward()
    assert rel_err(yy.detach().cpu(), wy2.detach()) <= 1e-5
    bad = [(n, _l2rel(p.grad.cpu(), m2[n].grad)) for n, p in u.named_parameters() if _l2rel(p.grad.cpu(), m2[n].grad) > 1e-4]
    assert not bad, bad


def test_harness_adam_is_torch_adam_in_fused_form():
    """`harness.adam` (what the bench's training legs step with) = the reference's `torch.optim.Adam(params, lr)`:
    same parameters after three steps as the default (foreach) form, up to fp32 rounding of the reordered update"""
    from ammcnet_aaai2021_amd import harness
    g = torch.Generator().manual_seed(5)
    shapes = [(64, 12, 3, 3), (64,), (128, 64, 3, 3), (256, 512), (3,)]
    init = [torch.randn(sh, generator=g) for sh in shapes]
    grads = [[torch.randn(sh, generator=g) * 10.0 ** (-k) for sh in shapes] for k in range(3)]
    outs = []
    for make in (lambda ps: harness.adam(ps, lr=1e-3), lambda ps: torch.optim.Adam(ps, lr=1e-3)):
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        opt = make(ps)
        for gs in grads:
            for p_, g_ in zip(ps, gs):
                p_.grad = g_.clone().to(DEV)
            opt.step()
        outs.append([p_.detach().cpu() for p_ in ps])
    assert harness.adam([torch.nn.Parameter(init[0].clone().to(DEV))], lr=1e-3).defaults["fused"] is True
    for a, b, t0 in zip(outs[0], outs[1], init):
        assert float((a - b).abs().max()) <= 5e-7 * max(1.0, float(t0.abs().max())), float((a - b).abs().max())
        assert float((a - t0).abs().max()) > 1e-4            # (the steps did move the parameters)


def test_adam_steps_track_the_oracle():
    """three optimiser steps end to end (weights change -> filters are re-packed every step)"""
    sd = S.make_twostream_state()
    net = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    msd = O.clone_state(sd, requires_grad=True)
    params = [v for v in msd.values() if v.requires_grad]
    wopt = torch.optim.Adam(params, lr=1e-4)
    losses, wlosses = [], []
    for step in range(3):
        rgb_x, op_x, rgb_t, op_t = S.make_clips(2, 64, 64, tag=f"adam{step}")
        opt.zero_grad()
        loss = O.generator_loss(net(rgb_x.to(DEV), op_x.to(DEV)), rgb_t.to(DEV), op_t.to(DEV))
        loss.backward()
        opt.step()
        wopt.zero_grad()
        wl = O.generator_loss(O.twostream_forward(msd, rgb_x, op_x, 2, training=True), rgb_t, op_t)
        wl.backward()
        wopt.step()
        losses.append(float(loss))
        wlosses.append(float(wl))
    assert np.allclose(losses, wlosses, rtol=2e-4), (losses, wlosses)


def test_train_step_at_sizes_the_halo_patch_kernels_take():
    """batch 4 at 128x128: the 128x128 and 64x64 levels go through conv_tap_s16 (fp32 outputs, fp32 residual of the
    input-gradient convs) and wgrad_tap3_s16, which the 64x64 fixtures above are too small to reach; compared with
    the oracle: outputs and buffers to 1e-4, gradients to the same-branch fp64 truth (tests/truth.py)."""
    sd = S.make_twostream_state()
    net = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    net.load_state_dict(sd)
    net = net.to(DEV)
    out, loss, want, wloss, msd = _train_step(net, sd, 4, 128, "train-128")
    assert rel_err(out[0].detach().cpu(), want[0]) <= 1e-4 and rel_err(out[1].detach().cpu(), want[1]) <= 1e-4
    assert abs(float(loss) - float(wloss)) <= 1e-4 * abs(float(wloss))
    _truth_gate(net, sd, S.make_clips(4, 128, 128, tag="train-128"), what="128x128 batch 4")
    nsd = net.state_dict()
    for key, v in msd.items():
        if key not in dict(net.named_parameters()):
            assert rel_err(nsd[key].cpu().double(), v.double()) <= 1e-4, key


@pytest.mark.parametrize("train_precision", ["s16", "fp32"])
@pytest.mark.parametrize("B,H,W", [(2, 100, 100)])
def test_train_step_at_sizes_not_divisible_by_8(B, H, W, train_precision):
    """100 -> 50 -> 25 -> 12: MaxPool2d floors, the 12 -> 24 ConvTranspose output is padded to 25 on the right / bottom
    (`up.forward`, models/unet_parts.py) and the pad's gradient dropped; the un-pooled last row / column of an odd level
    gets the skip gradient alone.  Same gates as the 128x128 test (and the mask-free 1e-4 test runs at this size too)."""
    sd = S.make_twostream_state()
    net = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    net.load_state_dict(sd)
    net = net.to(DEV)
    out, loss, want, wloss, msd = _train_step(net, sd, B, (H, W), f"train-{H}x{W}", train_precision=train_precision)
    assert rel_err(out[0].detach().cpu(), want[0]) <= 1e-4 and rel_err(out[1].detach().cpu(), want[1]) <= 1e-4
    assert abs(float(loss) - float(wloss)) <= 1e-4 * abs(float(wloss))
    _truth_gate(net, sd, S.make_clips(B, H, W, tag=f"train-{H}x{W}"), what=f"{H}x{W} batch {B}, {train_precision}")
    nsd = net.state_dict()
    for key, v in msd.items():
        if key not in dict(net.named_parameters()):
            assert rel_err(nsd[key].cpu().double(), v.double()) <= 1e-4, key


@pytest.mark.parametrize("B,H,W,C", [(2, 16, 32, 64), (3, 9, 7, 128), (1, 32, 32, 512)])
def test_fused_bn_backward_writes_the_s16_twin(B, H, W, C):
    """`ammc_bn_bwd_reduce_bound_f32` -> `ammc_bn_bwd_finalize_f32` -> `ammc_bn_bwd_apply_s16_f32` (the gradient of
    BatchNorm(batch stats) + ReLU straight into an S16 image, its power-of-two scale taken from a BOUND of max|dc| that
    the reduction pass yields) against the fp64 formula of `unet.py:11-16`'s backward: dbeta / dgamma 1e-5, dc 2e-6 of
    max|dc| after decoding the twin, the bound really bounds, and it is not looser than 8x."""
    from ammcnet_aaai2021_amd import _lib
    from ammcnet_aaai2021_amd.engine import Act, _ptr
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    tag = f"bnbwd-{B}-{H}-{W}-{C}"
    craw = Act(torch.zeros(B, H + 2, W + 2, C, device=DEV), B, H, W, C, 0, 1)
    dy = Act(torch.zeros(B, H + 2, W + 2, C, device=DEV), B, H, W, C, 0, 1)
    craw.interior().copy_(S.hashed_normal(tag + "c", (B, H, W, C), 1.5).to(DEV))
    dy.interior().copy_((S.hashed_normal(tag + "g", (B, H, W, C), 1.0) * 3e-6).to(DEV))        # gradient-sized values
    gamma = (S.hashed_uniform(tag + "ga", (C,)) + 1.5).to(DEV)
    beta = (S.hashed_uniform(tag + "be", (C,)) * 0.2).to(DEV)
    x = craw.interior().double()
    mean, var = x.mean((0, 1, 2)), x.var((0, 1, 2), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale, shift = gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd
    g = dy.interior().double() * ((x * scale + shift) > 0)
    xhat = (x - mean) * invstd
    M = B * H * W
    sg, sgx = g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))
    want = scale * (g - sg / M - xhat * sgx / M)
    f32 = lambda t: t.float().contiguous()
    mean32, invstd32, scale32, shift32 = f32(mean), f32(invstd), f32(scale), f32(shift)
    nblk = lib.ammc_chan_reduce_blocks(M)
    partial = torch.zeros(nblk, 4, C, device=DEV)
    _lib.check(lib.ammc_bn_bwd_reduce_bound_f32(craw.pix0(), *craw.strides, dy.pix0(), *dy.strides, _ptr(mean32),
                                                _ptr(invstd32), _ptr(scale32), _ptr(shift32), 1, B, H, W, C,
                                                _ptr(partial), s), "reduce_bound")
    sums = torch.empty(2 * C, device=DEV)
    amax = torch.zeros(256, dtype=torch.int32, device=DEV)
    _lib.check(lib.ammc_bn_bwd_finalize_f32(_ptr(partial), nblk, C, M, _ptr(scale32), _ptr(sums), amax.data_ptr(), s), "fin")
    assert float((sums[:C].double() - sg).abs().max() / sg.abs().max()) <= 1e-5
    assert float((sums[C:].double() - sgx).abs().max() / sgx.abs().max()) <= 1e-5
    bound = float(amax.max().reshape(1).view(torch.float32))                # the slots hold float bit patterns
    true_max = float(want.abs().max())
    assert true_max <= bound <= 8.0 * true_max, (true_max, bound)
    dc16 = Act(torch.zeros(B, H + 2, W + 2, C, device=DEV), B, H, W, C, 0, 1)
    dc32 = Act(torch.zeros(B, H + 2, W + 2, C, device=DEV), B, H, W, C, 0, 1)
    inv = torch.empty(16, device=DEV)
    _lib.check(lib.ammc_bn_bwd_apply_s16_f32(craw.pix0(), *craw.strides, dy.pix0(), *dy.strides, _ptr(mean32), _ptr(invstd32),
                                             _ptr(scale32), _ptr(shift32), _ptr(sums), 1, dc16.pix0(), dc32.pix0(),
                                             *dc16.strides, B, H, W, C, amax.data_ptr(), _ptr(inv), 16, s), "apply_s16")
    back = torch.empty(B, C, H, W, device=DEV)
    _lib.check(lib.ammc_s16_to_nchw_f32(dc16.pix0(), *dc16.strides, B, C, H, W, _ptr(back), s), "decode")
    got = back.permute(0, 2, 3, 1).double() * float(inv[0])
    assert float(inv[0]) == float(inv[15]) and 2.0 ** -12 <= true_max / float(inv[0]) < 2048.0
    assert float((got - want).abs().max() / true_max) <= 2e-6
    assert float((dc32.interior().double() - want).abs().max() / true_max) <= 2e-6
    assert float(dc16.buf[:, 0].abs().max()) == 0.0 and float(dc16.buf[:, :, 0].abs().max()) == 0.0      # halo untouched


def test_scale_shift_act_with_s16_output():
    """`ammc_scale_shift_act_s16_f32`: y = relu(x * scale + shift) + res as an S16 image (and optionally fp32) against
    the fp32 kernel's output: the fp32 copies are bit-identical, the decoded S16 image is within 2^-21 of them."""
    from ammcnet_aaai2021_amd import _lib
    from ammcnet_aaai2021_amd.engine import Act, _ptr
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    B, H, W, C = 2, 10, 12, 72
    mk = lambda: Act(torch.zeros(B, H + 2, W + 2, C, device=DEV), B, H, W, C, 0, 1)
    x, r, y_ref, y32, y16 = mk(), mk(), mk(), mk(), mk()
    x.interior().copy_(S.hashed_normal("ssa-x", (B, H, W, C), 2.0).to(DEV))
    r.interior().copy_(S.hashed_normal("ssa-r", (B, H, W, C), 0.5).to(DEV))
    scale = (S.hashed_uniform("ssa-s", (C,)) + 1.5).to(DEV)
    shift = S.hashed_uniform("ssa-b", (C,)).to(DEV)
    _lib.check(lib.ammc_scale_shift_act_f32(x.pix0(), *x.strides, _ptr(scale), _ptr(shift), r.pix0(), *r.strides,
                                            y_ref.pix0(), *y_ref.strides, 1, B, H, W, C, s), "ref")
    _lib.check(lib.ammc_scale_shift_act_s16_f32(x.pix0(), *x.strides, _ptr(scale), _ptr(shift), r.pix0(), *r.strides,
                                                y32.pix0(), y16.pix0(), *y16.strides, 1, B, H, W, C, s), "s16")
    assert torch.equal(y32.buf, y_ref.buf)
    back = torch.empty(B, C, H, W, device=DEV)
    _lib.check(lib.ammc_s16_to_nchw_f32(y16.pix0(), *y16.strides, B, C, H, W, _ptr(back), s), "decode")
    want = y_ref.interior().permute(0, 3, 1, 2)
    assert bool(((back - want).abs() <= 2.0 ** -21 * want.abs() + 2e-11).all())
    assert float(y16.buf[:, 0].abs().max()) == 0.0 and float(y16.buf[:, :, 0].abs().max()) == 0.0
    # without the fp32 copy
    y16b = mk()
    _lib.check(lib.ammc_scale_shift_act_s16_f32(x.pix0(), *x.strides, _ptr(scale), _ptr(shift), None, 0, 0, 0,
                                                None, y16b.pix0(), *y16b.strides, 0, B, H, W, C, s), "s16 only")
    _lib.check(lib.ammc_s16_to_nchw_f32(y16b.pix0(), *y16b.strides, B, C, H, W, _ptr(back), s), "decode")
    want = (x.interior() * scale + shift).permute(0, 3, 1, 2)
    assert float((back - want).abs().max()) <= 1e-6 * float(want.abs().max())


def _block_state(mod, tag):
    """deterministic parameters for a stand-alone block, BatchNorm affine as in `_mask_free_state` (no ReLU flips)"""
    sd = {}
    for k, v in mod.state_dict().items():
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[k] = torch.zeros_like(v)
        elif v.dim() == 1 and (k[:-len(leaf)] + "running_mean") in mod.state_dict():
            if leaf == "weight":
                sd[k] = 0.2 * torch.sign(S.hashed_uniform(f"{tag}.{k}", tuple(v.shape)))
            elif leaf == "bias":
                sd[k] = torch.full_like(v, 2.0)
            elif leaf == "running_var":
                sd[k] = S.hashed_uniform(f"{tag}.{k}", tuple(v.shape), 0.5, 1.5)
            else:
                sd[k] = S.hashed_uniform(f"{tag}.{k}", tuple(v.shape)) * 0.1
        else:
            fan = v[0].numel() if v.dim() > 1 else 1
            sd[k] = S.hashed_uniform(f"{tag}.{k}", tuple(v.shape)) * (1.5 / max(fan, 1)) ** 0.5
    return sd


@pytest.mark.parametrize("hw", [(32, 32), (27, 21)])
@pytest.mark.parametrize("kind", ["double_conv", "inconv", "down", "up", "bridge"])
def test_standalone_blocks_in_training_mode(kind, hw):
    """the reference's sub-modules are trainable on their own (models/unet.py:8-59, 956-965): outputs, parameter
    gradients, INPUT gradients and the BatchNorm running statistics of one training-mode call of each block against
    the oracle's autograd in float64 (mask-free BatchNorm affine: 1e-4 gates; `inconv`'s 12-channel input gets no
    gradient - it is data).  27x21: `down` floors, `up` pads the 26x20 ConvTranspose output on the right / bottom."""
    torch.manual_seed(0)
    mod = {"double_conv": lambda: A.double_conv(64, 128), "inconv": lambda: A.inconv(12, 64), "down": lambda: A.down(64, 128),
           "up": lambda: A.up(128, 64), "bridge": lambda: A.bridge(64)}[kind]()
    sd = _block_state(mod, kind)
    mod.load_state_dict(sd)
    mod = mod.to(DEV).train()
    B, (H, W) = 2, hw
    if kind == "up":
        ins = [S.hashed_uniform("blk-x1", (B, 128, H // 2, W // 2)), S.hashed_uniform("blk-x2", (B, 64, H, W))]
    elif kind == "bridge":
        ins = [S.hashed_uniform("blk-zx", (B, 64, H, W)), S.hashed_uniform("blk-zy", (B, 64, H, W))]
    else:
        ins = [S.hashed_uniform("blk-x", (B, 12 if kind == "inconv" else 64, H, W))]
    if kind == "down":
        # the block pools its INPUT, on the S16 image of it: a 24-bit-grid value keeps 22 bits there, and two window elements
        # that differ in the last two bits tie - the gradient then goes to the other one (2e-3 of the input gradient, the
        # gate this test used to carry).  On a 2^-16 grid every input is exact in S16: the routes are the fp64 oracle's.
        ins = [(t * 65536.0).round() / 65536.0 for t in ins]
    want_dx = kind != "inconv"
    xs = [t.to(DEV).requires_grad_(want_dx) for t in ins]
    outs = mod(*xs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    probes = [S.hashed_uniform(f"blk-r{i}", tuple(o.shape)).to(DEV) for i, o in enumerate(outs)]
    sum((o * r).sum() for o, r in zip(outs, probes)).backward()
    # oracle, float64
    pref = "bridge." if kind == "bridge" else "p."
    m = O.clone_state({pref + k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, requires_grad=True)
    xd = [t.double().requires_grad_(want_dx) for t in ins]
    if kind == "double_conv":
        w = (O.double_conv(m, "p.conv", xd[0], training=True),)
    elif kind == "inconv":
        w = (O.double_conv(m, "p.conv.conv", xd[0], training=True),)
    elif kind == "down":
        w = (O.down(m, "p", xd[0], training=True),)
    elif kind == "up":
        w = (O.up(m, "p", xd[0], xd[1], training=True),)
    else:
        w = O.bridge(m, xd[0], xd[1], training=True)
    sum((o * r.double().cpu()).sum() for o, r in zip(w, probes)).backward()
    for o, wo in zip(outs, w):
        assert rel_err(o.detach().cpu(), wo.detach()) <= 1e-5
    for name, p in mod.named_parameters():
        assert _l2rel(p.grad.cpu(), m[pref + name].grad) <= 1e-4, name
    if want_dx:
        for x, xw in zip(xs, xd):
            assert _l2rel(x.grad.cpu(), xw.grad) <= 1e-4
    nsd = mod.state_dict()
    for k, v in m.items():
        if not v.requires_grad and v.is_floating_point():
            assert rel_err(nsd[k[len(pref):]].cpu().double(), v) <= 1e-5, k


def test_memory_block_alone_in_training_mode():
    """`Quantize_topk`, `enc_quan_dec_topk`, `enc_quan_dec_res_topk` called on their own in .train(), as the reference's
    modules can be (models/unet.py:282-331, 379-387): lookups, EMA update of the buffers after the lookups, commit
    gradient + straight-through gradient.  Against the reference-recorded `ema.*` vectors of quantize_cases.npz
    (gathered rows bit-exact) and the oracle's autograd on the whole block."""
    from ammcnet_aaai2021_amd import unet as U
    d = np.load(os.path.join(GOLDEN, "quantize_cases.npz"))
    name = "quantize_cases"
    q = U.Quantize_topk(64, 256, k=2).to(DEV).train()
    q.embed.copy_(S.hashed_normal(f"{name}:ema:embed", (64, 256), 0.9))
    q.cluster_size.copy_(S.hashed_uniform(f"{name}:ema:cs", (256,), 0.5, 4.0))
    q.embed_avg.copy_(S.hashed_normal(f"{name}:ema:ea", (64, 256), 1.5))
    x = S.hashed_normal(f"{name}:ema:x", (2, 8, 8, 64), 0.8).to(DEV).requires_grad_(True)
    qk, diff, q1 = q(x)
    assert not qk.requires_grad and diff.requires_grad and q1.requires_grad
    diff.backward()
    assert np.array_equal(qk.cpu().numpy(), d["ema.qk"])
    assert rel_err(diff.detach().cpu(), d["ema.diff"]) <= 1e-5
    for key in ("embed", "cluster_size", "embed_avg"):
        assert rel_err(getattr(q, key).cpu(), d[f"ema.{key}"]) <= 1e-5, key
    assert rel_err(x.grad.cpu(), d["ema.dx"]) <= 1e-5
    # straight-through output: d(sum(w * quantize)) / dx = w
    x2 = x.detach().clone().requires_grad_(True)
    wgt = S.hashed_normal("st:w", (2, 8, 8, 64), 1.0).to(DEV)
    (q(x2)[2] * wgt).sum().backward()
    assert rel_err(x2.grad.cpu(), wgt.cpu()) <= 1e-6

    # the whole block (1x1 enc -> memory -> 1x1 dec [+ x]) against the oracle's autograd, both forms
    sd_all = S.make_twostream_state()
    pre = "rgb.vq_down3.quan."
    for residual in (False, True):
        mod = (U.enc_quan_dec_res_topk if residual else U.enc_quan_dec_topk)(512, 64, 256, k=2)
        tgt = mod.quan if residual else mod
        tgt.load_state_dict({k[len(pre):]: v for k, v in sd_all.items() if k.startswith(pre)})
        mod = mod.to(DEV).train()
        xin = S.hashed_normal(f"vqblock:{residual}", (2, 512, 8, 8), 0.7)
        xg = xin.to(DEV).requires_grad_(True)
        out, df, q_one = mod(xg)
        wo, wq = S.hashed_normal("vq:wo", tuple(out.shape), 1.0), S.hashed_normal("vq:wq", tuple(q_one.shape), 1.0)
        ((out * wo.to(DEV)).sum() + 3.0 * df.sum() + (q_one * wq.to(DEV)).sum()).backward()
        osd = O.clone_state({k: v.double() if v.is_floating_point() else v for k, v in sd_all.items()}, requires_grad=True)
        xo = xin.double().requires_grad_(True)
        wout, wdf, wq1, _ = O.vq_block(osd, "rgb.vq_down3", xo, 2, training=True)
        if not residual:
            wout = wout - xo
        ((wout * wo.double()).sum() + 3.0 * wdf.sum() + (wq1 * wq.double()).sum()).backward()
        assert rel_err(out.detach().cpu(), wout.detach()) <= 1e-5 and rel_err(df.detach().cpu(), wdf.detach()) <= 1e-5
        assert rel_err(q_one.detach().cpu(), wq1.detach()) <= 1e-5
        assert rel_err(xg.grad.cpu(), xo.grad) <= 1e-4, residual
        for leaf in ("enc.weight", "enc.bias", "dec.weight", "dec.bias"):
            got = dict(tgt.named_parameters())[leaf].grad
            assert _l2rel(got.cpu(), osd[pre + leaf].grad) <= 1e-4, (leaf, residual)
        for key in ("embed", "cluster_size", "embed_avg"):
            assert rel_err(getattr(tgt.quantize, key).cpu().double(), osd[pre + "quantize." + key].detach()) <= 1e-5, key


@pytest.mark.parametrize("train_precision", ["s16", "fp32"])
def test_twostream_train_step_256_vs_reference_vectors(train_precision):
    """the training benchmark's frame size (BASELINE.json configs[2]: 256x256; batch 2 here): loss, strided frames,
    commit terms, every gradient and the buffers updated inside forward against vectors recorded from the reference's own
    forward + autograd (tests/golden/twostream_256_b2_train.npz, written by make_golden.py).  This is the test that
    reaches the 256x256-level training instances end to end: `wgrad_tap3_s16<1,2,4,4>` / `<2,1,4,4>`, the 32-channel
    output-layer gradient, the halo-patch forward / input-gradient kernels with fp32 output at 1024 and 4096 tiles.
    Gates: 1e-4 on loss / frames / buffers (measured 0 / 5e-6 / 2e-7); gradients: the fp64 truth on this evaluation's
    branch, norms within max(1e-3, 2x the witnesses') and entries within twice the envelope of the reference's own recorded
    gradients (4096 entries per tensor + its lookups, `make_golden.py train_small`) and of the oracle's fp32 evaluation
    on the device (tests/truth.py, small_batch; measured: norms 5.5e-4 max, entries 4.7e-3 max / 1.7e-3 median against the
    reference's 3.9e-3 / 1.1e-3)."""
    d = np.load(os.path.join(GOLDEN, "twostream_256_b2_train.npz"))
    cfg = json.loads(str(d["cfg"]))
    assert (cfg["hw"], cfg["batch"], cfg["n_embed"]) == (256, 2, 256)
    sd = S.make_twostream_state()
    net = A.get_twostream((12, 6), (3, 2), 64, cfg["n_embed"], cfg["k"])
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    net.train_precision = train_precision
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(cfg["batch"], cfg["hw"], cfg["hw"], tag=cfg["tag"]))
    out = net(rgb_x, op_x)
    loss = O.generator_loss(out, rgb_t, op_t)
    loss.backward()
    assert net._train_engine.precision == train_precision
    st = int(d["out_step"])
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-4 * abs(float(d["loss"]))
    assert rel_err(out[0].detach().cpu()[..., ::st, ::st], d["rgb"]) <= 1e-4
    assert rel_err(out[1].detach().cpu()[..., ::st, ::st], d["op"]) <= 1e-4
    assert rel_err(out[2][0].detach().cpu(), d["rgb_diff"]) <= 1e-4 and rel_err(out[2][1].detach().cpu(), d["op_diff"]) <= 1e-4
    names = [n for n, _ in net.named_parameters()]
    _truth_gate(net, sd, S.make_clips(cfg["batch"], cfg["hw"], cfg["hw"], tag=cfg["tag"]), ref=_fixture_ref(d, names),
                what=f"256x256 batch 2, {train_precision}")
    nsd = net.state_dict()
    for key in d.files:
        if key.startswith("buf."):
            assert rel_err(nsd[key[4:]].cpu().double(), d[key].astype(np.float64)) <= 1e-4, key


def test_twostream_train_step_256_batch32_vs_reference_vectors():
    """The batch the training benchmark TIMES (BASELINE.json configs[2]: batch 32 at 256x256): 16x
    the tiles per launch of the batch-2 fixture - several rounds per persistent grid, the split decisions of the weight
    gradients at 32768 / 131072 pixels per channel block - against vectors recorded from the reference's own forward +
    autograd on the same 32 clips (tests/golden/twostream_256_b32_train.npz: loss, strided frames of clips 0 and 31,
    every gradient's norm and 64 samples, the buffers the forward updates; `make_golden.py train_b32`).  bench.py
    computes the same comparison from its timed model's first step (`train.parity`).

    Gates, from `tools/train_b32_debug.py` on one MI355X (three fp32-accurate evaluations of this step - the reference on
    the CPU, the exact-fp32 MFMA kernels, the split-fp16 kernels - and their mutual distances):
      loss / frames / commit / BatchNorm buffers   1e-4        measured 2.5e-7 / 7.5e-5 / 7e-8 / 5e-5
      memory lookups that pick another slot        <= 3 of the 2 x 32768 (1e-4 of a stream's rows): S16 re-routes ONE row of
                                                   the flow stream (a near-tie inside fp32 noise; the exact-fp32 kernels none),
                                                   which moves that stream's cluster_size / embed_avg / embed by 1-2e-4:
                                                   the codebook buffers are held to 1e-3 and the count is asserted
      gradients                                    against the fp64 truth, next test."""
    d = np.load(os.path.join(GOLDEN, "twostream_256_b32_train.npz"))
    cfg = json.loads(str(d["cfg"]))
    assert (cfg["hw"], cfg["batch"], cfg["n_embed"]) == (256, 32, 256)
    net = A.get_twostream((12, 6), (3, 2), 64, cfg["n_embed"], cfg["k"])
    net.load_state_dict(S.make_twostream_state())
    net = net.to(DEV).train()
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(cfg["batch"], cfg["hw"], cfg["hw"], tag=cfg["tag"]))
    out = net(rgb_x, op_x)
    loss = O.generator_loss(out, rgb_t, op_t)
    loss.backward()
    st, rows = int(d["out_step"]), [int(r) for r in d["rows"]]
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-4 * abs(float(d["loss"]))
    assert rel_err(out[0].detach().cpu()[rows][..., ::st, ::st], d["rgb"]) <= 1e-4
    assert rel_err(out[1].detach().cpu()[rows][..., ::st, ::st], d["op"]) <= 1e-4
    assert rel_err(out[2][0].detach().cpu(), d["rgb_diff"]) <= 1e-4 and rel_err(out[2][1].detach().cpu(), d["op_diff"]) <= 1e-4
    # (gradients: `test_batch32_gradients_against_the_fp64_truth` below - two fp32-accurate evaluations cannot gate each
    # other entry by entry, their distance is set by which way one or two near-tie memory lookups fall)
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    nsd = net.state_dict()
    for key in d.files:
        if not key.startswith("buf."):
            continue
        got, want = nsd[key[4:]].cpu().double(), d[key].astype(np.float64)
        if ".quantize." in key:
            assert rel_err(got, want) <= 1e-3, key
            if key.endswith("cluster_size"):          # EMA decay 0.99: a re-routed row moves 0.01 out of one slot, into another
                moved = float((got - torch.as_tensor(want)).abs().sum()) / 0.01 / 2
                assert moved <= 3.01, (key, moved)
        else:
            assert rel_err(got, want) <= 1e-4, key


def _dense(g: torch.Tensor, n: int = 4096) -> torch.Tensor:
    """the sample positions of `gs4k.*` / `gs64*.*` (tests/golden/make_golden.py, make_fp64_truth.py)"""
    return g.flatten()[:: max(1, g.numel() // n)][:n].contiguous()


def test_batch32_gradients_against_the_fp64_truth():
    """Round-4 review, weak #1: the gradient gates of the TIMED training batch (32 clips at 256x256) were set from the
    distances between fp32-accurate evaluations; nobody had shown that the HIP gradients are no farther from the TRUTH
    than the reference's own fp32 gradients are.  The truth: the oracle in FLOAT64 (tests/golden/make_fp64_truth.py -
    on the GPU box's host cores, 149 s, committed as twostream_256_b32_train_fp64.npz; here re-evaluated on the device,
    6 s, which agrees with the host file to 6e-12).

    What the comparison has to respect (tools/flip_count.py, tools/grad_truth.py): the step is piecewise
    smooth, and its one violent discontinuity is the memory lookup.  ONE of the 2 x 32768 top-2 lookups falling the
    other way - two slots whose fp64 distances differ by less than fp32 resolution - moves the bottleneck by 5e-3 and
    every gradient downstream of it by ~1e-2, for ANY fp32 evaluation: the reference's own gradients are 3.6e-3 (median)
    / 3e-2 (max) from the unconstrained fp64 evaluation, the HIP ones 5e-3 / 3.5e-2, the exact-fp32 HIP ones 3.5e-3 /
    2.6e-2, depending only on whose near-ties happened to fall like fp64's.  So every evaluation is compared with the
    truth ON ITS OWN BRANCH: the oracle in fp64 taking the lookups that evaluation made (`force_idx`, test
    instrumentation of oracle.quantize_topk; the reference's lookups are in its fixture).  What is left is arithmetic
    plus the ReLU masks / pool routes that flip inside fp32 noise (10-30 per 1e8 activations and layer for all three).

    Asserted:
      * the lookups: at most 3 of a stream's 32768 differ from the unconstrained fp64 evaluation's (measured: 1 and 1; the
        reference: 0 and 1; the exact-fp32 kernels: 1 and 0);
      * SURVEY 8(d)'s gate itself - gradient norm of every tensor within 1e-3 of the truth (measured 5.3e-4 max, the
        reference 4.0e-4; round 6, with the engine's recorded max-pool routes forced as well - tests/truth.py: 4.7e-4);
      * entry by entry (L2 over the whole tensor): e_hip <= max(1e-3, 2 e_ref) for every tensor and the median over the
        tensors of e_hip / e_ref <= 1.5, e_ref = the reference's recorded 4096 entries per tensor against the truth on
        the reference's branch.  Measured: median ratio 1.29, max 1.82 (a 64-entry BatchNorm weight; the ratio of two
        errors that are each a handful of flipped masks has that spread).  The split-fp16 operands carry 22 bits where
        fp32 storage carries 24: its forward noise per layer is 1.1-1.25x oneDNN's (tools/flip_count.py), its flips
        accordingly."""
    d = np.load(os.path.join(GOLDEN, "twostream_256_b32_train.npz"))
    t64 = np.load(os.path.join(GOLDEN, "twostream_256_b32_train_fp64.npz"))
    cfg = json.loads(str(d["cfg"]))
    sys.path.insert(0, GOLDEN)
    from make_fp64_truth import oracle_step
    sd = S.make_twostream_state()
    clips = S.make_clips(cfg["batch"], cfg["hw"], cfg["hw"], tag=cfg["tag"])
    net = A.get_twostream((12, 6), (3, 2), 64, cfg["n_embed"], cfg["k"])
    net.load_state_dict(sd)
    net = net.to(DEV).train()
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in clips)
    out = net(rgb_x, op_x)
    loss = O.generator_loss(out, rgb_t, op_t)
    loss.backward()
    torch.cuda.synchronize()
    branch = T.hip_lookups(net)                    # lookups + (round 6) the routes of the max-pools
    idx_hip = {p: branch[p] for p in ("rgb", "op")}
    g_hip = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    loss_hip = float(loss.detach())
    del net, out, loss
    torch.cuda.empty_cache()
    # the unconstrained truth (host file) and the device re-evaluation of it: the same numbers
    loss64, g64, idx64 = oracle_step(sd, clips, torch.float64, DEV, want_idx=True)
    assert abs(loss64 - float(t64["loss64"])) <= 1e-12 * loss64
    assert max(_l2rel(_dense(g64[n]).cpu(), torch.as_tensor(t64[f"gs64.{n}"])) for n in g64) <= 1e-9
    assert abs(loss_hip - loss64) <= 1e-6 * loss64
    # which way the near-ties fell
    for p in ("rgb", "op"):
        rows = (idx_hip[p] != idx64[p]).any(dim=1).nonzero().flatten()
        assert rows.numel() <= 3, (p, rows.numel())
    del g64
    torch.cuda.empty_cache()
    # the truth on the branch the HIP evaluation took, the reference's own error from its recorded vectors on ITS branch:
    # the per-tensor gates of tests/truth.py (norms 1e-3; entries max(1e-3, 2 e_ref); median ratio 1.5) - what bench.py's
    # `train.parity.vs_fp64` computes from the timed model's first step
    names = list(g_hip)
    v = T.same_branch_verdict(T.g_stepper(sd, clips), g_hip, branch, DEV, "timed_batch", ref=_fixture_ref(d, names),
                              what="the timed training batch: 32 clips at 256x256")
    T.assert_ok(v)
    assert v["grad_norm_rel"]["max"] <= 1e-3 and v["ratio_over_reference"]["median"] <= 1.5
