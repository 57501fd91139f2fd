"""The three concurrency switches that are ON by default - the eval forward's two network streams on two HIP streams
(engine.EVAL_LANES, AMMC_EVAL_LANES), the training step's rgb / flow halves on two HIP streams (train.TWO_STREAMS,
AMMC_TWO_STREAMS) and the adversarial iteration's D update on a second HIP stream (harness.GAN_OVERLAP,
AMMC_GAN_OVERLAP) - against the same launches on ONE stream.  Same kernels, disjoint buffers: the forward outputs, the
losses and the buffers must be BIT-identical; gradients that end in fp32 atomics are held to the run-to-run noise of one
configuration."""
import numpy as np
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import engine as E, synthetic as S, train as T
from ammcnet_aaai2021_amd import harness as Hn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _eval_once(lanes: bool, hw, batch, n_embed):
    keep = E.EVAL_LANES
    E.EVAL_LANES = lanes
    try:
        net = A.get_twostream((12, 6), (3, 2), 64, n_embed, 2)
        net.load_state_dict(S.make_twostream_state(n_embed=n_embed))
        net = net.to(DEV).eval()
        rgb_x, op_x, _, _ = (t.to(DEV) for t in S.make_clips(batch, hw, hw, tag="lanes"))
        with torch.no_grad():
            outs = [net(rgb_x, op_x) for _ in range(2)]          # twice: the second forward re-uses every workspace buffer
        torch.cuda.synchronize()
        used = getattr(net._engine, "_lanes", None) is not None
        return outs, used
    finally:
        E.EVAL_LANES = keep


@pytest.mark.parametrize("hw,batch,n_embed", [(64, 2, 256), (256, 4, 2000)])
def test_eval_lanes_on_equals_off(hw, batch, n_embed):
    on, used_on = _eval_once(True, hw, batch, n_embed)
    off, used_off = _eval_once(False, hw, batch, n_embed)
    assert used_on and not used_off                               # the switch did switch
    for o in (on, off):                                           # and a forward is repeatable within a configuration
        assert torch.equal(o[0][0], o[1][0]) and torch.equal(o[0][1], o[1][1])
    a, b = on[1], off[1]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                      # predicted frames, both streams
    assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])          # commit values
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])          # quantised maps


def _train_once(two: bool, hw, batch):
    keep = T.TWO_STREAMS
    T.TWO_STREAMS = two
    try:
        net = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
        net.load_state_dict(S.make_twostream_state())
        net = net.to(DEV).train()
        rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(batch, hw, hw, tag="lanes-train"))
        out = net(rgb_x, op_x)
        loss = Hn.generator_loss(out, rgb_t, op_t)
        loss.backward()
        torch.cuda.synchronize()
        side = net._train_engine._last["ops"].side is not None
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
        bufs = {k: v.detach().clone() for k, v in net.state_dict().items() if k not in grads}
        return (out[0].detach().clone(), out[1].detach().clone(), float(loss.detach())), grads, bufs, side
    finally:
        T.TWO_STREAMS = keep


@pytest.mark.parametrize("hw,batch", [(64, 2), (256, 2)])
def test_training_two_streams_on_equals_off(hw, batch):
    on = _train_once(True, hw, batch)
    off = _train_once(False, hw, batch)
    off2 = _train_once(False, hw, batch)
    assert on[3] and not off[3]
    assert torch.equal(on[0][0], off[0][0]) and torch.equal(on[0][1], off[0][1]) and on[0][2] == off[0][2]
    for k in off[2]:                                              # BatchNorm statistics, step counters, EMA codebook
        assert torch.equal(on[2][k], off[2][k]), k
    for n in off[1]:
        # (some weight gradients are accumulated with fp32 atomics: their run-to-run noise on ONE stream is the gate)
        noise = float((off[1][n] - off2[1][n]).abs().max())
        assert float((on[1][n] - off[1][n]).abs().max()) <= max(4.0 * noise, 0.0) + 1e-7 * float(off[1][n].abs().max()), n


def _gan_once(case, overlap: bool, monkeypatch, hw=64, batch=2):
    """one adversarial iteration (lr 0: both steps run, the gradients stay readable) with the D lane on / off ->
    (g_loss, d_loss, predicted frames, gradients of G and D, times the side stream was requested)"""
    requested = []
    real = Hn._gan_side_stream
    monkeypatch.setattr(Hn, "GAN_OVERLAP", overlap)
    monkeypatch.setattr(Hn, "_gan_side_stream", lambda *a, **k: (requested.append(a), real(*a, **k))[1])
    try:
        rgb_x, op_x, rgb_t, op_t = S.make_clips(batch, hw, hw, tag=f"lanes-gan-{case}")
        rgb = torch.cat([rgb_x.view(batch, 4, 3, hw, hw), rgb_t[:, None]], 1).to(DEV)
        op = torch.cat([op_x.view(batch, 3, 2, hw, hw), op_t[:, None]], 1).to(DEV)
        if case == "joint":
            G = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
            G.load_state_dict(S.make_twostream_state())
        else:
            G = A.get_unet_vq_topk_res(12, 3, 64, 256, 2)
            G.load_state_dict({k[4:]: v for k, v in S.make_twostream_state().items() if k.startswith("rgb.")})
        D = A.PixelDiscriminator(3, [128, 256, 512, 512])
        D.load_state_dict(S.make_discriminator_state())
        F2 = A.FlowNet2SD()
        F2.load_state_dict(S.make_flownet2sd_state())
        G, D, F2 = G.to(DEV).train(), D.to(DEV).train(), F2.to(DEV).eval()
        opt_g, opt_d = torch.optim.SGD(G.parameters(), lr=0.0), torch.optim.SGD(D.parameters(), lr=0.0)
        out = {}
        if case == "joint":
            gl, dl = Hn.train_step_gan(G, D, opt_g, opt_d, rgb, op, Hn.flownet_flow_fn(F2), outputs=out)
            preds = (out["rgb"].clone(), out["op"].clone())
        else:
            gl, dl = Hn.train_step_single_gan(G, D, opt_g, opt_d, rgb, Hn.flownet_flow_fn(F2), outputs=out)
            preds = (out["pred"].clone(),)
        torch.cuda.synchronize()
        grads = {"G." + n: p.grad.detach().clone() for n, p in G.named_parameters()}
        grads.update({"D." + n: p.grad.detach().clone() for n, p in D.named_parameters()})
        return gl.clone(), dl.clone(), preds, grads, len(requested)
    finally:
        monkeypatch.undo()


@pytest.mark.parametrize("case", ["joint", "rgb"])
def test_gan_overlap_on_equals_off(case, monkeypatch):
    """`train_step_gan` (twostream + PixelDiscriminator(3) + FlowNet2-SD) and `train_step_single_gan` (the rgb stage with
    its flow term) at 64 x 64, the smallest frame FlowNet2-SD takes: every fork / join of the D lane exists"""
    on = _gan_once(case, True, monkeypatch)
    off = _gan_once(case, False, monkeypatch)
    off2 = _gan_once(case, False, monkeypatch)
    assert on[4] == 1 and off[4] == 0 and off2[4] == 0           # the switch did switch
    print(f"{case}: g_loss on/off {float(on[0])!r} {float(off[0])!r}  d_loss on/off {float(on[1])!r} {float(off[1])!r}")
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert len(on[2]) == len(off[2]) and all(torch.equal(a, b) for a, b in zip(on[2], off[2]))
    assert sorted(on[3]) == sorted(off[3])
    for n in off[3]:
        # (some weight gradients are accumulated with fp32 atomics: their run-to-run noise on ONE stream is the gate)
        noise = float((off[3][n] - off2[3][n]).abs().max())
        assert float((on[3][n] - off[3][n]).abs().max()) <= max(4.0 * noise, 0.0) + 1e-7 * float(off[3][n].abs().max()), n
