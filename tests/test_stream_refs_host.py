"""tests/stream_refs.py is right: every fp64 reference against torch's own operator or autograd in float64, the EMA and
the commit gradient against the oracle's `quantize_topk` / `codebook_ema_update` in double - and the grid inputs of
tests/stream_cases.py make the reference results exactly representable in fp32 (what makes the GPU test's bit equality
fair).  No device."""
import pytest
import torch
import torch.nn.functional as F

from ammcnet_aaai2021_amd import synthetic as S
from oracle import ammc_oracle as O

import stream_cases as K
import stream_refs as R

TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = R.d(a), R.d(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _nchw(t):
    return R.d(t).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("relu", [0, 1])
def test_batchnorm_group_against_torch(relu):
    b, h, w, c = 3, 5, 7, 8
    x = S.hashed_normal("hbn-x", (b, h, w, c)).double() + 0.3
    dy = S.hashed_normal("hbn-g", (b, h, w, c)).double()
    gamma, beta = S.hashed_uniform("hbn-ga", (c,), -1.5, 1.5).double(), S.hashed_normal("hbn-be", (c,), 0.5).double()
    rm, rv = S.hashed_normal("hbn-rm", (c,)).double(), S.hashed_uniform("hbn-rv", (c,), 0.5, 2.0).double()
    s, ss = R.chan_sums(x)
    fin = R.bn_finalize(s, ss, b * h * w, gamma, beta, 1e-5, 0.1, rm, rv)
    xt = _nchw(x).requires_grad_(True)
    trm, trv = rm.clone(), rv.clone()
    y = F.batch_norm(xt, trm, trv, gamma, beta, True, 0.1, 1e-5)
    out = F.relu(y) if relu else y
    out.backward(_nchw(dy))
    _close(fin["mean"], _nchw(x).mean((0, 2, 3)))
    _close(fin["var"], _nchw(x).var((0, 2, 3), unbiased=False))
    _close(fin["running_mean"], trm)
    _close(fin["running_var"], trv)
    _close((x * fin["scale"] + fin["shift"]), y.detach().permute(0, 2, 3, 1))              # the folded form is the forward
    sg, sgx = R.bn_bwd_sums(x, dy, fin["mean"], fin["invstd"], fin["scale"], fin["shift"], relu)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y2 = F.batch_norm(_nchw(x), None, None, gt, bt, True, 0.1, 1e-5)
    (F.relu(y2) if relu else y2).backward(_nchw(dy))
    _close(sg, bt.grad, 1e-11)
    _close(sgx, gt.grad, 1e-11)
    dc = R.bn_bwd_apply(x, dy, fin["mean"], fin["invstd"], fin["scale"], fin["shift"], sg, sgx, relu)
    _close(dc, xt.grad.permute(0, 2, 3, 1), 1e-11)
    if relu:
        assert 0.2 < float((R.bn_masked_grad(x, dy, fin["scale"], fin["shift"], 1) == 0).double().mean()) < 0.8


def test_bn_fold_is_eval_batchnorm():
    c = 12
    gamma, beta = S.hashed_normal("hf-g", (c,)).double(), S.hashed_normal("hf-b", (c,)).double()
    mean, var = S.hashed_normal("hf-m", (c,)).double(), S.hashed_uniform("hf-v", (c,), 0.1, 2.0).double()
    x = S.hashed_normal("hf-x", (2, c, 3, 3)).double()
    scale, shift = R.bn_fold(gamma, beta, mean, var, 1e-5)
    _close(x * scale.view(1, c, 1, 1) + shift.view(1, c, 1, 1), F.batch_norm(x, mean, var, gamma, beta, False, 0.1, 1e-5))


@pytest.mark.parametrize("fh,fw", [(4, 6), (5, 7), (2, 3), (3, 2), (6, 6)])
def test_maxpool_forward_and_backward_against_autograd(fh, fw):
    b, c = 2, 4
    x, dp, add = K.pool_bwd_case("cont", b, fh, fw, c)
    xt = _nchw(x).requires_grad_(True)
    y = F.max_pool2d(xt, 2)
    y.backward(_nchw(dp))
    _close(R.maxpool2x2(x), y.detach().permute(0, 2, 3, 1), 0.0)
    _close(R.maxpool2x2_bwd(x, dp), xt.grad.permute(0, 2, 3, 1), 0.0)
    _close(R.maxpool2x2_bwd(x, dp, add), xt.grad.permute(0, 2, 3, 1) + add.double(), 0.0)


def test_maxpool_backward_tie_goes_to_the_first_maximum():
    x = torch.tensor([[1.0, 3.0, 0.0], [3.0, 3.0, 0.0], [9.0, 9.0, 9.0]]).view(1, 3, 3, 1)
    dp = torch.tensor([5.0]).view(1, 1, 1, 1)
    want = torch.tensor([[0.0, 5.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]).view(1, 3, 3, 1)
    _close(R.maxpool2x2_bwd(x, dp), want, 0.0)
    assert int(R.maxpool2x2_arg(torch.full((1, 2, 2, 1), 2.0))) == 0
    add = torch.arange(9.0).view(1, 3, 3, 1)
    _close(R.maxpool2x2_bwd(x, dp, add), want + add, 0.0)                   # the odd row / column gets `add` alone


def test_activations_against_autograd():
    b, c, h, w = 2, 3, 5, 7
    pre = S.hashed_normal("ha-p", (b, c, h, w)).double().requires_grad_(True)
    dout = S.hashed_normal("ha-d", (b, c, h, w)).double()
    out = torch.tanh(pre)
    out.backward(dout)
    y = R.tanh_bwd_nhwc(dout, out.detach(), 8)
    _close(y[..., :c], pre.grad.permute(0, 2, 3, 1))
    assert float(y[..., c:].abs().max()) == 0.0
    for slope in (0.1, 0.0):
        p = S.hashed_normal("ha-l", (b, h, w, 8)).double()
        p[0, 0, 0, :2] = torch.tensor([0.0, -0.0])
        pt = p.clone().requires_grad_(True)
        o = F.leaky_relu(pt, slope)
        g = S.hashed_normal("ha-lg", (b, h, w, 8)).double()
        o.backward(g)
        _close(R.lrelu(p, slope), o.detach(), 0.0)
        if slope > 0:                                      # sign(y) == sign(pre-activation): the backward reads the output
            _close(R.lrelu_bwd(o.detach(), g, slope), pt.grad, 0.0)
        else:                                              # slope 0: y = 0 wherever pre <= 0, the same mask
            _close(R.lrelu_bwd(o.detach(), g, slope), torch.where(p > 0, g, torch.zeros_like(g)), 0.0)


@pytest.mark.parametrize("h,w", K.UP_SHAPES)
@pytest.mark.parametrize("premul", [1.0, 5.0, 20.0])
def test_upsample4_against_interpolate(h, w, premul):
    x = S.hashed_normal(f"hu-{h}-{w}", (2, h, w, 2)).double()
    want = F.interpolate(_nchw(x) * premul, scale_factor=4, mode="bilinear", align_corners=False)
    _close(R.upsample4(x, premul), want)


def test_flownet_prep_and_layouts():
    x = K.prep_case("cont", 2, 5, 6).double()
    b = x.shape[0]
    mean = x.contiguous().view(b, 3, -1).mean(dim=-1).view(b, 3, 1, 1, 1)                  # models.py:16-18 as the oracle has it
    y = (x - mean) / 255.0
    want = torch.cat((y[:, :, 0], y[:, :, 1]), dim=1).permute(0, 2, 3, 1)
    _close(R.flownet_prep(x, 255.0), want)
    t = S.hashed_normal("hl", (2, 3, 4, 5)).double()
    n = R.nchw_to_nhwc(t, 8)
    _close(n[..., :3], t.permute(0, 2, 3, 1), 0.0)
    assert float(n[..., 3:].abs().max()) == 0.0
    _close(R.nhwc_to_nchw(n[..., :3]), t, 0.0)
    e = S.hashed_normal("he", (6, 9)).double()
    e_md, norm = R.pack_codebook(e)
    _close(e_md, e.t(), 0.0)
    _close(norm, e.pow(2).sum(0))


def test_ema_and_commit_gradient_against_the_oracle():
    """`quantize_topk` + `codebook_ema_update` (the oracle's restatement of Quantize_topk, unet.py:282-311) in double"""
    bb, h, w, dim, m, k = 2, 3, 5, 8, 11, 2
    z = S.hashed_normal("ho-z", (bb, h, w, dim)).double().requires_grad_(True)
    sd = {"q.embed": S.hashed_normal("ho-e", (dim, m)).double(), "q.cluster_size": S.hashed_uniform("ho-c", (m,), 0.5, 4.0).double(),
          "q.embed_avg": S.hashed_normal("ho-a", (dim, m)).double()}
    embed0, cs0, ea0 = (sd[n].clone() for n in ("q.embed", "q.cluster_size", "q.embed_avg"))
    qk, diff, idxk, idx1, flatten, q1 = O.quantize_topk(z, sd["q.embed"], k)
    q_one = z + (q1 - z).detach()
    ddiff = torch.tensor([0.37], dtype=torch.float64)
    dq = S.hashed_normal("ho-q", (bb, h, w, dim)).double()
    (diff * ddiff[0] + (q_one * dq).sum()).backward()
    idx = idxk.reshape(-1, k)
    assert torch.equal(idx[:, 0], idx1)
    e_md = embed0.t().contiguous()
    zf = z.detach().reshape(-1, dim)
    _close(R.commit_bwd(zf, e_md, idx, ddiff, dq.reshape(-1, dim)), z.grad.reshape(-1, dim))
    _close(R.commit_bwd(zf, e_md, idx, None, dq.reshape(-1, dim)), dq.reshape(-1, dim), 0.0)
    _close(R.commit_bwd(zf, e_md, idx, None, None), torch.zeros(bb * h * w, dim), 0.0)
    O.codebook_ema_update(sd, "q", flatten, idx1)
    counts, sums = R.ema_counts_sums(zf, idx, m)
    assert float(counts.sum()) == bb * h * w
    cs, ea, embed = R.ema_update(cs0, ea0, counts, sums, O.VQ_DECAY, 1 - O.VQ_DECAY, O.VQ_EPS)
    _close(cs, sd["q.cluster_size"])
    _close(ea, sd["q.embed_avg"])
    _close(embed, sd["q.embed"])


# ---- the grid inputs: reference results exactly representable in fp32 ------------------------------------------------

@pytest.mark.parametrize("shape", K.CHAN_SHAPES)
def test_grid_reductions_are_exact_in_fp32(shape):
    m = shape[0] * shape[1] * shape[2]
    for relu in (0, 1):
        x, dy, mean, invstd, scale, shift = K.bn_bwd_case("grid", shape, relu)
        s, ss = R.chan_sums(x)
        sg, sgx = R.bn_bwd_sums(x, dy, mean, invstd, scale, shift, relu)
        assert all(R.fits_f32(t) for t in (s, ss, sg, sgx))
        # every intermediate of the kernel too: x^2, xhat, pre, g xhat, and every partial sum (bounded by sum |terms| < 2^24 units)
        xh = (x.double() - mean.double()) * invstd.double()
        assert R.fits_f32(x.double() ** 2) and R.fits_f32(xh) and R.fits_f32(x.double() * scale.double() + shift.double())
        assert float((dy.double() * xh).abs().sum((0, 1, 2)).max()) * 128 < 2 ** 24 and float((x.double() ** 2).sum((0, 1, 2)).max()) * 64 < 2 ** 24
        if relu:
            pre = x.double() * scale.double() + shift.double()
            assert float(pre[0, 0, 0, 0]) == 0.0 and float(dy[0, 0, 0, 0]) != 0.0
        if K.is_pow2(m):
            sa, sb = K.bn_apply_sums("grid", shape)
            assert R.fits_f32(R.bn_bwd_apply(x, dy, mean, invstd, scale, shift, sa, sb, relu))
            fin = R.bn_finalize(s, ss, m, scale, shift, 1e-5, 0.5, mean, invstd)
            assert R.fits_f32(fin["mean"]) and R.fits_f32(fin["running_mean"])


def test_grid_elementwise_cases_are_exact_in_fp32():
    for fh, fw in K.POOL_BWD_SIZES:
        x, dp, add = K.pool_bwd_case("grid", 2, fh, fw, 4)
        assert R.fits_f32(R.maxpool2x2_bwd(x, dp, add))
        arg = R.maxpool2x2_arg(x)[..., 0].reshape(-1)
        win = R._windows(x.double())[..., 0].reshape(-1, 4)
        for n in range(arg.numel()):                                       # the planted tie: the first of the pair wins
            pair = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))[n % 6]
            assert int(arg[n]) == pair[0] and float(win[n, pair[1]]) == 2.0
    out, dout = R.grid("hg-o", (2, 3, 5, 7)), R.grid("hg-d", (2, 3, 5, 7))
    assert R.fits_f32(R.tanh_bwd_nhwc(dout, out, 4))
    for n, dim, k in K.COMMIT_CASES:
        z, e, idx, ddiff, dq = K.commit_case("grid", n, dim, k)
        assert R.fits_f32(R.commit_bwd(z, e, idx, None, dq))
        if K.is_pow2(n * dim):
            assert R.fits_f32(R.commit_bwd(z, e, idx, ddiff, dq))
    for b, h, w in K.PREP_SHAPES:
        x = K.prep_case("grid", b, h, w)
        assert float(x.min()) >= 0 and R.fits_f32(R.flownet_prep(x, 256.0))
        assert float((x.double().view(b, 3, -1).sum(-1) % (2 * h * w)).abs().max()) == 0.0
    for h, w in K.UP_SHAPES:
        for premul in (1.0, 5.0, 20.0):
            assert R.fits_f32(R.upsample4(R.grid(f"hg-u{h}{w}", (2, h, w, 2)), premul))


@pytest.mark.parametrize("n,dim,m,k,pattern", K.EMA_CASES)
def test_grid_ema_is_exact_and_the_patterns_do_what_they_say(n, dim, m, k, pattern):
    x, idx, cs, ea, decay = K.ema_case("grid", n, dim, m, k, pattern)
    counts, sums = R.ema_counts_sums(x, idx, m)
    cs2, ea2, _ = R.ema_update(cs, ea, counts, sums, decay, 1 - decay, 1e-5)
    assert R.fits_f32(sums) and R.fits_f32(cs2) and R.fits_f32(ea2)
    assert int(idx.min()) >= 0 and int(idx.max()) < m and float(counts.sum()) == n
    chunk = K.ema_chunk(n)
    if pattern == "one":
        assert float(counts[m // 2]) == n
    if pattern == "half":
        assert float(counts[1::2].sum()) == 0
    if pattern == "last":
        rows = torch.nonzero(idx[:, 0] == m - 1).reshape(-1)
        assert rows.numel() > 0 and bool(((rows % chunk) >= chunk - 64).all())
