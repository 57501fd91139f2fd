"""Plain fp64 references of the training engine's streaming kernels (csrc/train_kernels.hip, flownet.hip, layout_pool.hip).

One small function per operation, torch float64 on CPU tensors, written with indexing, `where` and sums only (no
torch.nn.functional): tests/test_stream_refs_host.py checks each against torch's own operator or autograd, and
tests/test_gpu_stream_kernels.py checks the HIP kernels against these.  Activations are NHWC [B, H, W, C] unless a
docstring says NCHW; semantics are those of the kernel comments and include/ammc_hip.h."""
import torch

F64 = torch.float64


def d(t):
    return torch.as_tensor(t).detach().to("cpu", F64)


def grid(tag, shape, lo=-8, hi=8, den=8.0):
    """hashed integers in [lo, hi] divided by `den`, fp32: every value a small dyadic rational"""
    from ammcnet_aaai2021_amd import synthetic as S
    n = hi - lo + 1
    return ((torch.floor(S.hashed_uniform(tag, shape, 0.0, float(n)).double()).clamp(max=n - 1) + lo) / den).float()


def fits_f32(t) -> bool:
    """every value of the fp64 tensor is exactly representable in fp32: the condition under which a grid case may ask for
    bit equality"""
    t = d(t)
    return bool(torch.equal(t.float().double(), t))


# ---- BatchNorm -------------------------------------------------------------------------------------------------------

def chan_sums(x):
    """per-channel sum x, sum x^2 over every pixel"""
    x = d(x)
    return x.sum((0, 1, 2)), (x * x).sum((0, 1, 2))


def bn_finalize(s, ss, count, gamma, beta, eps, momentum, running_mean, running_var):
    """training-mode BatchNorm2d from the sums: mean, biased var clamped at 0, invstd, folded scale / shift, running
    statistics (the unbiased variance)"""
    s, ss, gamma, beta = d(s), d(ss), d(gamma), d(beta)
    mean = s / count
    var = (ss / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": shift,
            "running_mean": (1.0 - momentum) * d(running_mean) + momentum * mean,
            "running_var": (1.0 - momentum) * d(running_var) + momentum * unbiased}


def bn_masked_grad(x, dy, scale, shift, relu):
    """g = dy [pre > 0], pre = x scale + shift (the forward's own expression); relu = 0: g = dy"""
    x, dy = d(x), d(dy)
    if not relu:
        return dy.clone()
    pre = x * d(scale) + d(shift)
    return torch.where(pre > 0, dy, torch.zeros_like(dy))


def bn_bwd_sums(x, dy, mean, invstd, scale, shift, relu):
    """sum g, sum g xhat per channel; xhat = (x - mean) invstd"""
    g = bn_masked_grad(x, dy, scale, shift, relu)
    xhat = (d(x) - d(mean)) * d(invstd)
    return g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))


def bn_bwd_apply(x, dy, mean, invstd, scale, shift, sum_g, sum_gx, relu):
    """dc = scale (g - sum_g / M - xhat sum_gx / M)"""
    x = d(x)
    m = x.shape[0] * x.shape[1] * x.shape[2]
    g = bn_masked_grad(x, dy, scale, shift, relu)
    xhat = (x - d(mean)) * d(invstd)
    return d(scale) * (g - d(sum_g) / m - xhat * d(sum_gx) / m)


def bn_fold(gamma, beta, mean, var, eps):
    scale = d(gamma) / torch.sqrt(d(var) + eps)
    return scale, d(beta) - d(mean) * scale


# ---- max-pool 2x2 ----------------------------------------------------------------------------------------------------

def _windows(x):
    """[B, h, w, 4, C]: the four elements of every 2x2 window in row-major order (floor semantics)"""
    b, fh, fw, c = x.shape
    h, w = fh // 2, fw // 2
    v = x[:, :2 * h, :2 * w]
    return torch.stack([v[:, 0::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 0::2], v[:, 1::2, 1::2]], 3)


def maxpool2x2(x):
    win = _windows(d(x))
    return torch.maximum(torch.maximum(win[:, :, :, 0], win[:, :, :, 1]), torch.maximum(win[:, :, :, 2], win[:, :, :, 3]))


def maxpool2x2_arg(x):
    """window position (0..3, row-major) of the FIRST maximum"""
    win = _windows(d(x))
    best, arg = win[:, :, :, 0].clone(), torch.zeros_like(win[:, :, :, 0], dtype=torch.int64)
    for j in range(1, 4):
        better = win[:, :, :, j] > best
        best = torch.where(better, win[:, :, :, j], best)
        arg = torch.where(better, torch.full_like(arg, j), arg)
    return arg


def maxpool2x2_bwd(x, dp, add=None):
    """dx = add + dp routed to the first maximum of its window; a last odd row / column gets `add` (or zero) alone"""
    x, dp = d(x), d(dp)
    b, fh, fw, c = x.shape
    h, w = fh // 2, fw // 2
    arg = maxpool2x2_arg(x)
    dx = torch.zeros_like(x)
    for j in range(4):
        dx[:, (j >> 1):2 * h:2, (j & 1):2 * w:2] = torch.where(arg == j, dp, torch.zeros_like(dp))
    return dx + d(add) if add is not None else dx


def unpool2x2(dp, arg, fh, fw):
    """MaxPool2d(2) backward from recorded window positions: dp [B, h, w, C] routed to position arg (0..3, row-major) of its
    window in an fh x fw tensor; a last odd row / column is in no window and stays zero"""
    dp, arg = d(dp), torch.as_tensor(arg).to("cpu", torch.int64)
    b, h, w, c = dp.shape
    dx = torch.zeros(b, fh, fw, c, dtype=F64)
    for j in range(4):
        dx[:, (j >> 1):2 * h:2, (j & 1):2 * w:2] = torch.where(arg == j, dp, torch.zeros_like(dp))
    return dx


# ---- activations -----------------------------------------------------------------------------------------------------

def scale_shift_act(x, scale, shift, res=None, relu=0):
    """y = act(x scale + shift) + res (the apply pass of a BatchNorm unit on its folded scale / shift)"""
    y = d(x) * d(scale) + d(shift)
    if relu:
        y = y.clamp_min(0.0)
    return y + d(res) if res is not None else y


def tanh_bwd_nhwc(dout_nchw, out_nchw, cp):
    """dout (1 - out^2), NCHW -> NHWC with channels [C, cp) zero"""
    dout, out = d(dout_nchw), d(out_nchw)
    b, c, h, w = out.shape
    y = torch.zeros(b, h, w, cp, dtype=F64)
    y[..., :c] = (dout * (1.0 - out * out)).permute(0, 2, 3, 1)
    return y


def lrelu(x, slope):
    x = d(x)
    return torch.where(x > 0, x, x * slope)


def lrelu_bwd(y, g, slope):
    """g (y > 0 ? 1 : slope), on the layer OUTPUT y"""
    y, g = d(y), d(g)
    return torch.where(y > 0, g, g * slope)


# ---- memory module ---------------------------------------------------------------------------------------------------

def commit_bwd(z, e_md, idx, ddiff=None, dq=None):
    """dz = ddiff 2 (z - E[idx[:, 0]]) / (N D) + dq; z [N, D], e_md [M, D], idx [N, k]"""
    z, e = d(z), d(e_md)
    n, dim = z.shape
    g = float(d(ddiff).reshape(-1)[0]) if ddiff is not None else 0.0
    dz = g * 2.0 * (z - e[idx[:, 0].long()]) / (n * dim)
    return dz + d(dq) if dq is not None else dz


def ema_counts_sums(x, idx, m):
    """counts [M] and sums [D, M] of the rows x [N, D] over their nearest slot idx[:, 0]"""
    x = d(x)
    i0 = idx[:, 0].long()
    counts = torch.zeros(m, dtype=F64)
    sums = torch.zeros(x.shape[1], m, dtype=F64)
    for j in range(m):
        hit = i0 == j
        counts[j] = float(hit.sum())
        if bool(hit.any()):
            sums[:, j] = x[hit].sum(0)
    return counts, sums


def ema_update(cluster_size, embed_avg, counts, sums, decay, omd, eps):
    """the blend and the Laplace-smoothed normalisation: (cluster_size', embed_avg' [D, M], embed [D, M])"""
    cs = decay * d(cluster_size) + omd * d(counts)
    ea = decay * d(embed_avg) + omd * d(sums)
    n = cs.sum()
    smoothed = (cs + eps) / (n + cs.numel() * eps) * n
    return cs, ea, ea / smoothed.unsqueeze(0)


def pack_codebook(e_dm):
    """[D, M] -> rows [M, D] and their squared norms"""
    e = d(e_dm)
    return e.t().contiguous(), (e * e).sum(0)


# ---- FlowNet2-SD element-wise ----------------------------------------------------------------------------------------

def flownet_prep(inputs, rgb_max):
    """inputs [B, 3, 2, H, W] -> NHWC [B, H, W, 6]: (x - mean over (frame, H, W) per (sample, colour)) / rgb_max at
    channel 3 frame + colour"""
    x = d(inputs)
    b, _, _, h, w = x.shape
    mean = x.reshape(b, 3, -1).sum(-1) / (2 * h * w)
    y = (x - mean.view(b, 3, 1, 1, 1)) / rgb_max
    return y.permute(0, 3, 4, 2, 1).reshape(b, h, w, 6)


def _lin_index(n_in):
    """source rows and weights of a x4 bilinear resize with align_corners=False (negative source clamped to 0)"""
    o = torch.arange(4 * n_in, dtype=F64)
    f = ((o + 0.5) * 0.25 - 0.5).clamp_min(0.0)
    i0 = torch.floor(f).long()
    i1 = torch.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, f - i0.double()


def upsample4(x, premul):
    """NHWC [B, H, W, c] -> NCHW [B, c, 4H, 4W] of bilinear x4 (x premul)"""
    v = d(x).permute(0, 3, 1, 2) * premul
    y0, y1, ly = _lin_index(v.shape[2])
    x0, x1, lx = _lin_index(v.shape[3])
    ly = ly.view(-1, 1)
    top = (1.0 - lx) * v[:, :, y0][:, :, :, x0] + lx * v[:, :, y0][:, :, :, x1]
    bot = (1.0 - lx) * v[:, :, y1][:, :, :, x0] + lx * v[:, :, y1][:, :, :, x1]
    return (1.0 - ly) * top + ly * bot


# ---- layout ----------------------------------------------------------------------------------------------------------

def nchw_to_nhwc(x, cp):
    x = d(x)
    b, c, h, w = x.shape
    y = torch.zeros(b, h, w, cp, dtype=F64)
    y[..., :c] = x.permute(0, 2, 3, 1)
    return y


def nhwc_to_nchw(x):
    return d(x).permute(0, 3, 1, 2).contiguous()
