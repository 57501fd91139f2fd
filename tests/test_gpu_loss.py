"""The fused generator-loss kernels (csrc/loss.hip, `ammcnet_aaai2021_amd.losses`, `harness.FUSED_LOSS`) against the
harness's own torch functions evaluated in float64 on the same inputs (autograd for the gradients); the float32
evaluation of the same functions - the flag-off path - is the witness.

Gates (u = 2^-24):
  value     |v - v64| <= (P + 3) u v64.  Every summand is non-negative; P is the largest number of elements one fp32
            partial accumulates - `AMMC_PRED_LOSS_ROWS * W` pixels for the prediction terms (a workgroup owns that many
            image rows, include/ammc_hip.h), `AMMC_L1_CHUNK` elements for `l1_mean`; + 3 = the summand's own rounding, the
            fp32 1 / count of the combine and the final cast (the combine itself runs in double).
  gradient  per entry |g - g64| <= max(2 |g_torch32 - g64|, R u max|g64|), R = 17 = the fp32 roundings of the kernel's
            expression for an entry plus one (see `R` below).
"""
import pytest
import torch

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import _lib, harness as Hn, losses as L, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
# d_pred = fl(fl(p - t) * fl(ci / fl(sqrt(n2))) + fl(k * cg))      k an integer in [-4, 4]
#   inv = fl(1 / BHW) 1, g_int in fp32 1, ci = fl(g_int * inv) 1, p - t 1, n2 = three products and two sums 5, sqrt 1,
#   the quotient 1, the product 1, g_gdl in fp32 1, cg = fl(g_gdl * inv) 1, k * cg 1, the final sum 1: 16 roundings
R = 16 + 1
SHAPES = [(2, 8, 8), (3, 27, 21), (2, 64, 64), (2, 256, 256)]
CASES = [(b, c, h, w) for (b, h, w) in SHAPES for c in (3, 2)]


@pytest.fixture(autouse=True)
def _flag_off(monkeypatch):
    monkeypatch.setattr(Hn, "FUSED_LOSS", False)          # truth and witness are the torch path whatever the environment


def _torch_terms(pred, target, gdl):
    """the harness's torch expressions: `single_stream_loss`'s "int" (= `generator_loss`'s) and `gradient_loss`"""
    i = Hn.single_stream_loss("op", pred, target, pred.new_zeros(1))[1]["int"]
    return i, (Hn.gradient_loss(pred, target) if gdl else None)


def _weighted(terms, w_int, w_gdl):
    return w_int * terms[0] + (w_gdl * terms[1] if terms[1] is not None else 0.0)


def _reference(pred, target, gdl, w_int, w_gdl, dtype):
    p = pred.detach().to(dtype).requires_grad_(True)
    terms = _torch_terms(p, target.to(dtype), gdl)
    _weighted(terms, w_int, w_gdl).backward()
    return terms[0].detach(), (terms[1].detach() if gdl else None), p.grad


def _fused(pred, target, gdl, w_int, w_gdl):
    p = pred.detach().clone().requires_grad_(True)
    terms = L.prediction_terms(p, target, gdl)
    assert (terms[1] is None) == (not gdl)
    _weighted(terms, w_int, w_gdl).backward()
    return terms[0].detach(), (terms[1].detach() if gdl else None), p.grad


def _value_gate(v, v64, p_elems, what):
    err, bound = abs(float(v.double()) - float(v64)), (p_elems + 3) * U * float(v64)
    print(f"{what}: value {float(v):.9g} fp64 {float(v64):.12g} |err| {err:.3g} bound {bound:.3g} (P = {p_elems})")
    assert err <= bound, what


def _grad_gate(g, g32, g64, what, keep=None):
    err = (g.double() - g64).abs()
    bound = torch.maximum(2.0 * (g32.double() - g64).abs(), R * U * g64.abs().max())
    over = err > bound
    if keep is not None:
        over &= keep
    print(f"{what}: gradient max|err| {float(err.max()):.3g} floor {float(R * U * g64.abs().max()):.3g} over {int(over.sum())}")
    assert not bool(over.any()), what


def _grid_pair(b, c, h, w):
    g = torch.Generator().manual_seed(1000 * b + 100 * c + 10 * h + w)
    pred = torch.randint(-256, 257, (b, c, h, w), generator=g).float() / 256.0
    target = torch.randint(-256, 257, (b, c, h, w), generator=g).float() / 256.0
    # exact ties that touch the borders: norm = 0 (gradient 0) and sign(0) = 0
    pred[:, :, :min(3, h), :min(5, w)] = target[:, :, :min(3, h), :min(5, w)]
    pred[-1, :, h - min(4, h):, w - min(3, w):] = target[-1, :, h - min(4, h):, w - min(3, w):]
    pred[0, :, h // 2, :] = target[0, :, h // 2, :]
    return pred.to(DEV), target.to(DEV)


@pytest.mark.parametrize("b,c,h,w", CASES)
def test_grid_inputs_values_and_gradients(b, c, h, w):
    """multiples of 2^-8 in [-1, 1]: every difference and channel sum is exact in fp32, no sign is in doubt"""
    pred, target = _grid_pair(b, c, h, w)
    P = _lib.AMMC_PRED_LOSS_ROWS * w
    for gdl, w_int, w_gdl in ((True, 0.7, 1.3), (False, 0.7, 0.0)):
        i, g, dp = _fused(pred, target, gdl, w_int, w_gdl)
        i64, g64, dp64 = _reference(pred, target, gdl, w_int, w_gdl, torch.float64)
        _, _, dp32 = _reference(pred, target, gdl, w_int, w_gdl, torch.float32)
        what = f"grid {b}x{c}x{h}x{w} gdl={gdl}"
        _value_gate(i, i64, P, what + " int")
        if gdl:
            _value_gate(g, g64, P, what + " gdl")
        _grad_gate(dp, dp32, dp64, what)
        tie = (pred == target).all(dim=1, keepdim=True).expand_as(pred)
        if not gdl:
            assert bool((dp[tie] == 0).all()), "norm = 0 must give gradient 0"
        assert bool(torch.isfinite(dp).all())


def _doubtful_signs(pred, target):
    """entries whose gradient depends on a difference |tx - gx| or |ty - gy| (fp64) below 4 u max|s|"""
    sp, st = pred.double().sum(1, keepdim=True), target.double().sum(1, keepdim=True)

    def dxy(s):
        dx = torch.cat([s[..., :1], s[..., 1:] - s[..., :-1]], dim=-1)
        dy = torch.cat([s[..., :1, :], s[..., 1:, :] - s[..., :-1, :]], dim=-2)
        return dx, dy
    gx, gy = dxy(sp)
    tx, ty = dxy(st)
    thr = 4 * U * float(torch.maximum(sp.abs().max(), st.abs().max()))
    sx, sy = (tx - gx).abs() < thr, (ty - gy).abs() < thr
    bad = sx | sy
    bad[..., :-1] |= sx[..., 1:]
    bad[..., :-1, :] |= sy[..., 1:, :]
    return bad.expand_as(pred)


@pytest.mark.parametrize("b,c,h,w", CASES)
def test_continuous_inputs_values_and_gradients(b, c, h, w):
    """U(-1, 1); the target is the last frame of a clip batch, in place (batch-strided, as the harness hands it over)"""
    pred = S.hashed_uniform(f"loss-pred-{b}-{c}-{h}-{w}", (b, c, h, w)).to(DEV)
    clips = S.hashed_uniform(f"loss-clip-{b}-{c}-{h}-{w}", (b, 3, c, h, w)).to(DEV)
    target = clips[:, -1]
    assert not target.is_contiguous() or b == 1
    P = _lib.AMMC_PRED_LOSS_ROWS * w
    bad = _doubtful_signs(pred, target)
    share = float(bad.double().mean())
    print(f"continuous {b}x{c}x{h}x{w}: excluded share {share:.3g}")
    assert share <= 1e-4
    i, g, dp = _fused(pred, target, True, 0.7, 1.3)
    i64, g64, dp64 = _reference(pred, target, True, 0.7, 1.3, torch.float64)
    _, _, dp32 = _reference(pred, target, True, 0.7, 1.3, torch.float32)
    what = f"continuous {b}x{c}x{h}x{w}"
    _value_gate(i, i64, P, what + " int")
    _value_gate(g, g64, P, what + " gdl")
    _grad_gate(dp, dp32, dp64, what, keep=~bad)


def test_two_runs_are_bit_identical():
    for (b, c, h, w) in ((3, 3, 27, 21), (2, 2, 256, 256)):
        pred, target = _grid_pair(b, c, h, w)
        r1, r2 = _fused(pred, target, True, 0.7, 1.3), _fused(pred, target, True, 0.7, 1.3)
        for a, bb in zip(r1, r2):
            assert torch.equal(a, bb)
        fa, fb = S.hashed_uniform("det-a", (b, c, h, w)).to(DEV), S.hashed_uniform("det-b", (b, c, h, w)).to(DEV)
        assert torch.equal(L.l1_mean(fa, fb), L.l1_mean(fa, fb))


def test_side_stream_equals_default_stream():
    pred, target = _grid_pair(2, 3, 64, 64)
    fa, fb = S.hashed_uniform("str-a", (2, 2, 64, 64)).to(DEV), S.hashed_uniform("str-b", (2, 2, 64, 64)).to(DEV)
    want, want_l1 = _fused(pred, target, True, 0.7, 1.3), L.l1_mean(fa, fb)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got, got_l1 = _fused(pred, target, True, 0.7, 1.3), L.l1_mean(fa, fb)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for a, bb in zip(want + (want_l1,), got + (got_l1,)):
        assert torch.equal(a, bb)


def test_preconditions_raise_instead_of_falling_back():
    p, t = torch.zeros(2, 3, 8, 8, device=DEV), torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(_lib.AmmcHipError):
        L.prediction_terms(p.transpose(2, 3), t, True)                     # a non-contiguous view
    with pytest.raises(_lib.AmmcHipError):
        L.prediction_terms(p, t.transpose(2, 3), True)
    with pytest.raises(_lib.AmmcHipError):
        L.prediction_terms(p.double(), t.double(), True)
    with pytest.raises(_lib.AmmcHipError):
        L.prediction_terms(torch.zeros(2, 4, 8, 8, device=DEV), torch.zeros(2, 4, 8, 8, device=DEV), False)
    with pytest.raises(_lib.AmmcHipError):
        L.prediction_terms(p.cpu(), t.cpu(), True)
    with pytest.raises(_lib.AmmcHipError):
        L.l1_mean(p.cpu(), t.cpu())
    with pytest.raises(_lib.AmmcHipError):
        L.l1_mean(p.double(), t.double())
    with pytest.raises(_lib.AmmcHipError):
        L.l1_mean(p.transpose(2, 3), t.transpose(2, 3))


@pytest.mark.parametrize("n,offset", [(2 * 2 * 8 * 8, 0), (3 * 2 * 27 * 21, 0), (2 * 2 * 64 * 64, 0), (10730, 0), (10730, 1),
                                      (2 * 2 * 256 * 256, 0)])
def test_l1_mean_against_float64(n, offset):
    """below one chunk, tails that are no multiple of the vector, several chunks, a slice that starts off a 16-byte boundary"""
    a = S.hashed_uniform(f"l1-a-{n}", (n + offset,)).to(DEV)[offset:]
    b = S.hashed_uniform(f"l1-b-{n}", (n + offset,)).to(DEV)[offset:]
    v, v64 = L.l1_mean(a, b), Hn.flow_loss(a.double(), b.double())
    assert v.dim() == 0 and not v.requires_grad
    _value_gate(v, v64, _lib.AMMC_L1_CHUNK, f"l1_mean n={n} offset={offset}")


# ---- integration: the harness's loss functions with the flag on and off, on one recorded generator output -----------

@pytest.fixture(scope="module")
def recorded():
    G = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    G.load_state_dict(S.make_twostream_state())
    G = G.to(DEV).train()
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(2, 64, 64, tag="loss-int"))
    out = G(rgb_x, op_x)
    rec = dict(rgb=out[0].detach().clone(), op=out[1].detach().clone(), rd=out[2][0].detach().clone(),
               od=out[2][1].detach().clone(), rgb_t=rgb_t, op_t=op_t,
               d_gen=S.hashed_uniform("loss-dgen", (2, 1, 6, 6)).to(DEV),
               flow_pred=S.hashed_uniform("loss-fp", (2, 2, 64, 64)).to(DEV) * 0.1,
               flow_gt=S.hashed_uniform("loss-fg", (2, 2, 64, 64)).to(DEV) * 0.1)
    del G, out
    return rec


def _count_calls(monkeypatch):
    calls = {"pred": 0, "l1": 0}
    real_pred, real_l1 = L.prediction_terms, L.l1_mean

    def pred(*a, **k):
        calls["pred"] += 1
        return real_pred(*a, **k)

    def l1(*a, **k):
        calls["l1"] += 1
        return real_l1(*a, **k)
    monkeypatch.setattr(L, "prediction_terms", pred)
    monkeypatch.setattr(L, "l1_mean", l1)
    return calls


def _term_budget(rec, lam):
    """sum of the value gates of the fused terms (fp64 terms from the torch functions) for weights `lam` = {term: weight}"""
    d = {k: v.double() for k, v in rec.items()}
    P = _lib.AMMC_PRED_LOSS_ROWS * 64
    t = {"int_rgb": (_torch_terms(d["rgb"], d["rgb_t"], False)[0], P), "gdl": (Hn.gradient_loss(d["rgb"], d["rgb_t"]), P),
         "int_op": (_torch_terms(d["op"], d["op_t"], False)[0], P),
         "flow": (Hn.flow_loss(d["flow_pred"], d["flow_gt"]), _lib.AMMC_L1_CHUNK)}
    return sum(abs(w) * (t[k][1] + 3) * U * float(t[k][0]) for k, w in lam.items())


def _check_loss(v, v32, v64, budget, what):
    """the fused terms within their gates; the torch-side terms (latent, adversarial) and the fp32 weighting of the 0-d
    terms are the same operations with the flag on and off: they get what the witness is away from the truth, plus 16 u
    of the loss for the roundings of at most six products and five sums of terms that are not all positive in general"""
    err, bound = abs(float(v.double()) - float(v64)), budget + abs(float(v32.double()) - float(v64)) + 16 * U * abs(float(v64))
    print(f"{what}: loss {float(v):.9g} witness {float(v32):.9g} fp64 {float(v64):.12g} |err| {err:.3g} bound {bound:.3g}")
    assert err <= bound, what


def test_generator_loss_full_flag_on_against_flag_off_and_float64(recorded, monkeypatch):
    lam = Hn.LAMS_ANOPRED

    def run(flag, dtype):
        monkeypatch.setattr(Hn, "FUSED_LOSS", flag)
        r = {k: v.to(dtype) if v.is_floating_point() else v for k, v in recorded.items()}
        rgb, op = r["rgb"].clone().requires_grad_(True), r["op"].clone().requires_grad_(True)
        loss = Hn.generator_loss_full((rgb, op, (r["rd"], r["od"]), None), r["rgb_t"], r["op_t"], r["d_gen"], r["flow_pred"],
                                      r["flow_gt"], **lam)
        loss.backward()
        return loss.detach(), rgb.grad, op.grad
    v64, gr64, go64 = run(False, torch.float64)
    v32, gr32, go32 = run(False, torch.float32)
    budget = _term_budget(recorded, {"int_rgb": lam["lam_lp"], "gdl": lam["lam_gdl"], "int_op": lam["lam_lp_op"],
                                     "flow": lam["lam_flow"]})
    budget_g = _term_budget(recorded, {"int_rgb": 1.0, "int_op": 1.0})
    calls = _count_calls(monkeypatch)
    v, gr, go = run(True, torch.float32)
    assert calls == {"pred": 2, "l1": 1}                   # each prediction pair visited once, the flow term on its kernel
    _check_loss(v, v32, v64, budget, "generator_loss_full")
    _grad_gate(gr, gr32, gr64, "generator_loss_full d/d rgb", keep=~_doubtful_signs(recorded["rgb"], recorded["rgb_t"]))
    _grad_gate(go, go32, go64, "generator_loss_full d/d op")
    # the G-only objective takes the same route
    monkeypatch.setattr(Hn, "FUSED_LOSS", True)
    out = (recorded["rgb"], recorded["op"], (recorded["rd"], recorded["od"]), None)
    g_on = Hn.generator_loss(out, recorded["rgb_t"], recorded["op_t"])
    monkeypatch.setattr(Hn, "FUSED_LOSS", False)
    g_off = Hn.generator_loss(out, recorded["rgb_t"], recorded["op_t"])
    d = {k: v.double() for k, v in recorded.items()}
    g64 = Hn.generator_loss((d["rgb"], d["op"], (d["rd"], d["od"]), None), d["rgb_t"], d["op_t"])
    assert calls["pred"] == 4
    _check_loss(g_on, g_off, g64, budget_g, "generator_loss")


@pytest.mark.parametrize("stream", ["rgb", "op"])
def test_single_stream_loss_flag_on_against_flag_off_and_float64(recorded, monkeypatch, stream):
    def run(flag, dtype):
        monkeypatch.setattr(Hn, "FUSED_LOSS", flag)
        r = {k: v.to(dtype) for k, v in recorded.items()}
        pred = r[stream].clone().requires_grad_(True)
        if stream == "rgb":
            loss, terms = Hn.single_stream_loss("rgb", pred, r["rgb_t"], r["rd"], r["d_gen"], r["flow_pred"], r["flow_gt"])
        else:
            loss, terms = Hn.single_stream_loss("op", pred, r["op_t"], r["od"])
        loss.backward()
        return loss.detach(), terms, pred.grad
    v64, t64, g64 = run(False, torch.float64)
    v32, t32, g32 = run(False, torch.float32)
    lam = Hn.SINGLE_LAMS[stream]
    weights = ({"int_rgb": lam["lam_lp"], "gdl": lam["lam_gdl"], "flow": lam["lam_flow"]} if stream == "rgb"
               else {"int_op": lam["lam_lp_op"]})
    budget = _term_budget(recorded, weights)
    calls = _count_calls(monkeypatch)
    v, t, g = run(True, torch.float32)
    monkeypatch.setattr(Hn, "FUSED_LOSS", False)
    assert calls == {"pred": 1, "l1": 1 if stream == "rgb" else 0}
    assert list(t) == list(t32) == list(t64)               # same keys, same order, same meaning
    P = _lib.AMMC_PRED_LOSS_ROWS * 64
    for k in t:
        if k in ("int", "gdl", "flow"):
            _value_gate(t[k].detach(), t64[k].detach(), _lib.AMMC_L1_CHUNK if k == "flow" else P, f"single_stream_loss {stream} {k}")
        else:
            assert torch.equal(t[k], t32[k]), k            # the torch-side terms are untouched
    _check_loss(v, v32, v64, budget, f"single_stream_loss {stream}")
    keep = ~_doubtful_signs(recorded["rgb"], recorded["rgb_t"]) if stream == "rgb" else None
    _grad_gate(g, g32, g64, f"single_stream_loss {stream} d/d pred", keep=keep)


def test_one_flagged_adversarial_iteration(monkeypatch):
    """`train_step_gan` with FUSED_LOSS on and AMMC_GAN_OVERLAP at its default: the node lives with the side lane and
    `_FiniteWatch`; both networks are updated"""
    monkeypatch.setattr(Hn, "FUSED_LOSS", True)
    calls = _count_calls(monkeypatch)
    B = 2
    G = A.get_twostream((12, 6), (3, 2), 64, 256, 2)
    G.load_state_dict(S.make_twostream_state())
    G = G.to(DEV).train()
    D = A.PixelDiscriminator(3, [128, 256, 512, 512])
    D.load_state_dict(S.make_discriminator_state())
    D = D.to(DEV).train()
    opt_g, opt_d = Hn.adam(G.parameters(), lr=2e-4), Hn.adam(D.parameters(), lr=2e-5)
    rgb_x, op_x, rgb_t, op_t = (t.to(DEV) for t in S.make_clips(B, 64, 64, tag="loss-iter"))
    rgb = torch.cat([rgb_x.view(B, 4, 3, 64, 64), rgb_t[:, None]], 1)
    op = torch.cat([op_x.view(B, 3, 2, 64, 64), op_t[:, None]], 1)
    g0 = [p.detach().clone() for p in G.parameters()]
    d0 = [p.detach().clone() for p in D.parameters()]

    def flow_fn(prev, cur):                                # stands in for FlowNet2-SD: any function of the pair, no gradient
        with torch.no_grad():
            return ((cur - prev)[:, :2] * 0.5).contiguous()
    outputs = {}
    g_loss, d_loss = Hn.train_step_gan(G, D, opt_g, opt_d, rgb, op, flow_fn, outputs=outputs, **Hn.LAMS_ANOPRED)
    torch.cuda.synchronize()
    assert calls == {"pred": 2, "l1": 1}
    assert bool(torch.isfinite(g_loss)) and bool(torch.isfinite(d_loss))
    assert outputs["rgb"].shape == (B, 3, 64, 64) and outputs["op"].shape == (B, 2, 64, 64)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(g0, G.parameters()))
    assert any(not torch.equal(a, p.detach()) for a, p in zip(d0, D.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in list(G.parameters()) + list(D.parameters()))
