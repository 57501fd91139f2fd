"""GPU tests of the memory-score pass (`ops.memory_scores`, csrc/memory_scores.hip): parity against
the float64 reference on the shared cases (tests/memory_score_cases.py), the quantities the header defines exactly,
the invariance the pass exists for (bit for bit), the model's bottleneck accessor and the fused block's `diff` scalar,
the harness loop and the `run_memory` entry.

The parity gate G is not a constant of this file: it is 4 x the worst err / scale of a CPU fp32 WITNESS on the same
inputs (`F.linear` in fp32, then the direct squared distance to the reference's nearest slot) over the case list; the
factor 4 covers an accumulation order that differs from the CPU library's blocked sums (DESIGN.md section 8 measured
1.5 x for the split-chain fp32 kernel).  Both numbers are printed by the parity test.
"""
import functools
import json
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import harness as Hn, ops, run_memory, run_test, synthetic as S

import memory_score_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("map", "idx", "commit", "worst", "worst_idx")
IDS = [K.name_of(c, v) for c, v in K.all_variants()]


@functools.lru_cache(maxsize=None)
def _gate():
    """(G, the witness's worst err / scale)"""
    worst = 0.0
    for case, variant in K.all_variants():
        t, ref = K.inputs(case, variant), K.reference(case, variant)
        z32 = F.linear(t["x"], t["enc_w"], t["enc_b"])
        near = t["embed"].t()[ref["idx"][..., 0].long()]
        s = ((near - z32) ** 2).sum(-1) / K.D
        worst = max(worst, float(((s.double() - ref["map"]).abs() / ref["scale"]).max()))
    return 4.0 * worst, worst


def _quan(t, k):
    """the attributes `ops.memory_scores` reads of an `enc_quan_dec_topk` module"""
    d, c = t["enc_w"].shape
    return types.SimpleNamespace(enc=types.SimpleNamespace(weight=t["enc_w"].to(DEV).view(d, c, 1, 1), bias=t["enc_b"].to(DEV)),
                                 quantize=types.SimpleNamespace(embed=t["embed"].to(DEV), k=k))


def _run(case, variant="", x=None, **kw):
    t = K.inputs(case, variant)
    x = t["x"].to(DEV) if x is None else x
    return ops.memory_scores(_quan(t, case[5]), x.permute(0, 3, 1, 2), **kw)


def _same(a, b, keys=KEYS, where=""):
    for key in keys:
        assert torch.equal(a[key], b[key]), f"{key} {where}"


def _check_against_reference(got, ref, k, label, planted=None):
    """gate 1: map / commit within G * scale of the float64 reference; idx equal to it wherever the ranking is decided
    by more than 1e-4 |z|^2, elsewhere every returned slot as near as the reference's slot of that rank up
    to that tolerance.  `planted` (variant a): the tied slots, whose zero gaps do not count as near ties - exactly equal
    keys come in ascending slot order, which is the order of the reference's stable sort."""
    G, witness = _gate()
    gm, gc = got["map"].double().cpu(), got["commit"].double().cpu()
    err = float(((gm - ref["map"]).abs() / ref["scale"]).max())
    mscale = ref["scale"].mean(dim=(1, 2))
    cerr = float(((gc - ref["commit"]).abs() / mscale).max())
    print(f"{label}: map err/scale {err:.3e}, commit err/mean(scale) {cerr:.3e}, G {G:.3e} (witness {witness:.3e})")
    assert bool(((gm - ref["map"]).abs() <= G * ref["scale"]).all()), (err, G)
    assert bool(((gc - ref["commit"]).abs() <= G * mscale).all()), (cerr, G)
    gi = got["idx"].cpu()
    assert gi.dtype == torch.int32 and tuple(gi.shape) == tuple(ref["idx"].shape)
    m = ref["dist"].shape[-1]
    assert int(gi.min()) >= 0 and int(gi.max()) < m
    tol = 1e-4 * ref["znorm"]
    margin = ref["margin"]
    if planted is not None:
        order = ref["order"]
        srt = torch.gather(ref["dist"], -1, order)
        gaps = srt[..., 1:] - srt[..., :-1]
        is_p = torch.zeros_like(order, dtype=torch.bool)
        for s in planted:
            is_p |= order == s
        gaps = torch.where(is_p[..., 1:] & is_p[..., :-1], torch.full_like(gaps, float("inf")), gaps)
        margin = gaps.min(-1).values
    decided = margin > tol
    assert torch.equal(gi[decided], ref["idx"][decided]), f"{label}: idx differs at a decided position"
    d_got = torch.gather(ref["dist"], -1, gi.long())
    d_ref = torch.gather(ref["dist"], -1, ref["idx"].long())
    assert bool(((d_got - d_ref).abs() <= tol[..., None])[~decided].all()), f"{label}: a near-tie slot is not as near"
    print(f"{label}: {int((~decided).sum())} of {decided.numel()} positions compared by distance")


# ---- 1. parity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,variant", K.all_variants(), ids=IDS)
def test_parity_against_fp64(case, variant):
    got = _run(case, variant, indices=True)
    ref = K.reference(case, variant)
    b, h, w, _, _, k = case
    assert tuple(got["map"].shape) == (b, h, w) and tuple(got["idx"].shape) == (b, h, w, k)
    _check_against_reference(got, ref, k, K.name_of(case, variant), planted=K.TIE_SLOTS if variant == "a" else None)
    gi = got["idx"].cpu()
    if variant == "a":
        first = ref["idx"][..., 0] == K.TIE_SLOTS[0]
        assert int(first.sum()) >= 1
        assert bool((gi[first] == torch.tensor(K.TIE_SLOTS[:2], dtype=torch.int32)).all())       # 3 then 5
    if variant == "b":
        G, _ = _gate()
        for s, (bb, y, xx) in zip(K.NEAR_SLOTS, K.near_rows(case)):
            assert int(gi[bb, y, xx, 0]) == s
            assert float(got["map"][bb, y, xx]) <= G * float(ref["scale"][bb, y, xx])


# ---- 2. what the header defines exactly ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.CASES, ids=[K.name_of(c) for c in K.CASES])
def test_exact_contracts_recomputed_from_the_returned_map(case):
    got = _run(case)
    mp = got["map"].cpu().numpy()
    b, h, w = mp.shape
    for i in range(b):
        total = 0.0                                   # Python floats are doubles: rows in order, then the rows in order
        for y in range(h):
            row = 0.0
            for x in range(w):
                row += float(mp[i, y, x])
            total += row
        assert np.float32(total / (h * w)).tobytes() == got["commit"][i].cpu().numpy().tobytes(), i
        flat = mp[i].reshape(-1)
        at = int(np.argmax(flat))                     # numpy: the first maximum
        assert int(got["worst_idx"][i]) == at and got["worst"][i].cpu().numpy().tobytes() == flat[at].tobytes(), i
    assert got["worst_idx"].dtype == torch.int32 and "idx" not in got


# ---- 3. invariance -----------------------------------------------------------------------------------------------------

INVARIANCE_CASES = [K.CASES[1], K.CASES[3], K.CASES[5]]


@pytest.mark.parametrize("case", INVARIANCE_CASES, ids=[K.name_of(c) for c in INVARIANCE_CASES])
def test_a_clip_scores_the_same_alone_and_at_each_place_of_a_batch(case):
    t = K.inputs(case)
    x = t["x"].to(DEV)
    _, h, w, c, _, _ = case
    alone = _run(case, x=x[:1].contiguous(), indices=True)
    g = torch.Generator().manual_seed(77)
    for n in (3, 5):
        others = torch.randn((n, h, w, c), generator=g).to(DEV) * 3.0
        for place in range(n):
            batch = others.clone()
            batch[place] = x[0]
            got = _run(case, x=batch, indices=True)
            _same({key: got[key][place:place + 1] for key in KEYS}, alone, where=f"place {place} of {n}")


@pytest.mark.parametrize("case", INVARIANCE_CASES, ids=[K.name_of(c) for c in INVARIANCE_CASES])
def test_order_does_not_depend_on_strides_alignment_indices_or_out(case):
    t = K.inputs(case)
    b, h, w, c, m, k = case
    x = t["x"].to(DEV)
    base = _run(case, x=x, indices=True)
    _same(_run(case, x=x, indices=True), base, where="second launch")
    _same(_run(case, x=x), base, keys=("map", "commit", "worst", "worst_idx"), where="without indices")
    for pad in (32, 1):                                # padded pixel, row and batch strides: 16-byte and 4-byte loads
        buf = torch.full((b + 1, h + 1, w + 2, c + pad), 7.0, device=DEV)
        view = buf[:b, :h, :w, :c]
        view.copy_(x)
        assert view.stride(3) == 1 and not view.is_contiguous()
        _same(_run(case, x=view, indices=True), base, where=f"padded strides (+{pad})")
    flat = torch.zeros(x.numel() + 1, device=DEV)
    off = flat[1:].view(b, h, w, c)                    # a base offset by one float
    off.copy_(x)
    assert off.data_ptr() % 16 == 4
    _same(_run(case, x=off, indices=True), base, where="offset base")
    # strided `out=` views of larger buffers, prefilled
    mbuf = torch.full((b, h * w + 5), -1.0, device=DEV)
    sbuf = torch.full((3, b + 2), -1.0, device=DEV)
    ibuf = torch.full((b + 2,), -1, device=DEV, dtype=torch.int32)
    kbuf = torch.full((b + 1, h, w, k), -1, device=DEV, dtype=torch.int32)
    out = {"map": mbuf[:, :h * w].view(b, h, w), "commit": sbuf[0, 1:b + 1], "worst": sbuf[2, :b], "worst_idx": ibuf[2:],
           "idx": kbuf[1:]}
    got = _run(case, x=x, indices=True, out=out)
    for key in KEYS:
        assert got[key].data_ptr() == out[key].data_ptr()
    _same(got, base, where="out= views")
    assert bool((mbuf[:, h * w:] == -1).all()) and bool((sbuf[1] == -1).all()) and bool((kbuf[0] == -1).all())
    assert float(sbuf[0, 0]) == -1 and float(sbuf[0, b + 1]) == -1 and bool((ibuf[:2] == -1).all())


def test_nchw_contiguous_input_takes_one_copy_and_gives_the_same_bits():
    case = K.CASES[1]
    x = K.inputs(case)["x"].to(DEV)
    nchw = x.permute(0, 3, 1, 2).contiguous()          # channel stride of the NHWC view is h * w: copied once inside
    got = ops.memory_scores(_quan(K.inputs(case), case[5]), nchw, indices=True)
    _same(got, _run(case, x=x, indices=True), where="NCHW-contiguous input")


# ---- 4. model level -------------------------------------------------------------------------------------------------------

N_EMBED = 96


@pytest.fixture(scope="module")
def model():
    m = A.get_twostream((12, 6), (3, 2), 64, N_EMBED, 2)
    m.load_state_dict(S.make_twostream_state(embed_dim=64, n_embed=N_EMBED, k=2))
    return m.to(DEV).eval()


@pytest.mark.parametrize("precision", ["s16", "fp32"])
@pytest.mark.parametrize("batch,hh,ww", [(3, 64, 64), (2, 40, 72)])
def test_bottleneck_inputs_and_the_fused_blocks_diff(model, precision, batch, hh, ww):
    model.precision = precision
    rgb_x = S.hashed_uniform(f"ms:rgb{hh}", (batch, 12, hh, ww)).to(DEV)
    op_x = S.hashed_normal(f"ms:op{hh}", (batch, 6, hh, ww), 2.0).to(DEV) / 256.0
    with torch.no_grad():
        _, _, diffs, _ = model(rgb_x, op_x)
    xs = model.bottleneck_inputs()
    assert len(xs) == 2
    befor = model.quant_befor
    assert torch.equal(xs[0].permute(0, 3, 1, 2), befor)
    for name, x4, vq, diff in zip(("rgb", "op"), xs, (model.rgb.vq_down3, model.op.vq_down3), diffs):
        assert tuple(x4.shape) == (batch, hh // 8, ww // 8, 512) and x4.dtype == torch.float32 and x4.stride(3) == 1
        got = ops.memory_scores(vq, x4.permute(0, 3, 1, 2), indices=True)
        blk = vq.quan                                   # enc_quan_dec_res_topk wraps the block it adds its input to
        ref = Hn.memory_scores_reference(blk.enc.weight.detach().cpu(), blk.enc.bias.detach().cpu(),
                                         blk.quantize.embed.detach().cpu(), x4.cpu(), blk.quantize.k)
        _check_against_reference(got, ref, blk.quantize.k, f"{name} {precision} {hh}x{ww}")
        _same(ops.memory_scores(blk, x4.permute(0, 3, 1, 2), indices=True), got, where="the inner block")
        mean = float(got["commit"].double().mean())
        fused = float(diff)
        rel = abs(mean - fused) / abs(fused)
        print(f"{name} {precision} {hh}x{ww}: mean_b commit {mean:.9e}, the forward's diff {fused:.9e}, rel {rel:.3e}")
        assert rel <= 1e-4                              # `diff` scalars


# ---- 5. harness and entry -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [16, 3])
def test_memory_subvideo(model, batch):
    model.precision = "s16"
    t, size = 23, 64
    (rgb, op), = run_test.synthetic_dataset(1, t, size)[0]
    rgb, op = rgb.to(DEV), op.to(DEV)
    rec = Hn.memory_subvideo(model, rgb, op, batch=batch, indices=True)
    loc = Hn.localise_subvideo(model, rgb, op, 16, False, batch)
    assert np.array_equal(rec["rgb_comm"], loc["rgb_comm"]) and np.array_equal(rec["op_comm"], loc["op_comm"])
    g = size // 8
    for st, lc in (("rgb", Hn.RGB_LEN_CLIP), ("op", Hn.OP_LEN_CLIP)):
        assert rec[f"{st}_clip_comm"].shape == (t,) and rec[f"{st}_commit_map"].shape == (t, g, g)
        assert rec[f"{st}_commit_worst"].shape == (t,) and rec[f"{st}_commit_worst_idx"].dtype == np.int32
        assert rec[f"{st}_slots"].shape == (t, g, g, 2) and rec[f"{st}_slots"].dtype == np.int32
        assert rec[f"{st}_psnr"].shape == (t,) and np.isfinite(rec[f"{st}_psnr"]).all()
        assert 0 <= rec[f"{st}_slots"].min() and rec[f"{st}_slots"].max() < N_EMBED
        for s, e in Hn.subvideo_batches(t, batch):       # per batch: the clips' mean is the reference's one value
            mean = float(rec[f"{st}_clip_comm"][s + lc - 1:e + lc - 1].astype(np.float64).mean())
            comm = float(rec[f"{st}_comm"][s + lc - 1])
            assert abs(mean - comm) <= 1e-4 * abs(comm), (st, s, e, mean, comm)
        for key in ("clip_comm", "commit_map", "commit_worst", "commit_worst_idx", "slots"):
            a = rec[f"{st}_{key}"]
            for i in range(lc - 1):                      # the head copies the first predicted frame
                assert np.array_equal(a[i], a[lc - 1]), (st, key, i)
        worst = rec[f"{st}_commit_map"].reshape(t, -1)
        assert np.array_equal(rec[f"{st}_commit_worst"], worst.max(1))
        assert np.array_equal(rec[f"{st}_commit_worst_idx"], worst.argmax(1).astype(np.int32))
    for key in ("clip_comm", "commit_map", "commit_worst", "commit_worst_idx", "slots", "comm"):
        assert np.array_equal(rec[f"op_{key}"][t - 1], rec[f"op_{key}"][t - 2]), key     # the flow stream's last frame


def test_run_memory_entry(tmp_path, capsys):
    argv = ["--synthetic", "--videos", "2", "--frames", "12", "--size", "64", "--n_embed", str(N_EMBED)]
    maps = tmp_path / "maps"
    run_memory.main(argv + ["--maps_dir", str(maps), "--slots"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["maps"] == 2 and 0.0 <= line["auc"] <= 1.0 and 0.0 <= line["auc_clip"] <= 1.0
    assert line["videos"] == 2 and line["predicted_frames"] == (12 - 4) + (19 - 4) and line["gpus"] == 1
    for v, t in enumerate((12, 19)):
        with np.load(maps / f"{v:04d}.npz") as z:
            want = {"rgb_comm", "op_comm"}
            for st in ("rgb", "op"):
                want |= {f"{st}_{key}" for key in ("clip_comm", "commit_map", "commit_worst", "commit_worst_idx", "psnr", "slots")}
            assert set(z.files) == want
            assert z["rgb_commit_map"].shape == (t, 8, 8) and z["op_slots"].shape == (t, 8, 8, 2)
            assert z["rgb_clip_comm"].shape == (t,) and z["rgb_comm"].shape == (t,)
    run_memory.main(argv)                                # no folder asked for: nothing is written
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["maps"] == 0 and "auc_clip" in line
