"""Stage 1 of the reference's recipe on the HIP path: one `UNetMem_v7` stream trained on its own (`run_train --stage
rgb|op`, `harness.train_step_single_gan` / `train_step_single`, `ammc_gather_clips_one`).

* The one-kind gather against the two-kind gather and the evaluation pipeline's loaders, bit for bit.
* One iteration of each stage against the fp64 truth on the branch the HIP evaluation took (memory lookups AND max-pool
  routes forced, tests/truth.py), built here from the oracle's blocks: `unetmem_forward` forces lookups but not pool
  routes.  Judged by `truth.same_branch_verdict` at batch 2 (small_batch) and batch 32 at 256² (timed_batch).
* `run_train --stage rgb` / `--stage op` end to end on a tiny JPEG + .flo set, their checkpoints feeding `--stage joint`.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ammcnet_aaai2021_amd as A
from ammcnet_aaai2021_amd import _lib, harness as Hn, pipeline as P, run_train, synthetic as S
from oracle import ammc_oracle as O
import truth as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- the one-kind gather ---------------------------------------------------------------------------------------------

def _tree(root, lens_rgb, lens_op, h, w, seed):
    rng = np.random.default_rng(seed)
    vids = []
    for v, (nr, no) in enumerate(zip(lens_rgb, lens_op)):
        dr, do = root / "rgb" / f"{v + 1:02d}", root / "op" / f"{v + 1:02d}"
        dr.mkdir(parents=True)
        do.mkdir(parents=True)
        fr = rng.integers(0, 256, (nr, h, w, 3), dtype=np.uint8)
        fl = rng.normal(0, 3, (no, h, w, 2)).astype(np.float32)
        for i in range(nr):
            np.save(dr / f"{i:04d}.npy", fr[i])
        for i in range(no):
            np.save(do / f"{i:04d}.npy", fl[i])
        vids.append((fr, fl))
    return vids


@pytest.mark.parametrize("h,w,size", [(240, 360, 256), (3, 5, 8)])
def test_one_kind_gather_is_bit_identical_to_the_two_kind_gather_and_the_loaders(tmp_path, h, w, size):
    lens_rgb, lens_op = (7, 9), (6, 8)
    vids = _tree(tmp_path, lens_rgb, lens_op, h, w, h + w)
    rgb_root, op_root = str(tmp_path / "rgb"), str(tmp_path / "op")
    both = P.ClipBank(rgb_root, op_root, size, DEV, workers=2, budget_gb=4.0)
    only_rgb = P.ClipBank(rgb_root, None, size, DEV, workers=2, budget_gb=4.0)
    only_op = P.ClipBank(None, op_root, size, DEV, workers=2, budget_gb=4.0)
    assert only_rgb.kinds == ("rgb",) and only_rgb.op is None and only_rgb.nbytes == P.bank_bytes(sum(lens_rgb), 0, size)
    assert only_op.kinds == ("op",) and only_op.rgb is None and only_op.nbytes == P.bank_bytes(0, sum(lens_op), size)
    assert torch.equal(only_rgb.rgb, both.rgb) and torch.equal(only_op.op, both.op)
    rs = np.array([0, 2, 7, 10, 1, 7])                                 # every start of each video's first / last drawable clip
    os_ = np.array([0, 1, 6, 9, 2, 6])
    want_rgb, want_op = both.gather(rs, os_)
    got_rgb, got_op = only_rgb.gather(rs), only_op.gather(os_)
    assert got_rgb.shape == want_rgb.shape and got_op.shape == want_op.shape
    assert torch.equal(got_rgb, want_rgb) and torch.equal(got_op, want_op)
    # (video, start) pairs through the one-kind global index, against the evaluation pipeline's kernels
    vid, start = np.array([0, 1, 1]), np.array([2, 0, 4])
    got_rgb, got_op = only_rgb.gather(only_rgb.global_index(vid, start)), only_op.gather(only_op.global_index(vid, start))
    for i in range(3):
        fr, fl = vids[vid[i]]
        ev_rgb = P.frames_to_device(torch.from_numpy(fr[start[i]:start[i] + 5]).to(DEV), (size, size))
        ev_op = P.flows_to_device(torch.from_numpy(fl[start[i]:start[i] + 4]).to(DEV), (size, size))
        assert torch.equal(got_rgb[i], ev_rgb) and torch.equal(got_op[i], ev_op), i
    # bad indices raise on the host, before anything is launched
    for bank, bad in ((only_rgb, [3]), (only_rgb, [-1]), (only_rgb, [sum(lens_rgb) - 4]), (only_op, [3]),
                      (only_op, [2.0]), (only_op, [])):
        with pytest.raises(_lib.AmmcHipError):
            bank.gather(np.array(bad))
    with pytest.raises(_lib.AmmcHipError):
        only_rgb.validate(np.array([0]), np.array([0]))


# ---- one iteration of each stage against the fp64 truth on the HIP branch -------------------------------------------

K, N_EMBED = 2, 256
CASES = {                     # stage -> (stream, discriminator, loss weights)
    "rgb": ("rgb", True, Hn.SINGLE_LAMS["rgb"]),
    "op": ("op", False, dict(lam_lp_op=1.0, lam_latent=1.0)),
    "op_adv": ("op", True, dict(lam_lp_op=1.0, lam_adv_op=0.05, lam_latent=1.0)),
}


def _stream_state(stream):
    return {k[len(stream) + 1:]: v for k, v in S.make_twostream_state(n_embed=N_EMBED, k=K).items()
            if k.startswith(stream + ".")}


def _hip_branch(G) -> dict:
    """the lookups and max-pool routes of the HIP training forward that just ran (cf. truth.hip_lookups)"""
    st = G._train_engine._last["streams"][0]
    out = {"idx": st.idx.reshape(-1, K).long().clone(), "pool": {}}
    pi = getattr(st, "pool_idx", None)
    if pi:
        for lvl, t in enumerate(pi):
            out["pool"][f"down{lvl + 1}"] = t.permute(0, 3, 1, 2).long().contiguous()
    else:
        for lvl in range(3):
            out["pool"][f"down{lvl + 1}"] = O.maxpool2x2_routes(st.skip[lvl].interior().permute(0, 3, 1, 2).float())[1]
    return out


def single_step(sd_g, sd_d, sd_f, x, t, stream, lams, dtype, device, force=None):
    """One iteration of the reference's single-stream loop in the oracle (`inference_v3` / `inference_v4` /
    `inference_v4_1`, train_helper.py:1592-1766 and the op stage without D): `UNetMem_v7` forward in training mode with
    the given lookups and pool routes, FlowNet2-SD on (target, prediction.detach()) and (target, target), D(prediction),
    `rgb_vq_Loss` / `op_vq_Loss` (loss_zoo.py:101-137, 171-198), `Discriminate_Loss` on (D(target), D(prediction.detach())).
    -> ({"G." / "D." name: gradient}, branch)"""
    x, t = x.to(device=device, dtype=dtype), t.to(device=device, dtype=dtype)
    mg = T._cast(sd_g, dtype, device, True)
    md = T._cast(sd_d, dtype, device, True) if sd_d is not None else None
    fi = force or {}
    fpool = fi.get("pool", {})
    aux = {}
    x1 = O.double_conv(mg, "inc.conv.conv", x, True)
    x2 = O.down(mg, "down1", x1, True, fpool.get("down1"), aux)
    x3 = O.down(mg, "down2", x2, True, fpool.get("down2"), aux)
    x4 = O.down(mg, "down3", x3, True, fpool.get("down3"), aux)
    x4, diff, _, idxk = O.vq_block(mg, "vq_down3", x4, K, True, fi.get("idx"))
    y = O.up(mg, "up1", x4, x3, True)
    y = O.up(mg, "up2", y, x2, True)
    y = O.up(mg, "up3", y, x1, True)
    pred = torch.tanh(F.conv2d(y, mg["outc.weight"], mg["outc.bias"], padding=1))
    lam = {**Hn.SINGLE_LAMS[stream], **lams}
    g_int, g_latent = O.intensity_l2(pred, t), diff.sum()
    d_gen = O.pixel_discriminator(md, pred) if md is not None else None
    if stream == "rgb":
        g_loss = lam["lam_adv"] * O.adversarial_loss(d_gen) + lam["lam_gdl"] * O.gradient_loss(pred, t)
        if sd_f is not None:
            mf = T._cast(sd_f, dtype, device, False)
            with torch.no_grad():
                def flow(cur):
                    pair = torch.cat([t.unsqueeze(2), cur.unsqueeze(2)], 2)
                    return O.flownet2sd_forward(mf, (pair * 0.5 + 0.5) * 255.0) / 255.0
                fp, fg = flow(pred.detach()), flow(t)
            del mf
            g_loss = g_loss + lam["lam_flow"] * O.flow_loss(fp, fg)
        g_loss = g_loss + lam["lam_lp"] * g_int + lam["lam_latent"] * g_latent
    else:
        g_loss = lam["lam_lp_op"] * g_int
        if d_gen is not None:
            g_loss = g_loss + lam["lam_adv_op"] * O.adversarial_loss(d_gen)
        g_loss = g_loss + lam["lam_latent"] * g_latent
    gn = [k for k, v in mg.items() if v.requires_grad]
    grads = {"G." + n: g for n, g in zip(gn, torch.autograd.grad(g_loss, [mg[k] for k in gn]))}
    losses = {"g_loss": float(g_loss.detach())}
    if md is not None:
        d_loss = O.discriminate_loss(O.pixel_discriminator(md, t), O.pixel_discriminator(md, pred.detach()))
        dn = [k for k, v in md.items() if v.requires_grad]
        grads.update({"D." + n: g for n, g in zip(dn, torch.autograd.grad(d_loss, [md[k] for k in dn]))})
        losses["d_loss"] = float(d_loss.detach())
    branch = {"idx": idxk.reshape(-1, K).detach(),
              "pool": {**{k[:-5]: v for k, v in aux.items()}, **fpool}}
    return grads, branch, losses


def _single_case(case, batch):
    stream, with_d, lams = CASES[case]
    c = 3 if stream == "rgb" else 2
    sd_g = _stream_state(stream)
    sd_d = S.make_discriminator_state(input_nc=c) if with_d else None
    sd_f = S.make_flownet2sd_state() if stream == "rgb" else None
    rgb_x, op_x, rgb_t, op_t = S.make_clips(batch, 256, 256, tag=f"single-{case}-{batch}")
    x, t = (rgb_x, rgb_t) if stream == "rgb" else (op_x, op_t)
    clips = torch.cat([x.view(batch, -1, c, 256, 256), t[:, None]], 1).to(DEV)
    G = A.get_unet_vq_topk_res(x.shape[1], c, 64, N_EMBED, K)
    G.load_state_dict(sd_g)
    G = G.to(DEV).train()
    opt_g = torch.optim.SGD(G.parameters(), lr=0.0)      # lr 0: both steps run, parameters and gradients stay in place
    if with_d:
        D = A.PixelDiscriminator(c, [128, 256, 512, 512])
        D.load_state_dict(sd_d)
        D = D.to(DEV).train()
        opt_d = torch.optim.SGD(D.parameters(), lr=0.0)
        flow_fn = None
        if sd_f is not None:
            F2 = A.FlowNet2SD()
            F2.load_state_dict(sd_f)
            F2 = F2.to(DEV).eval()
            flow_fn = Hn.flownet_flow_fn(F2)
        out = {}
        gl, dl = Hn.train_step_single_gan(G, D, opt_g, opt_d, clips, flow_fn, outputs=out, **lams)
        g_hip = {"G." + n: p.grad.detach().clone() for n, p in G.named_parameters()}
        g_hip.update({"D." + n: p.grad.detach().clone() for n, p in D.named_parameters()})
    else:
        out = {}
        gl, dl = Hn.train_step_single(G, opt_g, clips, outputs=out, **lams), None
        g_hip = {"G." + n: p.grad.detach().clone() for n, p in G.named_parameters()}
    assert out["pred"].shape == t.shape and sorted(out["terms"]) == sorted(
        {"rgb": ["adv", "gdl", "flow", "int", "latent"], "op": ["int", "latent"], "op_adv": ["adv", "int", "latent"]}[case])
    branch = _hip_branch(G)
    del G, out
    torch.cuda.empty_cache()
    x, t = x.to(DEV), t.to(DEV)

    def step(dtype, device, force):
        g, br, _ = single_step(sd_g, sd_d, sd_f, x, t, stream, lams, dtype, device, force)
        return g, br
    _, _, losses = single_step(sd_g, sd_d, sd_f, x, t, stream, lams, torch.float64, DEV, branch)
    assert abs(float(gl) - losses["g_loss"]) <= 1e-4 * abs(losses["g_loss"]), (float(gl), losses)
    if dl is not None:
        assert abs(float(dl) - losses["d_loss"]) <= 1e-4 * abs(losses["d_loss"]), (float(dl), losses)
    return T.same_branch_verdict(step, g_hip, branch, DEV, "timed_batch" if batch >= 16 else "small_batch",
                                 what=f"single-stream {case} iteration, batch {batch}")


@pytest.mark.parametrize("case", sorted(CASES))
def test_single_stage_iteration_256_batch2_against_the_fp64_truth(case):
    T.assert_ok(_single_case(case, 2))


@pytest.mark.parametrize("case", ["rgb", "op"])
def test_single_stage_iteration_256_batch32_against_the_fp64_truth(case):
    """the batch run_train trains at: every gradient within 1e-3 (norm) of the same-branch truth, entry by entry within
    max(1e-3, 2 x the fp32 witness's own error) per tensor"""
    T.assert_ok(_single_case(case, 32))


# ---- run_train --stage rgb / op end to end ---------------------------------------------------------------------------

N_VIDEOS, N_FRAMES, H, W = 3, 12, 64, 96


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from oracle.pipeline_oracle import write_flo
    root = tmp_path_factory.mktemp("train_single_set")
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:H, 0:W]
    for v in range(N_VIDEOS):
        dr, do = root / "rgb" / f"{v + 1:02d}", root / "op" / f"{v + 1:02d}"
        dr.mkdir(parents=True)
        do.mkdir(parents=True)
        for i in range(N_FRAMES):
            base = 128 + 60 * np.sin((xx + 3 * i + 10 * v) / 9.0)[..., None] * np.cos(yy / 7.0)[..., None]
            img = np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(dr / f"{i:04d}.jpg", quality=90)
        for i in range(N_FRAMES - 1):
            write_flo(str(do / f"{i:04d}.flo"), rng.normal(0, 2, (H, W, 2)).astype(np.float32))
    return str(root / "rgb"), str(root / "op")


def _args(dataset, stage, out, iterations, *extra):
    roots = {"rgb": ["--rgb_root", dataset[0], "--flownet", "synthetic"], "op": ["--op_root", dataset[1]],
             "joint": ["--rgb_root", dataset[0], "--op_root", dataset[1], "--flownet", "synthetic"]}[stage]
    return ["--stage", stage, *roots, "--out", str(out), "--size", "64", "--batch", "4", "--iterations", str(iterations),
            "--save_every", "2", "--log_every", "1", "--workers", "4", *extra]


def _log(out):
    with open(os.path.join(out, "train_log.jsonl")) as fp:
        return [json.loads(ln) for ln in fp]


@pytest.fixture(scope="module")
def runs(dataset, tmp_path_factory):
    base = tmp_path_factory.mktemp("single_runs")
    out = {k: base / k for k in ("rgb_a", "rgb_b", "rgb_c", "op", "op_adv")}
    run_train.main(_args(dataset, "rgb", out["rgb_a"], 4))
    run_train.main(_args(dataset, "rgb", out["rgb_b"], 4))
    run_train.main(_args(dataset, "rgb", out["rgb_c"], 2))
    run_train.main(_args(dataset, "rgb", out["rgb_c"], 4, "--resume"))
    run_train.main(_args(dataset, "op", out["op"], 4))
    run_train.main(_args(dataset, "op", out["op_adv"], 2, "--lam_adv_op", "0.05"))
    return {k: str(v) for k, v in out.items()}


def test_stage_checkpoints_load_strictly_into_the_single_stream_models(runs):
    names = ["step_000003.pth", "step_000005.pth"]
    for run in ("rgb_a", "op"):
        assert sorted(os.listdir(os.path.join(runs[run], "generator"))) == names
        assert sorted(os.listdir(os.path.join(runs[run], "train_state"))) == names
    assert sorted(os.listdir(os.path.join(runs["rgb_a"], "discriminator"))) == names
    assert not os.path.exists(os.path.join(runs["op"], "discriminator"))           # lam_adv_op 0: no discriminator
    assert sorted(os.listdir(os.path.join(runs["op_adv"], "discriminator"))) == ["step_000003.pth"]
    for run, (cin, cout) in (("rgb_a", (12, 3)), ("op", (6, 2)), ("op_adv", (6, 2))):
        G = A.get_unet_vq_topk_res(cin, cout, 64, 256, 2)
        name = "step_000003.pth" if run == "op_adv" else "step_000005.pth"
        G.load_state_dict(torch.load(os.path.join(runs[run], "generator", name), map_location="cpu"), strict=True)
    D = A.PixelDiscriminator(2, [128, 256, 512, 512])
    D.load_state_dict(torch.load(os.path.join(runs["op_adv"], "discriminator", "step_000003.pth"), map_location="cpu"),
                      strict=True)
    st = torch.load(os.path.join(runs["op"], "train_state", "step_000005.pth"), map_location="cpu", weights_only=True)
    assert st["stage"] == "op" and st["g_step"] == 4 and "opt_d" not in st


def test_stage_logs_carry_the_loss_terms_and_the_stream_psnr(runs):
    want = {"rgb_a": ("rgb", ["g_adv", "g_gdl", "g_flow", "g_int", "g_latent", "d_loss", "psnr_rgb"]),
            "op": ("op", ["g_int", "g_latent", "psnr_op"]),
            "op_adv": ("op", ["g_int", "g_latent", "g_adv", "d_loss", "psnr_op"])}
    for run, (stage, keys) in want.items():
        log = _log(runs[run])
        head, steps, done = log[0], [r for r in log if "step" in r], log[-1]
        assert head["event"] == "start" and head["stage"] == stage and done["skipped"] == 0
        assert head[("op" if stage == "rgb" else "rgb") + "_frames"] == 0
        for r in steps:
            for k in ["g_loss", "ms_per_iter", *keys]:
                assert np.isfinite(r[k]), (run, k, r)
            assert ("d_loss" in r) == (run != "op") and ("lr_d" in r) == (run != "op")
            assert not any(k in r for k in ("psnr_rgb", "psnr_op") if k != f"psnr_{stage}")


def test_first_rgb_iteration_equals_train_step_single_gan_on_pipeline_clips(dataset, runs, tmp_path):
    a = run_train.parse(_args(dataset, "rgb", tmp_path, 1))
    vids = P.list_subvideos(dataset[0], None)
    vid, start = P.SingleClipSampler([len(f) for f, _ in vids], 5, seed=a.seed).draw(a.batch)
    clips = torch.stack([P.frames_to_device(torch.from_numpy(np.stack([P.read_image(p) for p in
                                                                       vids[vid[i]][0][start[i]:start[i] + 5]])).to(DEV),
                                            (64, 64)) for i in range(a.batch)])
    G, D, F2 = run_train.build_models(a)
    G, D, flow_fn = run_train.to_device(G, D, F2, a, torch.device(DEV))
    opt_g, opt_d = Hn.adam(G.parameters(), lr=a.lr_g), Hn.adam(D.parameters(), lr=a.lr_d)
    gl, dl = Hn.train_step_single_gan(G, D, opt_g, opt_d, clips, flow_fn, **run_train.lams_of(a))
    first = [r for r in _log(runs["rgb_a"]) if r.get("step") == 1][0]
    assert abs(first["g_loss"] - float(gl)) <= 1e-5 * abs(float(gl)), (first, float(gl))
    assert abs(first["d_loss"] - float(dl)) <= 1e-5 * abs(float(dl)), (first, float(dl))


def test_rgb_stage_resume_ends_where_the_uninterrupted_run_ends(runs):
    """as test_gpu_run_train.py's resume test: two identical runs are not bitwise equal, so the 2 + 2 resume is held to
    the spread of two identical 4-step runs - or, since one pair of runs is a small sample of that noise, to a hundredth
    of what the next clip does to the loss"""
    def state(out):
        return {"G." + k: v for k, v in torch.load(os.path.join(out, "generator", "step_000005.pth")).items()} | \
               {"D." + k: v for k, v in torch.load(os.path.join(out, "discriminator", "step_000005.pth")).items()}
    a, b, c = (state(runs[k]) for k in ("rgb_a", "rgb_b", "rgb_c"))
    la, lb, lc = ([(r["g_loss"], r["d_loss"]) for r in _log(runs[k]) if "step" in r] for k in ("rgb_a", "rgb_b", "rgb_c"))
    assert len(la) == len(lb) == len(lc) == 4
    loss_ab = max(abs(x - y) / abs(x) for ra, rb in zip(la, lb) for x, y in zip(ra, rb))
    loss_ac = max(abs(x - y) / abs(x) for ra, rc in zip(la, lc) for x, y in zip(ra, rc))
    float_keys = [k for k in a if a[k].is_floating_point()]

    def spread(x, y):
        return max(float((x[k].double() - y[k].double()).abs().max()) / (2e-4 if k[0] == "G" else 2e-5) for k in float_keys)
    ab, ac = spread(a, b), spread(a, c)
    # what another clip does to the loss: consecutive iterations of one run (a wrong draw after the resume would move the
    # losses by that much, not by a hundredth of it)
    jump = min(abs(la[i][0] - la[i + 1][0]) / abs(la[i][0]) for i in range(3))
    print(f"rgb stage: identical runs {loss_ab:.2e} / {ab:.3f} lr apart; 2 + 2 resumed vs 4: {loss_ac:.2e} / {ac:.3f} lr; "
          f"next clip {jump:.2e}")
    assert lc[:2] == la[:2] or np.allclose(lc[:2], la[:2], rtol=1e-5, atol=0)
    assert loss_ac <= max(4 * loss_ab, 1e-5, jump / 100)
    assert ac <= max(4 * ab, 24.0)
    for k in a:
        if not a[k].is_floating_point():
            assert torch.equal(a[k], c[k]), k
    assert [r for r in _log(runs["rgb_c"]) if r.get("event") == "start"][1]["resumed"] is True


def test_resume_refuses_a_train_state_of_another_stage(dataset, runs, tmp_path):
    import shutil
    out = tmp_path / "mixed"
    shutil.copytree(runs["op_adv"], out)
    with pytest.raises(SystemExit, match="--stage op, not of --stage rgb"):
        run_train.main(_args(dataset, "rgb", out, 4, "--resume"))


def test_joint_stage_starts_from_the_two_stage_checkpoints(dataset, runs, tmp_path):
    ck_rgb = os.path.join(runs["rgb_a"], "generator", "step_000005.pth")
    ck_op = os.path.join(runs["op"], "generator", "step_000005.pth")
    argv = _args(dataset, "joint", tmp_path / "joint", 1, "--pretrain_rgb", ck_rgb, "--pretrain_op", ck_op)
    G, _, _ = run_train.build_models(run_train.parse(argv))
    sd = G.state_dict()
    for prefix, ck in (("rgb", ck_rgb), ("op", ck_op)):
        for k, v in torch.load(ck, map_location="cpu").items():
            assert torch.equal(sd[f"{prefix}.{k}"], v), (prefix, k)
    done = run_train.main(argv)
    assert done["skipped"] == 0 and np.isfinite(done["last"]["g_loss"]) and np.isfinite(done["last"]["psnr_op"])
