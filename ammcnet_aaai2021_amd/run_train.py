"""Training entry, the counterpart of the reference's trainers (Code/run_helper/train_helper.py): frame and / or flow
folders in the reference's layout -> `pipeline.ClipBank` (every frame decoded once, resized once into device memory) ->
per iteration one gather launch -> one training step -> MultiStepLR on the optimisers, as train_helper.py:342-343 steps
them.  The reference's recipe has two stages, both run here (`--stage`):

  1. `--stage rgb` / `--stage op` (`train_single_Helper.train_base`, train_helper.py:1323-1846): one `UNetMem_v7` on its
     own.  rgb: 4 frames -> the 5th, `harness.train_step_single_gan` with a PixelDiscriminator(3) and the optional
     FlowNet2-SD term (`rgb_vq_Loss`).  op: 3 flows -> the 4th, prediction + commit loss (`harness.train_step_single`);
     with `--lam_adv_op` > 0 a PixelDiscriminator(2) on the predicted flow joins (`op_vq_Loss`).
  2. `--stage joint` (the default; train_helper.py:218-420): `twostream`, AMFT bridge included, from the two stage-1
     generators (`--pretrain_rgb`, `--pretrain_op`), `harness.train_step_gan`.

    python -m ammcnet_aaai2021_amd.run_train --stage rgb --rgb_root DIR --out RGB --iterations N [--flownet F.pth.tar]
    python -m ammcnet_aaai2021_amd.run_train --stage op --op_root DIR --out OP --iterations N [--lam_adv_op W]
    python -m ammcnet_aaai2021_amd.run_train --rgb_root DIR --op_root DIR --out RUN --iterations 80000 \\
        [--flownet FlowNet2-SD_checkpoint.pth.tar] [--pretrain_rgb RGB/generator/step_...pth \\
         --pretrain_op OP/generator/step_...pth] [--resume]

Clips follow the reference's draw rules.  Joint (`pipeline.ClipSampler`): per sample an rgb clip of 5 and an
INDEPENDENTLY drawn op clip of 4, each from a uniformly drawn sub-video, one `RandomState(seed)` stream.  A single stage
(`pipeline.SingleClipSampler`, two_stream_dataset.py:287-333): per sample one clip of its kind, drawn the same way.

Outputs, under --out: `generator/step_XXXXXX.pth` and `discriminator/step_XXXXXX.pth` (the reference's `saver` names:
the number is the iteration count + 1, utils.py:182-189), so `run_test --ckpt <out>/generator/step_...pth` loads a joint
generator and `--pretrain_rgb` / `--pretrain_op` take a single stage's (the bare `UNetMem_v7` state dict); the op stage
without a discriminator writes no `discriminator/`.  `train_state/step_XXXXXX.pth` holds the stage, the optimiser and
scheduler states, the sampler's RNG state, `g_step` and the arguments; `train_log.jsonl`, one JSON line per log step
(also printed; a single stage logs its loss terms and its stream's train PSNR).  `--resume` continues from the latest
train_state, of the same stage only.  (The reference restarts `g_step` at 0 on a restart and saves no optimiser state:
resuming here continues the learning-rate schedule and the Adam moments, a deliberate improvement.)

One GPU per process: multi-GPU training from folders (per-rank banks and sampler streams, `parallel.BucketedGradReducer`)
is not built yet.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

from . import harness, pipeline, synthetic
from .discriminator import PixelDiscriminator
from .flownet import FlowNet2SD
from .unet import get_twostream, get_unet_vq_topk_res

LAM_NAMES = tuple(harness.LAMS_ANOPRED)
STAGES = ("joint", "rgb", "op")


def parse(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--stage", choices=STAGES, default="joint",
                   help="joint: twostream (stage 2); rgb / op: one UNetMem_v7 stream on its own (stage 1)")
    p.add_argument("--rgb_root", default=None, help="folder of sub-video folders of frames (jpg/png/.npy); joint, rgb")
    p.add_argument("--op_root", default=None, help="folder of sub-video folders of flows (.flo/.npy); joint, op")
    p.add_argument("--out", required=True, help="run folder: checkpoints, train state, train_log.jsonl")
    p.add_argument("--iterations", type=int, required=True)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--embed_dim", type=int, default=64)
    p.add_argument("--n_embed", type=int, default=256)
    p.add_argument("--k", type=int, default=2)
    p.add_argument("--lr_g", type=float, default=2e-4)
    p.add_argument("--lr_d", type=float, default=2e-5)
    p.add_argument("--milestones", type=int, nargs="*", default=[],
                   help="MultiStepLR milestones (gamma 0.5, both optimisers, stepped every iteration); none = constant")
    for name, val in harness.LAMS_ANOPRED.items():
        p.add_argument(f"--{name}", type=float, default=val)
    p.add_argument("--lam_adv_op", type=float, default=0.0,
                   help="--stage op: weight of the adversarial term on the predicted flow; 0 = no discriminator")
    p.add_argument("--pretrain_rgb", default=None, help="single-stream rgb checkpoint (with --pretrain_op)")
    p.add_argument("--pretrain_op", default=None, help="single-stream op checkpoint (with --pretrain_rgb)")
    p.add_argument("--flownet", default=None,
                   help="FlowNet2-SD .pth.tar (['state_dict']) or 'synthetic'; without it the flow term is off")
    p.add_argument("--seed", type=int, default=2017, help="sampler RandomState seed (the reference's 2017) and torch seed")
    p.add_argument("--workers", type=int, default=8, help="decoder threads of the bank fill")
    p.add_argument("--bank_budget_gb", type=float, default=None, help="default: 80%% of the free device memory")
    p.add_argument("--log_every", type=int, default=10)
    p.add_argument("--save_every", type=int, default=1000)
    p.add_argument("--resume", action="store_true")
    p.add_argument("--precision", choices=("s16", "fp32"), default="s16",
                   help="training kernels of the generator, discriminator and flow network")
    a = p.parse_args(argv)
    need = {"joint": ("rgb_root", "op_root"), "rgb": ("rgb_root",), "op": ("op_root",)}[a.stage]
    for root in ("rgb_root", "op_root"):
        if root in need and getattr(a, root) is None:
            p.error(f"--stage {a.stage} needs --{root}")
        if root not in need and getattr(a, root) is not None:
            p.error(f"--{root} is not read by --stage {a.stage}")
    if a.stage != "joint" and (a.pretrain_rgb is not None or a.pretrain_op is not None):
        p.error("--pretrain_rgb / --pretrain_op load stage-1 generators into --stage joint")
    if a.stage != "op" and a.lam_adv_op != 0:
        p.error("--lam_adv_op applies to --stage op")
    if a.lam_adv_op < 0:
        p.error("--lam_adv_op must be >= 0")
    if a.stage == "op" and a.flownet:
        p.error("--flownet: the flow term belongs to the rgb and joint stages")
    if (a.pretrain_rgb is None) != (a.pretrain_op is None):
        p.error("--pretrain_rgb and --pretrain_op go together")
    if a.iterations <= 0 or a.batch <= 0 or a.log_every <= 0 or a.save_every <= 0:
        p.error("--iterations, --batch, --log_every and --save_every must be positive")
    return a


def lams_of(a) -> dict:
    """the loss weights of the stage"""
    if a.stage != "joint":
        return {n: getattr(a, n) for n in harness.SINGLE_LAMS[a.stage]}
    return {n: getattr(a, n) for n in LAM_NAMES}


def build_models(a):
    """(generator, discriminator or None, FlowNet2-SD or None) in their initial state: the reference's from-scratch init
    (`weights_init_normal` on both networks, torch seeded with --seed) and, with --pretrain_*, the single-stream branches
    on top (`loader_rgb_op_branch`).  A single stage: `get_unet_vq_topk_res(12, 3)` (rgb) / `(6, 2)` (op) and a
    PixelDiscriminator on its output channels - for op only with --lam_adv_op > 0 (models/__init__.py:118-125).  Models
    are returned on the CPU."""
    torch.manual_seed(a.seed)
    if a.stage == "joint":
        G = get_twostream((12, 6), (3, 2), a.embed_dim, a.n_embed, a.k)
        D = PixelDiscriminator(3, [128, 256, 512, 512])
    else:
        cin, cout = (12, 3) if a.stage == "rgb" else (6, 2)
        G = get_unet_vq_topk_res(cin, cout, a.embed_dim, a.n_embed, a.k)
        D = PixelDiscriminator(cout, [128, 256, 512, 512]) if a.stage == "rgb" or a.lam_adv_op > 0 else None
    harness.weights_init_normal(G)
    if D is not None:
        harness.weights_init_normal(D)
    if a.pretrain_rgb:
        harness.load_pretrained_branches(G, a.pretrain_rgb, a.pretrain_op)
    F2 = None
    if a.flownet:
        F2 = FlowNet2SD()
        if a.flownet == "synthetic":
            F2.load_state_dict(synthetic.make_flownet2sd_state())
        else:
            F2.load_state_dict(torch.load(a.flownet, map_location="cpu")["state_dict"])
    return G, D, F2


def to_device(G, D, F2, a, dev):
    G = G.to(dev).train()
    G.train_precision = a.precision
    if D is not None:
        D = D.to(dev).train()
        D.precision = a.precision
    flow_fn = None
    if F2 is not None:
        F2 = F2.to(dev).eval()
        F2.precision = a.precision
        flow_fn = harness.flownet_flow_fn(F2)
    return G, D, flow_fn


def _latest(folder: str):
    names = sorted(n for n in os.listdir(folder) if n.startswith("step_") and n.endswith(".pth")) if os.path.isdir(folder) else []
    return names[-1] if names else None


def save_all(out: str, G, D, state: dict, g_step: int) -> str:
    """generator / discriminator (where there is one) state dicts under the reference's names, then the train state
    under the same name (written last: a train state exists only beside its checkpoints)"""
    harness.save_checkpoint(G.state_dict(), os.path.join(out, "generator"), g_step)
    if D is not None:
        harness.save_checkpoint(D.state_dict(), os.path.join(out, "discriminator"), g_step)
    return harness.save_checkpoint(state, os.path.join(out, "train_state"), g_step)


def main(argv=None) -> dict:
    a = parse(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("run_train trains on one GPU per process; multi-GPU training from folders (per-rank banks and "
                         "sampler streams through parallel.BucketedGradReducer) is not built yet - run it without torchrun")
    if a.flownet and a.size % 64:
        raise SystemExit(f"--size {a.size}: FlowNet2-SD needs a multiple of 64 (drop --flownet to train without the flow term)")
    if not torch.cuda.is_available():
        raise SystemExit("run_train needs a GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(a.out, exist_ok=True)

    bank = pipeline.ClipBank(a.rgb_root, a.op_root, a.size, dev, workers=a.workers, budget_gb=a.bank_budget_gb,
                             rgb_len=harness.RGB_LEN_CLIP, op_len=harness.OP_LEN_CLIP)
    if a.stage == "joint":
        sampler = pipeline.ClipSampler(bank.rgb_count, bank.op_count, harness.RGB_LEN_CLIP, harness.OP_LEN_CLIP,
                                       seed=a.seed)
    elif a.stage == "rgb":
        sampler = pipeline.SingleClipSampler(bank.rgb_count, harness.RGB_LEN_CLIP, seed=a.seed, what="rgb")
    else:
        sampler = pipeline.SingleClipSampler(bank.op_count, harness.OP_LEN_CLIP, seed=a.seed, what="op")

    G, D, F2 = build_models(a)
    g_step, resumed = 0, None
    if a.resume:
        name = _latest(os.path.join(a.out, "train_state"))
        if name is None:
            raise SystemExit(f"--resume: no train state under {os.path.join(a.out, 'train_state')}")
        resumed = torch.load(os.path.join(a.out, "train_state", name), map_location="cpu", weights_only=True)
        if resumed.get("stage", "joint") != a.stage:
            raise SystemExit(f"--resume: {os.path.join(a.out, 'train_state', name)} is a train state of --stage "
                             f"{resumed.get('stage', 'joint')}, not of --stage {a.stage}")
        G.load_state_dict(torch.load(os.path.join(a.out, "generator", name), map_location="cpu"), strict=True)
        if D is not None:
            D.load_state_dict(torch.load(os.path.join(a.out, "discriminator", name), map_location="cpu"), strict=True)
        g_step = int(resumed["g_step"])
        sampler.set_state(resumed["sampler"])
    G, D, flow_fn = to_device(G, D, F2, a, dev)
    opt_g = harness.adam(G.parameters(), lr=a.lr_g)
    sched_g = torch.optim.lr_scheduler.MultiStepLR(opt_g, milestones=a.milestones, gamma=0.5)
    opt_d = sched_d = None
    if D is not None:
        opt_d = harness.adam(D.parameters(), lr=a.lr_d)
        sched_d = torch.optim.lr_scheduler.MultiStepLR(opt_d, milestones=a.milestones, gamma=0.5)
    if resumed is not None:
        opt_g.load_state_dict(resumed["opt_g"])
        sched_g.load_state_dict(resumed["sched_g"])
        if D is not None:
            opt_d.load_state_dict(resumed["opt_d"])
            sched_d.load_state_dict(resumed["sched_d"])
    lams = lams_of(a)
    args_rec = {k: v for k, v in vars(a).items()}

    head = {"event": "start", "stage": a.stage, "g_step": g_step, "iterations": a.iterations, "rgb_frames": bank.n_rgb, "op_frames": bank.n_op,
            "sub_videos": len(bank.videos), "bank_GB": round(bank.nbytes / 1e9, 3), "fill_seconds": round(bank.fill_seconds, 3),
            "workers": a.workers, "batch": a.batch, "size": a.size, "precision": a.precision,
            "flow_term": ("off: no --flownet" if flow_fn is None else f"on ({a.flownet})"), "resumed": resumed is not None}
    log_path = os.path.join(a.out, "train_log.jsonl")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(log_path, "a") as fp:
            fp.write(line + "\n")

    emit(head)
    psnr_names = ("psnr_rgb", "psnr_op") if a.stage == "joint" else (f"psnr_{a.stage}",)
    skipped = 0
    host_data_s = 0.0
    t_last, it_last, host_last = time.perf_counter(), g_step, 0.0
    t0 = time.perf_counter()

    def draw():                                     # the next iteration's global first frames, as `bank.gather` takes them
        idx = bank.global_index(*sampler.draw(a.batch))
        return idx if a.stage == "joint" else (idx,)
    state_before = sampler.get_state()              # the RNG as it stands before the pending draw (what a resume restores)
    pending = draw()
    last = None
    while g_step < a.iterations:
        g_step += 1
        log_now = g_step % a.log_every == 0 or g_step == a.iterations
        th = time.perf_counter()
        clips = bank.gather(*pending)               # joint: (rgb, op); a single stage: its clips
        host_data_s += time.perf_counter() - th
        outputs = {} if log_now else None
        try:
            if a.stage == "joint":
                gl, dl = harness.train_step_gan(G, D, opt_g, opt_d, *clips, flow_fn, outputs=outputs, **lams)
            elif D is not None:
                gl, dl = harness.train_step_single_gan(G, D, opt_g, opt_d, clips, flow_fn, outputs=outputs, **lams)
            else:
                gl, dl = harness.train_step_single(G, opt_g, clips, outputs=outputs, **lams), None
        except FloatingPointError:
            skipped += 1                            # `_FiniteWatch` refused the step: no update of either network
            gl = dl = None
        if log_now and gl is not None:              # (the outputs may alias engine buffers: read them before the next step)
            if a.stage == "joint":
                psnr = {"psnr_rgb": harness.psnr_per_sample(outputs["rgb"], clips[0][:, -1]).mean(),
                        "psnr_op": harness.psnr_per_sample(outputs["op"], clips[1][:, -1]).mean()}
            else:
                psnr = {f"psnr_{a.stage}": harness.psnr_per_sample(outputs["pred"], clips[:, -1]).mean()}
                terms = outputs["terms"]
        # iteration g_step + 1's clips are drawn while the device runs this one
        th = time.perf_counter()
        state_before = sampler.get_state()
        pending = draw()
        host_data_s += time.perf_counter() - th
        sched_g.step()
        if sched_d is not None:
            sched_d.step()
        if log_now:
            rec = {"step": g_step, "g_loss": float(gl) if gl is not None else None}
            if D is not None:
                rec["d_loss"] = float(dl) if dl is not None else None
            if a.stage != "joint" and gl is not None:
                rec.update({f"g_{k}": float(v) for k, v in terms.items()})
            rec.update({n: float(psnr[n]) if gl is not None else None for n in psnr_names})
            rec["lr_g"] = opt_g.param_groups[0]["lr"]
            if D is not None:
                rec["lr_d"] = opt_d.param_groups[0]["lr"]
            now = time.perf_counter()
            n = g_step - it_last
            rec["ms_per_iter"] = round(1e3 * (now - t_last) / n, 3)
            rec["data_host_ms_per_iter"] = round(1e3 * (host_data_s - host_last) / n, 4)
            rec["skipped"] = skipped
            t_last, it_last, host_last = now, g_step, host_data_s
            emit(rec)
            last = rec
        if g_step % a.save_every == 0 or g_step == a.iterations:
            state = {"stage": a.stage, "g_step": g_step, "opt_g": opt_g.state_dict(), "sched_g": sched_g.state_dict(),
                     "sampler": state_before, "skipped": skipped, "args": args_rec}
            if D is not None:
                state.update(opt_d=opt_d.state_dict(), sched_d=sched_d.state_dict())
            save_all(a.out, G, D, state, g_step)
    torch.cuda.synchronize()
    done = {"event": "done", "g_step": g_step, "seconds": round(time.perf_counter() - t0, 3), "skipped": skipped,
            "fill_seconds": round(bank.fill_seconds, 3), "workers": a.workers, "last": last}
    emit(done)
    return done


if __name__ == "__main__":
    main()
