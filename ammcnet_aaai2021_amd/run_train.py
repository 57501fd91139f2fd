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

Several GPUs: one process per GPU under `torchrun` (or plain RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), data parallel:

    torchrun --nproc-per-node N -m ammcnet_aaai2021_amd.run_train --rgb_root DIR --op_root DIR --out RUN \
        --iterations 80000 --batch 32 [--sync_stats] [--resume]

  * `--batch` is the batch of ONE rank: the step trains on `world x batch` clips.  The learning rates are taken as
    given - nothing is scaled with the world size; choose --lr_g / --lr_d for the global batch.
  * ONE global sampler stream: every rank owns the same sampler (`--seed`), draws `world x batch` samples per iteration
    and takes rows [rank * batch, (rank + 1) * batch).  The global batch of an N-rank run with per-rank batch b is, clip
    for clip, the batch of a one-rank run with `--batch N*b` and the same seed; the train state holds one sampler state,
    and a run may be resumed with another world as long as `world x batch` is unchanged (anything else is refused).
  * Every rank fills its own FULL `ClipBank` (ShanghaiTech at 256 x 256 is ~126 GB: it fits one MI355X); `--workers` is
    per rank.  A bank sharded over the ranks is the follow-up, not part of this entry.
  * `--bank_host_gb G` (default 0: off) lets a set larger than the device budget train: what `--bank_budget_gb` does not
    hold goes to a second tier of the bank in pinned host memory, up to G GB (`pipeline.bank_tiers`; one gather launch
    reads both tiers, bit-identical to the all-device gather).  With a host tier the loop prefetches: iteration i takes
    its clips, draws iteration i + 1's indices from the one sampler stream (the same order as without), enqueues their
    gather on the bank's side stream (`ClipBank.prefetch`) and then launches its step.  Measured: a
    bank entirely in host memory costs 1.2 ms per iteration at batch 32, 256 x 256, and the prefetch does not hide it
    yet.  The train state is the same (the sampler state before the draw of the first iteration a resume
    runs), so --resume and the world x batch rule hold unchanged.  EVERY rank pins its own full host tier: N ranks on
    one host cost N x G GB of pinned host memory; sharing the tier between the ranks is not part of this entry.
  * The models are built and seeded alike on every rank and then broadcast from rank 0 (`parallel.broadcast_state`);
    gradients are averaged by one `parallel.BucketedGradReducer` per network, fed stage by stage by the backward.
    BatchNorm and EMA-codebook statistics stay per rank (stock DDP semantics, see parallel.py) unless `--sync_stats`
    shares them (`parallel.sync_statistics`): N ranks x b clips then compute the step of one rank on N*b clips.
  * Rank 0 alone writes the checkpoints, the train state (it gains `world`) and the log, with a barrier behind every
    save; without `--sync_stats` the saved buffers are rank 0's, and every rank continues from them (they are broadcast
    at the save), so that a resumed run goes on exactly as the uninterrupted one.  Logged losses and PSNRs are means over the ranks;
    `clips_per_s` counts the global batch; `skipped` counts the steps all ranks refused together.
  * At every save and at the end a float64 checksum of all parameters is compared across the ranks (averaged gradients
    and the fused Adam keep them bit-identical); ranks that disagree exit loudly, the `done` record says
    `ranks_agree: true`.
  * `--dist_backend gloo` lets several ranks share one GPU (RCCL refuses that): for tests.
No run on more than one physical GPU has been measured yet.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

import torch.distributed as dist

from . import harness, parallel, pipeline, synthetic, train
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
    p.add_argument("--batch", type=int, default=32, help="clips per rank and step (the global batch is world x batch)")
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
    p.add_argument("--workers", type=int, default=8, help="decoder threads of the bank fill (per rank)")
    p.add_argument("--bank_budget_gb", type=float, default=None, help="default: 80%% of the free device memory")
    p.add_argument("--bank_host_gb", type=float, default=0.0,
                   help="pinned host memory (GB, per rank) for the frames the device budget does not hold; 0 = none: a "
                        "set over the device budget is refused")
    p.add_argument("--log_every", type=int, default=10)
    p.add_argument("--save_every", type=int, default=1000)
    p.add_argument("--resume", action="store_true")
    p.add_argument("--precision", choices=("s16", "fp32"), default="s16",
                   help="training kernels of the generator, discriminator and flow network")
    p.add_argument("--deterministic", action="store_true",
                   help="bit-reproducible training (one rank): every weight gradient without atomics, in a fixed summation "
                        "order (`model.deterministic` on the generator and the discriminator; also AMMC_DETERMINISTIC=1); "
                        "recorded in the train state, and --resume refuses a run whose recorded flag differs")
    p.add_argument("--dist_backend", choices=("nccl", "gloo"), default="nccl",
                   help="process group of a multi-rank run: nccl (RCCL), or gloo so that ranks may share one GPU")
    p.add_argument("--sync_stats", action="store_true",
                   help="multi-rank: share the BatchNorm / EMA-codebook statistics (the step of ONE rank on world x batch "
                        "clips); default: per-rank statistics")
    p.add_argument("--fused_loss", action="store_true",
                   help="the intensity / gradient-difference / flow terms of the loss on the library's fused kernels "
                        "(harness.FUSED_LOSS; also AMMC_FUSED_LOSS=1), any --stage; default: the torch chains")
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
    if a.bank_host_gb < 0:
        p.error("--bank_host_gb must be >= 0")
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
    G.deterministic = deterministic_on(a)
    if D is not None:
        D = D.to(dev).train()
        D.precision = a.precision
        D.deterministic = deterministic_on(a)
    flow_fn = None
    if F2 is not None:
        F2 = F2.to(dev).eval()
        F2.precision = a.precision
        flow_fn = harness.flownet_flow_fn(F2)
    return G, D, flow_fn


def deterministic_on(a) -> bool:
    """--deterministic, or the process-wide default AMMC_DETERMINISTIC"""
    return bool(a.deterministic or train.DETERMINISTIC)


def check_resume_deterministic(state: dict, a) -> None:
    """a deterministic run goes on deterministically and the other way round: the flag is part of what a run is"""
    saved = bool(state.get("deterministic", False))
    if saved != deterministic_on(a):
        raise SystemExit(f"--resume: the train state was written {'with' if saved else 'without'} --deterministic and this "
                         f"run is {'deterministic' if deterministic_on(a) else 'not'}: resume it as it was started")


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


def rank_rows(drawn, rank: int, batch: int):
    """rows [rank * batch, (rank + 1) * batch) of every array of a `world x batch` draw: this rank's clips of the step"""
    return tuple(x[rank * batch:(rank + 1) * batch] for x in drawn)


def check_resume_batch(state: dict, world: int, batch: int) -> None:
    """A train state holds ONE sampler stream, consumed `world x batch` samples per iteration: it continues under any
    world that keeps the global batch (2 x 2 -> 1 x 4 or 4 x 1), and under no other."""
    saved_world, saved_batch = int(state.get("world", 1)), int(state["args"]["batch"])
    if saved_world * saved_batch != world * batch:
        raise SystemExit(f"--resume: the train state was written with a global batch of {saved_world * saved_batch} "
                         f"(world {saved_world} x --batch {saved_batch}); this run has {world * batch} (world {world} x "
                         f"--batch {batch}): the sampler stream and the schedule continue only under the same global batch")


def params_checksum(*models) -> torch.Tensor:
    """float64 [2]: the sum and the sum of squares of every parameter of `models`"""
    ps = [p.detach().double() for m in models if m is not None for p in m.parameters()]
    return torch.stack([torch.stack([p.sum() for p in ps]).sum(), torch.stack([(p * p).sum() for p in ps]).sum()])


def ranks_agree(*models) -> bool:
    """the desync guard: MIN and MAX of the parameter checksum over the ranks in one collective ([c, -c] under MAX)"""
    c = params_checksum(*models)
    both = torch.cat([c, -c])
    dist.all_reduce(both, op=dist.ReduceOp.MAX)
    hi, lo = both[:2], -both[2:]
    return bool((hi == lo).all())


def launch_world(env=None) -> int:
    """WORLD_SIZE of the launch environment.  A multi-rank start names every process: WORLD_SIZE > 1 without RANK would
    make each process rank 0 of a group nobody else joins (a wait until the rendezvous times out), so it is refused."""
    env = os.environ if env is None else env
    world = int(env.get("WORLD_SIZE", "1"))
    if world > 1 and "RANK" not in env:
        raise SystemExit(f"WORLD_SIZE={world} without RANK: run_train trains on one GPU per process - start one process per "
                         "GPU with `torchrun --nproc-per-node N -m ammcnet_aaai2021_amd.run_train ...`, or set RANK, "
                         "LOCAL_RANK and WORLD_SIZE (and MASTER_ADDR / MASTER_PORT) for each of them")
    return world


def main(argv=None) -> dict:
    a = parse(argv)
    if a.flownet and a.size % 64:
        raise SystemExit(f"--size {a.size}: FlowNet2-SD needs a multiple of 64 (drop --flownet to train without the flow term)")
    launched = launch_world()
    if not torch.cuda.is_available():
        raise SystemExit("run_train needs a GPU: the HIP path has no CPU fallback")
    rank, world, own_group = 0, 1, False
    if launched > 1:
        own_group = not dist.is_initialized()
        rank, world, dev = parallel.init_distributed(a.dist_backend)
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    try:
        return _train(a, dev, rank, world)
    finally:
        if own_group and dist.is_initialized():
            dist.destroy_process_group()


def _train(a, dev, rank: int, world: int) -> dict:
    os.makedirs(a.out, exist_ok=True)

    bank = pipeline.ClipBank(a.rgb_root, a.op_root, a.size, dev, workers=a.workers, budget_gb=a.bank_budget_gb,
                             rgb_len=harness.RGB_LEN_CLIP, op_len=harness.OP_LEN_CLIP, host_budget_gb=a.bank_host_gb)
    prefetch = bank.host_nbytes > 0                 # exactly when there is a host tier: the all-device loop is untouched
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
        check_resume_batch(resumed, world, a.batch)
        check_resume_deterministic(resumed, a)
        g_step = int(resumed["g_step"])
    G, D, flow_fn = to_device(G, D, F2, a, dev)
    nets = [m for m in (G, D) if m is not None]
    reducers = []
    if world > 1:
        for m in nets:                              # rank 0 wins; then one gradient reducer per network
            parallel.broadcast_state(m, 0)
            reducers.append(parallel.BucketedGradReducer())
            parallel.attach_reducer(m, reducers[-1])
        if a.sync_stats:
            parallel.sync_statistics(G, True)
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
    if a.fused_loss:
        harness.FUSED_LOSS = True
    args_rec = {k: v for k, v in vars(a).items()}

    # the stage, resolved once: its sampler, its step (-> g_loss, d_loss or None), how its train PSNRs are read from the
    # step's outputs and clips (joint: clips = (rgb, op); a single stage: its clips), and whether it logs its loss terms
    if a.stage == "joint":
        sampler = pipeline.ClipSampler(bank.rgb_count, bank.op_count, harness.RGB_LEN_CLIP, harness.OP_LEN_CLIP,
                                       seed=a.seed)
        psnr_names, log_terms = ("psnr_rgb", "psnr_op"), False

        def step(clips, outputs):
            return harness.train_step_gan(G, D, opt_g, opt_d, *clips, flow_fn, outputs=outputs, **lams)

        def psnr_pairs(outputs, clips):
            return (outputs["rgb"], clips[0][:, -1]), (outputs["op"], clips[1][:, -1])
    else:
        count, clip_len = (bank.rgb_count, harness.RGB_LEN_CLIP) if a.stage == "rgb" else (bank.op_count, harness.OP_LEN_CLIP)
        sampler = pipeline.SingleClipSampler(count, clip_len, seed=a.seed, what=a.stage)
        psnr_names, log_terms = (f"psnr_{a.stage}",), True

        if D is None:
            def step(clips, outputs):
                return harness.train_step_single(G, opt_g, clips, outputs=outputs, **lams), None
        else:
            def step(clips, outputs):
                return harness.train_step_single_gan(G, D, opt_g, opt_d, clips, flow_fn, outputs=outputs, **lams)

        def psnr_pairs(outputs, clips):
            return ((outputs["pred"], clips[:, -1]),)
    if resumed is not None:
        sampler.set_state(resumed["sampler"])

    head = {"event": "start", "stage": a.stage, "g_step": g_step, "iterations": a.iterations, "rgb_frames": bank.n_rgb, "op_frames": bank.n_op,
            "sub_videos": len(bank.videos), "bank_GB": round(bank.nbytes / 1e9, 3),
            "bank_device_GB": round(bank.device_nbytes / 1e9, 6), "bank_host_GB": round(bank.host_nbytes / 1e9, 6), "prefetch": prefetch, "fill_seconds": round(bank.fill_seconds, 3),
            "workers": a.workers, "batch": a.batch, "world": world, "global_batch": world * a.batch, "size": a.size,
            "precision": a.precision, "fused_loss": bool(harness.FUSED_LOSS), "sync_stats": bool(a.sync_stats and world > 1),
            "deterministic": deterministic_on(a),
            "flow_term": ("off: no --flownet" if flow_fn is None else f"on ({a.flownet})"), "resumed": resumed is not None}
    log_path = os.path.join(a.out, "train_log.jsonl")

    def emit(rec):                                  # rank 0 alone prints and writes
        if rank != 0:
            return
        line = json.dumps(rec)
        print(line, flush=True)
        with open(log_path, "a") as fp:
            fp.write(line + "\n")

    emit(head)
    skipped = 0
    host_data_s = 0.0
    t_last, it_last, host_last = time.perf_counter(), g_step, 0.0
    t0 = time.perf_counter()

    def draw():                                     # the next iteration's global first frames, as `bank.gather` takes them
        drawn = sampler.draw(world * a.batch)       # ONE global stream: every rank draws the step's whole batch
        idx = bank.global_index(*(rank_rows(drawn, rank, a.batch) if world > 1 else drawn))
        return idx if isinstance(idx, tuple) else (idx,)
    state_before = sampler.get_state()              # the RNG as it stands before the pending draw (what a resume restores)
    pending = draw()
    last = None
    while g_step < a.iterations:
        g_step += 1
        log_now = g_step % a.log_every == 0 or g_step == a.iterations
        th = time.perf_counter()
        clips = bank.gather(*pending)               # joint: (rgb, op); a single stage: its clips
        if prefetch:
            # a host tier: iteration g_step + 1's clips are drawn NOW (the same stream, the same order) and their gather
            # is enqueued on the bank's stream before this step is launched
            state_before = sampler.get_state()
            pending = draw()
            if g_step < a.iterations:
                bank.prefetch(*pending)
        host_data_s += time.perf_counter() - th
        outputs = {} if log_now else None
        try:
            gl, dl = step(clips, outputs)
        except FloatingPointError:
            skipped += 1                            # `_FiniteWatch` refused the step: no update of either network
            gl = dl = None
        if log_now and gl is not None:              # (the outputs may alias engine buffers: read them before the next step)
            psnr = {n: harness.psnr_per_sample(gen, gt).mean() for n, (gen, gt) in zip(psnr_names, psnr_pairs(outputs, clips))}
            # one read of the step's figures (below, behind the next draw); several ranks: their mean (equal batches: the mean over the global batch).
            # A refused step is refused by all ranks together (`_FiniteWatch` votes), so all of them skip this collective
            named = {"g_loss": gl} | ({"d_loss": dl} if D is not None else {}) | \
                    ({f"g_{k}": v for k, v in outputs["terms"].items()} if log_terms else {}) | psnr
            vals = torch.stack([v.detach().float().reshape(()) for v in named.values()])
            if world > 1:
                vals = vals.double()
                dist.all_reduce(vals)
                vals /= world
        # iteration g_step + 1's clips are drawn while the device runs this one
        if not prefetch:
            th = time.perf_counter()
            state_before = sampler.get_state()
            pending = draw()
            host_data_s += time.perf_counter() - th
        sched_g.step()
        if sched_d is not None:
            sched_d.step()
        if log_now:
            figures = dict(zip(named, vals.tolist())) if gl is not None else {}
            rec = {"step": g_step, "g_loss": figures["g_loss"] if gl is not None else None}
            if D is not None:
                rec["d_loss"] = figures["d_loss"] if dl is not None else None
            if log_terms and gl is not None:
                rec.update({k: v for k, v in figures.items() if k.startswith("g_") and k != "g_loss"})
            rec.update({n: figures[n] if gl is not None else None for n in psnr_names})
            rec["lr_g"] = opt_g.param_groups[0]["lr"]
            if D is not None:
                rec["lr_d"] = opt_d.param_groups[0]["lr"]
            now = time.perf_counter()
            n = g_step - it_last
            rec["ms_per_iter"] = round(1e3 * (now - t_last) / n, 3)
            rec["data_host_ms_per_iter"] = round(1e3 * (host_data_s - host_last) / n, 4)
            rec["clips_per_s"] = round(world * a.batch * n / (now - t_last), 2)
            rec["buckets"] = sum(r.last_step_buckets for r in reducers)
            rec["skipped"] = skipped
            t_last, it_last, host_last = now, g_step, host_data_s
            emit(rec)
            last = rec
        if g_step % a.save_every == 0 or g_step == a.iterations:
            if world > 1 and not ranks_agree(*nets):
                raise SystemExit(f"rank {rank}: the parameters differ between the ranks at step {g_step} (checksum MIN != MAX): "
                                 "the run has desynchronised - nothing was saved for this step")
            if rank == 0:
                state = {"stage": a.stage, "g_step": g_step, "world": world, "opt_g": opt_g.state_dict(),
                         "sched_g": sched_g.state_dict(), "sampler": state_before, "skipped": skipped, "args": args_rec,
                         "deterministic": deterministic_on(a)}
                if D is not None:
                    state.update(opt_d=opt_d.state_dict(), sched_d=sched_d.state_dict())
                save_all(a.out, G, D, state, g_step)
            if world > 1:
                # every rank goes on from what was saved: with per-rank statistics the saved buffers (BatchNorm running
                # statistics, the EMA codebook the next forward reads) are rank 0's, and a resumed run, which loads them
                # on every rank, must continue as this one does
                for m in nets:
                    parallel.broadcast_state(m, 0)
                dist.barrier()                      # no rank runs ahead of a resume-visible state
    torch.cuda.synchronize()
    done = {"event": "done", "g_step": g_step, "seconds": round(time.perf_counter() - t0, 3), "skipped": skipped,
            "fill_seconds": round(bank.fill_seconds, 3), "workers": a.workers, "world": world,
            "ranks_agree": True if world == 1 else ranks_agree(*nets), "last": last}
    if not done["ranks_agree"]:
        raise SystemExit(f"rank {rank}: the parameters differ between the ranks at the end of the run (checksum MIN != MAX)")
    emit(done)
    return done


if __name__ == "__main__":
    main()
