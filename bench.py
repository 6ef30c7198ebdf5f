#!/usr/bin/env python3
"""Throughput of the HIP UNet training step (BASELINE.json metric).

One step = zero_grad -> forward (models/model.py:53-73) -> BCEWithLogits + Dice
(utils/trainer.py:85-90, ratios 1/1) -> backward -> AdamW (utils/trainer.py:41,92), on a
synthetic bs=32 x 1x256x256 batch per GPU (BASELINE config 2; config 3 = 8 ranks x 32),
inputs resident in HBM before the timed region.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
        N > 1 without a launcher: this process starts N rank processes of itself (one per
        GPU, RCCL over xGMI; rank env + 127.0.0.1 rendezvous) and exits with their status
    torchrun --nproc-per-node N bench.py --gpus N ...   (same ranks, started by torchrun)
    BENCH_DIST_BACKEND=gloo python bench.py --gpus 2    (DP rehearsal on one GPU)
    python bench.py --config 4      models/mod.py UNet(base 128, depth 5), 512x512, bs 8
                                    (BASELINE config 4; not the headline metric)

Prints ONE JSON line on rank 0.  ``value`` = images/s of the whole job (sum over ranks,
time = max over ranks) over the K timed steps, ``ms_per_step`` = the wall time of one timed
step.  ``step_ms_median`` / ``step_ms_p90`` are per-step device times (HIP events at the step
boundaries on the launch stream).  A plain run does nothing else: set up, W warm-up steps,
K timed steps, the result line.

``--dump-outputs DIR`` writes what the last timed step computed (rank 0) as DIR/<name>.npy:
``loss`` ([total, bce, dice], float64), ``logits`` (float32, the whole batch), ``bn_stats``
(the BatchNorm running statistics, float32) and fixed seeded samples of the updated
parameters and of their gradients (``param_sample`` / ``grad_sample`` at flat-arena indices
``sample_index``).  Inputs and initial weights are seeded, so two builds run with the same
arguments can be compared output for output.

``--full`` adds what takes runs of its own.  ``roofline`` is for the dominant kernel (most
GPU time in one extra untimed profiling step), from per-launch HIP events recorded on the
launch stream inside the library around that kernel's launches in the timed region:
achieved = algorithmic FLOP of its launches / their summed duration (``--verbose`` prints
the profiling step's per-kernel breakdown).  ``cpu_baseline`` times the CPU oracle
(oracle/unet_ref_cpu.py, a torch-CPU restatement of the reference's step) on a bounded
sample (bs=4, median of 3 steps) on rank 0 only, and ``dice_vs_ref`` compares the HIP
path's first step with it -- the only use of oracle/ here.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md chip table, dense fp32 matrix
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 matrix (no 2:1 sparsity)
# f32 GEMMs on the bf16 matrix cores through exact three-way operand splits (option x3,
# kernels_gemm_x3.hip): six bf16 MFMA products per f32 product
X3_MFMA_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 6
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="2", choices=("2", "4", "res"),
                    help="BASELINE config: 2 = models/model.py UNet (3 = 2 on N ranks), "
                         "4 = models/mod.py UNet(base 128, depth 5) at 512x512; res = "
                         "models/mod.py ResUNet(64, 5) at 512x512, bs 16 (what the reference "
                         "main.py:122 trains; not a BASELINE config)")
    ap.add_argument("--mfma", default="fp32", choices=("fp32", "bf16"),
                    help="config 4 only: conv GEMM arithmetic (BASELINE config 4 is bf16)")
    ap.add_argument("--batch", type=int, default=0, help="images per GPU (default 32 / 8)")
    ap.add_argument("--base", type=int, default=64, help="config res: base_filters (e.g. 32, the "
                    "reference grid's narrow ResUNet; default 64 = main.py's ResUNet())")
    ap.add_argument("--depth", type=int, default=5, help="config res: depth")
    ap.add_argument("--size", type=int, default=0, help="image side (default 256 / 512)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also the profiling step and the dominant kernel's roofline, the CPU "
                         "baseline and dice_vs_ref (off by default: a plain run only times "
                         "the steps)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU oracle")
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--verbose", action="store_true",
                    help="--full: per-kernel / per-layer breakdown of the profiling step on stderr")
    ap.add_argument("--adamw", default="fused", choices=("fused", "plain"),
                    help="fused: AdamW with the next forward's weight repack (unet_adamw_repack, "
                         "the default); plain: unet_adamw + the forward's repack (A/B runs)")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="kernel-schedule option of the native context (unet_set_option; "
                         "A/B runs), repeatable")
    ap.add_argument("--timing", default="dominant", choices=("dominant", "all"),
                    help="per-launch events in the timed region: around the dominant kernel "
                         "only (default) or around every launch")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher plumbing check: every rank prints its rank environment as "
                         "one JSON line and exits (no torch, no GPU)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.verbose and not args.full:
        ap.error("--verbose prints the breakdown of --full's profiling step: add --full")
    return args


_RANK_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_envs(n, port, base=None):
    """Environment of each of the n rank processes `launch` starts (one process per GPU,
    as torch.distributed.run would set it up on one node; rendezvous on 127.0.0.1)."""
    base = dict(os.environ if base is None else base)
    envs = []
    for r in range(n):
        e = dict(base)
        e.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                 LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        envs.append(e)
    return envs


def launch(n, argv):
    """`python bench.py --gpus N` without a launcher: start N fresh child processes of this
    script, one per GPU (the reference drives every GPU from one command through
    nn.DataParallel, utils/trainer.py:28-30).  Nothing here touches torch or the GPU, and
    the children are started with Popen (no exec of the parent).  Rank 0's stdout is the
    children's shared stdout, so its one JSON line is the command's output.  If any rank
    fails the others are stopped (they would wait in a collective) and the exit status is
    non-zero."""
    import signal
    import subprocess
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=e,
                              start_new_session=True)
             for e in rank_envs(n, _free_port())]
    status = 0
    live = list(procs)

    def stop_ranks(signum, frame):
        # the ranks run in sessions of their own, so a SIGTERM / SIGHUP to this launcher (a
        # scheduler's timeout) would not reach them: they would keep their GPUs and wait in a
        # collective.  Forward it to every rank's process group, give them a moment, exit.
        for q in live:
            try:
                os.killpg(q.pid, signal.SIGTERM)
            except ProcessLookupError:
                pass
        deadline = time.time() + 10
        for q in live:
            try:
                q.wait(timeout=max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(q.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
        sys.exit(128 + signum)

    signal.signal(signal.SIGTERM, stop_ranks)
    signal.signal(signal.SIGHUP, stop_ranks)
    try:
        while procs:
            for p in list(procs):
                rc = p.poll()
                if rc is None:
                    continue
                procs.remove(p)
                live.remove(p)
                if rc != 0 and status == 0:
                    status = rc if rc > 0 else 128 - rc
                    print(f"bench.py: rank process {p.pid} exited with {rc}; stopping the "
                          f"other ranks", file=sys.stderr, flush=True)
                    for q in procs:
                        try:
                            os.killpg(q.pid, signal.SIGTERM)
                        except ProcessLookupError:
                            pass
            time.sleep(0.05)
    except KeyboardInterrupt:
        for q in procs:
            try:
                os.killpg(q.pid, signal.SIGTERM)
            except ProcessLookupError:
                pass
        raise
    return status


def cpu_baseline(steps, size, config=2):
    """Oracle step on the host CPU (utils/trainer.py:81-93 restated by oracle/unet_ref_cpu.py:
    forward, BCE + Dice, backward, AdamW).  models/model.py: BASELINE.md's two CPU samples, bs=4
    (median of `steps` steps after one warm-up) and bs=32, the headline batch (one warm-up, one
    timed step: ~13 s each on 16 threads); `value` is the bs=32 rate.  For config 4 one 256x256
    image of mod.py UNet(128, 5) (a quarter of one 512x512 image's work, scaled to images/s of
    the 512x512 workload)."""
    import torch
    from oracle import mod_ref_cpu as MO
    from oracle import unet_ref_cpu as O
    from oracle import weights as Wt
    # the GPU box exposes every host CPU in os.cpu_count() but gives a job a 16-CPU share
    # (OMP_NUM_THREADS is set to it); oversubscribing makes torch CPU ops 20x slower
    threads = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or len(os.sched_getaffinity(0))
    threads = max(1, min(threads, 16, os.cpu_count() or 1))
    torch.set_num_threads(threads)
    cpu_model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass

    def timed(run, P, B, opt, x, t, n):
        first = run(P, B, opt, x, t)  # warm-up (bs=4: also the reference side of dice_vs_ref)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            run(P, B, opt, x, t)
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return first, ts[len(ts) // 2]

    if config == 4:
        side = size // 2
        P = MO.make_params(42, 128, 5)
        B = MO.init_buffers(128, 5)

        def run(P, B, opt, x, t):
            return MO.train_step(P, B, opt, x, t, depth=5)
        opt = O.AdamWState(P, lr=1e-5)
        x = torch.from_numpy(Wt.make_input(21, 1, 1, side, side))
        t = torch.from_numpy(Wt.make_target(21, 1, side, side))
        _, med = timed(run, P, B, opt, x, t, steps)
        return None, {"value": round(0.25 / med, 4), "unit": "images/sec", "cores": threads, "kind": "port",
                      "sample": f"oracle/mod_ref_cpu.py UNet(128, 5) train step (fwd+BCE+Dice+bwd+AdamW), "
                                f"bs=1, 1x{side}x{side} (scaled x0.25 to 512x512 images), median of {steps} "
                                f"steps after 1 warm-up, torch CPU {threads} threads, {cpu_model}"}
    rates, sample = {}, None
    for nb, n in ((4, steps), (32, 1)):
        P = O.make_params(42)
        B = O.init_buffers()
        opt = O.AdamWState(P, lr=1e-5)
        x = torch.from_numpy(Wt.make_input(21, nb, 1, size, size))
        t = torch.from_numpy(Wt.make_target(21, nb, size, size))
        first, med = timed(O.train_step, P, B, opt, x, t, n)
        rates[nb] = round(nb / med, 4)
        if nb == 4:
            sample = (x, t, first)
        del P, B, opt, first
    return sample, {"value": rates[32], "unit": "images/sec", "cores": threads, "kind": "port",
                    "value_bs4": rates[4],
                    "sample": f"oracle/unet_ref_cpu.py train step (fwd+BCE+Dice+bwd+AdamW), 1x{size}x{size}: "
                              f"bs=32 (value; one warm-up, one timed step) and bs=4 (value_bs4; median of "
                              f"{steps} steps after one warm-up), torch CPU {threads} threads, {cpu_model}"}


def dice_vs_ref(sample, dev):
    """BASELINE metric's "Dice vs ref": the first training step of the HIP path on the CPU
    baseline's sample (same counter-hash weights, fresh BN buffers, same 4 images), against
    the oracle's step on the host.  Dice loss (models/loss.py:13-24) and the Dice score of
    the sigmoid > 0.5 masks vs the targets (utils/utils.py:225-251 F1) from both paths."""
    import torch
    import unet_hip
    from oracle import unet_ref_cpu as O
    x, t, ref = sample
    P = O.make_params(42)
    m = unet_hip.UNet(1, 1)
    m.load_state_dict({**P, **O.init_buffers()})
    m = m.to(dev).train()
    logits = m(x.to(dev))
    losses = unet_hip.seg_losses(logits, t.to(dev))
    torch.cuda.synchronize()
    lg = logits.detach().cpu()

    def mask_dice(lgt):
        pm = (torch.sigmoid(lgt) > 0.5)
        tm = t > 0
        tp = (pm & tm).sum().item()
        return 2.0 * tp / max(1, pm.sum().item() + tm.sum().item())
    d_hip, d_ref = float(losses[1].item()), float(ref["dice"].item())
    agree = float(((torch.sigmoid(lg) > 0.5) == (torch.sigmoid(ref["logits"]) > 0.5)).float().mean())
    return {"sample": "first train step, bs=4 1x256x256 (the cpu_baseline sample), oracle weights seed 42",
            "dice_loss": round(d_hip, 8), "dice_loss_ref": round(d_ref, 8),
            "abs_diff": float(f"{abs(d_hip - d_ref):.3g}"),
            "mask_dice": round(mask_dice(lg), 6), "mask_dice_ref": round(mask_dice(ref["logits"]), 6),
            "mask_agreement": round(agree, 8),
            "logits_max_rel": float(f"{float((lg - ref['logits']).abs().max() / ref['logits'].abs().max()):.3g}")}


DUMP_SAMPLE = 1 << 20  # parameters / gradients sampled by --dump-outputs (4 MiB each)


def dump_outputs(path, model, loss, logits, losses):
    """--dump-outputs: what the last timed step handed its caller, as <path>/<name>.npy --
    the losses, the logits, the BatchNorm running statistics, and the updated parameters and
    their gradients at DUMP_SAMPLE fixed (seeded) indices of the flat arenas (config 4 has
    497 M parameters; everything written stays far below 64 MB).  Returns the file names."""
    import numpy as np
    import torch
    st = model.flatten_()
    n = st.param_arena.numel()
    idx = torch.from_numpy(np.sort(np.random.default_rng(12345).integers(0, n, DUMP_SAMPLE)))
    didx = idx.to(st.param_arena.device)
    arrays = {
        "loss": np.array([loss.item(), losses[0].item(), losses[1].item()], dtype=np.float64),
        "logits": logits.detach().float().cpu().numpy(),
        "bn_stats": st.bn_arena.detach().float().cpu().numpy(),
        "sample_index": idx.numpy().astype(np.float64),
        "param_sample": st.param_arena.detach()[didx].float().cpu().numpy(),
        "grad_sample": st.grad_arena.detach()[didx].float().cpu().numpy(),
    }
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(name + ".npy" for name in arrays)


def load_pmc(kernel, config=2, mfma="fp32"):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC summary of this
    workload (profiles/pmc_summary.json: config 2; pmc_summary_c4_<mfma>.json), if any."""
    name = ("pmc_summary.json" if str(config) == "2" else
            f"pmc_summary_c4_{mfma}.json" if str(config) == "4" else f"pmc_summary_{config}.json")
    path = os.path.join(REPO, "profiles", name)
    try:
        d = json.load(open(path))
        return d.get("kernels", {}).get(kernel, {}).get("hbm_bytes_per_launch")
    except (OSError, ValueError):
        return None


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher: this process only starts the ranks (before any torch / HIP call)
        sys.exit(launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} "
                         f"ranks (WORLD_SIZE); n_gpus must equal the rank count")
    if args.dry_run:
        print(json.dumps({"dry_run": True, "argv": sys.argv[1:], "pid": os.getpid(),
                          **{k: os.environ.get(k) for k in _RANK_ENV}}), flush=True)
        fail = os.environ.get("BENCH_DRY_RUN_FAIL_RANK")  # launcher test: one rank fails,
        if fail is not None:                              # the others wait as if in a collective
            if str(rank) == fail:
                sys.exit(3)
            time.sleep(60)
        return
    import torch
    import torch.distributed as dist

    # BENCH_DIST_BACKEND=gloo: rehearsal of the N>1 path with several ranks on one GPU
    # (RCCL refuses two ranks per device); the real runs use "nccl" (= RCCL over xGMI)
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and world > ndev:
        raise SystemExit(f"bench.py: {world} ranks but only {ndev} visible GPU(s); one rank "
                         f"per GPU over RCCL (BENCH_DIST_BACKEND=gloo rehearses on fewer)")
    local = local % ndev if backend != "nccl" and ndev else local
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
        else:
            dist.init_process_group(backend)
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)

    import unet_hip
    from unet_hip.dist import DistributedUNet
    from unet_hip.flops import res_train_flops_per_image, train_flops_per_image

    c4 = args.config == "4"
    cres = args.config == "res"
    args.batch = args.batch or (8 if c4 else 16 if cres else 32)
    args.size = args.size or (512 if c4 or cres else 256)
    torch.manual_seed(42)
    if cres:
        model = unet_hip.ResUNet(1, 1, base_filters=args.base, depth=args.depth).to(dev).train()
    elif c4:
        model = unet_hip.ModUNet(1, 1, base_filters=128, depth=5,
                                 mfma_dtype=args.mfma).to(dev).train()
    else:
        model = unet_hip.UNet(1, 1).to(dev).train()
    opt = unet_hip.HipAdamW(model.parameters(), lr=1e-5)
    if args.adamw == "plain":
        import unet_hip.module as UM
        UM.arena_owner = lambda flat: None
    ddp = DistributedUNet(model, opt) if world > 1 else None
    for kv in args.opt:
        name, _, val = kv.partition("=")
        model.flatten_().rt.set_option(name, int(val))

    g = torch.Generator(device="cpu").manual_seed(1000 + rank)
    B, S = args.batch, args.size
    x = torch.rand(B, 1, S, S, generator=g).to(dev)
    t = (torch.rand(B, 1, S, S, generator=g) > 0.5).float().to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        logits = model(x)
        # DP: the gathered batch's losses (nn.DataParallel semantics), gradients summed
        losses = ddp.losses(logits, t) if ddp is not None else unet_hip.seg_losses(logits, t)
        loss = losses[0] + losses[1]
        loss.backward()
        if ddp is not None:
            ddp.reduce_gradients()
        opt.step()
        return loss, logits, losses

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()

    rt = model._state.rt

    def aggregate(recs):
        """label = family/kernel instance|layer -> per family, kernel instance, layer."""
        fam, kern, layer = {}, {}, {}
        for label, t_ms, flop in recs:
            f, _, rest = label.partition("/")
            k, _, li = rest.partition("|")
            for d, key in ((fam, f), (kern, k or f), (layer, f"{f}|{li}" if li else None)):
                if key is None:
                    continue
                e = d.setdefault(key, [0, 0.0, 0.0])
                e[0] += 1
                e[1] += t_ms
                e[2] += flop
        return fam, kern, layer

    if args.full:
        # 1. one untimed profiling step with an event pair around every launch: the per-kernel
        #    breakdown and which kernel instance dominates the GPU time
        rt.timing(True)
        step()
        torch.cuda.synchronize()
        fam, kern, layer = aggregate(rt.timing_records())
        rt.timing(False)
        # the dominant MFMA kernel: most GPU time among the kernel instances with algorithmic
        # FLOPs (GEMMs; bandwidth passes carry none and have no MFMA roofline)
        dom = max((k for k in kern if kern[k][2] > 0), key=lambda k: kern[k][1])
        # 2. the timed region: events only around the dominant kernel's launches (so the
        #    per-launch markers of ~400 other launches do not inflate the step time)
        rt.timing(True, only=None if args.timing == "all" else f"/{dom}|")
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # step boundaries as HIP events on the launch stream (the library enqueues on torch's
    # current stream): per-step device times for the median / p90
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(args.steps):
        loss, logits, losses = step()
        evs[i + 1].record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if args.full:
        recs = rt.timing_records()
        rt.timing(False)
    if world > 1:
        te = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed = te.item()
    if not torch.isfinite(loss).item():
        raise RuntimeError("non-finite loss")

    images = B * world * args.steps
    value = images / elapsed
    ms = 1000 * elapsed / args.steps
    step_ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps))
    step_med = step_ms[len(step_ms) // 2]
    step_p90 = step_ms[min(len(step_ms) - 1, int(0.9 * len(step_ms)))]
    bf16 = c4 and args.mfma == "bf16"
    if args.full:
        _, kern_t, _ = aggregate(recs)
        prof_steps = 1
        n_l, t_l, f_l = kern_t[dom]
        achieved = f_l / (t_l * 1e-3) / 1e12 if t_l > 0 else 0.0
        per_launch_flop = f_l / n_l
        pmc = load_pmc(dom, args.config, args.mfma)
        conv_flop = (train_flops_per_image(S, S, 128, 5) if c4 else
                     res_train_flops_per_image(S, S, args.base, args.depth) if cres else
                     train_flops_per_image(S, S)) * B

        def kpeak(k):
            """MFMA peak of one kernel instance's arithmetic: x3 kernels (exact 3-way splits on
            the bf16 matrix cores) bf16 / 6; the bf16 network's GEMMs bf16; the rest f32 MFMA."""
            if k.startswith("x3") or k.startswith("wx3"):
                return X3_MFMA_PEAK_TFLOPS
            return BF16_MFMA_PEAK_TFLOPS if bf16 else FP32_MFMA_PEAK_TFLOPS
        x3 = kpeak(dom) == X3_MFMA_PEAK_TFLOPS
        peak = kpeak(dom)
        # the step's conv work runs on several kernel families with different peaks (ResUNet's
        # 32-channel levels and 1x1 skips stay on f32 MFMA beside the x3 GEMMs): price the step
        # against the FLOP-weighted peak of the families that ran it (profiling step's FLOPs)
        fam_flop = {}
        for k, (_, _, fl) in kern.items():
            if fl > 0:
                fam_flop[kpeak(k)] = fam_flop.get(kpeak(k), 0.0) + fl
        tot_flop = sum(fam_flop.values())
        step_peak = tot_flop / sum(fl / pk for pk, fl in fam_flop.items()) if tot_flop else peak
        names = {X3_MFMA_PEAK_TFLOPS: "x3", BF16_MFMA_PEAK_TFLOPS: "bf16", FP32_MFMA_PEAK_TFLOPS: "f32_mfma"}
        peak_mix = {names[pk]: round(fl / tot_flop, 4) for pk, fl in sorted(fam_flop.items())} if tot_flop else {}
        roofline = {"bound": "mfma", "kernel": dom, "achieved": round(achieved, 3),
                    "peak": peak, "unit": "TFLOP/s",
                    "frac": round(achieved / peak, 4),
                    "traffic": pmc, "launches": n_l, "avg_launch_ms": round(t_l / n_l, 4),
                    "flop_per_launch": per_launch_flop,
                    "kernel_share_of_gpu_time": round(kern[dom][1] / max(1e-9, sum(v[1] for v in kern.values())), 4),
                    "step_conv_tflops": round(conv_flop / (ms * 1e-3) / 1e12, 3),
                    "step_conv_frac": round(conv_flop / (ms * 1e-3) / 1e12 / step_peak, 4),
                    "step_peak_tflops": round(step_peak, 2),
                    "step_flop_share_by_arith": peak_mix}
        if x3:
            roofline["peak_note"] = ("f32 GEMM on bf16 MFMA through exact 3-way operand splits: 6 bf16 "
                                     "products per f32 product, so the peak is the bf16 dense peak / 6")
            roofline["fp32_mfma_peak_frac"] = round(achieved / FP32_MFMA_PEAK_TFLOPS, 4)
            roofline["step_conv_fp32_mfma_frac"] = round(conv_flop / (ms * 1e-3) / 1e12 /
                                                         FP32_MFMA_PEAK_TFLOPS, 4)

    if cres:
        metric = f"images/sec fwd+bwd, mod.ResUNet(base {args.base}, depth {args.depth}) {S}x{S}x1 bs={B}/GPU"
        which = ("reference main.py:122" if (args.base, args.depth) == (64, 5)
                 else "reference config/config.yaml grid")
        workload = (f"models/mod.py ResUNet base-{args.base} depth-{args.depth} ({which}), 1x{S}x{S}, "
                    f"bs={B}/GPU, fwd+BCE+Dice+bwd+AdamW, f32 MFMA (not a BASELINE config; "
                    f"step_conv_* over the unpadded FLOPs)")
        mname = f"mod.ResUNet(in=1,out=1,base_filters={args.base},depth={args.depth})"
    elif c4:
        metric = f"images/sec fwd+bwd, mod.UNet(base 128, depth 5) {S}x{S}x1 bs={B}/GPU"
        if bf16:
            workload_note = " (conv GEMMs bf16 MFMA, f32 accumulate)"
        else:
            workload_note = " (conv GEMMs f32 MFMA)"
        workload = (f"models/mod.py UNet base-128 depth-5, 1x{S}x{S}, bs={B}/GPU, "
                    f"fwd+BCE+Dice+bwd+AdamW (BASELINE config 4){workload_note}")
        mname = "mod.UNet(in=1,out=1,base_filters=128,depth=5) 497,438,849 params"
    else:
        metric = "images/sec fwd+bwd, UNet 256x256x1 bs=32/GPU (Dice+BCE, AdamW)"
        if world == 1:
            tag = "BASELINE config 2"
        elif backend == "nccl" and ndev >= world:
            tag = "BASELINE config 3" if (world, B) == (8, 32) else f"config-3 shape on {world} GPUs"
        else:  # several ranks sharing devices over gloo: exercises the DP code path only
            tag = (f"DP rehearsal: {world} ranks on {max(ndev, 1)} GPU(s) over {backend}, "
                   f"not BASELINE config 3")
        gemms = ("f32 GEMMs on bf16 MFMA via exact 3-way operand splits, split f32 accumulators"
                 if model.flatten_().rt.get_option("x3") else "f32 MFMA")
        workload = (f"models/model.py UNet depth-4 base-64, 1x{S}x{S}, bs={B}/GPU, "
                    f"fwd+BCE+Dice+bwd+AdamW ({tag}; {gemms})")
        mname = "UNet(in=1,out=1) 31,042,369 params"
    out = {"metric": metric,
           "value": round(value, 3), "unit": "images/sec", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(ms, 3),
           "step_ms_median": round(step_med, 3), "step_ms_p90": round(step_p90, 3),
           "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "bf16" if bf16 else "fp32",
           "data": "synthetic",
           "config": {"workload": workload, "model": mname, "global_batch": B * world,
                      "image": [1, S, S], "parallelism": f"dp{world}"},
           "ranks": dist.get_world_size() if world > 1 else 1,
           "backend": (("rccl" if backend == "nccl" else backend) if world > 1 else None)}
    assert out["n_gpus"] == out["ranks"], (out["n_gpus"], out["ranks"])
    if rank == 0 and args.dump_outputs:
        out["outputs"] = dump_outputs(args.dump_outputs, model, loss, logits, losses)
    if args.full:
        out["roofline"] = roofline
        if rank == 0 and world == 1 and not args.no_cpu_baseline and not cres:
            sample, out["cpu_baseline"] = cpu_baseline(args.cpu_steps, S, int(args.config))
            if sample is not None:
                out["dice_vs_ref"] = dice_vs_ref(sample, dev)
        elif rank == 0:
            out["cpu_baseline"] = None
    if rank == 0:
        if args.verbose:
            for k, (n, tm, fl) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
                tf = fl / (tm * 1e-3) / 1e12 if tm > 0 and fl > 0 else 0
                print(f"  {k:22s} n={n:5d} {tm / prof_steps:9.3f} ms/step  {tf:7.2f} TF/s",
                      file=sys.stderr)
            for k, (n, tm, fl) in sorted(kern.items(), key=lambda kv: -kv[1][1])[:8]:
                print(f"  [{k}] n={n} {tm / prof_steps:.3f} ms/step", file=sys.stderr)
            print("  per layer (conv i = 0..17, convT 100..103):", file=sys.stderr)
            for k, (n, tm, fl) in sorted(layer.items(), key=lambda kv: -kv[1][1]):
                tf = fl / (tm * 1e-3) / 1e12 if tm > 0 else 0
                print(f"    {k:18s} {tm / prof_steps:8.3f} ms/step {tf:7.2f} TF/s", file=sys.stderr)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
