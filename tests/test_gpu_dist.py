"""The data-parallel product path on a real GPU: two ranks (gloo, both on cuda:0 -- the
pool's boxes have one GPU, and RCCL refuses two ranks on one device) run the HIP UNet
through ``unet_hip.dist.DistributedUNet``: parameters broadcast from rank 0, per-rank
train-mode BN on its shard (DataParallel's torch.chunk scatter), the loss of the GATHERED
batch (``DistributedUNet.losses``: native loss statistics -> all-reduce of the 8 batch
sums -> native finalize), the native per-bucket events gating the side-stream all-reduce
that SUMS the gradients.  Loss values and summed gradients must match the reference's own
nn.DataParallel fixtures -- BCE + Dice (tests/golden/unet_dp2_64.npz) and the default
FocalTversky mix on equal and unequal shards (tests/golden/unet_dpf_64.npz) -- and both
ranks must hold identical parameters after the AdamW step."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, seed, B, ratios, average):
    import sys
    for p in (REPO, PKG, os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import unet_hip
        from _helpers import hip_model
        from oracle import unet_ref_cpu as O
        from oracle import weights as Wt
        from unet_hip.dist import DistributedUNet
        dev = torch.device("cuda:0")
        # rank 1 starts from different weights: the broadcast must replace them
        m = hip_model(O.make_params(42 if rank == 0 else 7), dev)
        opt = unet_hip.HipAdamW(m.parameters(), lr=1e-5)
        ddp = DistributedUNet(m, opt, average=average)
        x = torch.from_numpy(Wt.make_input(seed, B, 1, 64, 64))
        t = torch.from_numpy(Wt.make_target(seed, B, 64, 64))
        xs, ts = torch.chunk(x, world)[rank].to(dev), torch.chunk(t, world)[rank].to(dev)
        opt.zero_grad(set_to_none=True)
        logits = ddp(xs)
        if average:  # per-rank local losses, averaged gradients
            losses = unet_hip.seg_losses(logits, ts)
        else:        # the gathered batch's losses, summed gradients
            losses = ddp.losses(logits, ts)
        loss = ratios[0] * losses[0] + ratios[1] * losses[1] + ratios[2] * losses[2]
        loss.backward()
        scale = ddp.reduce_gradients()
        grads = m._state.grad_arena.detach().clone() * scale
        opt.step()
        params = m._state.param_arena.detach().clone()
        vals = torch.cat([losses.detach().double(), loss.detach().double().reshape(1)]).cpu()
        if average:
            dist.all_reduce(vals)
            vals /= world
        pd = params.cpu()
        dist.broadcast(pd, src=0)
        same = bool(torch.equal(pd, params.cpu()))
        if rank == 0:
            rt = m._state.rt
            norms = [float(grads[off:off + int(np.prod(shape))].double().norm())
                     for name, shape, off in rt.params]
            q.put((vals.tolist(), norms, scale, same))
        else:
            q.put(("rank1", vals.tolist(), same))
    finally:
        dist.destroy_process_group()


def _run(seed, B, ratios, average):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, seed, B, ratios, average))
             for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=500), q.get(timeout=500)]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    r0 = [r for r in res if r[0] != "rank1"][0]
    r1 = [r for r in res if r[0] == "rank1"][0]
    return r0, r1


@pytest.mark.timeout(600)
def test_dp2_on_gpu_matches_dataparallel_golden(golden_dir):
    """BCE + Dice, equal shards, both DP modes: the gathered-batch loss with summed
    gradients (default) and per-rank local losses with averaged gradients."""
    f = np.load(os.path.join(golden_dir, "unet_dp2_64.npz"), allow_pickle=False)
    for average in (False, True):
        (vals, norms, scale, same0), r1 = _run(3, 4, (1.0, 1.0, 0.0), average)
        assert scale == (0.5 if average else 1.0)
        assert same0 and r1[2], "ranks diverged after the AdamW step"
        assert abs(vals[3] - float(f["loss"])) < 1e-5, (average, vals[3], float(f["loss"]))
        if not average:
            assert vals == r1[1], "ranks disagree on the gathered-batch loss"
        np.testing.assert_allclose(norms, f["grad_norm"], rtol=1e-2)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tag,B,seed", [("eq_", 4, 22), ("uneq_", 3, 23)])
def test_dp2_focal_on_gpu_matches_dataparallel_golden(golden_dir, tag, B, seed):
    """FocalTversky in the DP loss (global TP/FP/FN of the gathered batch): the CLI default
    ratios on equal shards, 1/1/1 on DataParallel's unequal scatter (3 -> 2 + 1)."""
    f = np.load(os.path.join(golden_dir, "unet_dpf_64.npz"), allow_pickle=False)
    ratios = tuple(float(v) for v in f[tag + "ratios"])
    (vals, norms, scale, same0), r1 = _run(seed, B, ratios, False)
    assert scale == 1.0
    assert same0 and r1[2], "ranks diverged after the AdamW step"
    assert vals == r1[1], "ranks disagree on the gathered-batch loss"
    for v, k in zip(vals, ("bce", "dice", "focal", "loss")):
        assert abs(v - float(f[tag + k])) < 1e-5, (k, v, float(f[tag + k]))
    np.testing.assert_allclose(norms, f[tag + "grad_norm"], rtol=1e-2)


def _trainer_worker(rank, world, port, q, tmp):
    import sys
    for p in (REPO, PKG, os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import argparse
        from data.data_loader import DataParallelShardSampler, SyntheticSegmentation, dp_collate
        from models.model import UNet
        from oracle import unet_ref_cpu as O
        from utils.trainer import Trainer
        from utils.utils import Config, create_logger
        torch.cuda.set_device(0)
        ns = argparse.Namespace(model_type="UNet", lr=1e-4, bce_ratio=1.0, dice_ratio=0.0,
                                focal_ratio=1.0, boundary_ratio=0.0, use_mixup=False,
                                mixup_prob=0.0, mixup_alpha=0.2, epochs=1, early_stop_patience=5,
                                batch_size=4, num_workers=0)
        cfg = Config(ns, base_dir=os.path.join(tmp, f"r{rank}"))
        cfg.device = torch.device("cuda:0")
        ds = SyntheticSegmentation(5, 64, seed=4)
        loaders = tuple(torch.utils.data.DataLoader(
            ds, batch_sampler=DataParallelShardSampler(5, 4, False, rank, world), collate_fn=dp_collate())
            for _ in range(3))
        P = O.make_params(42)
        m = UNet()
        m.load_state_dict({**P, **O.init_buffers()})
        tr = Trainer(cfg, loaders, create_logger(os.path.join(cfg.log_dir, "t.log")), m)
        avg = tr.train_one_epoch(0)
        params = tr.model._state.param_arena.detach().cpu().clone()
        pd = params.clone()
        dist.broadcast(pd, src=0)
        same = bool(torch.equal(pd, params))
        q.put((rank, avg, same, params.numpy() if rank == 0 else None))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_trainer_dp2_ragged_last_batch_matches_dataparallel(tmp_path):
    """utils.trainer.Trainer over two ranks, one epoch of 5 samples at batch_size 4 (the
    reference loader's drop_last=False): batch 1 splits 2 + 2, the last batch of one sample
    goes to rank 0 and leaves rank 1's shard empty (it joins the collectives with zeros).
    Loss = the CLI defaults BCE + FocalTversky on the gathered batch.  The epoch loss and
    the parameters after both AdamW steps must match the oracle's nn.DataParallel
    emulation; both ranks must hold identical parameters."""
    from data.data_loader import SyntheticSegmentation
    from oracle import unet_ref_cpu as O
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_trainer_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500), q.get(timeout=500)], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert res[0][2] and res[1][2], "ranks diverged"
    ds = SyntheticSegmentation(5, 64, seed=4)
    xs = torch.stack([ds[i][0] for i in range(5)])
    ts = torch.stack([ds[i][1] for i in range(5)])

    def dp_epoch(dtype, xscale=1.0):
        P = {k: v.to(dtype) for k, v in O.make_params(42).items()}
        B = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in O.init_buffers().items()}
        opt = O.AdamWState(P, lr=1e-4)
        losses = []
        for sl in (slice(0, 4), slice(4, 5)):  # global batches; DataParallel scatters each
            r = O.train_step(P, B, opt, xs[sl].to(dtype) * xscale, ts[sl].to(dtype), w_bce=1.0,
                             w_dice=0.0, w_focal=1.0, shards=2)
            losses.append(float(r["loss"]))
        flat = torch.cat([P[n].reshape(-1) for n, *_ in O.param_spec()]).double().numpy()
        return losses, flat

    losses, ref32 = dp_epoch(torch.float32)
    _, ref32p = dp_epoch(torch.float32, 1 + 1e-7)  # a second fp32 noise realisation
    _, ref64 = dp_epoch(torch.float64)
    want = (4 * losses[0] + 1 * losses[1]) / 5  # AverageMeter over the global batches
    assert abs(res[0][1] - want) < 1e-4, (res[0][1], want)
    # two Adam steps from fp32 gradients: elements whose gradient is rounding noise move by
    # up to lr per step in any fp32 evaluation, so the HIP trajectory is judged against the
    # fp64 one within 2x the fp32 oracle's own deviation from it (the larger of two fp32
    # realisations: x and x * (1 + 1e-7))
    d_hip = np.abs(res[0][3].astype(np.float64) - ref64)
    d_32 = max(np.abs(ref32 - ref64).mean(), np.abs(ref32p - ref64).mean())
    print(f"vs fp64: hip mean {d_hip.mean():.3e} max {d_hip.max():.3e}; "
          f"fp32 oracle mean {np.abs(ref32 - ref64).mean():.3e} / {np.abs(ref32p - ref64).mean():.3e}")
    assert d_hip.max() <= 4 * 1e-4 * 1.01
    assert d_hip.mean() <= 2 * d_32 + 1e-8


def _eval_worker(rank, world, port, q, tmp, tag, lr):
    import sys
    for p in (REPO, PKG, os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import argparse
        from _helpers import check_eval
        from data.data_loader import DataParallelShardSampler, SyntheticSegmentation, dp_collate
        from models.model import UNet
        from oracle import unet_ref_cpu as O
        from utils.trainer import Trainer
        from utils.utils import Config, create_logger
        torch.cuda.set_device(0)
        f = np.load(os.path.join(REPO, "tests", "golden", "unet_dpe_64.npz"), allow_pickle=False)
        ns = argparse.Namespace(model_type="UNet", lr=lr, bce_ratio=1.0, dice_ratio=0.0,
                                focal_ratio=1.0, boundary_ratio=0.0, use_mixup=False,
                                mixup_prob=0.0, mixup_alpha=0.2, epochs=1, early_stop_patience=5,
                                batch_size=4, num_workers=0)
        cfg = Config(ns, base_dir=os.path.join(tmp, f"r{rank}"))
        cfg.device = torch.device("cuda:0")

        def loader(seed, bs):
            return torch.utils.data.DataLoader(
                SyntheticSegmentation(5, 64, seed=seed),
                batch_sampler=DataParallelShardSampler(5, bs, False, rank, world), collate_fn=dp_collate())
        # val: global batches [0..3] -> 2 + 2 and [4] -> 1 + empty; test at batch 2: 1 + 1,
        # 1 + 1 and 1 + empty (Trainer.test must join the count reduction on an empty shard)
        loaders = (loader(4, 4), loader(5, 4), loader(6, 2))
        bufs = O.init_buffers()
        off = 0
        for name in O.BN_LAYERS:
            c = bufs[f"{name}.running_mean"].numel()
            bufs[f"{name}.running_mean"] = torch.from_numpy(f[tag + "init_running_mean"][off:off + c].copy())
            bufs[f"{name}.running_var"] = torch.from_numpy(f[tag + "init_running_var"][off:off + c].copy())
            bufs[f"{name}.num_batches_tracked"] = torch.tensor(30)
            off += c
        m = UNet()
        m.load_state_dict({**O.make_params(42), **bufs})
        tr = Trainer(cfg, loaders, create_logger(os.path.join(cfg.log_dir, "t.log")), m)
        tr.train_one_epoch(0)
        st = tr.model._state
        own = st.bn_arena.detach().clone()
        r0 = own.clone()
        dist.broadcast(r0, src=0)
        drifted = not torch.equal(own, r0)  # rank 1 trained on other shards: its EMA differs
        val_loss, val_iou = tr.validate(0)
        after = st.bn_arena.detach().clone()
        synced = torch.equal(after, r0) and torch.equal(st.nbt_arena.cpu(), torch.full((18,), 32))
        metrics = tr.test()
        # this rank's shards of the val set in eval mode, and the semantic check: the eval
        # forward equals the oracle's resynced from this rank's (now rank 0's) params + buffers
        ds = SyntheticSegmentation(5, 64, seed=5)
        mine = [i for b in loaders[1].batch_sampler for i in b]
        x = torch.stack([ds[i][0] for i in mine])
        t = torch.stack([ds[i][1] for i in mine])
        tr.model.eval()
        with torch.no_grad():
            lg = tr.model(x.to("cuda:0")).cpu().numpy()
        check_eval(tr.model, O.forward, x, t)
        nb = dict(tr.model.named_buffers())
        rs = np.concatenate([nb[f"{n}.running_mean"].cpu().numpy() for n in O.BN_LAYERS] +
                            [nb[f"{n}.running_var"].cpu().numpy() for n in O.BN_LAYERS])
        q.put((rank, drifted, synced, val_loss, val_iou, metrics, mine, lg,
               rs if rank == 0 else None,
               st.param_arena.detach().cpu().numpy() if rank == 0 else None))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tag,lr", [("lr0_", 0.0), ("lr4_", 1e-4)])
def test_trainer_dp2_eval_uses_replica0_buffers(tmp_path, golden_dir, tag, lr):
    """Trainer.validate / Trainer.test over two ranks after a DP training epoch evaluate
    every shard with rank 0's BN running statistics, as nn.DataParallel does (it
    re-replicates module 0, buffers included, for every forward: utils/trainer.py:28-30,
    139, 216), pinned by the reference-generated tests/golden/unet_dpe_64.npz.

    * rank 1's running statistics drift from rank 0's during training (the test is
      sensitive) and equal rank 0's bit for bit after validate();
    * lr = 0 (only the buffers move): eval logits of both ranks' shards vs the fixture at
      1e-4, validation loss at 1e-5, test confusion counts equal the fixture's up to
      pixels inside the forward error band;
    * lr = 1e-4: each rank's eval logits equal the oracle resynced from rank 0's params and
      buffers at 1e-4 (check_eval), the fixture within the two-step trajectory bar."""
    from _helpers import masks_agree, rel_max
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eval_worker, args=(r, 2, port, q, str(tmp_path), tag, lr))
             for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500), q.get(timeout=500)], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    f = np.load(os.path.join(golden_dir, "unet_dpe_64.npz"), allow_pickle=False)
    assert res[1][1], "rank 1's running statistics did not drift: the test would not see a bug"
    assert res[0][2] and res[1][2], "validate() did not give every rank rank 0's BN buffers"
    assert res[0][3] == res[1][3] and res[0][4] == res[1][4], "ranks disagree on val metrics"
    assert res[0][5] == res[1][5], "ranks disagree on test metrics"
    ref_vl = f[tag + "val_logits"]
    got = np.zeros_like(ref_vl)
    for r in res:
        got[r[6]] = r[7]
    rm = np.concatenate([f[tag + "running_mean"], f[tag + "running_var"]])
    n = rm.size // 2
    own = res[0][8]
    print(f"{tag}: val logits vs fixture {rel_max(got, ref_vl):.2e}; running stats "
          f"{np.abs(own - rm).max() / np.abs(rm).max():.2e}")
    lossw = f[tag + "val_losses"]
    want_loss = float((lossw[:, 3] * lossw[:, 4]).sum() / lossw[:, 4].sum())
    if lr == 0.0:
        assert rel_max(got, ref_vl) <= 1e-4
        np.testing.assert_allclose(own, rm, rtol=1e-4, atol=1e-5 * np.abs(rm).max())
        assert abs(res[0][3] - want_loss) < 1e-5, (res[0][3], want_loss)
        tol = 10 * 1e-4 * np.abs(f[tag + "test_logits"]).max()
        near = int((np.abs(f[tag + "test_logits"]) <= tol).sum())
        cm = res[0][5]
        got_c = [cm["TP"], cm["FP"], cm["FN"], cm["TN"]]
        assert sum(abs(int(a) - int(b)) for a, b in zip(got_c, f[tag + "test_counts"])) <= 2 * near, \
            (got_c, f[tag + "test_counts"].tolist(), near)
    else:
        # two Adam steps move rounding-noise gradients' elements by up to lr each, in any
        # fp32 evaluation: the bar is 2x the fp32 oracle's own spread from the fixture over
        # two noise realisations (x and x * (1 + 1e-7)) of the same DataParallel epoch
        from data.data_loader import SyntheticSegmentation
        from oracle import unet_ref_cpu as O

        def stack(seed):
            ds = SyntheticSegmentation(5, 64, seed=seed)
            return (torch.stack([ds[i][0] for i in range(5)]), torch.stack([ds[i][1] for i in range(5)]))
        (xtr, ttr), (xva, _) = stack(4), stack(5)
        spread = 0.0
        for xs in (1.0, 1 + 1e-7):
            P = O.make_params(42)
            B = O.init_buffers()
            off = 0
            for name in O.BN_LAYERS:
                c = B[f"{name}.running_mean"].numel()
                B[f"{name}.running_mean"] = torch.from_numpy(f[tag + "init_running_mean"][off:off + c].copy())
                B[f"{name}.running_var"] = torch.from_numpy(f[tag + "init_running_var"][off:off + c].copy())
                off += c
            opt = O.AdamWState(P, lr=lr)
            for sl in (slice(0, 4), slice(4, 5)):
                O.train_step(P, B, opt, xtr[sl] * xs, ttr[sl], w_bce=1.0, w_dice=0.0, w_focal=1.0, shards=2)
            with torch.no_grad():
                spread = max(spread, rel_max(O.forward(xva, P, B, False).numpy(), ref_vl))
        print(f"lr4_: fp32 oracle spread {spread:.2e}")
        assert rel_max(got, ref_vl) <= max(2 * spread, 1e-4)
        assert abs(res[0][3] - want_loss) < 1e-3, (res[0][3], want_loss)
    assert n == 5888


def _hygiene_worker(rank, world, port, q, tmp):
    import sys
    for p in (REPO, PKG, os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import argparse
        import random
        import unet_hip
        from data.data_loader import DataParallelShardSampler, SyntheticSegmentation, dp_collate
        from models.model import UNet
        from oracle import unet_ref_cpu as O
        from utils.trainer import Trainer
        from utils.utils import Config, create_logger
        torch.cuda.set_device(0)
        # per-rank host RNG streams (main.py seeds augmentations per rank): the mixup
        # decision, lam and permutation must still be rank 0's on every rank
        random.seed(100 + rank)
        np.random.seed(100 + rank)
        ns = argparse.Namespace(model_type="UNet", lr=1e-4, bce_ratio=1.0, dice_ratio=1.0,
                                focal_ratio=0.0, boundary_ratio=0.0, use_mixup=True,
                                mixup_prob=0.5, mixup_alpha=0.2, epochs=1, early_stop_patience=5,
                                batch_size=4, num_workers=0)
        cfg = Config(ns, base_dir=os.path.join(tmp, "exp"), stamp="shared")
        cfg.device = torch.device("cuda:0")

        def loader(n, bs, seed):
            return torch.utils.data.DataLoader(
                SyntheticSegmentation(n, 64, seed=seed),
                batch_sampler=DataParallelShardSampler(n, bs, True, rank, world, seed=3),
                collate_fn=dp_collate())
        # 7 samples at global batch 3: shards 2 + 1 (ragged) and a last batch 1 + empty
        loaders = (loader(7, 3, 4), loader(3, 2, 5), loader(3, 2, 6))
        m = UNet()
        m.load_state_dict({**O.make_params(42), **O.init_buffers()})
        log = os.path.join(tmp, "shared.log")  # the same file for both ranks, as in main.py
        tr = Trainer(cfg, loaders, create_logger(log), m)
        for ep in range(2):
            tr.train_one_epoch(ep)
        tr.validate(0)
        tr.test()
        params = tr.model._state.param_arena.detach().cpu().clone()
        pd = params.clone()
        dist.broadcast(pd, src=0)
        same = bool(torch.equal(pd, params))
        # validate() ran gathered eval losses: they must not license summing the gradients
        # of a per-rank LOCAL loss (DistributedUNet(average=False) refuses it)
        ds = SyntheticSegmentation(2, 64, seed=9)
        x = torch.stack([ds[i][0] for i in range(2)]).to("cuda:0")
        t = torch.stack([ds[i][1] for i in range(2)]).to("cuda:0")
        tr.model.train()
        tr.optimizer.zero_grad(set_to_none=True)
        unet_hip.seg_losses(tr.model(x), t)[0].backward()
        refused = False
        try:
            tr.ddp.reduce_gradients()
        except RuntimeError:
            refused = True
        dist.barrier()
        q.put((rank, same, refused))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_trainer_dp2_mixup_logging_hygiene(tmp_path):
    """Two ranks with different host RNG streams, mixup on (prob 0.5), ragged and empty
    shards (7 samples at global batch 3), two epochs + validate + test: no collective
    mismatch (rank 0's mixup draws are broadcast), identical parameters on both ranks,
    each log line written once to the shared log file (rank 0 only), and a local-loss
    gradient sum after validate() is still refused."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_hygiene_worker, args=(r, 2, port, q, str(tmp_path)))
             for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500), q.get(timeout=500)], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert res[0][1] and res[1][1], "ranks diverged"
    assert res[0][2] and res[1][2], "local-loss gradient sum was not refused after validate()"
    text = open(os.path.join(str(tmp_path), "shared.log")).read()
    assert text.count("Train Epoch: 1,") == 1 and text.count("Train Epoch: 2,") == 1, text
    assert text.count("Test Metrics") == 1, text


def _modres_worker(rank, world, port, q, tag):
    import sys
    for p in (REPO, PKG, os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import unet_hip
        from oracle import mod_ref_cpu as MO
        from oracle import weights as Wt
        from unet_hip.dist import DistributedUNet
        dev = torch.device("cuda:0")
        torch.cuda.set_device(0)
        if tag == "res_":
            m = unet_hip.ResUNet(1, 1, base_filters=64, depth=3)
            P, B = MO.res_make_params(42 if rank == 0 else 7, 64, 3), MO.res_init_buffers(64, 3)
        else:
            m = unet_hip.ModUNet(1, 1, base_filters=64, depth=3)
            P, B = MO.make_params(42 if rank == 0 else 7, 64, 3), MO.init_buffers(64, 3)
        sd = m.state_dict()
        sd.update({k: v.clone() for k, v in P.items()})
        sd.update({k: v.clone() for k, v in B.items()})
        m.load_state_dict(sd)
        m = m.to(dev).train()
        opt = unet_hip.HipAdamW(m.parameters(), lr=1e-4)
        ddp = DistributedUNet(m, opt)  # rank 1's different weights are replaced by rank 0's
        x = torch.from_numpy(Wt.make_input(17, 3, 1, 64, 64))
        t = torch.from_numpy(Wt.make_target(17, 3, 64, 64))
        xs, ts = torch.chunk(x, world)[rank].to(dev), torch.chunk(t, world)[rank].to(dev)
        res = []
        for s in range(2):
            opt.zero_grad(set_to_none=True)
            logits = ddp(xs)
            losses = ddp.losses(logits, ts)
            loss = losses[0] + losses[1]
            loss.backward()
            ddp.reduce_gradients()
            norms = [float(p.grad.detach().double().norm()) for _, p in m.named_parameters()]
            opt.step()
            parts = [torch.zeros(2, 1, 64, 64, device=dev) for _ in range(world)]
            pad = torch.zeros(2, 1, 64, 64, device=dev)
            pad[:logits.shape[0]].copy_(logits.detach())
            dist.all_gather(parts, pad)
            gl = torch.cat([p[:c] for p, c in zip(parts, [2, 1])]).cpu().numpy()
            res.append((gl, [float(v) for v in losses.detach().cpu()], float(loss.item()), norms))
        params = m._state.param_arena.detach().cpu().clone()
        pd = params.clone()
        dist.broadcast(pd, src=0)
        same = bool(torch.equal(pd, params))
        ddp.sync_buffers()
        m.eval()
        with torch.no_grad():
            ev = m(x.to(dev)).cpu().numpy()
        q.put((rank, res, same, ev))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tag", ["res_", "mod_"])
def test_dp2_modres_match_dataparallel_golden(golden_dir, tag):
    """Data parallelism of the networks the reference CLI trains (main.py:122 ResUNet;
    models/mod.py UNet) over two ranks on one GPU (gloo): B = 3 scattered 2 + 1, two AdamW
    steps, against the reference's nn.DataParallel fixture tests/golden/modres_dp_64.npz.
    The gradients are summed bucket by bucket on a side stream that waits on the native
    bucket events; for ResUNet a bucket that fired before conv1's input gradient was ADDED
    into the skip's (E_ADD) would sum an incomplete gradient, so step 0's gradient norms at
    1e-2 pin bucket readiness.  Step 1 (after one Adam step, where rounding-noise gradient
    elements move by up to lr) at the trajectory bars of the single-GPU golden tests."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_modres_worker, args=(r, 2, port, q, tag)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500), q.get(timeout=500)], key=lambda r: r[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    from _helpers import rel_max
    f = np.load(os.path.join(golden_dir, "modres_dp_64.npz"), allow_pickle=False)
    assert res[0][2] and res[1][2], "ranks diverged"
    for s in range(2):
        p = f"{tag}s{s}_"
        gl, l3, loss, norms = res[0][1][s]
        tol = 1e-4 if s == 0 else 2e-3
        assert rel_max(gl, f[p + "logits"]) <= tol, (s, rel_max(gl, f[p + "logits"]))
        assert abs(loss - float(f[p + "loss"])) <= (1e-5 if s == 0 else 1e-4), (s, loss)
        assert res[1][1][s][2] == loss, "ranks disagree on the gathered loss"
        gtol = 1e-2 if s == 0 else 1e-1
        np.testing.assert_allclose(norms, f[p + "grad_norm"], rtol=gtol)
        np.testing.assert_allclose(res[1][1][s][3], norms, rtol=0, atol=0)  # summed on both
    ev = res[0][3]
    assert rel_max(ev, f[tag + "eval_logits"]) <= 2e-3
    np.testing.assert_array_equal(res[0][3], res[1][3])  # replica 0's buffers on every rank


def _wrap_after_step_worker(rank, world, port, q):
    import sys
    import traceback
    for p in (REPO, PKG, os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import unet_hip
        from _helpers import hip_model, inputs
        from oracle import unet_ref_cpu as O
        from unet_hip.dist import DistributedUNet
        dev = torch.device("cuda:0")
        m = hip_model(O.make_params(42 if rank == 0 else 7), dev)
        opt = unet_hip.HipAdamW(m.parameters(), lr=1e-3)
        x, t = inputs(110 + rank, 2, 32, 32)  # its own batch
        opt.zero_grad()
        losses = unet_hip.seg_losses(m(x.to(dev)), t.to(dev))
        (losses[0] + losses[1]).backward()
        opt.step()  # fused: the context now holds the images of this rank's own weights
        DistributedUNet(m, opt)  # rank 0's parameters and buffers replace them
        xe, _ = inputs(112, 2, 32, 32)  # the same input on both ranks
        m.eval()
        with torch.no_grad():
            lg = m(xe.to(dev)).cpu()
        params = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()
        lg0, p0 = lg.clone(), params.clone()
        dist.broadcast(lg0, src=0)
        dist.broadcast(p0, src=0)
        q.put((rank, bool(torch.equal(p0, params)), bool(torch.equal(lg0, lg)),
               float((lg0 - lg).abs().max() / lg0.abs().max())))
    except Exception:
        q.put((rank, "error", traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp2_wrap_after_a_fused_step():
    """DistributedUNet built AFTER the model took a fused AdamW step: the broadcast writes the
    parameters through `.data`, which no version counter sees, so the wrapper declares it.
    Each rank trains one step from its own seed on its own batch, then wraps; rank 1's
    eval-mode logits of a common input and its parameters must then be rank 0's, bit for bit
    (without the declaration rank 1 runs on the images of its pre-broadcast weights)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_wrap_after_step_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500), q.get(timeout=500)], key=lambda r: r[0])
    for p in procs:
        p.join(120)
    for r in res:
        assert r[1] != "error", r[2]
    for p in procs:
        assert p.exitcode == 0
    print("rank 1 vs rank 0: params equal", res[1][1], "logits equal", res[1][2],
          f"max diff {res[1][3]:.2e} of max|ref|")
    assert res[0][1] and res[1][1], "parameters differ after the broadcast"
    assert res[1][2], f"rank 1's logits off by {res[1][3]:.2e} of max|ref|"
