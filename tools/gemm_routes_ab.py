"""Launch-by-launch A/B of two builds of libunet_hip.so (profiles/gemm_routes_ab.txt).

  UNET_HIP_LIB=/path/to/parent.so python tools/gemm_routes_ab.py record parent.json
  python tools/gemm_routes_ab.py record new.json          (the in-tree build)
  python tools/gemm_routes_ab.py compare parent.json new.json
  python tools/gemm_routes_ab.py table parent.json        (no GPU)
  python tools/gemm_routes_ab.py ws ws.json               (no GPU; compare works on its records too)
  python tools/gemm_routes_ab.py production prod.json ID  (one PRODUCTION configuration; a process each)

record: per network x option arm at N = 2, 64 x 64 with fixed seeds, the ordered launch labels
(unet_timing_read) of one training step (forward, BCE + Dice, backward, HipAdamW step =
unet_adamw_repack), of a second forward + backward on the repacked weight images and of one
inference forward; sha256 of the logits, the loss, the gradient / parameter / running-stat
arenas after each step; unet_workspace_size for training 0 and 1.
ws: unet_workspace_size (training 0 and 1) of the eight networks, the CASES of
tests/workspace_cases.py and the PRODUCTION configurations of tests/kernel_cases.py at their own
shapes, under default options and every setting of WS_SETTINGS one at a time.
production: one default-option training step of a PRODUCTION configuration at its own shape and
batch, fixed seeds: the label list and sha256 of the logits, the gradient and running-stat arenas,
added to the JSON file under its id.
compare: exit status 1 if any label list, hash or size differs.
table: the expected-family table of tests/test_gpu_routes.py against a record's label lists.
"""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "thyroid-nodule-image-segmentation-unet-ddti_amd"), REPO,
                os.path.join(REPO, "tests")]

ARMS = [None, "x3", "rg16", "wg16", "wg16t", "wg16_r3", "convt16", "pool_fuse", "head_fuse",
        "dz_in_wgrad", "x3_r3", "rg16_r3", "wgrad_row3"]
# the tile and threshold arms: option settings applied together
TILE_ARMS = [{"rg16_bn_k": 8192}, {"rg16_bn_k": 8192, "rg16_n128_bn": 1}, {"rg16_n128": -1},
             {"rg16_n128": 6}, {"wgrad_row3_big": -1}, {"x3_wtile": 4}]
# name -> (class, out_channels, base_filters, math): the networks of tests/test_gpu_routes.py
NETS = {
    "unet": ("UNet", 1, 64, "fp32"),
    "mod64_f32": ("ModUNet", 1, 64, "fp32"),
    "mod64_bf16": ("ModUNet", 1, 64, "bf16"),
    "mod128_bf16": ("ModUNet", 1, 128, "bf16"),
    "res64_f32": ("ResUNet", 1, 64, "fp32"),
    "res64_bf16": ("ResUNet", 1, 64, "bf16"),
    "mod16_f32": ("ModUNet", 1, 16, "fp32"),
    "mod64_out3": ("ModUNet", 3, 64, "fp32"),
}


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def _arm_id(arm):
    if isinstance(arm, dict):
        return ",".join(f"{k}={v}" for k, v in arm.items())
    return arm or "default"


def _set(rt, arm):
    rt.reset_options()
    for k, v in (arm.items() if isinstance(arm, dict) else [(arm, 0)] if arm else []):
        rt.set_option(k, v)


def _run(name, arm):
    import torch
    import unet_hip
    dev = torch.device("cuda:0")
    cls, out_ch, base, math = NETS[name]
    torch.manual_seed(1234)
    if cls == "UNet":
        m = unet_hip.UNet(1, out_ch)
    else:
        m = getattr(unet_hip, cls)(1, out_ch, base_filters=base, depth=3, mfma_dtype=math)
    m = m.to(dev).train()
    st = m.flatten_()
    rt = st.rt
    _set(rt, arm)
    out = {}
    try:
        g = torch.Generator(device="cpu").manual_seed(77)
        x = torch.rand(2, 1, 64, 64, generator=g).to(dev)
        t = (torch.rand(2, out_ch, 64, 64, generator=g) > 0.5).float().to(dev)
        out["ws"] = [rt.workspace_bytes(2, 64, 64, tr) for tr in (0, 1)]
        opt = unet_hip.HipAdamW(m.parameters(), lr=1e-3)
        rt.timing(True)
        for step in (1, 2):
            opt.zero_grad()
            logits = m(x)
            losses = unet_hip.seg_losses(logits, t)
            loss = losses[0] + losses[1]
            loss.backward()
            if step == 1:
                opt.step()
            torch.cuda.synchronize()
            out[f"labels_train{step}"] = [lab for lab, _, _ in rt.timing_records()]
            out[f"logits{step}"], out[f"loss{step}"] = _sha(logits), _sha(loss)
            out[f"grads{step}"], out[f"params{step}"] = _sha(st.grad_arena), _sha(st.param_arena)
            out[f"bn{step}"] = _sha(st.bn_arena)
        m.eval()
        with torch.no_grad():
            lg = m(x)
        torch.cuda.synchronize()
        out["labels_infer"] = [lab for lab, _, _ in rt.timing_records()]
        out["logits_infer"] = _sha(lg)
    finally:
        rt.timing(False)
        rt.reset_options()
    return out


def record(path):
    import unet_hip
    arms = ARMS + TILE_ARMS
    res = {name: {_arm_id(arm): _run(name, arm) for arm in arms} for name in NETS}
    with open(path, "w") as f:
        json.dump(res, f)
    print(f"{len(NETS) * len(arms)} runs of {unet_hip._lib.LIB_PATH} -> {path}")


def _variant(net):
    from unet_hip import _lib
    return {"unet": _lib.VARIANT_MODEL, "model": _lib.VARIANT_MODEL, "mod": _lib.VARIANT_MOD,
            "ModUNet": _lib.VARIANT_MOD, "UNet": _lib.VARIANT_MODEL, "res": _lib.VARIANT_RES,
            "ResUNet": _lib.VARIANT_RES}[net]


def ws(path):
    import kernel_cases as K
    import workspace_cases as Wc
    from unet_hip import _lib
    from unet_hip.runtime import UNetRuntime
    # (net, out_ch, base, depth, math, (N, H, W))
    cfgs = {f"net/{n}": (c, o, 0 if c == "UNet" else b, 0 if c == "UNet" else 3, m, (2, 64, 64))
            for n, (c, o, b, m) in NETS.items()}
    for c in Wc.CASES:
        model = c.net == "model"
        cfgs[f"case/{Wc.case_id(c)}"] = (c.net, c.out_ch, 0 if model else c.base, 0 if model else c.depth,
                                         c.math, (c.N, c.H, c.W))
    for c in K.PRODUCTION:
        unet = c["net"] == "unet"
        cfgs[f"prod/{c['id']}"] = (c["net"], 1, 0 if unet else c["base"], 0 if unet else c["depth"], c["math"],
                                   c["shape"])
    settings = [None] + [{k: v} for k, vs in Wc.OPTION_VALUES.items() for v in vs] + TILE_ARMS
    res = {}
    for name, (net, out_ch, base, depth, math, shape) in cfgs.items():
        rt = UNetRuntime("cuda:0", 1, out_ch, _variant(net), base, depth,
                         _lib.MATH_BF16 if math == "bf16" else _lib.MATH_F32)  # no device work
        res[name] = {}
        for arm in settings:
            if isinstance(arm, dict) and len(arm) == 1 and rt.get_option(*arm) == next(iter(arm.values())):
                continue  # the default value
            _set(rt, arm)
            res[name][_arm_id(arm)] = {"ws": [rt.workspace_bytes(*shape, tr) for tr in (0, 1)]}
        rt.reset_options()
    with open(path, "w") as f:
        json.dump(res, f)
    print(f"{sum(len(v) for v in res.values())} sizings x 2 of {len(cfgs)} configurations, {_lib.LIB_PATH} -> {path}")


def production(path, cid):
    import kernel_cases as K
    import torch
    import unet_hip
    c = next(c for c in K.PRODUCTION if c["id"] == cid)
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    if c["net"] == "unet":
        m = unet_hip.UNet(1, 1)
    else:
        cls = unet_hip.ResUNet if c["net"] == "res" else unet_hip.ModUNet
        m = cls(1, 1, base_filters=c["base"], depth=c["depth"], mfma_dtype=c["math"])
    m = m.to(dev).train()
    st = m.flatten_()
    rt = st.rt
    rt.reset_options()
    N, H, W = c["shape"]
    g = torch.Generator(device="cpu").manual_seed(77)
    x = torch.rand(N, 1, H, W, generator=g).to(dev)
    t = (torch.rand(N, 1, H, W, generator=g) > 0.5).float().to(dev)
    rt.timing(True)
    try:
        logits = m(x)
        losses = unet_hip.seg_losses(logits, t)
        (losses[0] + losses[1]).backward()
        torch.cuda.synchronize()
        out = {"labels": [lab for lab, _, _ in rt.timing_records()], "logits": _sha(logits),
               "grads": _sha(st.grad_arena), "bn": _sha(st.bn_arena),
               "ws": [rt.workspace_bytes(N, H, W, tr) for tr in (0, 1)]}
    finally:
        rt.timing(False)
    res = json.load(open(path)) if os.path.exists(path) else {}
    res[cid] = {"default": out}
    with open(path, "w") as f:
        json.dump(res, f)
    print(f"{cid}: {len(out['labels'])} timed launches of {unet_hip._lib.LIB_PATH} -> {path}")


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    for net in a:
        for arm in a[net]:
            for k, v in a[net][arm].items():
                w = b[net][arm].get(k)
                if w == v:
                    continue
                bad += 1
                print(f"DIFF {net} {arm} {k}")
                if k.startswith("labels"):
                    first = next((i for i, (p, q) in enumerate(zip(v, w)) if p != q), None)
                    print(f"   lengths {len(v)} {len(w)}; first difference at {first}")
        d = a[net]["default"]
        if "labels_train1" in d:
            print(f"  {net:12s} {len(a[net])} arms; default: {len(d['labels_train1'])} / "
                  f"{len(d['labels_train2'])} / {len(d['labels_infer'])} timed launches (training step / "
                  f"second forward + backward / inference); workspace {d['ws']}")
        else:
            print(f"  {net:28s} {len(a[net])} settings; default: {len(d.get('labels', []))} timed launches; "
                  f"workspace {d['ws']}")
    if set(a) != set(b) or any(set(a[n]) != set(b[n]) for n in a):
        bad += 1
        print("DIFF the two records hold different runs")
    print("identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


def table(path):
    import test_gpu_routes as T
    a = json.load(open(path))
    for name, arm in T.CASES:
        want, preps = T.expected(name, {} if arm == "default" else {arm: 0})
        T.check(a[name][arm]["labels_train1"], want, preps, f"{name} {arm}")
    print(f"{len(T.CASES)} cases of tests/test_gpu_routes.py agree with the labels in {path}")


if __name__ == "__main__":
    cmd, args = sys.argv[1], sys.argv[2:]
    sys.exit({"record": record, "compare": compare, "table": table, "ws": ws,
              "production": production}[cmd](*args) or 0)
