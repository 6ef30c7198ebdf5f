"""Launch-by-launch A/B of two builds of libunet_hip.so (profiles/gemm_routes_ab.txt).

  UNET_HIP_LIB=/path/to/parent.so python tools/gemm_routes_ab.py record parent.json
  python tools/gemm_routes_ab.py record new.json          (the in-tree build)
  python tools/gemm_routes_ab.py compare parent.json new.json
  python tools/gemm_routes_ab.py table parent.json        (no GPU)

record: per network x option arm at N = 2, 64 x 64 with fixed seeds, the ordered launch labels
(unet_timing_read) of one training step (forward, BCE + Dice, backward, HipAdamW step =
unet_adamw_repack), of a second forward + backward on the repacked weight images and of one
inference forward; sha256 of the logits, the loss, the gradient / parameter / running-stat
arenas after each step; unet_workspace_size for training 0 and 1.
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
    rt.reset_options()
    if arm:
        rt.set_option(arm, 0)
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
    res = {name: {arm or "default": _run(name, arm) for arm in ARMS} for name in NETS}
    with open(path, "w") as f:
        json.dump(res, f)
    print(f"{len(NETS) * len(ARMS)} runs of {unet_hip._lib.LIB_PATH} -> {path}")


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
        print(f"  {net:12s} {len(a[net])} arms; default: {len(d['labels_train1'])} / "
              f"{len(d['labels_train2'])} / {len(d['labels_infer'])} timed launches (training step / "
              f"second forward + backward / inference); workspace {d['ws']}")
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
    sys.exit({"record": record, "compare": compare, "table": table}[cmd](*args) or 0)
