"""Every conv / ConvT / skip GEMM runs on the kernel family the written rules give it.

The runtime decides per layer, once per workspace plan (csrc/runtime.hip make_routes), which of
three kernel families runs its forward, input-gradient and weight-gradient GEMM, and who writes
its operand image.  This test states those rules again, from the channel counts, the math mode
and the options alone (nothing is imported from the runtime), runs one timed training step per
network and option arm at N = 2, 64 x 64, and checks the launch labels against them:

* every conv, ConvT and skip GEMM has exactly one forward, one weight-gradient and one
  input-gradient label (conv 0 and the first residual block's skip are not GEMMs: none; conv 0
  and that block need no input gradient);
* each label names the expected family: ``/x3`` ``/wx3`` (f32 math on split bf16 operands),
  ``/rg16`` ``/wg16`` (LDS-DMA bf16), ``/rowgemm_`` ``/wgrad`` (f32 / register-staged);
* the count of ``prep16`` / ``prep_x3`` launches is the one the rules predict, given which images
  the ConvT and the max-pool write (option convt16: a decoder's first conv has no prep launch).

The rules ("Routes"):
  x3(cin, cout)   = option x3, f32 math, cin % 64 == 0 and cout % 64 == 0
  rg16(C, N)      = bf16 math, option rg16, C % 64 == 0 and N % 128 == 0
  wg16(CA, CB)    = bf16 math, option wg16, CA % 128 == 0 and CB % 128 == 0
  conv / ConvT forward: x3(cin, cout), else rg16(cin, cout), else register-staged
  input gradient: x3(cin, cout), else rg16(cout, cin), else register-staged
  conv weight gradient: x3, else wg16(cin, cout) and rg16(cin, cout), else register-staged
  ConvT weight gradient: x3, else option wg16t and wg16(cin, cout) and rg16(cin, 4 cout) and
                         rg16(cout, cin), else register-staged
  skip GEMMs (residual network): never x3; forward rg16(cin, cout), input gradient
                         rg16(cout, cin), weight gradient wg16 where the block's first conv's is
Depth 3 at 64 x 64 has rows of 64, 32, 16 and 8 pixels, so every tile predicate of the families
is true on one level and false on another.
"""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DEPTH, N, HW = 3, 2, 64

# name -> (class, out_channels, base_filters, math); "unet" is models/model.py (base 64, depth 4)
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
# Each arm is one option set to 0, on the networks where it can change a launch (csrc/
# runtime_internal.h Options): x3, x3_r3, dz_in_wgrad and wgrad_row3 choose among the f32-math
# kernels (x3_conv_on needs f32 math; dz_in_wgrad and wgrad_row3 act on the f32 register-staged
# weight gradient only), ...
F32_ARMS = ("x3", "convt16", "pool_fuse", "head_fuse", "dz_in_wgrad", "x3_r3", "wgrad_row3")
# ... rg16, rg16_r3, wg16, wg16t and wg16_r3 among the bf16-math ones (rg16_on / wg16_on need
# bf16 math); convt16, pool_fuse and head_fuse act on both the x3 and the bf16 path.
BF16_ARMS = ("rg16", "wg16", "wg16t", "wg16_r3", "convt16", "pool_fuse", "head_fuse", "rg16_r3")
CASES = [(n, a) for n, cfg in NETS.items()
         for a in ("default",) + (BF16_ARMS if cfg[3] == "bf16" else F32_ARMS)]
DEFAULTS = dict(x3=1, rg16=1, wg16=1, wg16t=1, convt16=1)

PREFIX = {"x3": ("x3",), "rg16": ("rg16",), "reg": ("rowgemm_",),
          "wx3": ("wx3",), "wg16": ("wg16",), "wreg": ("wgrad",)}


def channels(base, depth):
    """Channels per level as the kernels see them: level 0 the next power of two >= 32, deeper
    levels the next multiple of 32, an odd multiple of 32 from 96 on the next multiple of 64."""
    out = []
    for l in range(depth + 1):
        if l == 0:
            c = 32
            while c < base:
                c *= 2
        else:
            c = ((base << l) + 31) // 32 * 32
            if c % 64 == 32 and c >= 96:
                c += 32
        out.append(c)
    return out


def expected(name, opts):
    """{(site, layer): family} for every GEMM label the step must show once, and the expected
    (prep16, prep_x3) launch counts."""
    cls, _, base, math = NETS[name]
    o = dict(DEFAULTS, **opts)
    depth = 4 if cls == "UNet" else DEPTH
    res, bf16 = cls == "ResUNet", math == "bf16"
    ch = channels(base, depth)

    def x3(cin, cout):
        return bool(o["x3"]) and not bf16 and cin % 64 == 0 and cout % 64 == 0

    def rg(c, n):
        return bf16 and bool(o["rg16"]) and c % 64 == 0 and n % 128 == 0

    def wg(ca, cb):
        return bf16 and bool(o["wg16"]) and ca % 128 == 0 and cb % 128 == 0

    def level(b):
        return b if b <= depth else 2 * depth - b

    def conv_io(i):
        b, lv = i // 2, level(i // 2)
        if i % 2:
            return ch[lv], ch[lv]
        return (1 if b == 0 else ch[b - 1] if b <= depth else 2 * ch[lv]), ch[lv]

    want, fwd_fam, kept = {}, {}, {}
    for i in range(1, 2 * (2 * depth + 1)):
        cin, cout = conv_io(i)
        f = "x3" if x3(cin, cout) else "rg16" if rg(cin, cout) else "reg"
        w = "wx3" if f == "x3" else "wg16" if wg(cin, cout) and rg(cin, cout) else "wreg"
        fwd_fam[i], kept[i] = f, w != "wreg"
        want["conv_fwd", i] = f
        want["conv_dgrad", i] = "x3" if f == "x3" else "rg16" if rg(cout, cin) else "reg"
        want["conv_wgrad", i] = w
    prep = collections.Counter()
    convt_fwd = {}
    for k in range(depth):
        cin, cout = ch[depth - k], ch[depth - k - 1]
        f = "x3" if x3(cin, cout) else "rg16" if rg(cin, cout) else "reg"
        d = "x3" if f == "x3" else "rg16" if rg(cout, cin) else "reg"
        w = ("wx3" if f == "x3" else
             "wg16" if o["wg16t"] and wg(cin, cout) and rg(cin, 4 * cout) and rg(cout, cin) else "wreg")
        convt_fwd[k] = f
        want["convT_fwd", 100 + k], want["convT_dgrad", 100 + k], want["convT_wgrad", 100 + k] = f, d, w
        # its input image in the forward; the concat gradient's up half once in the backward
        prep[f] += f != "reg"
        prep["x3" if w == "wx3" else "rg16"] += w != "wreg" or d == "rg16"
    for b in range(1, 2 * depth + 1):
        if not res:
            break
        cin, cout = conv_io(2 * b)
        want["skip_fwd", b] = "rg16" if rg(cin, cout) else "reg"
        want["skip_dgrad", b] = "rg16" if rg(cout, cin) else "reg"
        want["skip_wgrad", b] = "wg16" if want["conv_wgrad", 2 * b] == "wg16" else "wreg"
    # the convs' own prep passes: one per conv on an image family, except where the max-pool
    # (the next encoder block's first conv: x3 always, bf16 where the image is kept for the
    # weight gradient) or the ConvT and the max-pool (option convt16: a decoder's first conv
    # whose image is kept, the ConvT on the same family) wrote the image; neither in the
    # residual network
    for i in range(1, 2 * (2 * depth + 1)):
        f, b = fwd_fam[i], i // 2
        if f == "reg":
            continue
        by_pool = not res and i % 2 == 0 and 1 <= b <= depth and (f == "x3" or kept[i])
        by_convt = (not res and i % 2 == 0 and b > depth and bool(o["convt16"]) and kept[i] and
                    convt_fwd[b - depth - 1] == f)
        prep[f] += not (by_pool or by_convt)
    return want, (prep["rg16"], prep["x3"])


def check(labels, want, preps, what):
    """The labels of one training step against expected()'s table."""
    seen = collections.Counter()
    for lab in labels:
        site, slash, rest = lab.partition("/")
        if not slash or "|" not in rest:
            continue
        kernel, _, layer = rest.partition("|")
        key = (site, int(layer))
        assert key in want, f"{what}: unexpected GEMM launch {lab}"
        assert kernel.startswith(PREFIX[want[key]]), f"{what}: {lab} is not on family {want[key]}"
        seen[key] += 1
    for key in want:
        assert seen[key] == 1, f"{what}: {key[0]}|{key[1]} launched {seen[key]} times"
    got = (labels.count("prep16"), labels.count("prep_x3"))
    assert got == preps, f"{what}: (prep16, prep_x3) launches {got}, the rules give {preps}"


def timed_step(name, arm):
    import unet_hip
    cls, out_ch, base, math = NETS[name]
    torch.manual_seed(5)
    if cls == "UNet":
        m = unet_hip.UNet(1, out_ch)
    else:
        m = getattr(unet_hip, cls)(1, out_ch, base_filters=base, depth=DEPTH, mfma_dtype=math)
    m = m.to(DEV).train()
    rt = m.flatten_().rt
    old = None if arm == "default" else rt.get_option(arm)
    if old is not None:
        rt.set_option(arm, 0)
    rt.timing(True)
    try:
        x = torch.rand(N, 1, HW, HW, device=DEV)
        t = (torch.rand(N, out_ch, HW, HW, device=DEV) > 0.5).float()
        losses = unet_hip.seg_losses(m(x), t)
        (losses[0] + losses[1]).backward()
        torch.cuda.synchronize()
        return [lab for lab, _, _ in rt.timing_records()]
    finally:
        rt.timing(False)
        if old is not None:
            rt.set_option(arm, old)


@pytest.mark.parametrize("name,arm", CASES, ids=[f"{n}-{a}" for n, a in CASES])
def test_gemm_families_follow_the_rules(name, arm):
    want, preps = expected(name, {} if arm == "default" else {arm: 0})
    labels = timed_step(name, arm)
    check(labels, want, preps, f"{name} {arm}=0")
