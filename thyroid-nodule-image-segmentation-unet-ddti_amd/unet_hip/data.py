"""Device-side input pipeline: the reference's Resize + ToTensor (utils/transforms.py:
143-156, applied per sample by data/data_loader.py:20-27) on the GPU.

The reference resizes every image AND mask with ``TF.resize`` -- for PIL images that is
Pillow's ``Image.resize(size, BILINEAR)`` (masks too: they become soft targets) -- and
then ``TF.to_tensor`` = float(u8) / 255.  Here the host only decodes (JPEG -> uint8), the
uint8 planes travel to HBM (1 B/pixel instead of 4), and ``unet_resize_u8`` produces the
fp32 batch directly, bit-identical to Pillow (tests/test_gpu_data.py).

    pipe = GpuResizeToTensor((512, 512), device="cuda")
    x, t = pipe(images, masks)           # lists of HxW uint8 arrays / tensors (any sizes)
                                         # -> (N, 1, 512, 512) fp32 each, on the device

Palette ("P") and bilevel ("1") images: Pillow's Image.resize switches to NEAREST for
those modes whatever filter is asked for.  Planes tagged ``resample="nearest"``
(data.data_loader.DecodeU8 does that) run the same kernel with a one-tap plan: source
index = int(x0), x0 = s/2 then += s per output pixel (s = in/out, Pillow's accumulated
double coordinate of ImagingScaleAffine), coefficient 1.0 in 22-bit fixed point.

Training augmentations (``pipe(images, masks, aug=records)``): the host workers draw each
sample's Flip / Rotate / AdjustBrightness / TGCAugment / CLAHE decisions
(utils.transforms.RecordAugment, the same RNG calls in the same order as the host chain) into
an ``AugRecord``; ``unet_augment_u8`` and ``unet_clahe_u8`` apply them to the uint8 planes on
the device before the resize, bit-identically to Pillow and the NumPy classes
(tests/test_aug_cpu.py, tests/test_gpu_augment.py).  The rotation matrix is formed here with
Python's own ``round`` and ``math``, exactly as Pillow's Image.rotate does, and reaches the
kernel as six 16.16 fixed-point integers.

With ``build_train_transform(cfg, device_augment="all")`` the record also carries the float64
fields of ElasticDeform (``elastic``: alpha, the 17 Gaussian taps computed in Python, and the
two ``np.random.rand`` fields) and SpeckleNoise (``speckle``: the ``np.random.normal`` field),
still drawn on the host so the MT19937 streams stay where they are.  They are uploaded with the
planes; ``unet_elastic_u8`` deforms image and mask under the one map before everything else,
and ``unet_augment_noise_u8`` is the point launch with the speckle step between the brightness
table and the TGC gain (tests/test_elastic_cpu.py, tests/test_gpu_elastic.py).
"""
import ctypes
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from .runtime import UNetRuntime


def resize_plan(in_size, out_size):
    """Pillow's coefficients (int32 [out, ksize]) and bounds (int32 [out, 2]) for one axis."""
    lib = _lib.load()
    ks = ctypes.c_int()
    _lib.check(lib.unet_resize_plan(in_size, out_size, None, None, ctypes.byref(ks)), None,
               "unet_resize_plan")
    k = np.zeros((out_size, ks.value), np.int32)
    b = np.zeros((out_size, 2), np.int32)
    _lib.check(lib.unet_resize_plan(in_size, out_size, k.ctypes.data, b.ctypes.data,
                                    ctypes.byref(ks)), None, "unet_resize_plan")
    return k, b


def nearest_plan(in_size, out_size):
    """One-tap plan reproducing Pillow's NEAREST scale (coefficient 1 << 22 at the nearest
    source index)."""
    k = np.full((out_size, 1), 1 << 22, np.int32)
    b = np.ones((out_size, 2), np.int32)
    step = float(in_size) / out_size
    xo = step * 0.5
    for x in range(out_size):
        b[x, 0] = min(int(xo), in_size - 1)
        xo += step
    return k, b


def _fix(v):
    """Pillow's FIX (Geometry.c): 16.16 fixed point, rounded half up."""
    return int(math.floor(v * 65536.0 + 0.5))


def rotate_plan(w, h, angle):
    """(mode, six int32) of Image.rotate(angle, NEAREST, expand=False, fillcolor=0) on a
    w x h image: Pillow's Python (Image.rotate: transposes for 0 / 180 and, for square images,
    90 / 270; else the rounded rotation matrix about the centre) and the coefficients its
    affine_fixed transform derives from that matrix."""
    angle = angle % 360.0
    zero = [0] * 6
    if angle == 0:
        return _lib.ROT_NONE, zero
    if angle == 180:
        return _lib.ROT_180, zero
    if angle in (90, 270) and w == h:
        return (_lib.ROT_90 if angle == 90 else _lib.ROT_270), zero
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0,
         round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    return _lib.ROT_AFFINE, [_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
                             _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def brightness_lut(factor):
    """ImageEnhance.Brightness(img).enhance(factor) of an "L" image as a 256-entry table:
    Pillow's ImagingBlend of a black image and the image, float32 factor * float32 value,
    0 at or below 0, 255 at or above 255, truncated in between."""
    t = np.float32(factor) * np.arange(256, dtype=np.float32)
    lut = np.zeros(256, np.uint8)
    mid = (t > 0) & (t < 255)
    lut[mid] = np.trunc(t[mid]).astype(np.uint8)
    lut[t >= 255] = 255
    return lut


_IDENTITY_LUT = np.arange(256, dtype=np.uint8)


@dataclasses.dataclass
class AugRecord:
    """One sample's augmentation draws (utils.transforms.RecordAugment): plain Python values,
    picklable, in the chain's order Flip -> Rotate -> AdjustBrightness -> TGCAugment -> CLAHE.
    ``None`` = that augmentation was not drawn (or is not on the device side of the chain)."""
    flip_h: bool = False
    flip_v: bool = False
    angle: float = None        # Rotate: degrees
    brightness: float = None   # AdjustBrightness: factor
    tgc: tuple = None          # TGCAugment: the num_bins gains
    clahe: tuple = None        # CLAHE: (clip, (gx, gy))
    # device_augment="all": the float64 fields the host drew, (h, w) ndarrays.  Left out of ==
    # (an ndarray has no truth value); without them the record compares and pickles as before.
    # ElasticDeform, first in the chain: (alpha, the Gaussian taps, rx, ry)
    elastic: tuple = dataclasses.field(default=None, compare=False)
    # SpeckleNoise, between AdjustBrightness and TGCAugment: the noise field
    speckle: np.ndarray = dataclasses.field(default=None, compare=False)

    def geometric(self):
        return self.flip_h or self.flip_v or self.angle is not None

    def elastic_params(self):
        """unet_elastic_params of the elastic draw."""
        alpha, taps = self.elastic[:2]
        p = _lib.ElasticParams()
        if len(taps) > 31:
            raise _lib.HipError(f"elastic blur of {len(taps)} taps: UNET_ERR_INVALID (31)")
        p.ksize, p.alpha = len(taps), float(alpha)
        p.k[:len(taps)] = [float(k) for k in taps]
        return p

    def params(self, h, w, is_mask):
        """unet_aug_params of an (h, w) plane, or None when the launch would copy (the mask
        takes the geometry only)."""
        point = not is_mask and (self.brightness is not None or self.tgc is not None or
                                 self.speckle is not None)
        if not (self.geometric() or point):
            return None
        p = _lib.AugParams()
        p.flip_h, p.flip_v = int(self.flip_h), int(self.flip_v)
        if self.angle is not None:
            p.mode, a = rotate_plan(w, h, self.angle)
            p.a[:] = a
        lut = _IDENTITY_LUT
        if not is_mask and self.brightness is not None:
            lut = brightness_lut(self.brightness)
        ctypes.memmove(p.lut, lut.ctypes.data, 256)
        if not is_mask and self.tgc is not None:
            if len(self.tgc) > 64:
                raise _lib.HipError(f"TGC with {len(self.tgc)} bands: UNET_ERR_UNSUPPORTED (64)")
            p.num_bins = len(self.tgc)
            p.gain[:len(self.tgc)] = [float(np.float32(g)) for g in self.tgc]
        return p


def _host_plane(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("expected an (H, W) uint8 plane")
    return a


def _field(a, h, w):
    """An (h, w) float64 field of a record, C-contiguous."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (h, w):
        raise ValueError(f"a field of shape {a.shape} for a {(h, w)} plane")
    return a


def apply_augment_host(plane, record, is_mask=False):
    """The device chain of ``record`` on one (H, W) uint8 plane through the host hooks
    (unet_elastic_u8_host, unet_augment_u8_host / unet_augment_noise_u8_host,
    unet_clahe_u8_host: the kernels' own source compiled for the host).  Keeps the plane's
    ``resample`` tag."""
    lib = _lib.load()
    src = _host_plane(plane)
    h, w = src.shape
    if record.elastic is not None:
        rx, ry = (_field(f, h, w) for f in record.elastic[2:])
        dst = np.empty_like(src)
        s, d = ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data)
        _lib.check(lib.unet_elastic_u8_host(None if is_mask else s, s if is_mask else None, h, w,
                                            None if is_mask else d, d if is_mask else None,
                                            rx.ctypes.data, ry.ctypes.data,
                                            ctypes.byref(record.elastic_params())),
                   None, "unet_elastic_u8_host")
        src = dst
    p = record.params(h, w, is_mask)
    if p is not None and not is_mask and record.speckle is not None:
        noise = _field(record.speckle, h, w)
        dst = np.empty_like(src)
        _lib.check(lib.unet_augment_noise_u8_host(src.ctypes.data, h, w, dst.ctypes.data,
                                                  ctypes.byref(p), noise.ctypes.data),
                   None, "unet_augment_noise_u8_host")
        src = dst
    elif p is not None:
        dst = np.empty_like(src)
        _lib.check(lib.unet_augment_u8_host(src.ctypes.data, h, w, dst.ctypes.data,
                                            ctypes.byref(p)), None, "unet_augment_u8_host")
        src = dst
    if not is_mask and record.clahe is not None:
        clip, (gx, gy) = record.clahe
        dst = np.empty_like(src)
        _lib.check(lib.unet_clahe_u8_host(src.ctypes.data, h, w, dst.ctypes.data, float(clip),
                                          int(gx), int(gy)), None, "unet_clahe_u8_host")
        src = dst
    if hasattr(plane, "resample"):
        src = src.view(type(plane))
        src.resample = plane.resample
    return src


class GpuResizeToTensor:
    """Batched Resize((H, W)) + ToTensor of (image, mask) pairs on the device, after the
    samples' recorded augmentations when ``aug`` is given."""

    def __init__(self, size, device="cuda"):
        self.oh, self.ow = (size, size) if isinstance(size, int) else tuple(size)
        self.device = torch.device(device)
        self.rt = UNetRuntime.get(self.device)
        self._plans = {}
        self._u8 = None  # intermediate planes of the augmentations (reused, stream-ordered)

    def _plan(self, n_in, n_out, nearest=False):
        key = (n_in, n_out, nearest)
        if key not in self._plans:
            k, b = nearest_plan(n_in, n_out) if nearest else resize_plan(n_in, n_out)
            self._plans[key] = (torch.from_numpy(k).to(self.device),
                                torch.from_numpy(b).to(self.device), k.shape[1])
        return self._plans[key]

    def _upload(self, img):
        if isinstance(img, np.ndarray):  # PIL-backed arrays are read-only views
            img = np.require(img, requirements=["C", "W"])
        t = torch.as_tensor(img)
        if t.dtype != torch.uint8 or t.dim() != 2:
            raise ValueError("expected an (H, W) uint8 image (decoded 'L' mode)")
        return t.to(self.device, non_blocking=True).contiguous()

    def upload(self, img):
        """One decoded (H, W) uint8 frame on the device (a device tensor is returned as it is)."""
        return self._upload(img)

    def _scratch(self, k, h, w):
        """Intermediate plane k of the reused device buffer: 0 / 1 the point and CLAHE launches,
        2 / 3 the elastic image / mask."""
        n = h * w
        if self._u8 is None or self._u8.shape[1] < n:
            self._u8 = torch.empty((4, n), dtype=torch.uint8, device=self.device)
        return self._u8[k, :n].view(h, w)

    def _upload_field(self, a, h, w):
        """An (H, W) float64 field of a record, on the device (stream-ordered like the planes:
        the caching allocator reuses the memory only behind the launches that read it)."""
        return torch.from_numpy(_field(a, h, w)).to(self.device, non_blocking=True)

    def elastic(self, ti, tm, rec):
        """The recorded ElasticDeform of an image and / or its mask ((H, W) uint8 device planes,
        either may be None) under the one map, in one call.  Returns views of the reused buffer
        (valid until the next elastic call)."""
        h, w = (ti if ti is not None else tm).shape
        rx, ry = (self._upload_field(f, h, w) for f in rec.elastic[2:])
        di = None if ti is None else self._scratch(2, h, w)
        dm = None if tm is None else self._scratch(3, h, w)
        _lib.check(self.rt.lib.unet_elastic_u8(
            self.rt.ctx, _lib.ptr(ti), _lib.ptr(tm), h, w, _lib.ptr(di), _lib.ptr(dm), _lib.ptr(rx),
            _lib.ptr(ry), ctypes.byref(rec.elastic_params()), _lib.stream_ptr(self.device)),
            self.rt.ctx, "unet_elastic_u8")
        return di, dm

    def augment(self, t, rec, is_mask, elastic_done=False):
        """The recorded augmentations of one (H, W) uint8 device plane: ElasticDeform if drawn
        (unless ``elastic_done``: the pair went through ``elastic`` together), flip + rotate (+
        brightness + speckle + TGC for an image) in one launch, then CLAHE if drawn.  Returns a
        view of the reused buffer (valid until the next call) or ``t`` itself when nothing
        applies."""
        h, w = t.shape
        if rec.elastic is not None and not elastic_done:
            t = self.elastic(None, t, rec)[1] if is_mask else self.elastic(t, None, rec)[0]
        p = rec.params(h, w, is_mask)
        if p is not None and not is_mask and rec.speckle is not None:
            d = self._scratch(0, h, w)
            noise = self._upload_field(rec.speckle, h, w)
            _lib.check(self.rt.lib.unet_augment_noise_u8(
                self.rt.ctx, _lib.ptr(t), h, w, _lib.ptr(d), ctypes.byref(p), _lib.ptr(noise),
                _lib.stream_ptr(self.device)), self.rt.ctx, "unet_augment_noise_u8")
            t = d
        elif p is not None:
            d = self._scratch(0, h, w)
            _lib.check(self.rt.lib.unet_augment_u8(
                self.rt.ctx, _lib.ptr(t), h, w, _lib.ptr(d), ctypes.byref(p),
                _lib.stream_ptr(self.device)), self.rt.ctx, "unet_augment_u8")
            t = d
        if not is_mask and rec.clahe is not None:
            clip, (gx, gy) = rec.clahe
            d = self._scratch(1, h, w)
            _lib.check(self.rt.lib.unet_clahe_u8(
                self.rt.ctx, _lib.ptr(t), h, w, _lib.ptr(d), float(clip), int(gx), int(gy),
                _lib.stream_ptr(self.device)), self.rt.ctx, "unet_clahe_u8")
            t = d
        return t

    def resize(self, img, out=None, aug=None, is_mask=False, elastic_done=False, nearest=None):
        """One HxW uint8 image -> (oh, ow) fp32 in [0, 1] on the device.  nearest: the resample of
        the plane when it no longer carries its ``resample`` tag (an uploaded tensor)."""
        if nearest is None:
            nearest = getattr(img, "resample", "bilinear") == "nearest"
        t = self._upload(img)
        if aug is not None:
            t = self.augment(t, aug, is_mask, elastic_done)
        h, w = t.shape
        if out is None:
            out = torch.empty((self.oh, self.ow), dtype=torch.float32, device=self.device)
        kh, bh, ksh = self._plan(w, self.ow, nearest)
        kv, bv, ksv = self._plan(h, self.oh, nearest)
        _lib.check(self.rt.lib.unet_resize_u8(
            self.rt.ctx, _lib.ptr(t), h, w, _lib.ptr(out), self.oh, self.ow, _lib.ptr(kh),
            _lib.ptr(bh), ksh, _lib.ptr(kv), _lib.ptr(bv), ksv, 255.0,
            _lib.stream_ptr(self.device)), self.rt.ctx, "unet_resize_u8")
        return out

    def __call__(self, images, masks=None, aug=None):
        """``aug``: one AugRecord (or None) per sample, applied to the image and the mask
        before the resize; ``None`` = no augmentation."""
        n = len(images)
        if aug is None:
            aug = [None] * n
        elif len(aug) != n:
            raise ValueError(f"{len(aug)} augmentation records for {n} images")
        x = torch.empty((n, 1, self.oh, self.ow), dtype=torch.float32, device=self.device)
        t = None if masks is None else torch.empty_like(x)
        paired = [t is not None and r is not None and r.elastic is not None for r in aug]
        for i, im in enumerate(images):
            if paired[i]:  # one elastic call deforms the image and its mask under the one map
                di, dm = self.elastic(self._upload(im), self._upload(masks[i]), aug[i])
                self.resize(di, x[i, 0], aug[i], elastic_done=True)
                self.resize(dm, t[i, 0], aug[i], is_mask=True, elastic_done=True)
            else:
                self.resize(im, x[i, 0], aug[i])
        if masks is None:
            return x
        for i, m in enumerate(masks):
            if not paired[i]:
                self.resize(m, t[i, 0], aug[i], is_mask=True)
        return x, t
