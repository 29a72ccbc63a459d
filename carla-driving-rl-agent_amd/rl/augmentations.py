"""Rollout-time image augmentation (reference rl/augmentations/* as used by CARLAgent.augment,
core/carla_agent.py:527-579) on the native kernels.

`draw_plan(alpha, rng)` makes the same sequence of random decisions as the reference's `augment_fn` (one
`tf_chance` per op compared with the op's probability times the intensity `alpha`, then the op's own random scalars);
`Augmenter()(images, plan)` applies the plan to one stack on the device through `cdrl_augment_images`; `Augmenter().batch(images,
plans)` applies E plans to the E stacks of an environment shard through `cdrl_augment_images_batch` (one copy of the images, one
upload of the packed plans, five launches for any E; every stack gets the bytes the one-stack call gives it).  The random *fields*
(salt & pepper masks, gaussian noise, dropout grid) are generated on the device from (plan seed, plan offset).

Contrastive views (the reference's rl/augmentations/simclr.py:pipeline): `draw_view_plans` draws one plan per view --
crop window, flip, colour jitter, colour drop, Gaussian blur -- as one numpy record array, vectorised over the views;
`Augmenter().views(rows, plans)` turns N rows into copies * N views through `cdrl_views_batch` (one upload of the plans, one library
call, four launches for any number of views, no doubled copy of the rows)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib


class AugPlan(C.Structure):
    _fields_ = [('jitter', C.c_int), ('brightness', C.c_float), ('contrast', C.c_float), ('saturation', C.c_float),
                ('hue', C.c_float), ('blur_size', C.c_int), ('blur_kernel', C.c_float * 75), ('salt_pepper', C.c_int),
                ('sp_amount', C.c_float), ('sp_prob', C.c_float), ('gauss_noise', C.c_int), ('gn_amount', C.c_float),
                ('gn_std', C.c_float), ('normalize', C.c_int), ('cutout_size', C.c_int), ('cutout_cell', C.c_int),
                ('dropout_size', C.c_int), ('dropout_amount', C.c_float), ('seed', C.c_uint64), ('offset', C.c_uint64)]


def empty_plan(seed=0, offset=0) -> dict:
    return dict(jitter=0, brightness=0.0, contrast=1.0, saturation=1.0, hue=0.0, blur_size=0, blur_kernel=[0.0] * 75,
                salt_pepper=0, sp_amount=0.1, sp_prob=0.5, gauss_noise=0, gn_amount=0.1, gn_std=0.075, normalize=0,
                cutout_size=0, cutout_cell=0, dropout_size=0, dropout_amount=0.04, seed=int(seed), offset=int(offset))


def draw_plan(alpha: float, rng: np.random.Generator, offset=0) -> dict:
    """Random decisions of CARLAgent.augment_fn (core/carla_agent.py:549-576) for intensity `alpha`."""
    plan = empty_plan(seed=int(rng.integers(0, 2 ** 63 - 1)), offset=offset)
    if alpha <= 0.0:
        return plan
    chance = lambda: float(rng.uniform(0.0, 1.0))
    if chance() < alpha:                                     # simclr.color_jitter(strength=alpha)
        plan.update(jitter=1, brightness=float(rng.uniform(-0.2 * alpha, 0.2 * alpha)),
                    contrast=float(rng.uniform(1.0 - 0.8 * alpha, 1.0 + 0.8 * alpha)),
                    saturation=float(rng.uniform(1.0 - 0.8 * alpha, 1.0 + 0.8 * alpha)),
                    hue=float(rng.uniform(-0.2 * alpha, 0.2 * alpha)))
    if chance() < 0.25 * alpha:                              # tf_gaussian_blur(size=3|5): random N(1, 0.25) kernel
        k = 3 if chance() >= 0.5 else 5
        kern = rng.normal(1.0, 0.25, size=(k, k, 3)).astype(np.float32).reshape(-1)
        plan.update(blur_size=k, blur_kernel=list(kern) + [0.0] * (75 - kern.size))
    if chance() < 0.2 * alpha:
        plan.update(salt_pepper=1, sp_amount=0.1, sp_prob=0.5)
    if chance() < 0.33 * alpha:
        plan.update(gauss_noise=1, gn_amount=0.10, gn_std=0.075)
    plan.update(normalize=1)
    if chance() < 0.15 * alpha:                              # tf_cutout_batch(size=6): the argmax cell of a random grid
        plan.update(cutout_size=6, cutout_cell=int(rng.integers(0, 36)))
    if chance() < 0.15 * alpha:
        plan.update(dropout_size=81, dropout_amount=0.04)
    return plan


def draw_plans(alpha: float, rng: np.random.Generator, count: int, first_offset: int) -> list:
    """`count` plans drawn one after the other from `rng`, with offsets first_offset, first_offset + 1, ...: what `count` successive
    draw_plan calls give (the shard path of CARLAgent.preprocess draws its environments' plans here, in environment order)."""
    return [draw_plan(alpha, rng, offset=first_offset + i) for i in range(count)]


def to_struct(plan: dict) -> AugPlan:
    p = AugPlan()
    for k, v in plan.items():
        if k == 'blur_kernel':
            for i, x in enumerate(v):
                p.blur_kernel[i] = float(x)
        else:
            setattr(p, k, v)
    return p


# AugPlan's layout as a numpy record (align=True pads as the C compiler does: `seed` starts on an 8-byte boundary)
PLAN_DTYPE = np.dtype([(n, np.float32, (75,)) if n == 'blur_kernel' else (n, np.dtype(t)) for n, t in AugPlan._fields_], align=True)
assert PLAN_DTYPE.itemsize == C.sizeof(AugPlan) and all(PLAN_DTYPE.fields[n][1] == getattr(AugPlan, n).offset
                                                        for n, _ in AugPlan._fields_)


def pack_plans(plans: list) -> np.ndarray:
    """The plans as one record array with AugPlan's byte layout (`.tobytes()` = the concatenated `to_struct` images), filled one
    COLUMN at a time.  A blur size the kernels do not have is refused here: the device code cannot report it."""
    out = np.zeros(len(plans), dtype=PLAN_DTYPE)
    for name in PLAN_DTYPE.names:
        if name == 'blur_kernel':
            for row, plan in zip(out[name], plans):
                kern = plan.get(name, ())
                row[:len(kern)] = kern
        else:
            out[name] = [plan.get(name, 0) for plan in plans]
    bad = ~np.isin(out['blur_size'], (0, 3, 5))
    if bad.any():
        raise ValueError(f'blur_size must be 0, 3 or 5, got {out["blur_size"][bad].tolist()} (plans {np.flatnonzero(bad).tolist()})')
    return out


# ---- contrastive views (csrc/views.hip)
VIEW_MAX_TAPS = 15


class ViewPlan(C.Structure):
    _fields_ = [('crop_y', C.c_int32), ('crop_x', C.c_int32), ('crop_h', C.c_int32), ('crop_w', C.c_int32), ('flip', C.c_int32),
                ('jitter', C.c_int32), ('brightness', C.c_float), ('contrast', C.c_float), ('saturation', C.c_float),
                ('hue', C.c_float), ('drop', C.c_int32), ('blur_taps', C.c_int32), ('blur_w', C.c_float * 16)]


VIEW_PLAN_DTYPE = np.dtype([(n, np.float32, (16,)) if n == 'blur_w' else (n, np.dtype(t)) for n, t in ViewPlan._fields_], align=True)
assert VIEW_PLAN_DTYPE.itemsize == C.sizeof(ViewPlan) and all(VIEW_PLAN_DTYPE.fields[n][1] == getattr(ViewPlan, n).offset
                                                              for n, _ in ViewPlan._fields_)

VIEW_OPTIONS = dict(crop_scale=(0.6, 1.0), flip_prob=0.0, jitter_prob=0.8, drop_prob=0.2, blur_prob=0.5, blur_sigma=(0.1, 2.0))


def empty_view_plans(count: int, H: int, W: int) -> np.ndarray:
    """`count` plans that change nothing: full-size crop, no flip, no colour op, no blur."""
    out = np.zeros(count, dtype=VIEW_PLAN_DTYPE)
    out['crop_h'], out['crop_w'], out['contrast'], out['saturation'] = H, W, 1.0, 1.0
    return out


def check_view_options(**options) -> dict:
    """The keyword options of draw_view_plans, completed with their defaults; an unknown name or a value out of range: ValueError."""
    unknown = sorted(set(options) - set(VIEW_OPTIONS))
    if unknown:
        raise ValueError(f'unknown view option(s) {unknown}: the options are {sorted(VIEW_OPTIONS)}')
    opt = dict(VIEW_OPTIONS, **options)
    for name in ('flip_prob', 'jitter_prob', 'drop_prob', 'blur_prob'):
        if not 0.0 <= float(opt[name]) <= 1.0:
            raise ValueError(f'{name}={opt[name]!r} is a probability: it must lie in [0, 1]')
    for name in ('crop_scale', 'blur_sigma'):
        if np.ndim(opt[name]) != 1 or len(opt[name]) != 2:
            raise ValueError(f'{name}={opt[name]!r} must be a (low, high) pair')
    lo, hi = (float(v) for v in opt['crop_scale'])
    if not 0.0 < lo <= hi <= 1.0:
        raise ValueError(f'crop_scale={opt["crop_scale"]!r} must satisfy 0 < low <= high <= 1')
    lo, hi = (float(v) for v in opt['blur_sigma'])
    if not 0.0 < lo <= hi:
        raise ValueError(f'blur_sigma={opt["blur_sigma"]!r} must satisfy 0 < low <= high')
    return opt


def view_blur_taps(H: int, W: int) -> int:
    """The blur's tap count for H x W frames: a tenth of the shorter side made odd, within 3..15 (9 at 90 x 120)."""
    return int(np.clip(int(0.1 * min(H, W)) | 1, 3, VIEW_MAX_TAPS))


def draw_view_plans(strength: float, rng: np.random.Generator, count: int, H: int, W: int, *, crop_scale=(0.6, 1.0), flip_prob=0.0,
                    jitter_prob=0.8, drop_prob=0.2, blur_prob=0.5, blur_sigma=(0.1, 2.0)) -> np.ndarray:
    """`count` view plans for H x W frames as a VIEW_PLAN_DTYPE record array: ONE generator call per field for all the plans, in a
    fixed order, so the plans are a pure function of the generator's state.
    crop: a side fraction s ~ U(crop_scale) per view, window round(s H) x round(s W) (at least 2, aspect ratio kept -- a panoramic
    90 x 360 frame is not squeezed) at an integer-uniform offset.  The default crop_scale is a choice nobody has tuned.
    flip: with flip_prob; 0 by default -- invariance to mirroring would give a left bend and a right bend one embedding.
    jitter: with jitter_prob, the ranges of draw_plan at alpha = strength (brightness and hue +-0.2 s, contrast and saturation
    1 +- 0.8 s).  drop: colour drop with drop_prob.  blur: with blur_prob, a normalised Gaussian of view_blur_taps(H, W) taps with
    sigma ~ U(blur_sigma); the weights are normalised in float64 and stored as float32."""
    opt = check_view_options(crop_scale=crop_scale, flip_prob=flip_prob, jitter_prob=jitter_prob, drop_prob=drop_prob,
                             blur_prob=blur_prob, blur_sigma=blur_sigma)
    count, H, W, s = int(count), int(H), int(W), float(strength)
    if count < 0 or H < 2 or W < 2 or s < 0.0:
        raise ValueError(f'draw_view_plans: count {count}, frames {H} x {W}, strength {strength}: need count >= 0, frames of at '
                         f'least 2 x 2 and strength >= 0')
    out = empty_view_plans(count, H, W)
    scale = rng.uniform(*opt['crop_scale'], size=count)
    out['crop_h'] = np.clip(np.rint(scale * H), 2, H)
    out['crop_w'] = np.clip(np.rint(scale * W), 2, W)
    out['crop_y'] = rng.integers(0, H - out['crop_h'] + 1)
    out['crop_x'] = rng.integers(0, W - out['crop_w'] + 1)
    out['flip'] = rng.random(count) < opt['flip_prob']
    jitter = rng.random(count) < opt['jitter_prob']
    out['jitter'] = jitter
    out['brightness'] = np.where(jitter, rng.uniform(-0.2 * s, 0.2 * s, size=count), 0.0)
    out['contrast'] = np.where(jitter, rng.uniform(1.0 - 0.8 * s, 1.0 + 0.8 * s, size=count), 1.0)
    out['saturation'] = np.where(jitter, rng.uniform(1.0 - 0.8 * s, 1.0 + 0.8 * s, size=count), 1.0)
    out['hue'] = np.where(jitter, rng.uniform(-0.2 * s, 0.2 * s, size=count), 0.0)
    out['drop'] = rng.random(count) < opt['drop_prob']
    blur = rng.random(count) < opt['blur_prob']
    sigma = rng.uniform(*opt['blur_sigma'], size=count)
    taps = view_blur_taps(H, W)
    x = np.arange(taps, dtype=np.float64) - taps // 2
    w = np.exp(-(x[None, :] ** 2) / (2.0 * sigma[:, None] ** 2))
    w /= w.sum(axis=1, keepdims=True)
    out['blur_taps'] = np.where(blur, taps, 0)
    out['blur_w'][:, :taps] = np.where(blur[:, None], w, 0.0)
    return out


def pack_view_plans(plans, H: int, W: int) -> np.ndarray:
    """The plans (a VIEW_PLAN_DTYPE record array, or a list of dicts over empty_view_plans' fields) as one contiguous record array
    with cdrl_view_plan's byte layout, validated for H x W frames: the device cannot report a bad plan.  ValueError names the plans
    whose crop window leaves the frame or is smaller than 2, whose tap count is not 0 or odd within 3..15, or whose weights do not
    sum to 1 within 1e-5."""
    if isinstance(plans, np.ndarray):
        if plans.dtype != VIEW_PLAN_DTYPE or plans.ndim != 1:
            raise ValueError(f'view plans must be a 1-D array of VIEW_PLAN_DTYPE, got {plans.dtype} with {plans.ndim} dimensions')
        out = np.ascontiguousarray(plans)
    else:
        out = empty_view_plans(len(plans), H, W)
        for i, plan in enumerate(plans):
            for name, value in plan.items():
                if name == 'blur_w':
                    out[i][name][:len(value)] = value
                else:
                    out[i][name] = value
    problems = []

    def refuse(bad, what):
        if bad.any():
            problems.append(f'{what} (plans {np.flatnonzero(bad).tolist()})')

    ch, cw, cy, cx = (out[n].astype(np.int64) for n in ('crop_h', 'crop_w', 'crop_y', 'crop_x'))
    refuse((ch < 2) | (cw < 2), 'crop window smaller than 2')
    refuse((cy < 0) | (cx < 0) | (cy + ch > H) | (cx + cw > W), f'crop window outside the {H} x {W} frame')
    taps = out['blur_taps']
    refuse((taps != 0) & ((taps < 3) | (taps > VIEW_MAX_TAPS) | (taps % 2 == 0)), f'blur_taps must be 0 or odd within 3..{VIEW_MAX_TAPS}')
    used = np.arange(16)[None, :] < taps[:, None]
    total = np.where(used, out['blur_w'].astype(np.float64), 0.0).sum(axis=1)
    refuse((taps != 0) & ~(np.abs(total - 1.0) <= 1e-5), 'blur weights do not sum to 1 within 1e-5')
    if problems:
        raise ValueError('bad view plans: ' + '; '.join(problems))
    return out


class Augmenter:
    """Holds the workspace / output buffers for one observation-stack shape."""

    def __init__(self, device='cuda:0'):
        self.lib = _lib.load()
        self.device = torch.device(device)
        self._ws = None
        self._shape = None
        self._batch_ws = None
        self._batch_shape = None
        self._staging = None
        self._staging_read = None
        self._views_ws = None
        self._views_shape = None

    def _stage(self, stacks) -> torch.Tensor:
        """E host stacks -> one (E, T, H, W, 3) device tensor: the stacks are gathered straight into a cached page-locked buffer
        (one pass over the host data, no fresh 0.5 MB x E array per step) and cross PCIe as one asynchronous copy."""
        shape = (len(stacks),) + tuple(np.shape(stacks[0]))
        if self._staging is None or tuple(self._staging.shape) != shape:
            self._staging = torch.empty(shape, dtype=torch.float32, pin_memory=True)
            self._staging_read = None
        if self._staging_read is not None:
            self._staging_read.synchronize()                # the previous step's copy out of the buffer has finished
        np.stack(stacks, axis=0, out=self._staging.numpy())
        x = self._staging.to(self.device, non_blocking=True)
        self._staging_read = torch.cuda.Event()
        self._staging_read.record()
        return x

    def batch(self, images, plans: list) -> torch.Tensor:
        """images: (E, T, H, W, 3), host or device, or a list of E host stacks (T, H, W, 3); plans: E dicts.  Stack e is augmented
        with plans[e], as `self(images[e], plans[e])` would: one host-to-device copy of the images, one of the packed plans, one
        library call."""
        if isinstance(images, (list, tuple)) and not any(isinstance(v, torch.Tensor) for v in images):
            x = self._stage(images)
        else:
            x = torch.as_tensor(images, dtype=torch.float32).to(self.device).contiguous()
        if x.dim() != 5 or x.shape[-1] != 3:
            raise ValueError(f'expected a shard of image stacks (E, T, H, W, 3), got {tuple(x.shape)}')
        E, T, H, W, _ = x.shape
        if len(plans) != E:
            raise ValueError(f'{E} image stacks but {len(plans)} plans')
        packed = pack_plans(plans)
        if self._batch_shape != (E, T, H, W):
            self._batch_ws = torch.empty(int(self.lib.cdrl_augment_batch_workspace_floats(E, T, H, W)), device=self.device)
            self._batch_shape = (E, T, H, W)
        plans_dev = torch.from_numpy(packed.view(np.uint8)).to(self.device)
        out = torch.empty_like(x)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.cdrl_augment_images_batch(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), E, T, H, W,
                                                      C.c_void_p(plans_dev.data_ptr()), C.c_void_p(self._batch_ws.data_ptr()), stream),
                   'cdrl_augment_images_batch')
        return out

    def views(self, rows, plans, copies=2) -> torch.Tensor:
        """rows: (N, T, H, W, 3), kept on the device; plans: copies * N view plans (pack_view_plans).  -> (copies * N, T, H, W, 3):
        view v is row v % N under plans[v].  One upload of the packed plans and one library call; the rows are not copied."""
        x = torch.as_tensor(rows, dtype=torch.float32).to(self.device).contiguous()
        if x.dim() != 5 or x.shape[-1] != 3:
            raise ValueError(f'expected image stacks (N, T, H, W, 3), got {tuple(x.shape)}')
        N, T, H, W, _ = x.shape
        V = int(copies) * N
        if V < 1 or len(plans) != V:
            raise ValueError(f'{copies} views of each of {N} rows need {V} plans (at least one), got {len(plans)}')
        packed = pack_view_plans(plans, H, W)
        if self._views_shape != (V, T, H, W):
            self._views_ws = torch.empty(int(self.lib.cdrl_views_workspace_floats(V, T, H, W)), device=self.device)
            self._views_shape = (V, T, H, W)
        plans_dev = torch.from_numpy(packed.view(np.uint8)).to(self.device)
        out = torch.empty((V, T, H, W, 3), dtype=torch.float32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.cdrl_views_batch(C.c_void_p(x.data_ptr()), N, C.c_void_p(out.data_ptr()), V, T, H, W,
                                             C.c_void_p(plans_dev.data_ptr()), C.c_void_p(self._views_ws.data_ptr()), stream),
                   'cdrl_views_batch')
        return out

    def __call__(self, images, plan: dict) -> torch.Tensor:
        x = torch.as_tensor(images, dtype=torch.float32).to(self.device).contiguous()
        if x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f'expected an image stack (T, H, W, 3), got {tuple(x.shape)}')
        T, H, W, _ = x.shape
        if self._shape != (T, H, W):
            self._ws = torch.empty(int(self.lib.cdrl_augment_workspace_floats(T, H, W)), device=self.device)
            self._shape = (T, H, W)
        out = torch.empty_like(x)
        st = to_struct(plan)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.cdrl_augment_images(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), T, H, W, C.byref(st),
                                                C.c_void_p(self._ws.data_ptr()), stream), 'cdrl_augment_images')
        return out
