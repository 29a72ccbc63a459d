"""numpy restatement of the contrastive view pipeline (csrc/views.hip): crop -> bilinear resize -> flip, colour
jitter (oracle.augment.color_jitter on the resized stack), colour drop, separable blur.  float64 by default; `dtype=np.float32` runs
the pixel arithmetic in float32 (the tap positions and fractions are index arithmetic and stay float64 in both runs: the kernel
computes them exactly, in integers)."""
import numpy as np

from oracle import augment as A

GRAY = (0.2989, 0.5870, 0.1140)         # tf.image.rgb_to_grayscale


def plan(H, W, **kw):
    """One view plan as a dict: nothing fires unless `kw` says so."""
    p = dict(crop_y=0, crop_x=0, crop_h=H, crop_w=W, flip=0, jitter=0, brightness=0.0, contrast=1.0, saturation=1.0, hue=0.0, drop=0,
             blur_taps=0, blur_w=[])
    p.update(kw)
    return p


def gaussian(taps, sigma):
    """Normalised in float64, stored as float32: the numbers the device reads."""
    x = np.arange(taps, dtype=np.float64) - taps // 2
    w = np.exp(-x ** 2 / (2.0 * sigma ** 2))
    return (w / w.sum()).astype(np.float32)


def _taps(full, crop):
    """tf.image.resize (bilinear, half-pixel centres, no antialias) of `crop` source pixels to `full`: lower tap, upper tap, fraction."""
    src = np.clip((np.arange(full, dtype=np.float64) + 0.5) * crop / full - 0.5, 0.0, crop - 1.0)
    i0 = np.floor(src).astype(np.int64)
    return i0, np.minimum(i0 + 1, crop - 1), src - i0


def crop_resize_flip(x, p):
    """x: (T, H, W, 3).  The crop window resized back to H x W, x first, then y; then the x-mirror."""
    T, H, W, _ = x.shape
    win = x[:, p['crop_y']:p['crop_y'] + p['crop_h'], p['crop_x']:p['crop_x'] + p['crop_w']]
    x0, x1, fx = _taps(W, p['crop_w'])
    y0, y1, fy = _taps(H, p['crop_h'])
    fx = fx.astype(x.dtype)[None, None, :, None]
    fy = fy.astype(x.dtype)[None, :, None, None]
    rows = win[:, :, x0] + (win[:, :, x1] - win[:, :, x0]) * fx
    out = rows[:, y0] + (rows[:, y1] - rows[:, y0]) * fy
    return out[:, :, ::-1] if p['flip'] else out


def color_drop(x):
    g = GRAY[0] * x[..., 0] + GRAY[1] * x[..., 1] + GRAY[2] * x[..., 2]
    return np.repeat(g[..., None], 3, axis=-1)


def blur(x, w):
    """Separable blur of (T, H, W, 3) with the 1-D weights w, horizontal then vertical, replicate edge."""
    T, H, W, _ = x.shape
    r = len(w) // 2
    w = np.asarray(w).astype(x.dtype)
    ix = np.clip(np.arange(W)[:, None] + np.arange(len(w))[None, :] - r, 0, W - 1)
    iy = np.clip(np.arange(H)[:, None] + np.arange(len(w))[None, :] - r, 0, H - 1)
    h = np.zeros_like(x)
    for k in range(len(w)):
        h = h + w[k] * x[:, :, ix[:, k]]
    v = np.zeros_like(x)
    for k in range(len(w)):
        v = v + w[k] * h[:, iy[:, k]]
    return v


def view(x, p, dtype=np.float64):
    x = crop_resize_flip(np.asarray(x).astype(dtype), p)
    if p['jitter']:
        x = A.color_jitter(x, dtype(p['brightness']), dtype(p['contrast']), dtype(p['saturation']), dtype(p['hue'])).astype(dtype)
    if p['drop']:
        x = color_drop(x)
    if p['blur_taps']:
        x = blur(x, np.asarray(p['blur_w'])[:p['blur_taps']])
    return x


def as_dicts(records):
    """A VIEW_PLAN_DTYPE record array as plan dicts holding the float32 numbers the device reads."""
    return [{n: (r[n].copy() if n == 'blur_w' else r[n].item() if n in INT_FIELDS else np.float32(r[n])) for n in records.dtype.names}
            for r in records]


INT_FIELDS = ('crop_y', 'crop_x', 'crop_h', 'crop_w', 'flip', 'jitter', 'drop', 'blur_taps')
JITTER = dict(jitter=1, brightness=0.13, contrast=1.4, saturation=0.6, hue=-0.11)       # the two sets of tests/test_gpu_augment.py
JITTER2 = dict(jitter=1, brightness=-0.2, contrast=0.3, saturation=1.7, hue=0.2)
SMALL, LARGE = (3, 2, 23, 31), (2, 4, 90, 120)          # (N, T, H, W): V = 2 N views


def rows_of(shape, equal_frames=False):
    N, T, H, W = shape
    x = np.random.default_rng(T * H + W).uniform(0.0, 1.0, (N, T, H, W, 3)).astype(np.float32)
    if equal_frames:
        x[:, 1:] = x[:, :1]
    return x


def _blur(taps, sigma):
    return dict(blur_taps=taps, blur_w=list(gaussian(taps, sigma)))


def cases():
    """name -> (shape, plan dicts, has jitter): the cases the device is compared with this file on (tests/test_gpu_views.py) and this
    file's float32 run is compared with its float64 run on (tests/test_views_host.py)."""
    N, T, H, W = SMALL
    P = lambda **kw: plan(H, W, **kw)
    win = lambda y, x, h, w, **kw: P(crop_y=y, crop_x=x, crop_h=h, crop_w=w, **kw)
    crops = [win(0, 0, 2, 2), win(H - 2, W - 2, 2, 2), win(0, 0, H - 1, W - 1), win(1, 1, H - 1, W - 1), win(0, W - 2, H - 1, 2, flip=1),
             win(H - 2, 0, 2, W - 1)]
    mixed = [win(3, 5, 14, 19, **JITTER), P(flip=1, drop=1, **_blur(3, 0.7)), win(0, 0, 2, 2, **JITTER2, **_blur(15, 2.0)),
             P(**JITTER, drop=1), win(H - 12, W - 20, 12, 20, flip=1, **_blur(9, 1.1)), win(1, 0, H - 1, W, **JITTER2, drop=1, **_blur(3, 0.1))]
    L = lambda **kw: plan(LARGE[2], LARGE[3], **kw)
    large = [L(**JITTER), L(crop_y=11, crop_x=17, crop_h=54, crop_w=72, **JITTER2, **_blur(9, 2.0)), L(drop=1, **_blur(9, 0.1)),
             L(crop_y=36, crop_x=48, crop_h=54, crop_w=72, flip=1, **JITTER, drop=1, **_blur(9, 1.0))]
    return {
        'crops': (SMALL, crops, False),
        'drop': (SMALL, [P(drop=1)] * 6, False),
        'blur3': (SMALL, [P(**_blur(3, s)) for s in (0.1, 0.5, 0.8, 1.0, 1.5, 2.0)], False),
        'blur9': (SMALL, [P(**_blur(9, s)) for s in (0.1, 0.5, 0.8, 1.0, 1.5, 2.0)], False),
        'blur15': (SMALL, [P(**_blur(15, s)) for s in (0.1, 0.5, 1.0, 2.0, 4.0, 8.0)], False),
        'jitter': (SMALL, [P(**JITTER)] * 6, True),
        'jitter2': (SMALL, [P(**JITTER2)] * 6, True),
        'mixed': (SMALL, mixed, True),
        'large': (LARGE, large, True),
    }


def check(got, ref, jitter) -> dict:
    """The bounds of the view pipeline against this file's float64 run.  Without jitter every stage is a convex combination of at
    most ~20 values in [0, 1] (float32 rounding stays below 2e-6): worst error <= 1e-5.  With jitter the project's bounds for that op
    (tests/test_gpu_augment.py): hue is discontinuous where channels tie, so a handful of pixels may take the other branch."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    figures = dict(max=float(err.max()), q9999=float(np.quantile(err, 0.9999)), share_above_1e3=float((err > 1e-3).mean()))
    if jitter:
        assert figures['q9999'] < 2e-5 and figures['share_above_1e3'] < 1e-4, figures
    else:
        assert figures['max'] <= 1e-5, figures
    return figures


def views(rows, plans, dtype=np.float64):
    """rows (N, T, H, W, 3), V plans -> (V, T, H, W, 3): view v is row v % N under plans[v]."""
    return np.stack([view(rows[v % len(rows)], p, dtype) for v, p in enumerate(plans)])
