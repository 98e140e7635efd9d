"""Checker of ldmae_crop_resize_flip_u8 (include/ldmae_hip.h): an f64 NumPy restatement of its contract, the per-element bound an f32 device
result has to keep against it, and an f32 emulation (with three deliberately wrong variants) that the CPU tests use to show the bound bites.

RESTATEMENT (`restate`).  PIL's crop(box).resize((S, S), BICUBIC) without its 8-bit rounding after each pass: per axis with input size n,
scale = n / S, fs = max(scale, 1), support = 2 fs; output i has center = (i + 0.5) scale, taps x in [max(int(center - support + 0.5), 0),
min(int(center + support + 0.5), n)), weights cubic((x - center + 0.5) / fs) (Keys, a = -0.5) divided by their sum.  Horizontal pass, clamp to
[0, 255], vertical pass, clamp, (v / 255 - mean) / std, columns mirrored when flip.  All in f64.

BOUND (`bound_f32`), from the tap sets the case really has.  u = 2^-24.
  1. A weight's argument t = ((2x + 1) S - (2i + 1) n) / 2 max(n, S) is one rounded quotient of two exact integers: |dt| <= u |t| <= 2 u, and
     |cubic'| <= 1.39, so 3 u from the argument.  The polynomial itself, Horner in f32: on |t| < 1 the intermediates 1.5 t, 1.5 t - 2.5, two
     products by t and the closing + 1 are at most 1.5, 2.5, 2.5, 2.5, 1 in size and nothing is amplified (|t| < 1): 10 u.  On 1 <= |t| < 2:
     t - 5 (4 u), times t (error doubled, + 8 u = 16 u), + 8 (+ 4 u = 20 u), times t (doubled, + 8 u = 48 u), - 4 (+ u), times 0.5: 24.5 u.
     With the argument: e_q = 32 u per un-normalised weight q (a fused multiply-add only removes roundings).
  2. Their ascending f32 sum over k taps, Q = sum |q|: e_s = k e_q + k u Q.
  3. A normalised weight w = q / s: e_w = (e_q + |w| e_s) / (s - e_s) + u |w|; over the tap set E = (k e_q + A e_s) / (s - e_s) + u A with
     A = sum |w|.
  4. An ascending chain of k fused multiply-adds on values in [0, 255]: gamma_k (A + E) 255 with gamma_k = k u / (1 - k u).
     Horizontal pass of column x:  e_h(x) = 255 (E_x + gamma (A_x + E_x)).  Clamping does not expand an error.
     Vertical pass of row y:       e_v(y, x) = (A_y + E_y) e_h(x) + 255 (E_y + gamma (A_y + E_y)).
  5. out = fl(fl(fl(v / 255) - mean) / std), |v / 255| <= 1:  e_v / (255 |std|) + u (3 + 2 |mean|) / |std|.
The device forms the tap bounds in integers, the restatement in f64 as PIL does: they can differ only by a tap whose argument is 2 to within
1e-15, of weight below 1e-30.  Nothing here was tuned on a device result.

DEPARTURE FROM PIL (`pil_bound`): PIL rounds to 8 bits after each pass, so the restatement differs from PIL's result by at most
(0.5 max_y sum|w_v| + 0.5) / 255 of the pixel range (half a step of the horizontal result carried through the vertical weights, plus half a step of
its own)."""
import numpy as np

U = 2.0 ** -24
E_Q = 32 * U

# The five geometries of the issue as (h, w, top, left, ch, cw, S).  Its "image 9 x 13 with box (1, 2, 12, 9)" reads either as h x w with a
# (left, top, right, bottom) box or as w x h with a (top, left, bottom, right) box -- the two readings are transposes of each other, and the two
# passes of the kernel are different code, so both are kept: GEOMS[:5] is the first reading, GEOMS[5:] the second.
_GEOMS_HW = [
    (9, 13, 2, 1, 7, 11, 8),               # box (1, 2, 12, 9)
    (31, 17, 0, 0, 31, 17, 16),            # the full box
    (12, 12, 4, 3, 7, 5, 16),              # a 5 x 7 crop, upscaled
    (64, 48, 7, 0, 50, 48, 8),             # a 48 x 50 crop, 6.25 x down, touching both side borders
    (200, 160, 10, 9, 181, 145, 128),      # a 145 x 181 crop
]
GEOMS = _GEOMS_HW + [(w, h, left, top, cw, ch, S) for h, w, top, left, ch, cw, S in _GEOMS_HW]


def cubic(t):
    t = np.abs(np.asarray(t, dtype=np.float64))
    return np.where(t < 1.0, ((1.5 * t - 2.5) * t) * t + 1.0, np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * -0.5, 0.0))


def axis_taps(n, S):
    """-> [(lo, hi, w[hi - lo] f64 normalised, q un-normalised)] per output index, PIL's precompute_coeffs in f64."""
    scale = n / S
    fs = max(scale, 1.0)
    support = 2.0 * fs
    out = []
    for i in range(S):
        center = (i + 0.5) * scale
        lo, hi = max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n)
        q = cubic((np.arange(lo, hi) - center + 0.5) / fs)
        s = 0.0
        for v in q:
            s += v
        out.append((lo, hi, q / s, q))
    return out


def axis_matrix(n, S):
    W = np.zeros((S, n))
    for i, (lo, hi, w, _) in enumerate(axis_taps(n, S)):
        W[i, lo:hi] = w
    return W


def restate(img, top, left, ch, cw, S, flip=0, mean=0.5, std=0.5):
    """img [h, w, 3] uint8 -> [3, S, S] f64."""
    crop = np.asarray(img)[top:top + ch, left:left + cw].astype(np.float64)
    H = np.clip(np.einsum("ix,yxc->yic", axis_matrix(cw, S), crop), 0.0, 255.0)
    V = np.clip(np.einsum("jy,yic->jic", axis_matrix(ch, S), H), 0.0, 255.0)
    out = ((V / 255.0 - mean) / std).transpose(2, 0, 1)
    return out[:, :, ::-1].copy() if flip else out


def _axis_terms(n, S):
    """Per output index: (A + E, 255 (E + gamma (A + E)))."""
    gain, own = np.zeros(S), np.zeros(S)
    for i, (lo, hi, w, q) in enumerate(axis_taps(n, S)):
        k, A, Q, s = hi - lo, np.abs(w).sum(), np.abs(q).sum(), abs(q.sum())
        e_s = k * E_Q + k * U * Q
        E = (k * E_Q + A * e_s) / (s - e_s) + U * A
        gamma = k * U / (1 - k * U)
        gain[i], own[i] = A + E, 255.0 * (E + gamma * (A + E))
    return gain, own


def bound_f32(ch, cw, S, flip=0, mean=0.5, std=0.5):
    """-> [S, S] bound on |device f32 - restate| per element (the same for the three channels), see the module docstring."""
    _, e_h = _axis_terms(cw, S)
    gain_v, own_v = _axis_terms(ch, S)
    e_v = gain_v[:, None] * e_h[None, :] + own_v[:, None]
    b = e_v / (255.0 * abs(std)) + U * (3 + 2 * abs(mean)) / abs(std)
    return b[:, ::-1].copy() if flip else b


def pil_bound(ch, S):
    """Largest difference from PIL's 8-bit result, as a fraction of the pixel range."""
    return (0.5 * max(np.abs(w).sum() for _, _, w, _ in axis_taps(ch, S)) + 0.5) / 255.0


def pil_reference(img, top, left, ch, cw, S, flip=0):
    """Image.crop(box).resize((S, S), BICUBIC) (+ FLIP_LEFT_RIGHT) -> [3, S, S] f64 in [0, 1]."""
    from PIL import Image
    im = Image.fromarray(np.asarray(img)).crop((left, top, left + cw, top + ch)).resize((S, S), Image.BICUBIC)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(im, dtype=np.float64).transpose(2, 0, 1) / 255.0


# ----------------------------------------------------------------------------- f32 emulation of the contract, and wrong variants of it
def _cubic32(t):
    f = np.float32
    t = np.abs(t.astype(np.float32))
    a = ((f(1.5) * t - f(2.5)) * t) * t + f(1.0)
    b = (((t - f(5.0)) * t + f(8.0)) * t - f(4.0)) * f(-0.5)
    return np.where(t < 1, a, np.where(t < 2, b, f(0.0))).astype(np.float32)


def _axis_matrix32(n, S, before, after, clip="box", antialias=True, half=True):
    """f32 weights [S, before + n + after] over the whole image axis (the box starts at `before`).  clip='image': taps clipped at the image
    instead of the box; antialias=False: support fixed at 2; half=False: centres at i * scale."""
    m = max(n, S) if antialias else S
    W = np.zeros((S, before + n + after), dtype=np.float32)
    for i in range(S):
        c = ((2 * i + 1) if half else 2 * i) * n + S                  # 2S (center + 0.5)
        lo, hi = (c - 4 * m) // (2 * S), (c + 4 * m) // (2 * S)
        lo, hi = (max(lo, -before), min(hi, n + after)) if clip == "image" else (max(lo, 0), min(hi, n))
        x = np.arange(lo, hi)
        num = (2 * x + 1) * S - ((2 * i + 1) if half else 2 * i) * n
        q = _cubic32(num.astype(np.float32) / np.float32(2 * m))
        s = np.float32(0)
        for v in q:
            s = np.float32(s + v)
        W[i, before + lo:before + hi] = q / s
    return W


def _fma_pass32(W, src):
    """acc[i, ...] = fma chain over the source index, ascending: W [S, n] f32, src [n, ...] f32 -> [S, ...] f32."""
    acc = np.zeros((W.shape[0],) + src.shape[1:], dtype=np.float32)
    Wd = W.astype(np.float64)
    for x in range(W.shape[1]):
        col = Wd[:, x].reshape((-1,) + (1,) * (src.ndim - 1))
        acc = np.where(col != 0, (col * src[x].astype(np.float64) + acc).astype(np.float32), acc)
    return acc


def emulate_f32(img, top, left, ch, cw, S, flip=0, mean=0.5, std=0.5, **variant):
    """The contract in f32 as the kernel states it (variant = {}), or one of the wrong variants -> [3, S, S] f32."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    f = np.float32
    Wh = _axis_matrix32(cw, S, left, w - left - cw, **variant)
    Wv = _axis_matrix32(ch, S, top, h - top - ch, **variant)
    src = img.astype(np.float32)                                                     # [h, w, 3]
    H = np.clip(_fma_pass32(Wh, src.transpose(1, 0, 2)), f(0), f(255))              # [S(x), h, 3]
    V = np.clip(_fma_pass32(Wv, H.transpose(1, 0, 2)), f(0), f(255))                # [S(y), S(x), 3]
    out = ((V / f(255) - f(mean)) / f(std)).astype(np.float32).transpose(2, 0, 1)
    return out[:, :, ::-1].copy() if flip else out


def make_image(w, h, kind, seed=0):
    """'noise': uniform bytes; 'smooth': a low-frequency pattern; 'checker': 0 / 255 squares of one pixel."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "checker":
        return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    ph = rng.uniform(0, 6.28, 3)
    return np.stack([127.5 + 120 * np.sin(xx / (3.0 + c) + ph[c]) * np.cos(yy / (4.0 + c)) for c in range(3)], axis=2).round().astype(np.uint8)
