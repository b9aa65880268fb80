"""A float64 statement of image-rs `resize(.., Lanczos3)` and of libcaesium's `compute_dimensions`, written from SURVEY.md B.11 / §2b
(not from oracle/jpeg_oracle.c or pipeline.cpp), and the acceptance rule every resize test here applies to 8- and 16-bit output.

What B.11 states in f32 is computed in f32 here too: the ratio, sratio, support, the centre, floor / ceil, the clamps and `centre - 0.5`.
image-rs computes these positions in f32, so their rounding is part of the operation (on a 16-bit 16000 -> 15999 resize f64 positions move
the result by tens of LSB).  Everything else is float64: the kernel sinc(x)·sinc(x/3), the normalisation by Σw, and both passes (vertical
first, no clamp or rounding between them, then horizontal; clamp to [0, M]).  `resize` returns the unrounded values and a per-sample bound
δ on what f32 weights and f32 accumulation may move them by.

Not pinned here, because B.11 cannot pin it: how image-rs treats an alpha channel (it is resampled like any other channel), and
libcaesium's exact `compute_dimensions` beyond the rule §2b states."""
import numpy as np

F32 = np.float32
EPS32 = 2.0 ** -24


def lanczos3(x):
    """K(x) = sinc(x)·sinc(x/3) for |x| < 3, else 0 (float64)"""
    x = np.asarray(x, np.float64)
    return np.where(np.abs(x) < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)


def axis_taps(n_in, n_out, f32_positions=True, variant=None):
    """the taps of one axis: -> (left[n_out], weights[n_out, nmax] float64, zero-padded; n[n_out] tap counts).
    variant names a deliberately wrong statement, used to show that the acceptance rule has power:
      "no_half"     the centre is not moved by -0.5;
      "no_sratio"   the kernel is not widened when downscaling (x = i - centre, support still 3·sratio);
      "no_norm"     the weights are not divided by their sum;
      "short_edge"  the window stops one tap short of the far border (clamped to in-1 instead of in)."""
    rows = []
    if f32_positions:
        ratio = F32(n_in) / F32(n_out)
        sratio = max(ratio, F32(1.0))
        support = F32(3.0) * sratio
    else:
        ratio = n_in / n_out
        sratio = max(ratio, 1.0)
        support = 3.0 * sratio
    half = F32(0.5) if f32_positions else 0.5
    for o in range(n_out):
        centre = (type(ratio)(o) + half) * ratio
        left = int(np.floor(centre - support))
        right = int(np.ceil(centre + support))
        left = min(max(left, 0), n_in - 1)
        right = min(max(right, left + 1), n_in)
        if variant == "short_edge" and right == n_in and right - left > 1:
            right -= 1
        c = centre if variant == "no_half" else centre - half
        i = np.arange(left, right, dtype=np.float64)
        x = (i - np.float64(c)) / (1.0 if variant == "no_sratio" else np.float64(sratio))
        w = lanczos3(x)
        if variant != "no_norm":
            w = w / w.sum()
        rows.append((left, w))
    nmax = max(len(w) for _, w in rows)
    W = np.zeros((n_out, nmax))
    left = np.empty(n_out, np.int64)
    n = np.empty(n_out, np.int64)
    for o, (lo, w) in enumerate(rows):
        W[o, :len(w)] = w
        left[o] = lo
        n[o] = len(w)
    return left, W, n


def _apply(img, axis, left, W, n_in):
    """Σ_k W[o,k]·img[left[o]+k] along axis 0 or 1 of an (h, w, c) float64 array; padded taps index a valid sample with weight 0"""
    idx = np.minimum(left[:, None] + np.arange(W.shape[1])[None, :], n_in - 1)
    if axis == 0:
        return np.einsum("ok,okwc->owc", W, img[idx])
    out = np.empty((img.shape[0], len(left), img.shape[2]))
    for y in range(img.shape[0]):
        out[y] = np.einsum("ok,okc->oc", W, img[y][idx])
    return out


def resize(img, nw, nh, maxval, f32_positions=True, variant=None, clamp=True):
    """image-rs resize(img, nw, nh, Lanczos3) over an (h, w[, c]) array of samples in [0, maxval].
    -> (v, delta): the clamped, unrounded float64 result (nh, nw, c) and the per-sample bound δ (nh, nw, 1) of
    δ = 2·(n_v + n_h + 16)·2⁻²⁴·M·L_v·L_h, n the tap count and L = Σ|w| of that output row / column."""
    a = np.asarray(img, np.float64)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w = a.shape[:2]
    if (nw, nh) == (w, h):
        return a.copy(), np.zeros((h, w, 1))
    lv, Wv, nv = axis_taps(h, nh, f32_positions, variant)
    lh, Wh, nh_ = axis_taps(w, nw, f32_positions, variant)
    v = _apply(_apply(a, 0, lv, Wv, h), 1, lh, Wh, w)
    if clamp:
        v = np.clip(v, 0.0, float(maxval))
    Lv, Lh = np.abs(Wv).sum(1), np.abs(Wh).sum(1)
    delta = 2.0 * (nv[:, None] + nh_[None, :] + 16) * EPS32 * maxval * Lv[:, None] * Lh[None, :]
    return v, delta[:, :, None]


def round_half_away(v):
    return np.floor(v + 0.5)   # v >= 0 after the clamp


def check(d, v, delta):
    """the acceptance rule: every output sample d is floor(v) or ceil(v), and equals round_half_away(v) unless v lies within δ of a
    .5 tie.  -> (number of samples in the tie band, number breaking the rule)"""
    d = np.asarray(d, np.float64).reshape(v.shape)
    delta = np.broadcast_to(delta, v.shape)
    near_tie = np.abs(v - np.floor(v) - 0.5) <= delta
    bracket = (d == np.floor(v)) | (d == np.ceil(v))
    ok = bracket & ((d == round_half_away(v)) | near_tie)
    return int(near_tie.sum()), int((~ok).sum())


def assert_rule(d, v, delta, what=""):
    """check(); fails with the worst offenders listed.  -> the tie-band count"""
    ties, bad = check(d, v, delta)
    if bad:
        dd = np.asarray(d, np.float64).reshape(v.shape)
        err = np.abs(dd - v)
        k = np.argsort(err, axis=None)[::-1][:5]
        worst = [(np.unravel_index(i, v.shape), float(dd.flat[i]), float(v.flat[i]), float(np.broadcast_to(delta, v.shape).flat[i])) for i in k]
        raise AssertionError(f"{what}: {bad} of {v.size} samples break the rule (index, device, model, δ): {worst}")
    return ties


def compute_dimensions(ow, oh, dw, dh):
    """libcaesium compute_dimensions as §2b / B.11 state it: both given -> exactly those; one given -> the other from the f32 aspect ratio,
    f32 round() (half away from zero); at least 1"""
    if dw > 0 and dh > 0:
        return dw, dh
    ratio = F32(ow) / F32(oh)
    if dw > 0:
        nw, nh = dw, int(round_half_away(np.float64(F32(F32(dw) / ratio))))
    elif dh > 0:
        nw, nh = int(round_half_away(np.float64(F32(F32(dh) * ratio)))), dh
    else:
        nw, nh = ow, oh
    return max(nw, 1), max(nh, 1)
