"""The float64 Lanczos3 model (tests/_lanczos_model.py) against an independent implementation, the oracle's f32 restatement
(oracle/jpeg_oracle.c cso_lanczos3_resize{,16}) against the model under the acceptance rule, the rule's power against wrong models, and
compute_dimensions.  CPU only; the device kernels are checked against the same model in test_resize_model_emul.py and on the MI355X.

Not pinned, because SURVEY.md B.11 cannot pin it: alpha handling inside image-rs, and libcaesium's exact compute_dimensions beyond §2b."""
import io

import numpy as np
import pytest

import _lanczos_model as M

PIL = pytest.importorskip("PIL.Image")

# (w, h, nw, nh): reductions and enlargements, ratios on and off the integers, one-tap and thousands-of-taps outputs, identity on one axis,
# and wide rows where f32 positions move the result
SHAPES = [(97, 61, 31, 20), (97, 61, 150, 90), (200, 140, 97, 201), (64, 48, 64, 30), (64, 48, 20, 48), (333, 7, 1000, 7),
          (3000, 2, 1, 1), (1, 300, 50, 1), (2, 3, 97, 61), (1, 1, 5, 3), (7, 5, 3, 2), (128, 96, 64, 48), (41, 17, 40, 16),
          (16000, 2, 15999, 1)]


def battery(seed, h, w, nc, maxval):
    """noise, and hard 0 / M edges (bars, a step, single-sample spikes) where the kernel's negative lobes ring past the range"""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, maxval + 1, (h, w, nc))
    edges = np.zeros((h, w, nc), np.int64)
    edges[:, w // 2:] = maxval
    edges[h // 2:, ::3] = maxval - edges[h // 2:, ::3]
    edges[::4, ::7] = maxval // 2
    return [("noise", noise), ("edges", edges)]


def oracle_resize(img, nw, nh, maxval):
    from oracle import oracle as O
    h, w, nc = img.shape
    if maxval == 255:
        return O.lanczos3_resize(img.astype(np.uint8), nw, nh)
    src = np.ascontiguousarray(img, dtype=np.uint16)
    out = np.empty((nh, nw, nc), np.uint16)
    O.lib().cso_lanczos3_resize16(src.ctypes.data, w, h, nc, nw, nh, out.ctypes.data)
    return out


def test_model_matches_pillow():
    """Pillow's Image.resize(LANCZOS) on mode "F" (float64 coefficients, its own code) against the model with f64 positions, one channel
    at a time.  Pillow's window rule differs from B.11 only by taps of zero weight."""
    worst = 0.0
    for k, (w, h, nw, nh) in enumerate(SHAPES):
        for name, a in battery(k, h, w, 1, 255) + [("float", np.random.default_rng(99 + k).random((h, w, 1)) * 255)]:
            got = np.asarray(PIL.fromarray(a[:, :, 0].astype(np.float32), "F").resize((nw, nh), PIL.LANCZOS), np.float64)
            v, _ = M.resize(a, nw, nh, 255, f32_positions=False, clamp=False)
            d = float(np.abs(got - v[:, :, 0]).max())
            assert d <= 1e-4, (w, h, nw, nh, name, d)
            worst = max(worst, d)
    print(f"model vs Pillow: max |difference| {worst:.3g} over {len(SHAPES)} shapes")


@pytest.mark.parametrize("maxval", [255, 65535], ids=["8bit", "16bit"])
def test_oracle_obeys_the_rule(maxval):
    ties, samples = [], 0
    for k, (w, h, nw, nh) in enumerate(SHAPES):
        for nc in ((1, 3) if w * h > 10000 else (1, 2, 3, 4)):
            for name, a in battery(10 * k + nc, h, w, nc, maxval):
                v, delta = M.resize(a, nw, nh, maxval)
                t = M.assert_rule(oracle_resize(a, nw, nh, maxval), v, delta, f"{w}x{h}->{nw}x{nh} c{nc} {name}")
                ties.append(t)
                samples += v.size
    print(f"oracle {maxval}: {samples} samples, {sum(ties)} in the tie band; per case {ties}")


@pytest.mark.parametrize("variant", ["no_half", "no_sratio", "no_norm", "short_edge"])
def test_the_rule_rejects_wrong_models(variant):
    """the oracle's output judged against a deliberately wrong model must break the rule somewhere on the battery -- and judged against the
    right model it does not (test_oracle_obeys_the_rule)"""
    broken = 0
    for maxval in (255, 65535):
        for k, (w, h, nw, nh) in enumerate(SHAPES[:-1]):
            for name, a in battery(10 * k + 3, h, w, 3, maxval):
                v, delta = M.resize(a, nw, nh, maxval, variant=variant)
                broken += M.check(oracle_resize(a, nw, nh, maxval), v, delta)[1]
    print(f"{variant}: {broken} samples break the rule")
    assert broken > 0


def test_positions_are_f32():
    """on a 16-bit 16000 -> 15999 resize, f64 positions move the result by many LSB: the model states them in f32, as image-rs does"""
    a = battery(5, 2, 16000, 1, 65535)[0][1]
    v32, delta = M.resize(a, 15999, 1, 65535)
    v64, _ = M.resize(a, 15999, 1, 65535, f32_positions=False)
    assert np.abs(v32 - v64).max() > 10
    assert M.check(oracle_resize(a, 15999, 1, 65535), v64, delta)[1] > 0
    M.assert_rule(oracle_resize(a, 15999, 1, 65535), v32, delta, "16000->15999")


# ---------------------------------------------------------------- compute_dimensions
SIZES = [(4, 3), (3, 2), (2, 3), (5, 2), (2, 5), (7, 3), (1000, 1), (1, 999), (33, 21), (1920, 1080), (97, 61), (3, 7)]
ASKS = [1, 2, 3, 5, 7, 10, 49, 333]


def test_compute_dimensions_battery_holds_ties():
    """the battery includes asks whose f32 quotient / product is exactly a .5 tie, where round-half-even would differ"""
    ties = 0
    for (w, h) in SIZES:
        r = np.float32(w) / np.float32(h)
        for a in ASKS:
            ties += float(np.float32(np.float32(a) / r)) % 1 == 0.5
            ties += float(np.float32(np.float32(a) * r)) % 1 == 0.5
    assert ties >= 5, ties
    assert M.compute_dimensions(1000, 1, 1, 0) == (1, 1) and M.compute_dimensions(3, 2, 0, 3) == (5, 3)


def test_oracle_compute_dimensions():
    from oracle import oracle as O
    for (w, h) in SIZES:
        for a in ASKS:
            for dw, dh in [(a, 0), (0, a), (a, a + 1)]:
                assert O.compute_dimensions(w, h, dw, dh) == M.compute_dimensions(w, h, dw, dh), (w, h, dw, dh)


def test_device_output_sizes_follow_compute_dimensions():
    """width only, height only and the long edge (the CLI's --long-edge sets the width of a landscape picture, the height otherwise), on
    the emulation build's PNG path"""
    from _util import emul_api, package
    from test_png_webp_emul import make_png
    api = emul_api()
    srcs = {(w, h): make_png(w, h, 8, 0, bytes(range(256)) * (w * h // 256) + bytes(w * h % 256)) for (w, h) in SIZES}
    for a in ASKS:
        for axis in ("width", "height", "long"):
            for side in ("width", "height"):
                pick = [(w, h) for (w, h) in SIZES if side == (axis if axis != "long" else ("width" if w > h else "height"))
                        and max(M.compute_dimensions(w, h, a if side == "width" else 0, a if side == "height" else 0)) <= 4000]
                if not pick:
                    continue
                outs = api.cs_batch_compress([srcs[s] for s in pick], package().default_parameters(png_optimize=True, png_optimization_level=0, **{side: a}))
                for (w, h), out in zip(pick, outs):
                    assert not isinstance(out, Exception), (w, h, side, a, out)
                    want = M.compute_dimensions(w, h, a if side == "width" else 0, a if side == "height" else 0)
                    assert PIL.open(io.BytesIO(out)).size == want, (w, h, side, a)
