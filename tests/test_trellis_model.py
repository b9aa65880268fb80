"""The trellis quantiser against its own stated cost model, in float64 (tests/_trellis_model.py): whatever levels the oracle and the
emulation build write must be admissible and of minimum model cost, block by block (AC) and row by row (DC), up to float32 rounding.
Byte parity with the oracle cannot see a mistake the oracle and the kernel share; this can.  The same checks run on the MI355X in
tests/test_trellis_model_gpu.py.  The model's constants stay unpinned (oracle/jpeg_oracle.c, the comment above quantize_trellis_row)."""
import functools
import io
from dataclasses import dataclass

import numpy as np
import pytest

import _trellis_model as M
from _util import emul_api, package
from gen_synth import synth_jpeg, synth_rgb
from test_trellis_emul import saturated_jpeg

SS = {444: 0, 422: 1, 420: 2}


@dataclass(frozen=True)
class Case:
    name: str
    src: bytes
    q: int = 80
    ss: int = 420
    width: int = 0


# profile -> (oracle switches, CSH_PROFILE of the device library, extra device parameters)
PROFILES = {"default": (dict(trellis=1, deringing=1, progressive=1), "mozjpeg", {}),
            "trellis": (dict(trellis=1, deringing=0, progressive=1), "mozjpeg-trellis", {}),
            "baseline": (dict(trellis=1, deringing=1, progressive=0), "mozjpeg", dict(jpeg_progressive=False))}


def _jpg(a, quality=100, subsampling=0):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8)).save(b, format="JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()


def _noise(seed, w, h, grey=False):
    rng = np.random.default_rng(seed)
    return _jpg(rng.integers(0, 256, (h, w) if grey else (h, w, 3)), 100)


def battery():
    """the inputs every check runs over; test_battery_reaches_its_edges asserts what each is for"""
    cases = []
    tex = synth_jpeg(21, 64, 48, texture=40)
    for q in (1, 5, 30, 80, 95, 100):                                              # 16-bit tables at q <= 10; 3, 5, 9 DC candidates
        cases.append(Case(f"q{q}", tex, q))
    for ss in (444, 422):
        cases.append(Case(f"ss{ss}", synth_jpeg(22, 72, 40, subsampling=SS[ss], texture=30), 80, ss))
    from PIL import Image
    g = io.BytesIO()
    Image.fromarray(synth_rgb(23, 57, 43, 25)).convert("L").save(g, format="JPEG", quality=90)
    cases.append(Case("grey", g.getvalue(), 80))
    for (w, h) in ((1, 1), (1, 17), (8, 9), (9, 8), (15, 16), (16, 15), (17, 17), (17, 1), (97, 61)):   # dummy blocks, one-block rows
        cases.append(Case(f"{w}x{h}", synth_jpeg(24 + w + h, w, h, texture=50), 80, 422 if w == 17 else 420))
    cases.append(Case("black_q100", _jpg(np.zeros((16, 24, 3))), 100, 444))     # scalar DC -1024: the DC candidates clamp to -1023
    yy, xx = np.mgrid[0:32, 0:48]
    sx, sy = np.isin(xx % 4, (0, 3)), np.isin(yy % 4, (0, 3))
    cases.append(Case("basis44_q100", _jpg(np.where(sx == sy, 255, 0)), 100, 444))   # with deringing: scalar AC levels past 1023
    cases.append(Case("saturated", saturated_jpeg(96, 72), 80, 420))
    cases.append(Case("noise_q100", _noise(25, 40, 24), 100, 444))                 # 63 keepable positions per block
    cases.append(Case("noise_grey_q100", _noise(26, 40, 40, grey=True), 100))      # every block runs to 63: no EOB in a sequential table
    cases.append(Case("noise_q60", _noise(27, 48, 32), 60, 420))                   # 15..17 keepable positions
    cases.append(Case("flat", synth_jpeg(28, 64, 32, texture=0), 30, 420))         # 0 and 1 keepable positions
    cases.append(Case("resized", synth_jpeg(29, 120, 90, texture=30), 80, 420, width=50))
    return cases


_BATTERY = None


def cached_battery():
    global _BATTERY
    if _BATTERY is None:
        _BATTERY = battery()
    return _BATTERY


def oracle_params(case, prof):
    from oracle import oracle as O
    sw = PROFILES[prof][0]
    return O.params(quality=case.q, progressive=sw["progressive"], subsampling=case.ss, qtable_profile=3, marker_style=1, scan_script=2,
                    trellis=sw["trellis"], deringing=sw["deringing"])


@functools.lru_cache(maxsize=None)
def oracle_file(case, prof):
    from oracle import oracle as O
    p = oracle_params(case, prof)
    return O.jpeg_compress_resized(case.src, p, case.width, 0) if case.width else O.jpeg_compress(case.src, p)


@functools.lru_cache(maxsize=None)
def export(case, prof, **switches):
    from oracle import oracle as O
    p = oracle_params(case, prof)
    for k, v in switches.items():
        setattr(p, k, v)
    return O.trellis_inputs(case.src, p, case.width, 0)


def device_params(case, prof):
    return package().default_parameters(jpeg_quality=case.q, jpeg_chroma_subsampling=case.ss, width=case.width, **PROFILES[prof][2])


def decoded_levels(blob):
    from oracle import oracle as O
    d = O.decode(blob)
    return [d.coefs(ci) for ci in range(d.im.ncomp)]


def verify(comps, blob, what, knobs=M.DEFAULT):
    """every component of a file's levels admissible and optimal under the model; returns the worst relative gap seen"""
    levels = decoded_levels(blob)
    assert len(levels) == len(comps), what
    worst = 0.0
    for ci, (lv, comp) in enumerate(zip(levels, comps)):
        assert lv.shape == comp["raw"].shape, (what, ci)
        ch = M.check_component(lv, comp, knobs)
        where = (what, ci)
        assert not ch.bad.any(), (where, "inadmissible blocks", np.argwhere(ch.bad)[:8].tolist())
        assert not ch.ac_flagged().any(), (where, "AC not optimal", np.argwhere(ch.ac_flagged())[:8].tolist(), ch.ac_gap.max())
        assert not ch.dc_flagged().any(), (where, "DC row not optimal", np.argwhere(ch.dc_flagged())[:8].tolist(), ch.dc_gap.max())
        # the solver must never be beaten: a cost below its optimum is a solver bug
        assert (ch.ac_gap >= -M.tolerance(ch.ac_opt, ch.ac_zero)).all() and (ch.dc_gap >= -M.tolerance(ch.dc_opt)).all(), (where, "solver beaten")
        worst = max(worst, float((ch.ac_gap / M.tolerance(ch.ac_opt, ch.ac_zero)).max(initial=0)), float((ch.dc_gap / M.tolerance(ch.dc_opt)).max(initial=0)))
    return worst


# ---------------------------------------------------------------- the solver against brute force
def _random_tables(rng, n):
    tabs = []
    for t in range(n):
        aclen = rng.integers(2, 17, 256)
        holes = rng.random(256) < (0.0, 0.15, 0.4)[t % 3]
        aclen[holes] = 0
        if t % 4 == 1:
            aclen[0xF0] = 0
        if t % 5 == 2:
            aclen[0] = 0
        tabs.append(aclen)
    return tabs


def test_ac_solver_equals_brute_force():
    """over a thousand seeded random blocks with up to 7 keepable positions, random tables (holes, no ZRL, free EOB), every knob"""
    rng = np.random.default_rng(1234)
    tabs = _random_tables(rng, 24)
    n = 0
    for knobs in (M.DEFAULT, M.Knobs(lam_scale=3.0, zrl=False), M.Knobs(eob=False, extra_cand=True)):
        for b in range(700):
            aclen = tabs[b % len(tabs)]
            qt = rng.integers(1, 40, 64)
            raw = np.zeros(64, np.int64)
            k = int(rng.integers(0, 8))
            pos = rng.choice(63, k, replace=False) + 1
            if b % 3 == 0:
                pos = np.sort(rng.choice(np.arange(30, 64), k, replace=False))      # long runs: ZRL
            z = M.ZZ[pos]
            raw[z] = rng.integers(-90, 91, k) * qt[z] * 8 // rng.integers(1, 16)
            raw[M.ZZ[np.setdiff1d(np.arange(1, 64), pos)]] = rng.integers(-3, 4, 63 - k) * qt[M.ZZ[np.setdiff1d(np.arange(1, 64), pos)]]
            raw[0] = rng.integers(-8000, 8000)
            cand = M._ac_setup(raw, qt, knobs)[5][0]
            if np.prod([1 + len(set(c[c > 0].tolist())) for c in cand[1:]]) > 2000:   # keep the enumeration small
                continue
            opt = M.ac_optimum(raw[None], qt, aclen, knobs)[0]
            bf = M.ac_bruteforce(raw, qt, aclen, knobs)
            assert abs(opt - bf) <= 1e-9 * max(1.0, abs(bf)) or (np.isinf(opt) and np.isinf(bf)), (knobs, b, opt, bf)
            n += 1
    assert n > 1200, n


def test_dc_solver_equals_brute_force():
    rng = np.random.default_rng(99)
    for t in range(200):
        qt0 = int(rng.choice([1, 2, 7, 13, 27, 40, 800]))
        nb = int(rng.integers(1, 4))
        raw_dc = rng.integers(-8192, 8192, nb)
        lam_row = rng.uniform(0.01, 0.4, nb)
        dclen = rng.integers(0, 12, 17)
        prev = int(rng.integers(-1023, 1024)) if t % 2 else 0
        raw = np.zeros((1, nb, 64), np.int64)
        raw[0, :, 0] = raw_dc
        # lambda enters dc_rows through the block's AC energy: give each block the AC that yields lam_row
        norm = M.LAMBDA_C1 / lam_row - M.LAMBDA_C2
        raw[0, :, 1] = np.sqrt(np.maximum(norm, 0) * 63).round().astype(np.int64)
        lam = M.lam(raw[0])
        comp = dict(real_bw=nb, real_bh=2, v=2, qt=np.r_[qt0, np.ones(63, np.int64)], dclen=dclen)
        raw2 = np.concatenate([np.zeros((1, nb, 64), np.int64), raw])        # row 1 continues row 0, which ends on `prev`
        lv = np.zeros((2, nb, 64), np.int64)
        lv[0, nb - 1, 0] = prev
        cand, _ = M._dc_setup(raw_dc, qt0, lam)
        lv[1, :, 0] = cand[:, 0]
        _, opt = M.dc_rows(raw2, lv, comp)
        bf = M.dc_bruteforce_row(raw_dc, lam, qt0, dclen, prev)
        assert abs(opt[1] - bf) <= 1e-9 * max(1.0, bf), (t, opt[1], bf)


# ---------------------------------------------------------------- the export against what is already pinned
def test_export_scalar_levels_are_the_oracles():
    """trellis off: the scalar quantiser of the exported DCT is the oracle's scalar quantiser, deringing on and off"""
    from oracle import oracle as O
    for case in (cached_battery()[3], cached_battery()[0], Case("saturated", saturated_jpeg(96, 72), 95, 444)):
        for der in (0, 1):
            comps = export(case, "default", trellis=0, deringing=der)
            for ci, c in enumerate(comps):
                r, rb = c["raw"][:c["real_bh"], :c["real_bw"]], c["coef"][:c["real_bh"], :c["real_bw"]]
                want = np.sign(r) * M.scalar_levels(r, c["qt"])
                assert np.array_equal(want, rb), (case.name, der, ci)
            blob = O.jpeg_compress(case.src, O.params(quality=case.q, subsampling=case.ss, scan_script=2, deringing=der))
            assert all(np.array_equal(a, c["coef"]) for a, c in zip(decoded_levels(blob), comps)), (case.name, der)


def test_export_dct_is_jfdctint_of_the_samples():
    """deringing off: every real block's DCT is the pinned jfdctint (cso_fdct_islow) of the exported samples"""
    import ctypes as C

    from oracle import oracle as O
    L = O.lib()
    d = np.zeros(64, np.int32)
    for case in cached_battery()[:12:3] + [c for c in cached_battery() if c.name in ("97x61", "resized", "saturated")]:
        for ci, c in enumerate(export(case, "trellis")):
            for by in range(c["real_bh"]):
                for bx in range(c["real_bw"]):
                    s = np.ascontiguousarray(c["samples"][by, bx])
                    L.cso_fdct_islow(s.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
                    assert np.array_equal(d, c["raw"][by, bx]), (case.name, ci, by, bx)


def test_export_levels_are_the_files():
    """the levels the export returns are those of the file the oracle writes"""
    for case in cached_battery()[::4]:
        for prof in PROFILES:
            comps = export(case, prof)
            assert all(np.array_equal(a, c["coef"]) for a, c in zip(decoded_levels(oracle_file(case, prof)), comps)), (case.name, prof)


# ---------------------------------------------------------------- the battery reaches its edges
def edge_counts(cases=None):
    """what the battery exercises, counted from the exported DCT and tables (default profile, plus the sequential tables)"""
    cases = cases or cached_battery()
    keep_hist = np.zeros(64, np.int64)
    out = dict(dc_clamp=0, ac_clamp=0, tables16=0, dc_ncand=set(), no_zrl_tables=0, free_eob_tables=0, dering_changes=0, dummy_blocks=0)
    for case in cases:
        comps = export(case, "default")
        for c in comps:
            r = c["raw"][:c["real_bh"], :c["real_bw"]].reshape(-1, 64)
            s = M.scalar_levels(r, c["qt"])
            keep_hist += np.bincount((s[:, 1:] > 0).sum(axis=1), minlength=64)
            out["dc_clamp"] += int((s[:, 0] > M.MAX_LEVEL).sum())
            out["ac_clamp"] += int((s[:, 1:] > M.MAX_LEVEL).sum())
            out["tables16"] += int(c["qt"].max() > 255)
            out["dc_ncand"].add(min(9, (2 + 60 // int(c["qt"][0])) | 1))
            out["dummy_blocks"] += c["bw"] * c["bh"] - c["real_bw"] * c["real_bh"]
        for prof in ("default", "baseline"):
            for c in (comps if prof == "default" else export(case, prof)):
                out["no_zrl_tables"] += int(c["aclen"][0xF0] == 0)
                out["free_eob_tables"] += int(c["aclen"][0] == 0)
        if any(not np.array_equal(a["raw"], b["raw"]) for a, b in zip(comps, export(case, "trellis"))):
            out["dering_changes"] += 1
    out["keepable"] = {k: int(keep_hist[k]) for k in (0, 1, 15, 16, 17, 63)}
    return out


def test_battery_reaches_its_edges():
    e = edge_counts()
    print("battery edges:", e)
    assert all(n > 0 for n in e["keepable"].values()), e["keepable"]   # k_trellis_ac: 16 list entries in LDS, the rest spill
    assert e["keepable"][16] + e["keepable"][17] + e["keepable"][63] > 20
    assert e["dc_clamp"] > 0                                            # black at q 100: scalar DC -1024
    # scalar AC levels past 1023 need deringing's overshoot: without it |AC| <= 127.5 * 8 = 1020 for 8-bit samples
    assert e["ac_clamp"] > 0
    assert e["tables16"] > 0                                            # q <= 10
    assert e["dc_ncand"] >= {3, 5, 9}, e["dc_ncand"]
    assert e["no_zrl_tables"] > 0 and e["free_eob_tables"] > 0
    assert e["dering_changes"] > 0 and e["dummy_blocks"] > 0


# ---------------------------------------------------------------- the producers are optimal and admissible
def test_oracle_optimal_and_admissible():
    worst = 0.0
    for case in cached_battery():
        for prof in PROFILES:
            worst = max(worst, verify(export(case, prof), oracle_file(case, prof), (case.name, prof)))
    print(f"oracle: worst gap {worst:.3g} of the tolerance")


@pytest.fixture(scope="module")
def api():
    return emul_api()


def test_emulation_optimal_admissible_and_the_oracles(api, monkeypatch):
    worst = 0.0
    for prof, (_, env, _) in PROFILES.items():
        monkeypatch.setenv("CSH_PROFILE", env)
        for case in cached_battery():
            out = api.compress_in_memory(case.src, device_params(case, prof))
            assert out == oracle_file(case, prof), (case.name, prof)
            worst = max(worst, verify(export(case, prof), out, (case.name, prof)))
    print(f"emulation: worst gap {worst:.3g} of the tolerance")


# ---------------------------------------------------------------- the check has teeth
def test_scalar_levels_are_flagged():
    """the scalar quantiser's levels are admissible but not optimal: most textured blocks are flagged"""
    flagged = total = 0
    for case in cached_battery()[:6]:
        for c in export(case, "default"):
            r = c["raw"][:c["real_bh"], :c["real_bw"]].reshape(-1, 64)
            textured = (M.scalar_levels(r, c["qt"])[:, 1:] > 0).sum(axis=1) >= 4
            if not textured.any():
                continue
            lv = np.sign(r) * np.minimum(M.scalar_levels(r, c["qt"]), M.MAX_LEVEL)
            opt = M.ac_optimum(r, c["qt"], c["aclen"])
            gap = M.ac_cost(lv, r, c["qt"], c["aclen"]) - opt
            zero = M.ac_cost(np.zeros_like(lv), r, c["qt"], c["aclen"], M.Knobs(eob=False))
            flagged += int((gap > M.tolerance(opt, zero))[textured].sum())
            total += int(textured.sum())
    assert total > 200 and flagged > 0.5 * total, (flagged, total)


KNOBS = {"lambda_x1.02": M.Knobs(lam_scale=1.02), "zrl_off": M.Knobs(zrl=False), "eob_off": M.Knobs(eob=False),
         "dc_row_reset": M.Knobs(dc_row_reset=True)}


@pytest.mark.parametrize("knob", list(KNOBS))
def test_each_term_is_constrained(knob):
    """each perturbation of the model makes the oracle's own output be flagged somewhere in the battery: that term is pinned by the check"""
    knobs = KNOBS[knob]
    flagged = 0
    for case in cached_battery():
        for prof in ("default", "baseline"):
            comps = export(case, prof)
            for ci, (lv, c) in enumerate(zip(decoded_levels(oracle_file(case, prof)), comps)):
                if knob == "dc_row_reset" and not (ci == 0 and c["v"] == 2):
                    continue
                ch = M.check_component(lv, c, knobs)
                flagged += int(ch.ac_flagged().sum() + ch.dc_flagged().sum() + ch.bad.sum())
    assert flagged > 0, knob


def test_extra_candidate_is_dominated_and_the_stated_ones_are_used():
    """the v - 1 knob cannot be flagged, whatever the input: v is the rounded level, so at the same size (hence the same rate) v - 1 is never
    closer to x than v, and when v = 2^k, v - 1 = 2^k - 1 is a candidate already.  What pins the candidate rule instead: the optimum is
    unchanged by the knob, and the producers do pick the intermediate candidates 2^k - 1 < v on many positions, so an optimiser that lacked
    them would be flagged as non-optimal"""
    picked = 0
    for case in cached_battery():
        for c in export(case, "default"):
            r = c["raw"][:c["real_bh"], :c["real_bw"]].reshape(-1, 64)
            a = M.ac_optimum(r, c["qt"], c["aclen"])
            b = M.ac_optimum(r, c["qt"], c["aclen"], M.Knobs(extra_cand=True))
            assert np.allclose(a, b, rtol=1e-12, atol=1e-9), case.name
            lv = np.abs(c["coef"][:c["real_bh"], :c["real_bw"]].reshape(-1, 64))[:, 1:]
            v = np.minimum(M.scalar_levels(r, c["qt"])[:, 1:], M.MAX_LEVEL)
            picked += int(((lv > 0) & (lv < v)).sum())
    assert picked > 100, picked
