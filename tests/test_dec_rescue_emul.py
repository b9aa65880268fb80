"""The rescue paths of the parallel JPEG decoder (k_decode_par.hip: k_dec_mark_pending, k_dec_dense<3>, k_dec_chain, and the hand-over to the sequential
kernel through need_seq = 2) on the CPU emulation build.  No ordinary input leaves a relaxation list behind the ~510 list rounds a run may take, so the
tests cap the rounds with CSH_TEST_DEC_ROUNDS = 0, 1, 3: whatever is still listed then goes through the label chain, which either settles the scan's
block-in-MCU labels or gives the image to the sequential kernel.  Either way the files must be the oracle's and those of the same call without the cap, and
csh_timing's counters (n_dec_rounds, n_dec_walked, n_dec_chain_scans, n_dec_chain_failed, n_par_fallback, n_seq_decoded) must agree with each other.
A second part builds a file whose labels really creep (one table pair for all three components), for the lanes that walk on (CSH_LIST_WALK).
Bodies shared with tests/test_zzz_dec_rescue_gpu.py."""
import functools
import io

import numpy as np
import pytest

import test_dec_group_emul as E
import test_pipeline_emul as P
from _util import emul_api, oracle_lossless, oracle_lossy
from gen_synth import synth_jpeg

CAPS = (0, 1, 3)
GROUPS = (1, 4)
ORDERS = (None, "jacobi", "reverse")   # the emulation's execution orders (csh_emul_set_*); a device has its own


@pytest.fixture(scope="module")
def api():
    return emul_api()


# ---- inputs: small files, every one of which lists something in the first relaxation pass (asserted with the cap at 0)
@functools.lru_cache(None)
def inputs(name):
    if name == "label_creep": return [synth_jpeg(9, 320, 240, optimize=True, texture=60), synth_jpeg(3, 640, 480, optimize=True, texture=25)]
    if name == "layouts": return [synth_jpeg(3 + ss, 200, 150, subsampling=ss, texture=20 + 10 * ss) for ss in (2, 1, 0)]
    # (the first scans of an ordinary progressive file synchronise inside a sub-sequence: the guesses are the fixed point and nothing is listed.  At quality 100 the
    # AC scans' blocks are long enough to list; k_dec_chain has no label to settle in such a scan and hands the image over)
    if name == "progressive": return [synth_jpeg(2, 104, 72, quality=100, progressive=True, texture=60), P.deep_refinement_file()]
    if name == "long_blocks": return [P.long_block_jpeg(), E.q100_noise()]
    if name == "restart": return [P.restart_cases()[0], P.restart_cases()[1]]   # several segments an image: some are still listed, some are not
    if name == "mixed": return [E.grey_by_pieces()[1], synth_jpeg(9, 320, 240, optimize=True, texture=60)]   # one sub-sequence: nothing to list, beside a file that lists
    raise KeyError(name)


NAMES = ("label_creep", "layouts", "progressive", "long_blocks", "restart", "mixed")


def counters(t):
    return {k: int(getattr(t, k)) for k in ("n_dec_rounds", "n_dec_walked", "n_dec_chain_scans", "n_dec_chain_failed", "n_par_fallback", "n_seq_decoded", "n_prog_decoded", "n_images")}


_runs = {}


def run(api, monkeypatch, name, cap, G, lossless, order=None, srcs=None):
    """files and counters of one call, cached: cap None = CSH_TEST_DEC_ROUNDS unset"""
    key = (id(api), name, cap, G, lossless, order)
    if key not in _runs:
        if cap is None: monkeypatch.delenv("CSH_TEST_DEC_ROUNDS", raising=False)
        else: monkeypatch.setenv("CSH_TEST_DEC_ROUNDS", str(cap))
        _, t, outs = E.run(api, monkeypatch, srcs or inputs(name), G, lossless, emul_mode=order)
        monkeypatch.delenv("CSH_TEST_DEC_ROUNDS", raising=False)
        assert t.n_dec_group == G
        _runs[key] = (outs, counters(t))
    return _runs[key]


@functools.lru_cache(None)
def oracle_files(name, lossless):
    return [oracle_lossless(s) if lossless else oracle_lossy(s) for s in inputs(name)]


def identities(c, cap, what):
    assert c["n_dec_rounds"] <= (cap if cap is not None else 510), what
    assert c["n_dec_chain_failed"] <= c["n_dec_chain_scans"], what
    assert (c["n_par_fallback"] >= 1) == (c["n_dec_chain_failed"] >= 1), what
    assert c["n_par_fallback"] <= c["n_images"], what
    assert c["n_par_fallback"] <= c["n_dec_chain_failed"], what   # (an image falls back because a scan of it failed)


def check_rescue(api, monkeypatch, name, cap, G, orders=(None,)):
    for lossless in (False, True):
        want = oracle_files(name, lossless)
        for order in orders:
            what = (name, cap, G, "lossless" if lossless else "lossy", order)
            free, cf = run(api, monkeypatch, name, None, G, lossless, order)
            outs, c = run(api, monkeypatch, name, cap, G, lossless, order)
            print(f"{name} cap={cap} G={G} {'lossless' if lossless else 'lossy'} order={order}: " + " ".join(f"{k}={v}" for k, v in c.items()) +
                  f" | uncapped: n_dec_rounds={cf['n_dec_rounds']} n_dec_chain_scans={cf['n_dec_chain_scans']} n_par_fallback={cf['n_par_fallback']}")
            for i, (o, w, f) in enumerate(zip(outs, want, free)):
                assert not isinstance(o, Exception), (what, i, o)
                assert o == w, (what, i, "oracle")
                assert o == f, (what, i, "CSH_TEST_DEC_ROUNDS unset")
            identities(c, cap, what)
            identities(cf, None, what)
            # every fallen-back image is one the sequential kernel did; the images it does anyway are the same with and without the cap
            assert c["n_seq_decoded"] - c["n_par_fallback"] == cf["n_seq_decoded"] - cf["n_par_fallback"], what
            assert cf["n_prog_decoded"] - c["n_par_fallback"] <= c["n_prog_decoded"] <= cf["n_prog_decoded"] + cf["n_par_fallback"], what   # (a progressive file that falls back leaves that count)
            if cap == 0:   # the first relaxation pass lists something whenever the guessed states are no fixed point, in whatever order the lanes run
                assert c["n_dec_rounds"] == 0 and c["n_dec_chain_scans"] >= 1, what


# ---- a file that really creeps.  Three components, 4:4:4, ALL with DC table 0 and AC table 0: a lane that enters a sub-sequence with a wrong block-in-MCU label
# decodes the same bits to the same positions, so nothing but the label is wrong and the correction travels one cut per evaluation through the whole scan.
def creeping_jpeg(w=512, h=384, seed=17):
    """baseline 4:4:4, standard luma tables named by every component, random short blocks (a DC difference and a few small AC coefficients)"""
    from PIL import Image
    b = io.BytesIO(); Image.new("RGB", (w, h), (128, 128, 128)).save(b, format="JPEG", quality=90, subsampling=0, optimize=False); ref = b.getvalue()
    segs = {}; i = 2
    while ref[i + 1] != 0xDA:
        L = int.from_bytes(ref[i + 2:i + 4], "big"); segs.setdefault(ref[i + 1], []).append(ref[i:i + 2 + L]); i += 2 + L
    sos = bytearray(ref[i:i + 2 + int.from_bytes(ref[i + 2:i + 4], "big")])
    assert sos[4] == 3
    for c in range(3): sos[5 + 2 * c + 1] = 0x00   # Td = Ta = 0 for Y, Cb and Cr
    tabs = {}
    for seg in segs[0xC4]:
        p = 4
        while p < len(seg):
            bits = seg[p + 1:p + 17]; n = sum(bits); vals = seg[p + 17:p + 17 + n]
            code, k, enc = 0, 0, {}
            for l in range(1, 17):
                for _ in range(bits[l - 1]): enc[vals[k]] = (code, l); code += 1; k += 1
                code <<= 1
            tabs[seg[p]] = enc; p += 17 + n
    rng = np.random.default_rng(seed)
    out = []; acc = 0; nb = 0
    def put(v, n):
        nonlocal acc, nb
        acc = (acc << n) | (v & ((1 << n) - 1)); nb += n
        while nb >= 8:
            byte = (acc >> (nb - 8)) & 255; out.append(byte)
            if byte == 255: out.append(0)
            nb -= 8
    def coef(table, run, v):
        a = abs(v); s = a.bit_length()
        c, l = table[(run << 4) | s]; put(c, l)
        if s: put(v if v > 0 else v - 1, s)
    pred = [0, 0, 0]
    for _ in range(((w + 7) // 8) * ((h + 7) // 8)):
        for c in range(3):
            dc = int(rng.integers(-60, 60)); coef(tabs[0x00], 0, dc - pred[c]); pred[c] = dc
            k = 1
            for _ in range(int(rng.integers(2, 7))):
                r = int(rng.integers(0, 3))
                if k + r > 63: break
                coef(tabs[0x10], r, int(rng.integers(1, 8)) * int(rng.choice([-1, 1]))); k += r + 1
            if k <= 63: put(*tabs[0x10][0x00])
    if nb: put((1 << (8 - nb)) - 1, 8 - nb)
    head = ref[:2] + b"".join(s for m in (0xE0, 0xDB, 0xC0, 0xC4) for s in segs.get(m, []))
    return head + bytes(sos) + bytes(out) + b"\xff\xd9"


@functools.lru_cache(None)
def creeping_file():
    src = creeping_jpeg()
    assert E.par_segments(src)[0] >= 300 * E.SUB   # at least 300 sub-sequences in the one scan
    return src


def check_creep(api, monkeypatch, G, orders=(None,), on_emulation=False):
    src = creeping_file()
    for lossless in (False, True):
        want = oracle_lossless(src) if lossless else oracle_lossy(src)
        for order in orders:
            what = ("creep", G, lossless, order)
            outs, c = run(api, monkeypatch, "creep", None, G, lossless, order, srcs=[src])
            print(f"creep G={G} {'lossless' if lossless else 'lossy'} order={order}: " + " ".join(f"{k}={v}" for k, v in c.items()))
            assert outs[0] == want, what
            identities(c, None, what)
            assert c["n_seq_decoded"] == c["n_par_fallback"], what
            # where the emulation creeps: in descending order every pass is a Jacobi sweep; the jacobi switch makes the list rounds read the states of before the
            # launch, but a group of 1 has its first relaxation pass (k_dec_dense<1>, in place and ascending) settle the chain before any list round
            if on_emulation and (order == "reverse" or (order == "jacobi" and G > 1)):
                assert c["n_dec_rounds"] > 12, what   # (the first twelve are launched without a look at the list: more means it was not empty behind them)
                assert c["n_dec_walked"] >= 1, what
            if on_emulation:
                assert c["n_par_fallback"] == 0, what   # holds in the emulation's three orders; a device's schedule is its own


# ---- the emulation's tests
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", NAMES)
def test_emul_rescue(api, monkeypatch, name, cap, G):
    check_rescue(api, monkeypatch, name, cap, G, orders=ORDERS)


def test_emul_rescue_both_outcomes(api, monkeypatch):
    """over the battery the chain both settles scans (the images stay with the parallel decoder) and fails (they go to the sequential kernel)"""
    settled = failed = 0
    for name in NAMES:
        for G in GROUPS:
            for order in ORDERS:
                _, c = run(api, monkeypatch, name, 0, G, False, order)
                if c["n_dec_chain_scans"] > c["n_dec_chain_failed"] and c["n_par_fallback"] < c["n_images"]: settled += c["n_dec_chain_scans"] - c["n_dec_chain_failed"]
                failed += c["n_dec_chain_failed"]
    print(f"scans the chain settled: {settled}, scans it handed to the sequential kernel: {failed}")
    assert settled >= 1 and failed >= 1


@pytest.mark.parametrize("G", GROUPS)
def test_emul_labels_creep_and_lanes_walk(api, monkeypatch, G):
    check_creep(api, monkeypatch, G, orders=ORDERS, on_emulation=True)
