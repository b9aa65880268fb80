"""Grouped speculation of the parallel JPEG decoder (k_decode_par.hip k_dec_spec_group, CSH_DEC_GROUP = G: a lane carries its state through G consecutive
128-byte sub-sequences; only the first of every group -- the seam -- starts from a guess and is relaxed) on the CPU emulation build.  Every check compares
three things: the files with the oracle's, the files with the same call under CSH_DEC_GROUP=1, and csh_timing's counters with a model computed from the
file itself: n_dec_group is what was asked for, n_dec_seeds the sum over the parallel-decoded scans and restart segments of ceil(live sub-sequences / G),
live = ceil(unstuffed bytes / 128).  Bodies shared with tests/test_dec_group_gpu.py."""
import ctypes
import functools
import io

import numpy as np
import pytest

import test_pipeline_emul as P
from _util import emul_api, oracle_lossless, oracle_lossy, package
from gen_synth import synth_jpeg, synth_rgb

GROUPS = (2, 4, 8, None)   # None: the switch unset -- the planner's choice, one lane per sub-sequence for batches this small
SUB = 128                  # CSH_SUBSEQ_BYTES


@pytest.fixture(scope="module")
def api():
    return emul_api()


def params(**kw):
    return package().default_parameters(**kw)


# ---- the model: what the parallel decoder cuts into sub-sequences, read from the file
def par_segments(src):
    """unstuffed lengths of the scans (restart segments) of a well-formed file that the parallel decoder speculates on: every scan of a sequential-mode
    file, the first scans (Ah = 0) of a progressive one"""
    out, i, dri = [], 2, 0
    while i + 4 <= len(src) and src[i] == 0xFF and src[i + 1] != 0xD9:
        m, L = src[i + 1], int.from_bytes(src[i + 2:i + 4], "big")
        if m == 0xDD:
            dri = int.from_bytes(src[i + 4:i + 6], "big")
        if m != 0xDA:
            i += 2 + L
            continue
        ah = src[i + 2 + L - 1] >> 4
        j = start = i + 2 + L
        pieces = []
        while j < len(src):
            if src[j] == 0xFF and j + 1 < len(src) and src[j + 1] != 0:
                if not (dri and 0xD0 <= src[j + 1] <= 0xD7):
                    break
                pieces.append(src[start:j]); j += 2; start = j
                continue
            j += 1
        pieces.append(src[start:j])
        if ah == 0:
            out += [len(p) - p.count(b"\xff\x00") for p in pieces]
        i = j
    return out


def model(srcs, G):
    segs = [n for s in srcs for n in par_segments(s)]
    live = [(n + SUB - 1) // SUB for n in segs]
    return sum((l + G - 1) // G for l in live), sum(live)


def run(api, monkeypatch, srcs, G, lossless=False, quality=80, emul_mode=None):
    if G is None: monkeypatch.delenv("CSH_DEC_GROUP", raising=False)
    else: monkeypatch.setenv("CSH_DEC_GROUP", str(G))
    setter = getattr(api.L, "csh_emul_set_" + emul_mode) if emul_mode else None
    if setter:
        setter.argtypes = [ctypes.c_int]
        setter(1)
    try:
        b = api.batch(srcs, params(jpeg_optimize=True) if lossless else params(jpeg_quality=quality))
        t = b.run()
        return b, t, b.fetch()
    finally:
        if setter: setter(0)


_want = {}


def check(api, monkeypatch, name, srcs, G, lossless=False, on_par=True, emul_mode=None):
    """the three comparisons; on_par: no image leaves the parallel decoder (what the pipeline tests assert for these inputs; streams that hardly
    synchronise may be handed to the sequential kernel on a GPU, whatever G)"""
    key = (name, lossless, emul_mode, id(api))
    if key not in _want:   # the oracle's files and the G = 1 run's, once per case
        _, t1, ungrouped = run(api, monkeypatch, srcs, 1, lossless, emul_mode=emul_mode)
        assert t1.n_dec_group == 1
        _want[key] = ([oracle_lossless(s) if lossless else oracle_lossy(s) for s in srcs], ungrouped)
    want, ungrouped = _want[key]
    b, t, outs = run(api, monkeypatch, srcs, G, lossless, emul_mode=emul_mode)
    for i, (o, w, u) in enumerate(zip(outs, want, ungrouped)):
        assert not isinstance(o, Exception), (name, i, o)
        assert o == w, (name, G, i, "oracle")
        assert o == u, (name, G, i, "CSH_DEC_GROUP=1")
    seeds, live = model(srcs, G or 1)
    assert t.n_dec_group == (G if G else (8 if live >= 1 << 20 else 4 if live >= 1 << 19 else 2 if live >= 1 << 16 else 1))   # (batch.hpp dec_group_for)
    if t.n_dec_group > 1:
        print(f"{name} G={G}: n_dec_seeds {t.n_dec_seeds} (model {seeds}), n_dec_relaxed {t.n_dec_relaxed} of {live} live sub-sequences")
        assert t.n_dec_seeds == seeds, (name, G)
        assert t.n_dec_relaxed >= seeds
    if on_par:
        assert t.n_par_fallback == 0 and t.n_seq_decoded == 0, (name, G)
    return b, t


# ---- inputs
@functools.lru_cache(None)
def grey_by_pieces():
    """grey baseline pictures of 8 x 8 up to 104 x 72 by the number of sub-sequences their scan has: 1 .. 17 = 2 G + 1 for G = 8"""
    from PIL import Image
    found = {}
    for w in range(8, 105, 8):
        for h in range(8, 73, 8):
            for q in (50, 75, 90, 95):
                b = io.BytesIO(); Image.fromarray(synth_rgb(31, w, h, 30)).convert("L").save(b, format="JPEG", quality=q)
                n = (par_segments(b.getvalue())[0] + SUB - 1) // SUB
                found.setdefault(n, b.getvalue())
    return found


def group_edge_files():
    g = grey_by_pieces()
    return [g[n] for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)]   # 1, G - 1, G, G + 1, 2 G + 1 pieces for G = 2, 4, 8


def cut_files(G):
    """a 4:2:0 baseline file cut in the first, a middle and the last sub-sequence of a group, and exactly on a group's boundary (positions in unstuffed bytes)"""
    src = synth_jpeg(6, 200, 150, texture=30)
    start = src.index(b"\xff\xda"); start += 2 + int.from_bytes(src[start + 2:start + 4], "big")
    data = src[start:src.rindex(b"\xff\xd9")]
    G = G or 4
    assert len(data) - data.count(b"\xff\x00") > 3 * G * SUB
    out = []
    for want in (G * SUB + 10, (G + G // 2) * SUB + 60, (2 * G - 1) * SUB + 100, 2 * G * SUB):
        n = u = 0   # n stuffed bytes hold u = want unstuffed ones
        while u < want:
            n += 2 if data[n:n + 2] == b"\xff\x00" else 1
            u += 1
        assert data[n - 1] != 0xFF or data[n - 2:n] == b"\xff\x00"
        out.append(src[:start] + data[:n] + b"\xff\xd9")
        assert par_segments(out[-1]) == [want]
    return out


def q100_noise():
    from PIL import Image
    b = io.BytesIO(); Image.fromarray(np.random.default_rng(11).integers(0, 256, (120, 160, 3), dtype=np.uint8)).save(b, format="JPEG", quality=100, subsampling=0)
    return b.getvalue()


# ---- bodies
def check_group_edges(api, monkeypatch, G):
    check(api, monkeypatch, "grey_edges", group_edge_files(), G)
    check(api, monkeypatch, "layouts", [synth_jpeg(3 + ss, 200, 150, subsampling=ss, texture=20 + 10 * ss) for ss in (2, 1, 0)], G)
    check(api, monkeypatch, "short_and_long", [grey_by_pieces()[1], synth_jpeg(1, 400, 300, texture=25)], G)   # max_sub and the grid are the other image's


def check_restart_intervals(api, monkeypatch, G):
    srcs = P.restart_cases()[:7] + [synth_jpeg(9, 320, 128, restart_rows=1, texture=15)]
    segs = [(n + SUB - 1) // SUB for s in srcs for n in par_segments(s)]
    assert min(segs) == 1 and any(n > 8 and n % 8 for n in segs)   # segments shorter than any group; segments whose last group is partial
    check(api, monkeypatch, "restart", srcs, G)


def check_streams_cut_short(api, monkeypatch, G):
    check(api, monkeypatch, f"cut{G or 4}", cut_files(G), G)
    check(api, monkeypatch, f"cut{G or 4}", cut_files(G), G, lossless=True)


def check_progressive_first_scans(api, monkeypatch, G):
    srcs = [synth_jpeg(2, 200, 150, progressive=True, texture=20), P.deep_refinement_file()]
    check(api, monkeypatch, "progressive", srcs, G, lossless=True)
    check(api, monkeypatch, "progressive", srcs, G)


def check_label_creep(api, monkeypatch, G, emul_modes=(None,)):
    srcs = [synth_jpeg(9, 320, 240, optimize=True, texture=60), synth_jpeg(3, 640, 480, optimize=True, texture=25)]
    for mode in emul_modes:
        check(api, monkeypatch, "label_creep", srcs, G, emul_mode=mode)


def check_slow_synchronisation(api, monkeypatch, G):
    check(api, monkeypatch, "long_blocks", [P.long_block_jpeg(), q100_noise()], G, on_par=False)
    check(api, monkeypatch, "six_tables", [P.six_tables(synth_jpeg(3, 203, 155, texture=30)), synth_jpeg(5, 160, 120, texture=20),
                                           P.six_tables(synth_jpeg(8, 333, 222, restart_rows=1, texture=25))], G)


def check_reruns(api, monkeypatch, G):
    """the clearing and the seeds are per run: the same batch three times, and a re-quantisation run between two full ones"""
    srcs = [synth_jpeg(i, 160 + 16 * i, 120, subsampling=(0, 2, 1)[i % 3], texture=10 + 9 * i) for i in range(3)]
    b, t = check(api, monkeypatch, "reruns", srcs, G)
    first = b.fetch()
    for _ in range(2):
        t2 = b.run()
        assert b.fetch() == first
        assert (t2.n_dec_group, t2.n_dec_seeds, t2.n_dec_relaxed) == (t.n_dec_group, t.n_dec_seeds, t.n_dec_relaxed)
    b.retain_dct()
    b.run()
    b.set_quality([33, 97, 61])
    tq = b.rerun_encode()
    assert (tq.n_dec_seeds, tq.n_dec_relaxed) == (0, 0)   # nothing is decoded in such a run
    for src, out, q in zip(srcs, b.fetch(), (33, 97, 61)):
        assert out == oracle_lossy(src, q)
    b.set_quality([80, 80, 80])
    t3 = b.run()
    assert b.fetch() == first and t3.n_dec_seeds == t.n_dec_seeds


# ---- the emulation's tests
@pytest.mark.parametrize("G", GROUPS)
def test_emul_group_edges(api, monkeypatch, G):
    check_group_edges(api, monkeypatch, G)


@pytest.mark.parametrize("G", GROUPS)
def test_emul_restart_intervals(api, monkeypatch, G):
    check_restart_intervals(api, monkeypatch, G)


@pytest.mark.parametrize("G", GROUPS)
def test_emul_streams_cut_short(api, monkeypatch, G):
    check_streams_cut_short(api, monkeypatch, G)


@pytest.mark.parametrize("G", GROUPS)
def test_emul_progressive_first_scans(api, monkeypatch, G):
    check_progressive_first_scans(api, monkeypatch, G)


@pytest.mark.parametrize("G", GROUPS)
def test_emul_label_creep(api, monkeypatch, G):
    check_label_creep(api, monkeypatch, G, emul_modes=("jacobi", "reverse"))


@pytest.mark.parametrize("G", GROUPS)
def test_emul_slow_synchronisation(api, monkeypatch, G):
    check_slow_synchronisation(api, monkeypatch, G)


@pytest.mark.parametrize("G", GROUPS)
def test_emul_reruns(api, monkeypatch, G):
    check_reruns(api, monkeypatch, G)
