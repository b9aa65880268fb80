"""JPEG files whose decoder state changes between two scans of one file (tests only).

DRI, DHT and DQT are state that the scans after them see.  libjpeg recomputes the restart interval of a file written with
restart_marker_rows for every scan (MCUs per row differ between an interleaved scan and a scan of one component), a component keeps the
quantisation table its slot holds when its first scan starts, and any number of 0xFF fill bytes may stand in front of a marker, RSTn included.
battery() makes the files: from Pillow / libjpeg-turbo, from the suite's own writer (tests/_jpeg_layout.py) and by splicing bytes into
either -- no re-encoding.  Each file's precondition (the DRI values per scan, the RSTn per scan, a wrap past RST7) is asserted here by
walking the markers, so a case cannot quietly stop holding the edge it is named after.
"""
import functools
import io

import numpy as np

from _jpeg_layout import LAYOUTS, write_jpeg
from gen_synth import synth_rgb

OK = "ok"
# a component was decoded with other contents than its slot holds at the end of the file: pixels as libjpeg decodes them, but the
# coefficient transcode is refused (libjpeg jpeg_copy_critical_parameters, JERR_MISMATCHED_QUANT_TABLE)
MISMATCHED = "mismatched quantisation table"


def seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _cdiv(a, b):
    return -(-a // b)


def walk(data):
    """-> [(marker, start, end)] in file order: every marker segment (start at its 0xFF, end behind its payload), ("data", start, end)
    for the entropy-coded bytes behind an SOS (RSTn included), 0xD9 for EOI.  Only for files without fill or stray bytes."""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m == 0xD9:
            out.append((m, i, i + 2))
            return out
        ln = int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, i, i + 2 + ln))
        i += 2 + ln
        if m == 0xDA:
            e = i
            while not (data[e] == 0xFF and data[e + 1] != 0 and not 0xD0 <= data[e + 1] <= 0xD7):
                e += 1
            out.append(("data", i, e))
            i = e


def scan_report(data):
    """-> per scan a dict: dri (the interval in force at its SOS), units (MCUs, or the blocks of its one component), rst (the RSTn
    numbers found in its data, in order)"""
    segs, dri, frame, scans = walk(data), 0, None, []
    for k, (m, a, b) in enumerate(segs):
        if m in (0xC0, 0xC1, 0xC2):
            h, w, n = int.from_bytes(data[a + 5:a + 7], "big"), int.from_bytes(data[a + 7:a + 9], "big"), data[a + 9]
            frame = (w, h, {data[a + 10 + 3 * c]: (data[a + 11 + 3 * c] >> 4, data[a + 11 + 3 * c] & 15) for c in range(n)})
        elif m == 0xDD:
            dri = int.from_bytes(data[a + 4:a + 6], "big")
        elif m == 0xDA:
            w, h, comps = frame
            ids = [data[a + 5 + 2 * c] for c in range(data[a + 4])]
            hmax, vmax = max(f[0] for f in comps.values()), max(f[1] for f in comps.values())
            if len(ids) > 1:
                units = _cdiv(w, 8 * hmax) * _cdiv(h, 8 * vmax)
            else:
                ch, cv = comps[ids[0]]
                units = _cdiv(_cdiv(w * ch, hmax), 8) * _cdiv(_cdiv(h * cv, vmax), 8)
            body = data[segs[k + 1][1]:segs[k + 1][2]]
            rst = [body[p + 1] - 0xD0 for p in range(len(body) - 1) if body[p] == 0xFF and 0xD0 <= body[p + 1] <= 0xD7]
            scans.append(dict(dri=dri, units=units, rst=rst))
    return scans


def check_restarts(data):
    """every scan carries the RSTn its interval asks for, numbered 0..7 round and round; -> the report"""
    rep = scan_report(data)
    for s in rep:
        want = -(-s["units"] // s["dri"]) - 1 if s["dri"] else 0
        assert s["rst"] == [k & 7 for k in range(want)], s
    return rep


# ---------------------------------------------------------------- splices
def between_scans(data, k, extra):
    """`extra` behind the data of scan k (0-based), in front of the marker that follows it"""
    ends = [b for (m, a, b) in walk(data) if m == "data"]
    return data[:ends[k]] + extra + data[ends[k]:]


def fill_before_rst(data, n):
    out, last = bytearray(), 0
    for (m, a, b) in walk(data):
        if m != "data":
            continue
        for p in range(a, b - 1):
            if data[p] == 0xFF and 0xD0 <= data[p + 1] <= 0xD7:
                out += data[last:p] + b"\xff" * n
                last = p
    return bytes(out + data[last:])


def fill_before_segments(data, n=1):
    out, last = bytearray(), 0
    for (m, a, b) in walk(data):
        if m != "data":
            out += data[last:a] + b"\xff" * n
            last = a
    return bytes(out + data[last:])


def renumber_components(data, ids=(0, 1, 2)):
    out = bytearray(data)
    old = None
    for (m, a, b) in walk(data):
        if m in (0xC0, 0xC1, 0xC2):
            old = [data[a + 10 + 3 * c] for c in range(data[a + 9])]
            for c in range(len(old)):
                out[a + 10 + 3 * c] = ids[c]
        elif m == 0xDA:
            for c in range(data[a + 4]):
                out[a + 5 + 2 * c] = ids[old.index(data[a + 5 + 2 * c])]
    return bytes(out)


def dqt(slot, table_zigzag):
    return seg(0xDB, bytes([slot]) + bytes(int(v) for v in table_zigzag))


def slot_table(data, slot):
    """the 8-bit table the file's last DQT for `slot` holds, zig-zag order"""
    found = None
    for (m, a, b) in walk(data):
        if m == 0xDB:
            p = a + 4
            while p < b:
                assert data[p] >> 4 == 0
                if data[p] & 15 == slot:
                    found = data[p + 1:p + 65]
                p += 65
    return found


def other_table(table):
    """a table that differs from `table` in every entry"""
    return bytes(min(255, 2 * v + 1) for v in table)


# T.81 Table K.3 (DC luminance): code lengths 2..9, where the writer's own DC code has twelve 4-bit codes
DHT_DC_K3 = seg(0xC4, bytes([0x00]) + bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + bytes(range(12)))


def pillow_jpeg(seed, w, h, texture=20.0, mode="RGB", **kw):
    from PIL import Image
    im = Image.fromarray(synth_rgb(seed, w, h, texture), "RGB")
    if mode != "RGB":
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, format="JPEG", quality=90, **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def battery():
    """-> [(name, file bytes, OK or MISMATCHED)]"""
    cases = []

    def add(name, data, expect=OK):
        cases.append((name, data, expect))
        return data

    # ---- Pillow / libjpeg-turbo: restart_marker_rows makes libjpeg write a DRI per scan
    a = add("prog_420_rows1_104x72", pillow_jpeg(1, 104, 72, progressive=True, subsampling=2, restart_marker_rows=1))
    assert [s["dri"] for s in check_restarts(a)][:3] == [7, 13, 7]        # MCUs per row, luma blocks per row, chroma blocks per row
    a = add("prog_422_rows1_104x72", pillow_jpeg(2, 104, 72, progressive=True, subsampling=1, restart_marker_rows=1))
    assert [s["dri"] for s in check_restarts(a)][:3] == [7, 13, 7]
    a = add("prog_420_rows2_97x61", pillow_jpeg(3, 97, 61, progressive=True, subsampling=2, restart_marker_rows=2))
    dris = {s["dri"] for s in check_restarts(a)}
    assert dris == {14, 26}                                                # luma: 13 real blocks a row, not the 14 of the padded grid
    big = add("prog_420_rows1_104x168", pillow_jpeg(4, 104, 168, progressive=True, subsampling=2, restart_marker_rows=1))
    rep = check_restarts(big)
    assert {s["dri"] for s in rep} == {7, 13} and all(len(s["rst"]) > 8 for s in rep)   # 11 MCU rows: every scan wraps past RST7
    a = add("prog_420_rows1_104x168_flat", pillow_jpeg(4, 104, 168, texture=0.0, progressive=True, subsampling=2, restart_marker_rows=1))
    assert {s["dri"] for s in check_restarts(a)} == {7, 13}
    a = add("prog_grey_rows1_104x72", pillow_jpeg(5, 104, 72, mode="L", progressive=True, restart_marker_rows=1))
    assert {s["dri"] for s in check_restarts(a)} == {13}
    for prog in (True, False):
        for blocks in (5, 3):       # one DRI: MCUs in an interleaved scan, blocks in a scan of one component; neither divides a row
            a = add(f"{'prog' if prog else 'base'}_420_blocks{blocks}_104x168", pillow_jpeg(6, 104, 168, progressive=prog, subsampling=2, restart_marker_blocks=blocks))
            rep = check_restarts(a)
            assert {s["dri"] for s in rep} == {blocks} and all(len(s["rst"]) > 8 for s in rep)
            if prog and blocks == 5:
                progb = a       # the progressive file the splices below start from: one DRI for all its scans
    a = add("prog_444_blocks5_97x61", pillow_jpeg(7, 97, 61, progressive=True, subsampling=0, restart_marker_blocks=5))
    assert {s["dri"] for s in check_restarts(a)} == {5}
    a = add("base_444_blocks5_97x61", pillow_jpeg(7, 97, 61, subsampling=0, restart_marker_blocks=5))
    assert {s["dri"] for s in check_restarts(a)} == {5}
    base = add("base_420_rows1_104x168", pillow_jpeg(8, 104, 168, subsampling=2, restart_marker_rows=1))   # 10 RSTn
    assert [len(s["rst"]) for s in check_restarts(base)] == [10]

    # ---- the suite's own writer: sequential files of one scan per component, a DRI in front of each
    rgb = synth_rgb(9, 97, 61, texture=6.0)
    l420, l444 = LAYOUTS["420"], ((1, 1), (1, 1), (1, 1))
    a = add("seq_420_dri_5_0_3", write_jpeg(rgb, l420, scans=[((0,), 5), ((1,), 0), ((2,), 3)]))   # 104 luma blocks in rows of 13, 28 chroma blocks in rows of 7
    assert [(s["dri"], len(s["rst"])) for s in check_restarts(a)] == [(5, 20), (0, 0), (3, 9)]
    a = add("seq_444_dri_7_0_11", write_jpeg(rgb, l444, scans=[((0,), 7), ((1,), 0), ((2,), 11)]))
    assert [(s["dri"], len(s["rst"])) for s in check_restarts(a)] == [(7, 14), (0, 0), (11, 9)]
    a = add("seq_444_dri_kept_then_changed", write_jpeg(rgb, l444, scans=[((0,), 6), ((1,), None), ((2,), 40)]))   # no DRI in front of Cb: the interval stays
    assert [(s["dri"], len(s["rst"])) for s in check_restarts(a)] == [(6, 17), (6, 17), (40, 2)]
    a = add("seq_420_dri_set_then_cleared", write_jpeg(rgb, l420, scans=[((0, 1, 2), (5, 0))]))
    assert [(s["dri"], len(s["rst"])) for s in check_restarts(a)] == [(0, 0)]
    a = add("seq_444_dri_set_then_cleared", write_jpeg(rgb, l444, scans=[((0,), (4, 0)), ((1,), None), ((2,), None)]))
    assert [(s["dri"], len(s["rst"])) for s in check_restarts(a)] == [(0, 0)] * 3

    # ---- splices: DQT and DHT between scans
    planar = write_jpeg(rgb, l444, scans=[((0,), None), ((1,), None), ((2,), None)])   # Cb and Cr both point at slot 1
    new1 = dqt(1, other_table(slot_table(planar, 1)))
    add("dqt_between_cb_and_cr", between_scans(planar, 1, new1), MISMATCHED)            # Cb keeps what it latched, Cr starts with the new table
    add("dqt_in_front_of_cb", between_scans(planar, 0, new1))                           # both chroma components start with the new table
    add("dqt_after_first_dc_scan", between_scans(progb, 0, dqt(1, other_table(slot_table(progb, 1)))), MISMATCHED)   # every component latched at scan 1: no pixel changes
    add("dqt_unused_slot_after_first_dc_scan", between_scans(progb, 0, dqt(3, bytes(range(1, 65)))))
    add("dht_redefined_after_luma", between_scans(planar, 0, DHT_DC_K3))                # slot DC 0 changes behind the only scan that uses it

    # ---- splices: fill, stray bytes, segments between scans, trailing bytes, component ids
    for n in (1, 3):
        add(f"base_fill{n}_before_rst", fill_before_rst(base, n))
        add(f"prog_fill{n}_before_rst", fill_before_rst(progb, n))
    add("base_fill_before_segments", fill_before_segments(base))
    add("prog_fill_before_segments", fill_before_segments(progb))
    add("prog_com_and_app5_between_scans", between_scans(between_scans(progb, 2, seg(0xE5, b"between two scans")), 0, seg(0xFE, b"a comment")))
    add("prog_stray_bytes_between_scans", between_scans(progb, 1, b"\x12\x34"))
    add("base_bytes_after_eoi", base + bytes(range(37)))
    add("prog_component_ids_0_1_2", renumber_components(progb))
    add("base_component_ids_0_1_2", renumber_components(base))
    assert len({c[0] for c in cases}) == len(cases)
    assert max(len(s["rst"]) for c in cases[:14] for s in scan_report(c[1])) > 8      # at least one case wraps past RST7
    return cases


# ---------------------------------------------------------------- what the judges compare against, computed once
def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def oracle_rgb(data):
    """the oracle's decode as RGB: its YCbCr samples through its libjpeg colour conversion, grey repeated"""
    from oracle import oracle as O
    px = O.decode(data).pixels()
    return O.ycc_to_rgb(px) if px.shape[2] == 3 else np.repeat(px, 3, axis=2)


def listed(bad):
    """the failing cases as one string: pytest prints an assertion message that is a string whole, a list cut short"""
    return "%d cases: " % len(bad) + "; ".join(str(b) for b in bad)


def same_coefficients(a, b):
    """two oracle decodes hold the same coefficients in every block of the image.  (The blocks that only complete an MCU are left out: a
    progressive file carries their AC coefficients in no scan, so a sequential file that has some there cannot keep them.)"""
    def real(ci, c):
        k = ci.im.comp[c]
        return ci.coefs(c)[:k.real_bh, :k.real_bw]
    return a.im.ncomp == b.im.ncomp and all(np.array_equal(real(a, c), real(b, c)) for c in range(a.im.ncomp))


@functools.lru_cache(maxsize=None)
def references():
    """name -> dict(rgb: Pillow's decode of the file, lossy: oracle_lossy, lossless: oracle_lossless or the oracle's refusal)"""
    from _util import oracle_lossless, oracle_lossy
    from oracle import oracle as O
    ref = {}
    for name, data, _ in battery() + ordinary():
        try:
            lossless = oracle_lossless(data)
        except O.OracleError as e:
            lossless = e
        ref[name] = dict(rgb=pillow_rgb(data), lossy=oracle_lossy(data), lossless=lossless)
    return ref


@functools.lru_cache(maxsize=None)
def ordinary():
    """files with nothing special about them, to stand between the battery's in one batch"""
    from gen_synth import synth_jpeg
    return [("ordinary_base_80x56", synth_jpeg(31, 80, 56, texture=10), OK), ("ordinary_prog_72x64", synth_jpeg(32, 72, 64, progressive=True, texture=15), OK),
            ("ordinary_base_444_57x35", synth_jpeg(33, 57, 35, subsampling=0, texture=5), OK), ("ordinary_prog_422_96x40", synth_jpeg(34, 96, 40, subsampling=1, progressive=True, texture=20), OK)]
