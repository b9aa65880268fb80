"""A reader of baseline JPEG files (one sequential scan), written from ITU-T T.81 (B.2 the markers, F.2.2 the decoding of a block, F.2.2.3 the
Huffman walk, B.1.1.5 byte stuffing) and independent of this repository's decoder: it walks the scan and counts how often every DC and AC symbol of
every table is used, so that tests/test_code_tables_emul.py can hold each DHT to the table tests/_prefix_model.py derives from those counts.

    info = read(jpeg_bytes)
    info.tables  {(class, id): (bits[17], vals)}     class 0 DC, 1 AC; as the DHT segments state them
    info.counts  {(class, id): [256 counts]}         the symbols the scan codes with each table
    info.width, info.height, info.components -> [(id, h, v, tq)], info.blocks (how many were walked)
"""


class Info:
    pass


def _lookup(bits, vals):
    """Annex C: the codes of a table; -> for every 16-bit window of the stream the (symbol, length) it starts with"""
    table, code, k = [None] * 65536, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l]):
            lo = code << (16 - l)
            for i in range(lo, lo + (1 << (16 - l))): table[i] = (vals[k], l)
            code += 1
            k += 1
        code <<= 1
    return table


def read(data):
    assert data[:2] == b"\xff\xd8"
    info, pos = Info(), 2
    info.tables, info.restart = {}, 0
    while True:
        assert data[pos] == 0xFF
        m, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + n]
        if m == 0xC0 or m == 0xC1:
            assert seg[0] == 8
            info.height, info.width = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            info.components = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                bits = [0] + list(seg[at + 1:at + 17])
                info.tables[(seg[at] >> 4, seg[at] & 15)] = (bits, list(seg[at + 17:at + 17 + sum(bits)]))
                at += 17 + sum(bits)
        elif m == 0xDD:
            info.restart = int.from_bytes(seg, "big")
        elif m == 0xDA:
            scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
            assert list(seg[1 + 2 * seg[0]:]) == [0, 63, 0], "not a sequential scan"
            pos += 2 + n
            break
        else:
            assert m not in (0xC2, 0xC9, 0xCA), "not a baseline file"
        pos += 2 + n
    assert [c for c, _, _ in scan] == [c[0] for c in info.components], "one scan with every component"
    assert not info.restart, "restart intervals are not read here"
    end = data.index(b"\xff\xd9", pos)
    assert end == len(data) - 2
    ecs = data[pos:end].replace(b"\xff\x00", b"\xff") + b"\0\0\0\0"
    hmax, vmax = max(c[1] for c in info.components), max(c[2] for c in info.components)
    if len(info.components) == 1:
        hmax = vmax = 1
        units = [(scan[0][1], scan[0][2], 1)]
    else:
        units = [(td, ta, c[1] * c[2]) for c, (_, td, ta) in zip(info.components, scan)]
    nmcu = -(-info.width // (8 * hmax)) * -(-info.height // (8 * vmax))
    look = {k: _lookup(*t) for k, t in info.tables.items()}
    info.counts = {k: [0] * 256 for k in info.tables}
    bit = 0

    def symbol(cls, tid):
        nonlocal bit
        s, l = look[(cls, tid)][(int.from_bytes(ecs[bit >> 3:(bit >> 3) + 3], "big") >> (8 - (bit & 7))) & 0xFFFF]
        bit += l
        info.counts[(cls, tid)][s] += 1
        return s
    info.blocks = 0
    for _ in range(nmcu):
        for td, ta, nb in units:
            for _ in range(nb):
                s = symbol(0, td)               # the DC difference's category, then that many bits
                bit += s
                k = 1
                while k < 64:
                    rs = symbol(1, ta)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15: break       # EOB (F.1.2.2.1; ZRL skips sixteen)
                        k += 16
                    else:
                        k += r + 1
                        bit += s
                assert k <= 64, "a run past the end of the block"
                info.blocks += 1
    assert 0 <= 8 * (len(ecs) - 4) - bit < 8, "the scan does not end where its blocks do"
    return info
