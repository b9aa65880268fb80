"""tests/_prefix_model.py, the Python statement of T.81 K.2 that the prefix-code units and the file-level table checks compare with, held to what is
known about such codes apart from any tie rule -- and to the oracle's cso_gen_optimal_table, which nothing else in the suite calls directly.  No GPU and
no build of the library: the model, the battery (tests/_devunit_cases.py) and the oracle."""
import pytest

import _deflate
import _devunit_cases as DU
import _prefix_model as M

ALPHABETS = DU.CODE_ALPHABETS + [(n, 15) for n in DU.WIDE_ALPHABETS if n > 288]


def test_jpeg_table_is_the_oracles_table_on_the_battery():
    from oracle import oracle as O
    cases, tabs = DU.jpeg_battery()
    for (name, f), (bits, vals, _, _, _) in zip(cases, tabs):
        obits, ovals = O.gen_optimal_table(f)
        assert obits.tolist() == list(bits) and ovals.tolist() == list(vals), name


def test_jpeg_tables_are_complete_but_for_the_reserved_code_and_optimal_where_16_bits_suffice():
    cases, tabs = DU.jpeg_battery()
    binding = 0
    for (name, f), (bits, vals, code, size, depth) in zip(cases, tabs):
        used = [s for s in range(256) if f[s]]
        assert sorted(vals) == used and [s for s in range(256) if size[s]] == used, name
        assert sum(bits) == len(used) and bits[0] == 0, name
        if not used:
            assert not any(bits), name
            continue
        longest = max(size)
        assert longest <= 16, name
        # complete but for ONE code of the longest length: 2^16 - 2^(16 - longest); 65535 wherever the longest length is 16
        assert M.kraft(size, 16) == 65536 - (1 << (16 - longest)), name
        assert all(code[s] != (1 << size[s]) - 1 for s in used), f"{name}: a code of all ones"
        assert len({(size[s], code[s]) for s in used}) == len(used), name
        by_code = sorted(used, key=lambda s: code[s] << (16 - size[s]))
        assert all((code[a] << (16 - size[a])) + (1 << (16 - size[a])) <= code[b] << (16 - size[b]) for a, b in zip(by_code, by_code[1:])), f"{name}: one code is a prefix of another"
        sizes257 = M.k2_sizes(list(f) + [1])
        assert sum(v * s for v, s in zip(list(f) + [1], sizes257)) == M.huffman_cost(list(f) + [1]), f"{name}: K.1's sizes are no Huffman code"
        if depth <= 16:
            assert list(size) == sizes257[:256], name   # nothing adjusted: the table is the Huffman code itself, the reserved entry at its longest length
        else:
            binding += 1
            assert longest == 16, name
    assert binding >= 20


@pytest.mark.parametrize("n,limit", ALPHABETS)
def test_limited_lengths_are_complete_within_the_limit_and_optimal_where_it_does_not_bind(n, limit):
    cases = DU.prefix_battery(n, n in DU.WIDE_ALPHABETS and n > 288)
    depths = []
    for name, f in cases:
        lengths, depth = M.limited_lengths(f, limit)
        depths.append(depth)
        M.check_lengths(f, lengths, limit)                       # never fewer than two codes, every used symbol coded, none above the limit, Kraft sum 1
        if sum(1 for v in f if v) >= 2:
            cost, least = sum(v * l for v, l in zip(f, lengths)), M.huffman_cost(f)
            assert cost == least if depth <= limit else cost >= least, (name, cost, least)
            order = sorted((s for s in range(n) if f[s]), key=lambda s: f[s])
            # where the limit binds, K.2 hands the adjusted lengths out by (unlimited size, index): two symbols of one unlimited size may then get their lengths
            # against their frequencies (libjpeg does the same); where it does not bind, a rarer symbol never has the shorter code
            assert depth > limit or all(lengths[a] >= lengths[b] for a, b in zip(order, order[1:]) if f[a] < f[b]), f"{name}: a rarer symbol has the shorter code"
        unreversed = [int(format(c, f"0{l}b")[::-1], 2) if l else None for c, l in zip(M.deflate_codes(lengths), lengths)]
        assert unreversed == _deflate.canonical(list(lengths)), name   # (the suite's other statement of RFC 1951 3.2.2, which the inflate tests build their streams with)
    DU.battery_coverage(cases, n, limit, depths)


def test_adjustment_keeps_the_number_of_codes_and_the_kraft_sum():
    for top in range(8, 33):
        bits = [0] * (top + 1)
        for l in range(1, top): bits[l] = 1
        bits[top] = 2                                            # the degenerate tree: one code of every length, two of the longest
        for limit in (7, 15, 16):
            if limit >= top: continue
            out = M.k2_adjust(bits, limit)
            assert len(out) == limit + 1 and sum(out) == sum(bits)
            assert sum(c << (limit - l) for l, c in enumerate(out) if l) == 1 << limit
