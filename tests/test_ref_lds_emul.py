"""The refinement kernels at the edges of what their LDS holds (k_aclist.hip k_list_refine and k_list_refine_pack), on the CPU emulation build:
the packer's token buffer is one ROUND of 256 tokens (a step of 256 entries can make 648), its code table the 32 codes of a refinement scan's alphabet
(tok_bits.h ref_code_index), pass 1's histogram 17 words a copy.  Crafted coefficients go through a lossless transcode; every file equals the oracle's and equals
the same call under CSH_REF_PACK=0 (the token path: the full 256-entry table, no rounds), in the default, `scalar` and `plain` profiles.  The emulation build stops
on a step of more than 648 tokens, on a chunk that does not start where its sizes say and on a run that does not end there.  The same bodies run on the MI355X
in tests/test_ref_lds_gpu.py.

The picture of check_alphabet is 2048 x 1032, not the 1024 x 1024 one would first think of: EOB runs of 1, 2, 4, ... 16 384 blocks in ONE scan are 32 767 blocks, and a
1024 x 1024 picture has 16 384."""
import numpy as np
import pytest

import test_ref_pack_emul as P
import test_refine_lists_emul as E
from _util import emul_api, oracle_lossless

PROFILES = E.PROFILES
params = E.params


@pytest.fixture(scope="module")
def api():
    return emul_api()


_files = {}


def coef_file(name, zz, w, h):
    """a grey picture of w x h whose AC coefficients are zz ([blocks][64], zig-zag order; the DC values are those of a noise picture), built once per name"""
    if name not in _files:
        from oracle import oracle as O
        base = O.forward(np.random.default_rng(11).integers(0, 255, (h, w), dtype=np.uint8), O.params(quality=90))
        flat = base.coefs_view(0).reshape(-1, 64)
        assert zz.shape == flat.shape, (zz.shape, flat.shape)
        flat[:, np.array(O.ZZ)[1:]] = zz[:, 1:]
        _files[name] = base.encode(O.params(progressive=1, marker_style=0))
    return _files[name]


def last_only(n, mag, k=63):
    """every block: one coefficient of magnitude `mag` at position k, nothing else.  Where it is new to the scan, k = 63 has 62 zeros in front of it: three ZRLs and a
    symbol for two list entries (a block that ends at 63 has no EOB), 512 tokens for a step of 256.  k = 62 has 61 zeros: three ZRLs, a symbol and the block's EOB,
    five tokens for two entries -- 640 for a step, the most the bound in the kernel's comment allows short of the two cut blocks"""
    zz = np.zeros((n, 64), np.int16)
    zz[:, k] = np.where(np.arange(n) % 3 == 0, -mag, mag)
    return zz


def dense(n, mag, seed=5):
    """every block: 63 coefficients of magnitude mag .. 2 mag - 1 with history in the scan that sees them one level down: 63 correction bits a block"""
    rng = np.random.default_rng(seed)
    zz = (rng.integers(mag, 2 * mag, (n, 64)) * rng.choice(np.array([-1, 1]), (n, 64))).astype(np.int16)
    zz[:, 0] = 0
    return zz


def entries_al0(zz):
    """list entries per block at level 0: its non-zero AC coefficients and its END entry"""
    return (zz[:, 1:] != 0).sum(axis=1) + 1


def mixed(n, mag):
    """blocks of both kinds, and empty ones, laid out so that the level-0 list's steps of 256 entries end inside a block of each kind: entry 255 is the coefficient of
    a last_only block (its END opens the next step), entries 457 .. 520 are one dense block.  Behind them a seeded mixture"""
    A, B, Z = last_only(1, mag)[0], None, np.zeros(64, np.int16)
    d = dense(n, 2 * mag, seed=9)
    kinds = [Z] + [B] * 3 + [A] * 31 + [A] + [A] * 100 + [B]
    rng = np.random.default_rng(17)
    while len(kinds) < n: kinds.append((A, B, Z)[int(rng.integers(0, 3))])
    zz = np.array([d[i] if k is None else k for i, k in enumerate(kinds)], np.int16)
    off = np.concatenate([[0], np.cumsum(entries_al0(zz))])
    assert off[35] == 255 and (zz[35] == A).all(), "the first step must end between a last_only block's coefficient and its END"
    assert off[136] == 457 and off[137] == 521 and (zz[136] != 0).sum() == 63, "the second step must end inside a dense block"
    return zz


def check_files(api, monkeypatch, prof, srcs):
    E.set_profile(monkeypatch, prof)
    P.check_group(api, monkeypatch, srcs, [1] * len(srcs), prof, oracle_lossless, p=params(jpeg_optimize=True))


# ---- 1. the most tokens per entry: magnitude 1 (new in the 1 -> 0 scan) and magnitude 2 (new in 2 -> 1, a correction bit in 1 -> 0); 256 blocks = 512 entries,
# two steps of 512 tokens (position 63: two rounds each) or of 640 (position 62: three rounds each)
def check_most_tokens(api, monkeypatch, prof):
    check_files(api, monkeypatch, prof, [coef_file("last1", last_only(256, 1), 128, 128), coef_file("last2", last_only(256, 2), 128, 128),
                                         coef_file("last1w", last_only(272, 1), 136, 128), coef_file("eob1", last_only(256, 1, 62), 128, 128),
                                         coef_file("eob2", last_only(272, 2, 62), 136, 128)])


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_most_tokens(api, monkeypatch, prof):
    check_most_tokens(api, monkeypatch, prof)


# ---- 2. the most bits per token: 63 coefficients with history in every block, 63 correction bits behind every EOB
def check_most_bits(api, monkeypatch, prof):
    check_files(api, monkeypatch, prof, [coef_file("dense2", dense(256, 2), 128, 128), coef_file("dense4", dense(256, 4), 128, 128)])


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_most_bits(api, monkeypatch, prof):
    check_most_bits(api, monkeypatch, prof)


# ---- 3. both in one chunk, a step ending inside each kind of block
def check_mixed(api, monkeypatch, prof):
    check_files(api, monkeypatch, prof, [coef_file("mixed1", mixed(256, 1), 128, 128), coef_file("mixed2", mixed(272, 2), 136, 128)])


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_mixed(api, monkeypatch, prof):
    check_mixed(api, monkeypatch, prof)


# ---- 4. the whole alphabet in one scan: runs 0 .. 15 in front of a new coefficient, a ZRL, and EOB runs of 1, 2, 4, ... 16 384 blocks
ALPHABET = sorted([n << 4 for n in range(15)] + [0xF0] + [(r << 4) | 1 for r in range(16)])
ALPHA_W, ALPHA_H = 2048, 1032   # 256 x 129 blocks


def alphabet_blocks():
    nblk = (ALPHA_W // 8) * (ALPHA_H // 8)
    zz = np.zeros((nblk, 64), np.int16)

    def put(b, runs):   # new coefficients with these zero runs in front of them
        k = 0
        for i, r in enumerate(runs):
            k += r + 1
            zz[b, k] = 1 if i & 1 else -1
        assert k < 63   # the block ends with an EOB: it opens a run
    starts = [(0, 1, 2, 3, 4, 5, 6, 7, 8, 9), (10, 11, 12, 13), (14, 15, 18)]   # 18: a ZRL and a run of 2
    b = 0
    for n in range(15):   # a block with coefficients, then 2^n - 1 empty ones: an EOB run of 2^n blocks
        put(b, starts[n % 3])
        b += 1 << n
    zz[b, 63] = 1         # ends the last run, and ends without an EOB itself
    assert b < nblk
    return zz


def dht_symbols_of_scan(data, want):
    """the symbols of the AC table that the scan want = (Ss, Se, Ah, Al) of component 1 uses, read off the file's DHT segments in front of it"""
    tables, i = {}, 2
    while i < len(data):
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + n]
        if m == 0xC4:
            j = 0
            while j < len(seg):
                cnt = sum(seg[j + 1:j + 17])
                tables[seg[j]] = sorted(seg[j + 17:j + 17 + cnt])
                j += 17 + cnt
        if m == 0xDA:
            ns = seg[0]
            scan = (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15)
            if ns == 1 and scan == want:
                return tables[0x10 | (seg[2] & 15)]
            i += 2 + n   # the entropy-coded bytes: to the next marker that is neither a stuffed zero nor RSTn
            while not (data[i] == 0xFF and data[i + 1] != 0 and not 0xD0 <= data[i + 1] <= 0xD7): i += 1
            continue
        i += 2 + n
    raise AssertionError(("no such scan", want))


def check_alphabet(api, monkeypatch, prof):
    src = coef_file("alphabet", alphabet_blocks(), ALPHA_W, ALPHA_H)
    E.set_profile(monkeypatch, prof)
    monkeypatch.setenv("CSH_REF_PACK", "1")
    outs, t = E.run_batch(api, [src], params(jpeg_optimize=True))
    monkeypatch.setenv("CSH_REF_PACK", "0")
    ref, t0 = E.run_batch(api, [src], params(jpeg_optimize=True))
    monkeypatch.delenv("CSH_REF_PACK", raising=False)
    assert t.n_ref_packed > 0 and t0.n_ref_packed == 0
    assert outs[0] == ref[0], "the 32-code table != the full one"
    assert outs[0] == oracle_lossless(src)
    # the stock script keeps the 1 -> 0 scan, and its table lists what it coded.  The scan search codes and sizes the same scan as a trial (n_ref_packed) and then
    # settles on Al = 0 for so sparse a picture: there the file's bytes are the check
    if prof == "plain": assert dht_symbols_of_scan(outs[0], (1, 63, 1, 0)) == ALPHABET


@pytest.mark.parametrize("prof", PROFILES)
def test_emul_alphabet(api, monkeypatch, prof):
    check_alphabet(api, monkeypatch, prof)
