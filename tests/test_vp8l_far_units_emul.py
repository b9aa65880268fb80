"""The link stage and the finder of CSH_VP8L=far (k_vp8l_far.hip) on raw arrays of residual words, through tests/devunit/du_vp8l_far.cpp on the emulation
build: prev[] and the candidates against tests/_vp8l_far_model.py, exactly.  The functions take the unit library: tests/test_zzz_vp8l_far_units_gpu.py runs them
on the MI355X."""
import functools

import numpy as np
import pytest

import _vp8l_far_model as M
from _devunit_cases import emul_lib, same

BLOCK = 4096   # VP8L_FAR_BLOCK = VP8L_CHUNK: entries per block of the sort, positions per wave of the finder
# every size with a width that divides it: below, at and above a group of 64 lanes and a block, three blocks and a tail, and 18 blocks (more than one block per
# digit column, and a column scan of one group of 64 blocks with a tail ... of none: 70 000 / 4096 = 17.1)
SIZES = [(1, 1), (2, 1), (2, 2), (3, 3), (63, 7), (64, 8), (65, 13), (4095, 65), (4096, 64), (4097, 241), (3 * 4096 + 5, 647), (70000, 250)]
KINDS = ["equal", "alternating", "four", "random32"]


def content(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "equal":                 # one bucket, all of it but position 0 inside a flat run
        return np.full(n, 0xFF2A6B01, np.uint32)
    if kind == "alternating":           # two buckets of n / 2, every link at the fixed distance 2
        return np.where(np.arange(n) % 2 == 0, 0xFF102030, 0xFF405060).astype(np.uint32)
    if kind == "four":                  # 64 different keys: long buckets, flat runs inside them
        return (np.array([0xFF000000, 0xFF00FF00, 0xFF0000FF, 0x00FFFFFF], np.uint32))[rng.integers(0, 4, n)]
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def decoys(count):
    """A | F | A' | F | A' ... | F | A with `count` copies of A' = A with every 8th word changed: at the last A's start the nearest `count` links are A's first
    seven words in the A's"""
    rng = np.random.default_rng(40 + count)
    word = lambda: rng.integers(0, 1 << 32, BLOCK, dtype=np.uint64).astype(np.uint32)
    A = word()
    A2 = A.copy()
    A2[7::8] ^= 0x00010000
    parts = [A]
    for _ in range(count):
        parts += [word(), A2]
    return np.concatenate(parts + [word(), A])


@functools.lru_cache(maxsize=None)
def case(name):
    """(words, width, the model's prev, the model's candidates)"""
    if name.startswith("decoys"):
        px, width = decoys(int(name[6:])), 64
    else:
        kind, n, width = name.split("_")
        n, width = int(n), int(width)
        px = content(kind, n, 7 * n + KINDS.index(kind))
    prev = M.links(px)
    return px, width, np.array(prev, np.uint32), M.tokens(px, width, prev)


CASES = ["%s_%d_%d" % (k, n, w) for n, w in SIZES for k in KINDS] + ["decoys1", "decoys%d" % (M.LINKS + 1)]


def run_case(lib, name):
    px, width, want_prev, want_tok = case(name)
    prev, tok = np.full(px.size, 0x77777777, np.uint32), np.full(px.size, 0x7777777777777777, np.uint64)
    lib.run("csdu_vp8l_far", px, px.size, width, prev, tok)
    same(name + ": prev", prev, want_prev)
    same(name + ": candidates", tok, want_tok)


def test_the_cases_are_what_their_names_say():
    """the model's answers on the decoy layouts are the ones the layouts were built for, and the battery has the buckets it names"""
    px, width, prev, tok = case("decoys1")
    last = 4 * BLOCK
    assert prev[last] == 2 * BLOCK and prev[2 * BLOCK] == 0 and prev[0] == M.NONE            # the second link reaches the first A
    assert int(tok[last]) == BLOCK | (last << 16)
    px, width, prev, tok = case("decoys%d" % (M.LINKS + 1))
    last = px.size - BLOCK
    q = last
    for _ in range(M.LINKS):
        q = int(prev[q])
        assert q != 0 and (last - q) % (2 * BLOCK) == 0                                   # eight A's, the first A behind them
    assert int(prev[q]) != M.NONE and int(tok[last]) == 7 | (2 * BLOCK << 16)              # the nearest A', its seven words: the first A is not found
    _, _, prev, tok = case("equal_70000_250")
    assert (prev == M.NONE).all() and int(tok[1]) == M.MAX_LEN | (1 << 16)
    _, _, prev, _ = case("alternating_70000_250")
    assert prev[2] == 0 and prev[69997] == 69995 and prev[69998] == M.NONE
    _, _, prev, _ = case("four_70000_250")
    assert 0 < np.count_nonzero(prev == M.NONE) < 70000 // 8                               # flat runs inside long buckets
    assert M.hash24(1, 2, 3) == ((((1 * 0x9E3779B1) ^ (2 * 0x85EBCA6B) ^ (3 * 0xC2B2AE35)) & M.M32) * 0x27D4EB2F & M.M32) >> 8


@pytest.mark.parametrize("name", CASES)
def test_emul_far_unit(name):
    run_case(emul_lib(), name)


def run_refusals(lib):
    px, prev, tok = np.zeros(16, np.uint32), np.zeros(16, np.uint32), np.zeros(16, np.uint64)
    for n, width in ((0, 1), (16, 0), (16, 3), (-4, 2), (16, 16385)):
        assert lib.call("csdu_vp8l_far", px, n, width, prev, tok) == -1, (n, width)


def test_emul_far_unit_refuses_what_the_coder_would():
    run_refusals(emul_lib())


def test_emul_far_unit_does_not_depend_on_the_order_of_execution():
    """the emulation runs a launch's blocks and lanes in either order (gpu_rt.h csh_emul_reverse): the same prev[] and the same candidates"""
    lib = emul_lib()
    lib.dll.csdu_set_reverse(1)
    try:
        for name in ("four_70000_250", "random32_12293_647", "alternating_4097_241", "decoys1"):
            run_case(lib, name)
    finally:
        lib.dll.csdu_set_reverse(0)
