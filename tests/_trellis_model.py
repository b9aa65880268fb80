"""An independent float64 statement of the trellis quantiser's cost model, for checking that whatever levels a producer writes (the oracle,
the emulation build, the MI355X) are a minimum-cost solution of it.

Written from the model as oracle/jpeg_oracle.c states it in the comment above quantize_trellis_row, not from that routine's code.  Per
component, with qt the quantisation table (natural order), x a block's unquantised DCT value (jfdctint output, scaled by 8) and q = 8 * qt:

  lambda      = 2^14.75 / (2^16.5 + mean of the 63 squared AC values of the block)
  weight      = lambda / qt^2 at that position; a level l at a value x costs (|l| q - |x|)^2 * weight, a zero costs x^2 * weight
  AC          over zig-zag positions 1..63.  Only a position whose scalar level v = (|x| + q/2) // q is non-zero may be kept; it takes one
              of the candidates 1, 3, 7, ..., 2^k - 1 < v and v itself (v clamped to 1023), with the sign of x.  Keeping a level of size s
              (bit length) after a run of r zeros costs aclen[16 (r & 15) + s] + s + (r >> 4) * aclen[0xF0].  Behind the last kept
              position an EOB costs aclen[0], unless that position is 63.
  DC          per row of real_bw blocks, a Viterbi path: each block offers n = min(9, (2 + 60 // qt[0]) | 1) magnitudes centred on the
              rounded one, (v - n // 2 + k) clamped to +-1023, times the sign of x; a step costs size + dclen[size] of the difference to
              the previous block's level.  The first block's predecessor is 0 at the start of an iMCU row, else the level the row above
              ended on.  Rows are solved one after the other, so a row is optimal given its predecessor.
  dummy       blocks outside real_bw x real_bh are not quantised: zero AC, the DC of the block to the left (right edge) or of the last block
              of the MCU above (bottom), as libjpeg's jccoefct.c fills them.

Quirks of the model, mirrored on purpose and not "fixed":
  - an AC symbol whose code length is 0 is absent from the table and cannot be used: neither a (run, size) symbol nor ZRL when a run of
    16 or more needs it;
  - a DC size whose dclen entry is 0 is free (sequential mode's optimal DC table leaves unused sizes at 0, and the model charges only
    the size bits for them);
  - aclen[0] == 0 makes the EOB free.

The constants (14.75, 16.5, the candidate rule, the DC reset rule) are mozjpeg's as recalled and stay UNPINNED; this module pins the
optimiser, not the model.  The knobs (Knobs) perturb one term each, for the tests that show the check constrains that term.
"""
import itertools
from dataclasses import dataclass

import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
               41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)
LAMBDA_C1 = 2.0 ** 14.75
LAMBDA_C2 = 2.0 ** 16.5
MAX_LEVEL = 1023
INF = np.inf


@dataclass(frozen=True)
class Knobs:
    lam_scale: float = 1.0       # lambda times this
    zrl: bool = True             # charge (run >> 4) * aclen[0xF0]
    eob: bool = True             # charge aclen[0] behind the last kept position
    extra_cand: bool = False     # offer v - 1 as an AC candidate too
    dc_row_reset: bool = False   # DC predecessor 0 at every row instead of every iMCU row


DEFAULT = Knobs()


def bitlen(a):
    """bit length of non-negative integers (0 -> 0)"""
    a = np.asarray(a, dtype=np.int64)
    out = np.zeros(a.shape, dtype=np.int64)
    t = a.copy()
    while np.any(t):
        nz = t > 0
        out += nz
        t >>= 1
    return out


def lam(raw, knobs=DEFAULT):
    """lambda per block; raw (..., 64) natural order"""
    r = np.asarray(raw, dtype=np.float64)
    norm = (r[..., 1:] ** 2).sum(axis=-1) / 63.0
    return LAMBDA_C1 / (LAMBDA_C2 + norm) * knobs.lam_scale


def scalar_levels(raw, qt):
    """the scalar quantiser's magnitudes (|x| + 4 qt) // (8 qt), natural order, unclamped"""
    q = 8 * np.asarray(qt, dtype=np.int64)
    return (np.abs(np.asarray(raw, dtype=np.int64)) + q // 2) // q


def _ac_setup(raw, qt, knobs):
    """zig-zag views of one batch of blocks: |x|, q = 8 qt, weights, scalar levels (clamped), candidate magnitudes (N, 64, K) with 0 = none"""
    raw = np.asarray(raw, dtype=np.int64).reshape(-1, 64)
    qt = np.asarray(qt, dtype=np.int64)
    x = np.abs(raw[:, ZZ])
    qz = 8 * qt[ZZ]
    w = 64.0 * lam(raw, knobs)[:, None] / (qz.astype(np.float64) ** 2)[None, :]   # lambda / qt^2
    v = np.minimum(scalar_levels(raw, qt)[:, ZZ], MAX_LEVEL)
    v[:, 0] = 0
    cands = [np.where((2 << k) - 1 < v, (2 << k) - 1, 0) for k in range(10)] + [v]
    if knobs.extra_cand:
        cands.append(np.where(v >= 2, v - 1, 0))
    return raw, x, qz, w, v, np.stack(cands, axis=-1)


def _sym_len(aclen, run, size):
    """code length of the (run & 15, size) symbol, INF where the table has none (size 0 or > 10 included)"""
    ok = (size >= 1) & (size <= 10)
    L = np.asarray(aclen, dtype=np.float64)[np.where(ok, 16 * (run & 15) + size, 0)]
    return np.where(ok & (L > 0), L, INF)


def _zrl_cost(aclen, run, knobs):
    nz = np.asarray(run) >> 4
    f0 = float(aclen[0xF0])
    return np.where(nz == 0, 0.0, np.where(f0 > 0, nz * (f0 if knobs.zrl else 0.0), INF))


def ac_optimum(raw, qt, aclen, knobs=DEFAULT):
    """minimum AC cost per block, (N,)"""
    raw, x, qz, w, v, cand = _ac_setup(raw, qt, knobs)
    N = raw.shape[0]
    aclen = np.asarray(aclen, dtype=np.int64)
    zd = (x.astype(np.float64) ** 2) * w
    zd[:, 0] = 0.0
    Z = np.cumsum(zd, axis=1)                                  # Z[:, i]: the zero cost of positions 1..i
    size = bitlen(cand)                                        # (N, 64, K)
    dist = np.where(cand > 0, (cand * qz[None, :, None] - x[:, :, None]).astype(np.float64) ** 2 * w[:, :, None], INF)
    acc = np.full((N, 64), INF)
    acc[:, 0] = 0.0
    runs = np.arange(16)
    eob = float(aclen[0]) if knobs.eob else 0.0
    for i in range(1, 64):
        keep = v[:, i] > 0
        if not keep.any():
            continue
        # cheapest symbol + candidate per run length mod 16
        rate = _sym_len(aclen, runs[None, :, None], size[:, i, None, :]) + size[:, i, None, :]
        best = np.min(rate + dist[:, i, None, :], axis=2)      # (N, 16)
        j = np.arange(i)
        run = i - 1 - j
        c = acc[:, :i] - Z[:, :i] + Z[:, i - 1, None] + _zrl_cost(aclen, run, knobs)[None, :] + best[:, run & 15]
        acc[:, i] = np.where(keep, c.min(axis=1), INF)
    tail = Z[:, 63:64] - Z
    ends = acc + tail
    ends[:, :63] += eob                                        # (column 0: nothing kept)
    return ends.min(axis=1)


def ac_cost(levels, raw, qt, aclen, knobs=DEFAULT):
    """model cost of the AC levels written, per block, (N,); INF where a symbol the levels need is absent"""
    raw = np.asarray(raw, dtype=np.int64).reshape(-1, 64)
    lv = np.asarray(levels, dtype=np.int64).reshape(-1, 64)[:, ZZ]
    qt = np.asarray(qt, dtype=np.int64)
    aclen = np.asarray(aclen, dtype=np.int64)
    x = np.abs(raw[:, ZZ])
    qz = 8 * qt[ZZ]
    w = 64.0 * lam(raw, knobs)[:, None] / (qz.astype(np.float64) ** 2)[None, :]   # lambda / qt^2
    a = np.abs(lv)
    d = np.where(a > 0, (a * qz[None, :] - x), x).astype(np.float64) ** 2 * w
    total = d[:, 1:].sum(axis=1)
    last = np.zeros(lv.shape[0], dtype=np.int64)
    for i in range(1, 64):
        nz = a[:, i] > 0
        if not nz.any():
            continue
        run = i - 1 - last
        s = bitlen(a[:, i])
        r = _sym_len(aclen, run, s) + s + _zrl_cost(aclen, run, knobs)
        total = total + np.where(nz, r, 0.0)
        last = np.where(nz, i, last)
    if knobs.eob:
        total = total + np.where(last < 63, float(aclen[0]), 0.0)
    return total


def ac_bruteforce(raw, qt, aclen, knobs=DEFAULT, max_keep=8):
    """minimum AC cost of one block by enumerating every choice at every keepable position (validates ac_optimum only)"""
    raw1, x, qz, w, v, cand = _ac_setup(raw, qt, knobs)
    pos = np.nonzero(v[0] > 0)[0]
    assert len(pos) <= max_keep, len(pos)
    sign = np.where(np.asarray(raw1[0], dtype=np.int64)[ZZ] < 0, -1, 1)
    choices = [[0] + sorted(set(int(c) for c in cand[0, p] if c > 0)) for p in pos]
    combos = list(itertools.product(*choices))
    combos = np.array(combos, dtype=np.int64).reshape(len(combos), len(pos))
    lz = np.zeros((combos.shape[0], 64), dtype=np.int64)
    lz[:, pos] = combos * sign[pos]
    nat = np.zeros_like(lz)
    nat[:, ZZ] = lz
    return ac_cost(nat, np.broadcast_to(raw1, nat.shape), qt, aclen, knobs).min()


def _dc_setup(raw_dc, qt0, lam_blocks):
    """DC candidates (levels, with sign) and their distortions, (..., n)"""
    x = np.abs(np.asarray(raw_dc, dtype=np.int64))
    q = 8 * int(qt0)
    n = min(9, (2 + 60 // int(qt0)) | 1)
    v = (x + q // 2) // q
    c = np.clip(v[..., None] - n // 2 + np.arange(n), -MAX_LEVEL, MAX_LEVEL)
    dist = ((c * q - x[..., None]).astype(np.float64) ** 2) * (lam_blocks[..., None] / float(qt0) ** 2)
    sgn = np.where(np.asarray(raw_dc) < 0, -1, 1)[..., None]
    return c * sgn, dist


def _dc_rate(diff, dclen):
    s = bitlen(np.abs(diff))
    return s + np.asarray(dclen, dtype=np.float64)[s]


def dc_rows(raw, levels, comp, knobs=DEFAULT):
    """per real row of blocks: (cost of the DC levels written, optimum given the same predecessor), both (real_bh,)"""
    rbw, rbh = comp["real_bw"], comp["real_bh"]
    r = np.asarray(raw, dtype=np.int64)[:rbh, :rbw]
    lv = np.asarray(levels, dtype=np.int64)[:rbh, :rbw, 0]
    qt0 = int(comp["qt"][0])
    dclen = comp["dclen"]
    lamb = lam(r, knobs)
    cand, dist = _dc_setup(r[:, :, 0], qt0, lamb)                          # (rbh, rbw, n)
    prev = np.zeros(rbh, dtype=np.int64)
    cont = np.arange(rbh) % comp["v"] != 0
    if knobs.dc_row_reset:
        cont[:] = False
    prev[cont] = lv[np.nonzero(cont)[0] - 1, rbw - 1]
    # the cost of the path written (INF where a level is no candidate)
    match = cand == lv[:, :, None]
    ldist = np.where(match.any(axis=2), np.where(match, dist, INF).min(axis=2), INF)
    steps = np.diff(np.concatenate([prev[:, None], lv], axis=1), axis=1)
    cost = (ldist + _dc_rate(steps, dclen)).sum(axis=1)
    # the Viterbi optimum
    acc = _dc_rate(cand[:, 0, :] - prev[:, None], dclen) + dist[:, 0, :]
    for bx in range(1, rbw):
        t = _dc_rate(cand[:, bx, None, :] - cand[:, bx - 1, :, None], dclen)   # (rbh, from, to)
        acc = (acc[:, :, None] + t).min(axis=1) + dist[:, bx, :]
    return cost, acc.min(axis=1)


def dc_bruteforce_row(raw_dc, lam_row, qt0, dclen, prev):
    """minimum DC cost of one short row by enumerating every path (validates dc_rows only)"""
    cand, dist = _dc_setup(np.asarray(raw_dc), qt0, np.asarray(lam_row, dtype=np.float64))
    best = INF
    for path in itertools.product(range(cand.shape[1]), repeat=len(raw_dc)):
        p, c = prev, 0.0
        for b, k in enumerate(path):
            c += dist[b, k] + _dc_rate(cand[b, k] - p, dclen)
            p = cand[b, k]
        best = min(best, c)
    return best


def admissible(levels, comp, knobs=DEFAULT):
    """(bh, bw) mask of blocks whose levels break a rule of the model: AC levels outside their position's candidates or of the wrong
    sign, a non-zero level where the scalar level is 0, a DC level outside the block's candidates, a dummy block not filled as
    jccoefct.c fills it"""
    lv = np.asarray(levels, dtype=np.int64)
    raw = np.asarray(comp["raw"], dtype=np.int64)
    bh, bw = lv.shape[:2]
    rbw, rbh, h = comp["real_bw"], comp["real_bh"], comp["h"]
    bad = np.zeros((bh, bw), dtype=bool)
    r = raw[:rbh, :rbw].reshape(-1, 64)
    l = lv[:rbh, :rbw].reshape(-1, 64)
    _, x, qz, w, v, cand = _ac_setup(r, comp["qt"], knobs)
    lz = l[:, ZZ]
    sgn_ok = (lz == 0) | (np.sign(lz) == np.where(r[:, ZZ] < 0, -1, 1))
    in_set = (lz == 0) | (np.abs(lz)[:, :, None] == cand).any(axis=2)
    ac_bad = ~(sgn_ok & in_set)[:, 1:].all(axis=1)
    dcc, _ = _dc_setup(r[:, 0], int(comp["qt"][0]), lam(r, knobs))
    dc_bad = ~(dcc == l[:, 0:1]).any(axis=1)
    bad[:rbh, :rbw] = (ac_bad | dc_bad).reshape(rbh, rbw)
    for by in range(bh):
        for bx in range(bw):
            if by < rbh and bx < rbw:
                continue
            blk = lv[by, bx]
            if by < rbh:
                want = lv[by, bx - 1, 0]
            else:
                m = bx // h
                want = lv[by - 1, m * h + h - 1, 0]
            bad[by, bx] = blk[0] != want or np.any(blk[1:])
    return bad


@dataclass
class Check:
    """one component's verdict: per-block AC gaps and per-row DC gaps (cost of the levels written minus the optimum), inadmissible blocks"""
    ac_gap: np.ndarray
    ac_opt: np.ndarray
    ac_zero: np.ndarray
    dc_gap: np.ndarray
    dc_opt: np.ndarray
    bad: np.ndarray

    def ac_flagged(self):
        return self.ac_gap > tolerance(self.ac_opt, self.ac_zero)

    def dc_flagged(self):
        return self.dc_gap > tolerance(self.dc_opt)

    def ok(self):
        return not (self.bad.any() or self.ac_flagged().any() or self.dc_flagged().any())


def tolerance(opt, zero=0.0):
    """what float32 arithmetic in mozjpeg's order may leave between the producer's choice and the float64 optimum.  The AC programme adds
    and subtracts running sums of the zero costs, which reach `zero` (the cost of the all-zero block, 1e6 at q 100 on noise) while the optimum
    stays near 500: one float32 ulp of that sum (2^-24 .. 2^-23 of it) is part of the tolerance.  Measured worst: 0.29 of one ulp."""
    return 1e-3 + 1e-5 * np.abs(opt) + 2.0 ** -23 * np.asarray(zero)


def check_component(levels, comp, knobs=DEFAULT):
    lv = np.asarray(levels, dtype=np.int64)
    rbw, rbh = comp["real_bw"], comp["real_bh"]
    raw = comp["raw"][:rbh, :rbw].reshape(-1, 64)
    l = lv[:rbh, :rbw].reshape(-1, 64)
    opt = np.concatenate([ac_optimum(raw[i:i + 8192], comp["qt"], comp["aclen"], knobs) for i in range(0, len(raw), 8192)] or [np.zeros(0)])
    cost = ac_cost(l, raw, comp["qt"], comp["aclen"], knobs)
    zero = ac_cost(np.zeros_like(l), raw, comp["qt"], comp["aclen"], Knobs(lam_scale=knobs.lam_scale, eob=False))
    dcost, dopt = dc_rows(comp["raw"], lv, comp, knobs)
    return Check(cost - opt, opt, zero, dcost - dopt, dopt, admissible(lv, comp, knobs))
