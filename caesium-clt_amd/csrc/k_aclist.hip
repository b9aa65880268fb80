// k_aclist.hip -- progressive AC scans coded from COMPACTED COEFFICIENT LISTS: the first-pass scans (Ah = 0) entirely, the refinement scans
// (Ah = Al + 1) too (k_list_refine and k_list_refine_pack, at the end of the file; CSH_REF_PACK=0: up to their tokens, which k_pack packs; CSH_REF_LIST=0 leaves
// them to k_tokens).
//
// Replaces, for those scans, the per-block sweeps of k_entropy.hip's k_tokens and the token stream between it and k_pack (mozjpeg
// jcphuff.c encode_mcu_AC_first + jchuff.c statistics, reached from /root/reference/src/compressor.rs:305).
//
// Why: the scan search codes ~30 first-pass candidates per file, and a lane that owns a block spends a step on each of its 63
// positions in every one of them although one coefficient in eight is non-zero.  Here the non-zero coefficients of a component are
// written down ONCE per point transform Al -- an NzList (types.h): per block its entries in zig-zag order, then an END entry -- and every
// candidate scan (Ss, Se, Al) is a FLAT walk over that list, one entry per lane:
//   * an entry with Ss <= k <= Se is a coded coefficient; its zero run is the distance to the entry in front of it when that one belongs
//     to the same block and band (the neighbouring lane: lists are sorted), else to the band's start;
//   * the first entry of a block that lies behind the band (k > Se; the END entry at the latest) stands for the block's end: it knows
//     whether the block coded anything (has-symbol) and whether it ends with an EOB -- the two flags k_ac_runs builds the EOB runs from --
//     and, in the pack pass, emits the EOBRUN symbol the block owns.
// No token is written: k_list_stats takes the histograms (and the flags), k_list_pack derives the same events again and turns them into bits
// with the optimal tables -- an event is a dozen instructions, a token was a 4-byte store and a 4-byte load.
// The kernels are written once for both builds (wave.h): the emulation runs the statements the device runs.
#include "kernels.h"
#include "wave.h"
#include "tok_bits.h"

namespace csh {

#define CSH_LP_WORDS 1024   // the packer's window of the bit stream, per wave, in LDS words (a step of 256 entries adds at most 256 x 79 bits = 632 words)

__device__ __forceinline__ static uint32_t lbitlen(uint32_t v) { return 32u - uint32_t(__clz(v)); }
__device__ __forceinline__ static int lwave() { return int(threadIdx.x) / CSP_WAVE_THREADS; }

// ------------------------------------------------------------------------------------------------ the builder
// Level 0 (k_nzlist): one wave per 256-block chunk of a component.  Lane (b, o) = (l >> 3, l & 7) holds octet o (coefficients 8 o .. 8 o + 7:
// one 16-byte load) of block 8 s + b in step s, so the lanes of a step, in lane order, hold 8 blocks' coefficients in list order: a wave
// scan of the per-lane counts places every lane's entries, and the lanes' stores land next to each other.  A wave takes half a chunk (16
// steps: 16 loads in flight per lane, 64 registers) and both passes -- the entry count, then, behind one atomic add on the list's cursor,
// the entries -- run from those registers: the kernel waits for memory once.
// The other levels (k_nzfilter): flat over the level-0 chunk, entry -> |c| >> Al, dropped when that is zero.
#define CSH_NZ_HALF 16   // steps of 8 blocks held in registers at a time: half a chunk
__device__ __forceinline__ static uint4 nz_load(const EncCtx &c, const NzSet &S, uint32_t u, int bx, int by, uint32_t oct) {
    uint4 q; q.x = q.y = q.z = q.w = 0u;
    if (u < S.nunits) {
        const int b = by * S.bw + bx;
        q = *reinterpret_cast<const uint4 *>(c.coef + (size_t(S.tile_base) + size_t(b >> 6)) * CSH_TILE_I16 + size_t((b & 63) * CSH_BLK_STRIDE) + size_t(oct) * CSH_OCT_STRIDE);
    }
    return q;
}
// bit i: coefficient i of the octet is a non-zero AC coefficient
__device__ __forceinline__ static uint32_t nz_mask8(const uint4 &q, uint32_t oct) {
    uint32_t m = 0;
    m |= (q.x & 0xFFFFu) ? 1u : 0u;   m |= (q.x >> 16) ? 2u : 0u;
    m |= (q.y & 0xFFFFu) ? 4u : 0u;   m |= (q.y >> 16) ? 8u : 0u;
    m |= (q.z & 0xFFFFu) ? 16u : 0u;  m |= (q.z >> 16) ? 32u : 0u;
    m |= (q.w & 0xFFFFu) ? 64u : 0u;  m |= (q.w >> 16) ? 128u : 0u;
    return oct ? m : (m & ~1u);
}
// half `half` (128 blocks, 16 steps) of the chunk that starts at block u0: every lane's 16 octets, all loads in flight at once
__device__ __forceinline__ static void nz_load_half(const EncCtx &c, const NzSet &S, uint32_t u0, int half, LV<uint4> (&q)[CSH_NZ_HALF]) {
    LFOR(l) {
        const uint32_t oct = uint32_t(l & 7);
        uint32_t u = u0 + 128u * uint32_t(half) + uint32_t(l >> 3);
        int by = int(u) / S.real_bw, bx = int(u) - by * S.real_bw;
        CSH_UNROLL
        for (int s = 0; s < CSH_NZ_HALF; s++) {
            q[s][l] = nz_load(c, S, u, bx, by, oct);
            u += 8u; bx += 8;
            while (bx >= S.real_bw) { bx -= S.real_bw; by++; }   // eight blocks on
        }
    }
}
// entries of the half per lane: its non-zero AC coefficients; the lane of octet 7 adds the block's END
__device__ __forceinline__ static void nz_count_half(const NzSet &S, uint32_t u0, int half, const LV<uint4> (&q)[CSH_NZ_HALF], LV<uint32_t> &cnt) {
    LFOR(l) {
        const uint32_t oct = uint32_t(l & 7);
        uint32_t n = 0;
        CSH_UNROLL
        for (int s = 0; s < CSH_NZ_HALF; s++)
            n += uint32_t(__popc(nz_mask8(q[s][l], oct))) + ((oct == 7u && u0 + 128u * uint32_t(half) + 8u * uint32_t(s) + uint32_t(l >> 3) < S.nunits) ? 1u : 0u);
        cnt[l] += n;
    }
}
__device__ __forceinline__ static void nz_write_half(const NzSet &S, uint32_t u0, int half, const LV<uint4> (&q)[CSH_NZ_HALF], uint32_t *dst, uint32_t run, uint8_t *blk_cnt, uint16_t *blk_off) {
    CSH_UNROLL
    for (int s = 0; s < CSH_NZ_HALF; s++) {
        LV<uint32_t> mk, cl;
        LFOR(l) {
            const uint32_t oct = uint32_t(l & 7);
            mk[l] = nz_mask8(q[s][l], oct);
            cl[l] = uint32_t(__popc(mk[l])) + ((oct == 7u && u0 + 128u * uint32_t(half) + 8u * uint32_t(s) + uint32_t(l >> 3) < S.nunits) ? 1u : 0u);
        }
        uint32_t tot;
        const LV<uint32_t> ex = lscan(cl, tot);
        if (blk_cnt) {   // the block's entries = where its END lands - where its first octet starts (seven lanes down)
            LV<uint32_t> first = ex;
            for (int d = 0; d < 7; d++) first = lprev(first, 0u);
            LFOR(l) {
                const uint32_t blk = 16u * 8u * uint32_t(half) + 8u * uint32_t(s) + uint32_t(l >> 3);
                if ((l & 7) == 7 && u0 + blk < S.nunits) blk_cnt[u0 + blk] = uint8_t(ex[l] + cl[l] - 1u - first[l]);
                if ((l & 7) == 7 && u0 + blk < S.nunits && blk_off) blk_off[u0 + blk] = uint16_t(run + first[l]);   // (a chunk holds at most 256 x 64 entries)
            }
        }
        LFOR(l) {
            const uint32_t oct = uint32_t(l & 7);
            const uint32_t blk = 16u * 8u * uint32_t(half) + 8u * uint32_t(s) + uint32_t(l >> 3);
            const uint32_t base = (8u * oct) | (blk << 23);
            const uint32_t w[4] = {q[s][l].x, q[s][l].y, q[s][l].z, q[s][l].w};
            uint32_t o = run + ex[l];
            CSH_UNROLL
            for (int i = 0; i < 8; i++)
                if ((mk[l] >> i) & 1u) {
                    const int h = (i & 1) ? (int(w[i >> 1]) >> 16) : (int(w[i >> 1] << 16) >> 16);
                    const uint32_t a = h == -32768 ? 32767u : uint32_t(h < 0 ? -h : h);   // 15 bits of magnitude: -32768 (a crafted progressive input; no encoder's coefficient) must not reach the block field
                    dst[o++] = (base + uint32_t(i)) | (h < 0 ? 128u : 0u) | (a << 8);
                }
            if (oct == 7u && u0 + blk < S.nunits) dst[o] = CSH_NZ_END | (base & 0x7F800000u);
        }
        run += tot;
    }
}
__global__ void __launch_bounds__(128, 3) k_nzlist(EncCtx c) {
    // two waves per chunk, one half each: a wave loads its 128 blocks once, counts, and -- behind the barrier at which wave 0 reserves the
    // chunk's room -- writes its entries from the same registers
    CSH_SHARED uint32_t s_cnt[2];
    CSH_SHARED uint32_t s_rel;      // the chunk's first entry, relative to the list's region; 0xFFFFFFFF: no room
    CSH_WPERSIST(LV<uint4>, q, CSH_NZ_HALF, 2);
    const NzChunk ch = c.nzchunks[blockIdx.x];
    const int half = lwave();
    const bool skip = !(ch.levels & 1u) || (c.work_active && !c.work_active[ch.work0]);
    CSH_PHASE_LOOP(3) {
        if (skip) continue;
        const NzSet S = c.nzsets[ch.set];
        const uint32_t u0 = ch.j * 256u;
        const NzList L0 = c.nzlists[S.list[0]];
        if (phase == 0) {
            LV<uint32_t> cnt;
            LFOR(l) cnt[l] = 0u;
            nz_load_half(c, S, u0, half, q);
            nz_count_half(S, u0, half, q, cnt);
            const uint32_t n = lsum32(cnt);
            LFOR(l) if (l == 0) s_cnt[half] = n;
            continue;
        }
        if (phase == 1) {
            if (half == 0) {
                const uint32_t n0 = s_cnt[0] + s_cnt[1], n0a = (n0 + 3u) & ~3u, rec0 = L0.chunk0 + ch.j;
                uint32_t rel = 0;
                LFOR(l) if (l == 0) rel = atomicAdd(&c.nz_cursor[S.list[0]], n0a);
                rel = uni(rel);
                const bool ok0 = uint64_t(rel) + n0a <= L0.cap;
                LFOR(l) if (l == 0) { c.nz_chunk_off[rec0] = rel; c.nz_chunk_cnt[rec0] = ok0 ? n0 : 0u; if (!ok0) c.overflow[1] = 1; s_rel = ok0 ? rel : 0xFFFFFFFFu; }
            }
            continue;
        }
        if (s_rel == 0xFFFFFFFFu) continue;
        uint32_t *dst = c.nz_pool + L0.base + s_rel;
        uint8_t *blk_cnt = (c.nz_blk_cnt && S.cnt_base != 0xFFFFFFFFu) ? c.nz_blk_cnt + S.cnt_base : nullptr;
        uint16_t *blk_off = (blk_cnt && c.nz_blk_off) ? c.nz_blk_off + S.cnt_base : nullptr;
        nz_write_half(S, u0, half, q, dst, half ? s_cnt[0] : 0u, blk_cnt, blk_off);
        if (half == 1) {   // padding to the next 16-byte boundary: entries that code nothing
            const uint32_t n0 = s_cnt[0] + s_cnt[1], n0a = (n0 + 3u) & ~3u;
            LFOR(l) if (n0 + uint32_t(l) < n0a) dst[n0 + uint32_t(l)] = 0u;
        }
    }
}
// the other point transforms of a chunk, filtered from its level 0 (which this stage's k_nzlist or an earlier stage's made): count, one
// atomic add per list, write.  Four entries per lane and step; the second pass reads the chunk out of the L2.
__global__ void __launch_bounds__(64) k_nzfilter(EncCtx c) {
    const NzChunk ch = c.nzchunks[blockIdx.x];
    const uint32_t others = ch.levels & ~1u;   // levels 1..3 to filter, and CSH_NZ_COMPACT0
    if (!others) return;
    const bool compact0 = (ch.levels & CSH_NZ_COMPACT0) != 0u;
    const NzSet S = c.nzsets[ch.set];
    if (c.work_active && !c.work_active[ch.work0]) return;
    const NzList L0 = c.nzlists[S.list[0]];
    const uint32_t n0 = c.nz_chunk_cnt[L0.chunk0 + ch.j];
    const uint32_t *src = c.nz_pool + L0.base + c.nz_chunk_off[L0.chunk0 + ch.j];
    auto kept = [](uint32_t x, int L) { return ((x & CSH_NZ_END) != 0u || (((x >> 8) & 0x7FFFu) >> L) != 0u) ? 1u : 0u; };   // an END entry, or a coefficient that is not zero at level L
    // (level 0 here only under CSH_NZ_COMPACT0: the list k_trellis_ac wrote its levels into -- the coefficients it dropped have magnitude 0 -- is
    // compacted IN PLACE: a step's 256 entries are in registers before any of them is written, and an entry never moves up)
    const int Lfirst = compact0 ? 0 : 1;
    LV<uint32_t> cntL[CSH_NZ_LEVELS];
    LFOR(l) for (int L = 0; L < CSH_NZ_LEVELS; L++) cntL[L][l] = 0u;
    for (uint32_t g0 = 0; g0 < n0; g0 += 256) {
        LFOR(l) {
            const uint32_t g = g0 + 4u * uint32_t(l);
            uint4 e; e.x = e.y = e.z = e.w = 0u;
            if (g < n0) e = *reinterpret_cast<const uint4 *>(src + g);
            if (g < n0) {   // (the padding behind the chunk's last entry is not an entry: it must not count as a level-0 END)
                CSH_UNROLL
                for (int L = 0; L < CSH_NZ_LEVELS; L++) cntL[L][l] += kept(e.x, L) + kept(e.y, L) + kept(e.z, L) + kept(e.w, L);
            }
        }
    }
    uint32_t *dstL[CSH_NZ_LEVELS];
    uint32_t runL[CSH_NZ_LEVELS];
    bool okL[CSH_NZ_LEVELS];
    uint32_t n0new = n0;
    dstL[0] = nullptr; runL[0] = 0; okL[0] = false;
    if (compact0 && n0) {   // same place, same room: nothing to reserve; the count and the padding are written behind the last step
        dstL[0] = c.nz_pool + L0.base + c.nz_chunk_off[L0.chunk0 + ch.j];
        okL[0] = true;
        n0new = lsum32(cntL[0]);
    }
    for (int L = 1; L < CSH_NZ_LEVELS; L++) {
        dstL[L] = nullptr; runL[L] = 0; okL[L] = false;
        if (!((others >> L) & 1u)) continue;
        const NzList LL = c.nzlists[S.list[L]];
        const uint32_t n = lsum32(cntL[L]), na = (n + 3u) & ~3u;
        uint32_t rel = 0;
        LFOR(l) if (l == 0) rel = atomicAdd(&c.nz_cursor[S.list[L]], na);
        rel = uni(rel);
        okL[L] = n0 != 0u && uint64_t(rel) + na <= LL.cap;
        dstL[L] = c.nz_pool + LL.base + rel;
        LFOR(l) {
            if (l == 0) { c.nz_chunk_off[LL.chunk0 + ch.j] = rel; c.nz_chunk_cnt[LL.chunk0 + ch.j] = okL[L] ? n : 0u; if (!okL[L]) c.overflow[1] = 1; }
            if (okL[L] && n + uint32_t(l) < na) dstL[L][n + uint32_t(l)] = 0u;   // padding
        }
    }
    for (uint32_t g0 = 0; g0 < n0; g0 += 256) {
        LV<uint32_t> e0, e1, e2, e3;
        LFOR(l) {
            const uint32_t g = g0 + 4u * uint32_t(l);
            uint4 e; e.x = e.y = e.z = e.w = 0u;
            if (g < n0) e = *reinterpret_cast<const uint4 *>(src + g);
            e0[l] = e.x; e1[l] = e.y; e2[l] = e.z; e3[l] = e.w;
        }
        for (int L = Lfirst; L < CSH_NZ_LEVELS; L++) {
            if (!okL[L]) continue;
            LV<uint32_t> k4;
            LFOR(l) k4[l] = kept(e0[l], L) + kept(e1[l], L) + kept(e2[l], L) + kept(e3[l], L);
            uint32_t tot;
            const LV<uint32_t> ex = lscan(k4, tot);
            LFOR(l) {
                const uint32_t e[4] = {e0[l], e1[l], e2[l], e3[l]};
                uint32_t o = runL[L] + ex[l];
                CSH_UNROLL
                for (int q = 0; q < 4; q++)
                    if (kept(e[q], L)) dstL[L][o++] = (e[q] & 0xFF8000FFu) | ((((e[q] >> 8) & 0x7FFFu) >> L) << 8);
            }
            runL[L] += tot;
        }
    }
    if (okL[0]) {
        const uint32_t na = (n0new + 3u) & ~3u;
        LFOR(l) {
            if (n0new + uint32_t(l) < na) dstL[0][n0new + uint32_t(l)] = 0u;   // padding to the 16-byte boundary: entries that code nothing
            if (l == 0) c.nz_chunk_cnt[L0.chunk0 + ch.j] = n0new;
        }
    }
}

// ---- the way back, for the debug tap (csh_batch_read_coefs): a component whose AC levels the run kept in its level-0 list alone (PlaneWork::ac_lists) gets them
// written into its tiles again.  One workgroup per 256-block chunk of the list: every block's AC is zeroed -- octets 1..7, and coefficients 1..7 of octet 0, which
// hold the scalar quantiser's levels whatever the trellis made of them; the DC stays --, then the chunk's entries go to their places, with their signs.  An entry of
// magnitude 0 (a coefficient the trellis dropped, in a list k_nzfilter has not compacted) writes the zero that is there already; END entries and padding write
// nothing.  The list is only read, and the tile's AC is written from nothing but the list: calling it again changes nothing, and no later run reads what it wrote
__global__ void __launch_bounds__(256) k_nz_to_tiles(const NzSet *nzsets, const NzList *nzlists, const uint32_t *nz_pool, const uint32_t *nz_chunk_off, const uint32_t *nz_chunk_cnt, uint32_t set,
                                                      int16_t *coef) {
    const NzSet S = nzsets[set];
    const NzList L0 = nzlists[S.list[0]];
    const uint32_t j = blockIdx.x, u0 = j * 256u;
    CSH_PHASE_LOOP(2) {
        if (phase == 0) {
            const uint32_t u = u0 + threadIdx.x;
            if (u >= S.nunits) continue;
            const int by = int(u) / S.real_bw, bx = int(u) - by * S.real_bw;
            int16_t *blk = coef + coef_index(S.tile_base, by * S.bw + bx, 0);
            uint4 z; z.x = z.y = z.z = z.w = 0u;
            z.x = uint32_t(uint16_t(blk[0]));
            CSH_UNROLL
            for (int o = 0; o < 8; o++) { *reinterpret_cast<uint4 *>(blk + CSH_OCT_STRIDE * o) = z; z.x = 0u; }
            continue;
        }
        const uint32_t n = nz_chunk_cnt[L0.chunk0 + j];
        const uint32_t *src = nz_pool + L0.base + nz_chunk_off[L0.chunk0 + j];
        for (uint32_t i = threadIdx.x; i < n; i += 256u) {
            const uint32_t e = src[i], k = e & 127u, u = u0 + ((e >> 23) & 255u);
            if (k == 0u || k >= CSH_NZ_END || u >= S.nunits) continue;
            const int by = int(u) / S.real_bw, bx = int(u) - by * S.real_bw, m = int((e >> 8) & 0x7FFFu);
            coef[coef_index(S.tile_base, by * S.bw + bx, int(k))] = int16_t((e & 128u) ? -m : m);
        }
    }
}
void launch_nz_to_tiles(hipStream_t st, const NzSet *nzsets, const NzList *nzlists, const uint32_t *nz_pool, const uint32_t *nz_chunk_off, const uint32_t *nz_chunk_cnt, uint32_t set,
                        uint32_t nchunks, int16_t *coef) {
    if (nchunks) CSH_LAUNCH_PHASED(k_nz_to_tiles, 2, dim3(nchunks), dim3(256), st, nzsets, nzlists, nz_pool, nz_chunk_off, nz_chunk_cnt, set, coef);
}

// ------------------------------------------------------------------------------------------------ the events of a first-pass scan
// What entry e means in scan (Ss, Se), given the entry p in front of it (the END of the block before: CSH_NZ_END):
//   coded   Ss <= k <= Se: symbol (run & 15) << 4 | size, run >> 4 ZRLs in front of it, `size` value bits
//   term    the block's first entry behind the band (the END entry included): the block's end -- has: it coded something;
//           eob: it ends with an EOB (nothing coded at Se)
struct NzEvent { uint32_t coded, term, run, size, bits, has, eob, blk; };
__device__ __forceinline__ static NzEvent nz_event(uint32_t e, uint32_t p, uint32_t Ss, uint32_t Se) {
    NzEvent v;
    const uint32_t k = e & 127u, pk = p & 127u;
    const bool same = !(p & CSH_NZ_END);            // p belongs to e's block (every block's last entry is its END)
    const bool pin = same && pk >= Ss;               // ... and to the band (pk < k: the list is sorted)
    v.coded = (k >= Ss && k <= Se) ? 1u : 0u;
    v.term = (k > Se && !(same && pk > Se)) ? 1u : 0u;
    v.run = k - (pin ? pk + 1u : Ss);
    const uint32_t m = (e >> 8) & 0x7FFFu;
    v.size = lbitlen(m);
    v.bits = ((e & 128u) ? ~m : m) & ((1u << v.size) - 1u);
    v.has = pin ? 1u : 0u;                           // (term: pk <= Se)
    v.eob = (pin && pk == Se) ? 0u : 1u;
    v.blk = (e >> 23) & 255u;
    return v;
}
struct ListSlot { const uint32_t *lst; uint32_t n; };
// chunk record `rec` of the list whose region starts at entry `base` of the pool: two independent loads.  A slot record names its list and its chunk record
// (k_make_slots), and the chunks of a work item stand in consecutive records: a wave that codes a run of chunks loads the slot record and the list's base once
__device__ __forceinline__ static ListSlot list_chunk(const EncCtx &c, uint64_t base, uint32_t rec) {
    ListSlot s;
    s.n = c.nz_chunk_cnt[rec];
    s.lst = c.nz_pool + base + c.nz_chunk_off[rec];
    return s;
}
// ---- LIST RUNS.  The three walkers below take ONE WAVE per run of up to EncCtx::list_run (CSH_LIST_RUN) consecutive chunks j0 .. j0 + n - 1 of one work item
// (EncCtx::list_runs / ref_runs name every run's first slot; n = min(list_run, nch - j0)).  A run never leaves its scan, so the slot record of its first chunk
// stands for all of them -- band, tables, list, gate, placement -- and what differs follows from j: slot cs0 + i, chunk record nzrec + i, units unit0 + 256 i,
// histogram rows hist_row + i ntables, correction words corr0 + 256 i.  Per run: the chain slot record -> list -> first entries, the LDS set-up, the atomics on
// the scan's statistics; per chunk: what the later kernels read per slot, bit for bit what one wave per chunk wrote.  list_run = 1 is that mapping.
__device__ __forceinline__ static uint32_t run_chunks(const EncCtx &c, const SlotRec &r) { const uint32_t left = r.nch - r.j; return left < c.list_run ? left : c.list_run; }
// four consecutive entries per lane (the chunk starts on a 16-byte boundary and is padded to one with entries that code nothing)
__device__ __forceinline__ static void list_load4(const ListSlot &s, uint32_t g, uint32_t &e0, uint32_t &e1, uint32_t &e2, uint32_t &e3) {
    uint4 q; q.x = q.y = q.z = q.w = 0u;
    if (g < s.n) q = *reinterpret_cast<const uint4 *>(s.lst + g);
    e0 = q.x; e1 = q.y; e2 = q.z; e3 = q.w;
}

// a chunk's histogram out of the wave's four LDS copies: lane l takes symbols 4 l .. 4 l + 3 (one 16-byte read per copy), leaves the copies at zero for the next
// chunk, writes the slot's row (one 8-byte store) and adds the counts to the run's sums
__device__ __forceinline__ static void hist_flush(uint32_t *hist, uint16_t *row, LV<uint32_t> (&freq)[4]) {
    LFOR(l) {
        uint4 s; s.x = s.y = s.z = s.w = 0u;
        CSH_UNROLL
        for (int cpy = 0; cpy < 4; cpy++) {
            uint4 *h = reinterpret_cast<uint4 *>(hist + 256 * cpy + 4 * l);
            const uint4 v = *h;
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            uint4 zero; zero.x = zero.y = zero.z = zero.w = 0u;
            *h = zero;
        }
        uint2 o; o.x = (s.x & 0xFFFFu) | (s.y << 16); o.y = (s.z & 0xFFFFu) | (s.w << 16);
        *reinterpret_cast<uint2 *>(row + 4 * l) = o;
        freq[0][l] += s.x; freq[1][l] += s.y; freq[2][l] += s.z; freq[3][l] += s.w;
    }
}
// the run's sums into the scan's symbol frequencies (integer sums: the order does not show)
__device__ __forceinline__ static void freq_flush(uint32_t *dst, const LV<uint32_t> (&freq)[4]) {
    LFOR(l) {
        CSH_UNROLL
        for (int q = 0; q < 4; q++) if (freq[q][l]) atomicAdd(&dst[4 * l + q], freq[q][l]);
    }
}
// ---- statistics: ONE WAVE per run of (scan, chunk) slots.  Symbol histogram in LDS (four copies, lane & 3: the frequent symbols -- 0x01, 0x11,
// 0x02 -- meet in most steps, and equal addresses serialise), raw-bit count, the has-symbol / ends-with-EOB bits of the chunk's 256 blocks: written per
// slot.  The scan's symbol frequencies (tables[].freq) take the sums of the whole run, from four registers per lane, behind its last chunk.
__global__ void __launch_bounds__(256) k_list_stats(EncCtx c) {
    CSH_SHARED alignas(16) uint32_t s_hist[4][4][256];
    CSH_SHARED uint32_t s_flag[4][16];    // words 0..7: has-symbol, 8..15: ends-with-EOB
    const int wv = int(uni(uint32_t(lwave())));   // (said to be wave-uniform: the run's records are then scalar loads into SGPRs, not a copy per lane in VGPRs)
    const uint32_t idx = blockIdx.x * 4u + uint32_t(wv);
    if (idx >= c.nlist_runs) return;
    const uint32_t cs0 = c.list_runs[idx];
    const SlotRec r = c.slots[cs0];
    if (c.work_active && !c.work_active[r.work]) return;
    const uint32_t nrun = run_chunks(c, r);
    const uint64_t lbase = c.nzlists[r.nzlist].base;
    ListSlot nx = list_chunk(c, lbase, r.nzrec);
    uint32_t *hist = &s_hist[wv][0][0], *flag = s_flag[wv];
    LFOR(l) {   // (a chunk's flush leaves them at zero for the next)
        uint4 zero; zero.x = zero.y = zero.z = zero.w = 0u;
        for (int i = 4 * l; i < 1024; i += 256) *reinterpret_cast<uint4 *>(hist + i) = zero;
        if (l < 16) flag[l] = 0u;
    }
    CSP_WAVE_SYNC();
    const uint32_t Ss = r.Ss, Se = r.Se;
    LV<uint32_t> freq[4];   // the run's count of symbols 4 l .. 4 l + 3
    LFOR(l) { freq[0][l] = 0u; freq[1][l] = 0u; freq[2][l] = 0u; freq[3][l] = 0u; }
    // (the next step's entries are asked for before this step's are looked at: a step is short, and what it waited for was its own load; behind a chunk's
    // last step they are the next chunk's first, whose record was asked for when this chunk began)
    LV<uint32_t> x0, x1, x2, x3;
    bool ahead = false;
    for (uint32_t ci = 0; ci < nrun; ci++) {
        const ListSlot ls = nx;
        const bool more = ci + 1u < nrun;
        if (more) nx = list_chunk(c, lbase, r.nzrec + ci + 1u);
        if (!ahead) LFOR(l) list_load4(ls, 4u * uint32_t(l), x0[l], x1[l], x2[l], x3[l]);
        ahead = false;
        uint32_t carry = CSH_NZ_END;
        LV<uint32_t> raw;
        LFOR(l) raw[l] = 0u;
        for (uint32_t g0 = 0; g0 < ls.n; g0 += 256) {
            const LV<uint32_t> e0 = x0, e1 = x1, e2 = x2, e3 = x3;
            if (g0 + 256u < ls.n) LFOR(l) list_load4(ls, g0 + 256u + 4u * uint32_t(l), x0[l], x1[l], x2[l], x3[l]);
            else if (more) { LFOR(l) list_load4(nx, 4u * uint32_t(l), x0[l], x1[l], x2[l], x3[l]); ahead = true; }
            const LV<uint32_t> p0 = lprev(e3, carry);
            carry = llast(e3);
            LFOR(l) {
                uint32_t *h = hist + 256 * (l & 3);
                const uint32_t e[4] = {e0[l], e1[l], e2[l], e3[l]}, p[4] = {p0[l], e0[l], e1[l], e2[l]};
                CSH_UNROLL
                for (int q = 0; q < 4; q++) {
                    const NzEvent v = nz_event(e[q], p[q], Ss, Se);
                    if (v.coded) {
                        atomicAdd(&h[((v.run & 15u) << 4) | v.size], 1u);
                        if (v.run >> 4) atomicAdd(&h[0xF0], v.run >> 4);
                        raw[l] += v.size;
                    } else if (v.term) {
                        if (v.has) atomicOr(&flag[v.blk >> 5], 1u << (v.blk & 31u));
                        if (v.eob) atomicOr(&flag[8u + (v.blk >> 5)], 1u << (v.blk & 31u));
                    }
                }
            }
        }
        CSP_WAVE_SYNC();
        const uint32_t rawbits = lsum32(raw);
        const uint32_t cs = cs0 + ci, j = r.j + ci, hist_row = r.hist_row + ci * uint32_t(r.ntables);
        hist_flush(hist, c.slot_hist + size_t(hist_row) * 256u, freq);
        LFOR(l) {
            if (l == 0) c.slot_raw[cs] = rawbits;
            if (l < 4 && j * 4u + uint32_t(l) < ((r.nunits_work + 63u) >> 6)) {   // lane = block bit, so the chunk's flags ARE four words of the scan's bit vectors
                c.sym_bits[r.word_base + j * 4u + uint32_t(l)] = uint64_t(flag[2 * l]) | (uint64_t(flag[2 * l + 1]) << 32);
                c.eob_bits[r.word_base + j * 4u + uint32_t(l)] = uint64_t(flag[8 + 2 * l]) | (uint64_t(flag[9 + 2 * l]) << 32);
            }
        }
        CSP_WAVE_SYNC();
        LFOR(l) if (l < 16) flag[l] = 0u;
        CSP_WAVE_SYNC();
    }
    freq_flush(c.tables[r.table_base].freq, freq);
}

// ---- pack: ONE WAVE per run of (scan, chunk) slots.  256 entries a step, four per lane: their bits (ZRLs, symbol + value bits; a block's EOBRUN
// symbol at its end), a wave scan of the lengths, every lane ORs its pieces into the wave's LDS window of the bit stream.  The window is
// word-aligned with the raw pool, so flushing it is a plain copy.  Chunk j + 1 of a scan starts at the bit where chunk j ended (chunk_off is an exclusive
// scan in slot order), so across the chunks of a run the position, the window and the code table simply carry on: only the RUN's first and last word can
// be shared with a neighbouring run and are ORed in (k_zero_edges cleared them, with every chunk's); the words at the chunk edges inside the run are
// plain stores by the wave that owns both sides of them.
__device__ __forceinline__ static void lor_bits(uint32_t *words, uint64_t pos, uint32_t v, uint32_t n) {   // n in 1..32, at bit `pos` of a big-endian-logical word array
    v &= n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
    const uint64_t t = uint64_t(v) << (64u - n - uint32_t(pos & 31u));
    const uint32_t hi = uint32_t(t >> 32), lo = uint32_t(t);
    if (hi) atomicOr(words + (pos >> 5), hi);
    if (lo) atomicOr(words + (pos >> 5) + 1, lo);
}
__global__ void __launch_bounds__(256) k_list_pack(EncCtx c) {
    CSH_SHARED alignas(16) uint32_t s_win[4][CSH_LP_WORDS];
    CSH_SHARED uint32_t s_lut[4][256];
    CSH_SHARED uint16_t s_eob[4][256];
    const int wv = int(uni(uint32_t(lwave())));   // (said to be wave-uniform: the run's records are then scalar loads into SGPRs, not a copy per lane in VGPRs)
    const uint32_t idx = blockIdx.x * 4u + uint32_t(wv);
    if (idx >= c.nlist_runs) return;
    const uint32_t cs0 = c.list_runs[idx];
    const SlotRec r = c.slots[cs0];
    if (c.work_active && !c.work_active[r.work]) return;
    const ScanWork &w = c.work[r.work];
    if (w.no_room) { LFOR(l) if (l == 0) c.status[w.image] = 20200; return; }   // decided per scan by k_scan_place
    const uint32_t nrun = run_chunks(c, r);
    const uint64_t lbase = c.nzlists[r.nzlist].base;
    ListSlot nx = list_chunk(c, lbase, r.nzrec);
    // the run's place: from bit raw_bit0 of the raw pool on; the scan's last chunk (the last of its run) also carries the 1-bits that fill the last byte
    const uint64_t scan0 = c.chunk_off[r.first_chunk];
    const uint64_t raw_bit0 = w.raw_off * 8 + (c.chunk_off[cs0] - scan0);
    uint32_t pad = 0;
    if (r.j + nrun == r.nch) { const uint64_t total = c.chunk_off[r.first_chunk + r.nch] - scan0; pad = uint32_t((8 - (total & 7)) & 7); }
    uint32_t *buf = s_win[wv], *lut = s_lut[wv];
    uint16_t *eobrun = s_eob[wv];
    LFOR(l) {
        for (int i = l; i < 256; i += 64) lut[i] = c.tables[r.table_base].lut[i];
        uint4 zero; zero.x = zero.y = zero.z = zero.w = 0u;
        for (int i = 4 * l; i < CSH_LP_WORDS; i += 256) *reinterpret_cast<uint4 *>(buf + i) = zero;
    }
    CSP_WAVE_SYNC();
    uint32_t *out = c.raw + (raw_bit0 >> 5);        // word 0 of the frame below
    uint64_t pos = raw_bit0 & 31u;                   // next bit, in the frame whose word 0 is the run's first word in the pool
    uint32_t ww = 0;                                 // first word of the window
    bool first_flush = true;
    const uint32_t Ss = r.Ss, Se = r.Se;
    const uint32_t zrl = lut[0xF0], zc = zrl & 0xFFFFu, zl = zrl >> 16;
    LV<uint32_t> x0, x1, x2, x3;   // the next step's entries, asked for a step ahead (behind a chunk's last step: the next chunk's first)
    bool ahead = false;
    for (uint32_t ci = 0; ci < nrun; ci++) {
        const ListSlot ls = nx;
        const bool more = ci + 1u < nrun;
        if (more) nx = list_chunk(c, lbase, r.nzrec + ci + 1u);
#ifdef CSH_EMUL
        {   // (where a pool had no room the pass is repeated and its sizes are not of these lists: even then a run never gets ahead of its sized place -- DESIGN 4.1)
            const uint64_t want = (raw_bit0 & 31u) + (c.chunk_off[cs0 + ci] - c.chunk_off[cs0]);
            if (c.overflow[1] ? pos > want : pos != want) { fprintf(stderr, "k_list_pack: chunk %u of a run does not start where the one before it ended\n", ci); abort(); }
        }
#endif
        CSP_WAVE_SYNC();   // (the steps of the chunk before have read their EOBRUN values)
        {
            const uint32_t u0 = r.unit0 + 256u * ci, left = r.nunits_work - 256u * (r.j + ci), nun = left < 256u ? left : 256u;
            LFOR(l) for (int i = l; i < 256; i += 64) eobrun[i] = uint32_t(i) < nun ? c.eobrun[u0 + uint32_t(i)] : uint16_t(0);
        }
        CSP_WAVE_SYNC();
        if (!ahead) LFOR(l) list_load4(ls, 4u * uint32_t(l), x0[l], x1[l], x2[l], x3[l]);
        ahead = false;
        uint32_t carry = CSH_NZ_END;
        const uint32_t cpad = more ? 0u : pad;
        const uint32_t n_ext = ls.n + (cpad ? 1u : 0u);   // the byte fill rides as one more entry
        for (uint32_t g0 = 0; g0 < n_ext; g0 += 256) {
            const LV<uint32_t> e0 = x0, e1 = x1, e2 = x2, e3 = x3;
            if (g0 + 256u < n_ext) LFOR(l) list_load4(ls, g0 + 256u + 4u * uint32_t(l), x0[l], x1[l], x2[l], x3[l]);
            else if (more) { LFOR(l) list_load4(nx, 4u * uint32_t(l), x0[l], x1[l], x2[l], x3[l]); ahead = true; }
            const LV<uint32_t> p0 = lprev(e3, carry);
            carry = llast(e3);
            // what every entry emits: nz[q] ZRLs, then the n[q] low bits of v[q]
            LV<uint32_t> v0, v1, v2, v3, n0, n1, n2, n3, z, len;
            LFOR(l) {
                const uint32_t e[4] = {e0[l], e1[l], e2[l], e3[l]}, p[4] = {p0[l], e0[l], e1[l], e2[l]};
                uint32_t v[4], n[4], zz = 0, ln = 0;
                CSH_UNROLL
                for (int q = 0; q < 4; q++) {
                    v[q] = 0; n[q] = 0;
                    const uint32_t g = g0 + 4u * uint32_t(l) + uint32_t(q);
                    const NzEvent ev = nz_event(e[q], p[q], Ss, Se);
                    if (g >= ls.n) { if (cpad && g == ls.n) { v[q] = (1u << cpad) - 1u; n[q] = cpad; } }
                    else if (ev.coded) {
                        const uint32_t t = lut[((ev.run & 15u) << 4) | ev.size];
                        v[q] = ((t & 0xFFFFu) << ev.size) | ev.bits; n[q] = (t >> 16) + ev.size;   // <= 16 + 15 bits
                        zz |= (ev.run >> 4) << (2 * q);
                        ln += (ev.run >> 4) * zl;
                    } else if (ev.term) {
                        const uint32_t run = eobrun[ev.blk];
                        if (run) {
                            const uint32_t nb = lbitlen(run) - 1u, t = lut[nb << 4];
                            v[q] = ((t & 0xFFFFu) << nb) | (run & ((1u << nb) - 1u)); n[q] = (t >> 16) + nb;   // <= 16 + 14 bits
                        }
                    }
                    ln += n[q];
                }
                v0[l] = v[0]; v1[l] = v[1]; v2[l] = v[2]; v3[l] = v[3]; n0[l] = n[0]; n1[l] = n[1]; n2[l] = n[2]; n3[l] = n[3]; z[l] = zz; len[l] = ln;
            }
            uint32_t tot;
            const LV<uint32_t> ex = lscan(len, tot);
            LFOR(l) {
                uint64_t at = pos + ex[l] - uint64_t(ww) * 32u;    // bit position inside the window
                const uint32_t v[4] = {v0[l], v1[l], v2[l], v3[l]}, n[4] = {n0[l], n1[l], n2[l], n3[l]};
                CSH_UNROLL
                for (int q = 0; q < 4; q++) {
                    for (uint32_t t = (z[l] >> (2 * q)) & 3u; t; t--) { lor_bits(buf, at, zc, zl); at += zl; }
                    if (n[q]) { lor_bits(buf, at, v[q], n[q]); at += n[q]; }
                }
            }
            pos += tot;
            // slide the window when another step's worth of bits might not fit any more
            const uint32_t done = uint32_t(pos >> 5) - ww;   // complete words in the window
            if (done > CSH_LP_WORDS - 640) {
                CSP_WAVE_SYNC();
                LFOR(l) for (uint32_t q = uint32_t(l); q < done; q += 64) {
                    const uint32_t v = buf[q];
                    if (first_flush && q == 0) { if (v) atomicOr(out + ww, v); } else out[ww + q] = v;
                }
                const uint32_t partial = buf[done];
                CSP_WAVE_SYNC();
                LFOR(l) for (int q = l; q < CSH_LP_WORDS; q += 64) buf[q] = (q == 0) ? partial : 0u;
                CSP_WAVE_SYNC();
                ww += done; first_flush = false;
            }
        }
    }
#ifdef CSH_EMUL
    {
        const uint64_t want = (raw_bit0 & 31u) + (c.chunk_off[cs0 + nrun] - c.chunk_off[cs0]) + pad;
        if (c.overflow[1] ? pos > want : pos != want) { fprintf(stderr, "k_list_pack: a run does not end where its sizes say\n"); abort(); }
    }
#endif
    CSP_WAVE_SYNC();
    const uint32_t last = uint32_t((pos + 31) >> 5) - ww;   // words in the window that carry bits
    LFOR(l) for (uint32_t q = uint32_t(l); q < last; q += 64) {
        const uint32_t v = buf[q];
        if ((first_flush && q == 0) || q == last - 1) { if (v) atomicOr(out + ww + q, v); } else out[ww + q] = v;
    }
}

// ------------------------------------------------------------------------------------------------ refinement scans (Ah = Al + 1)
// A refinement scan is a flat walk over the component's level-Al list too: an entry of magnitude 1 (after >> Al) is a newly significant
// coefficient (N), one of magnitude >= 2 a coefficient with history (H) whose bit 0 is its correction bit; no tile is read, no bit plane made,
// and no lane walks a block by itself.  What k_tokens' kind-0 chunks made for such a scan (k_entropy.hip emit_ac_refine, refine_room,
// correction_word: the specification) comes out of k_list_refine, ONE WAVE per run of (scan, chunk) slots (LIST RUNS above), four entries per lane and step:
//   per entry, segmented by the blocks' END entries and carried across the steps:
//     hex   H entries of the block in front of it (its correction bit is bit 63 - hex of the block's correction word)
//     z     zeros of the band in front of it:  k - Ss - (N and H entries of the block in front of it)
//     zp    z of the block's previous N (0: none): the zero run of the entry is z - zp
//     zq    z of the entry in front of it in the block's band (0: none)
//   a ZRL is due whenever sixteen more zeros of a gap have gone by, at the next entry of the gap -- and only in gaps an N closes (k <= the
//   block's last N): entry e emits ((z - zp) >> 4) - ((zq - zp) >> 4) of them, an N then its own token with run (z - zp) & 15.  The correction
//   bits a token takes along are those since the block's last emitting entry (jcphuff.c: they ride behind the next symbol): hex - cur for the
//   first token of an entry, none for further ones.  The block's END entry is its EOB (unless an N sits at Se), with the H entries left.
// Pass 1 takes everything but the tokens -- histogram, correction words, tails, flags, raw bits, the number of tokens -- and leaves per block
// its last N and its H count in LDS; pass 2 reads the chunk again (out of the L2) and writes the tokens behind one atomic add on the region's
// cursor.  All of a slot's tokens are its segment 0 (k_pack walks the four segments as one list).  Under CSH_REF_PACK (the default) pass 2 is not run here:
// k_list_refine_pack, below, runs its statements once the tables exist and turns the tokens into bits without storing them.
struct RefCarry { uint32_t runH, runN, base, prevN, prevNZ; };
__device__ __forceinline__ static uint32_t ref_isN(uint32_t e, uint32_t Ss, uint32_t Se) { const uint32_t k = e & 127u; return (k >= Ss && k <= Se && ((e >> 8) & 0x7FFFu) == 1u) ? 1u : 0u; }
__device__ __forceinline__ static uint32_t ref_isH(uint32_t e, uint32_t Ss, uint32_t Se) { const uint32_t k = e & 127u; return (k >= Ss && k <= Se && ((e >> 8) & 0x7FFFu) >= 2u) ? 1u : 0u; }
__device__ __forceinline__ static uint32_t ref_same(uint32_t key, uint32_t blk) { return (key >> 6) == blk + 1u ? (key & 63u) : 0u; }   // the value of a (block + 1) << 6 | value key, if it is of this block
// one step's entries e[q][l] -> hex, z, zp, and with WITH_ZQ (pass 2) zq -- pass 1 hands in an array that is neither read nor written;
// entries that are neither N nor H get values nobody reads
template <bool WITH_ZQ>
__device__ __forceinline__ static void ref_step(const LV<uint32_t> (&e)[4], uint32_t Ss, uint32_t Se, RefCarry &C, LV<uint32_t> (&hex)[4], LV<uint32_t> (&z)[4], LV<uint32_t> (&zp)[4],
                                                LV<uint32_t> (&zq)[4]) {
    LV<uint32_t> cnt;
    LFOR(l) {
        uint32_t s = 0;
        CSH_UNROLL
        for (int q = 0; q < 4; q++) s += ref_isH(e[q][l], Ss, Se) | (ref_isN(e[q][l], Ss, Se) << 16);
        cnt[l] = s;
    }
    uint32_t tot;
    const LV<uint32_t> ex = lscan(cnt, tot);   // (a step has 256 entries: the halves do not meet)
    // where the block started: the H and N counts at the last END in front of the entry (a chunk has < 2^14 entries)
    LV<uint32_t> kb[4];
    LFOR(l) {
        uint32_t ph = C.runH + (ex[l] & 0xFFFFu), pn = C.runN + (ex[l] >> 16);
        CSH_UNROLL
        for (int q = 0; q < 4; q++) {
            kb[q][l] = (e[q][l] & CSH_NZ_END) ? ((ph << 14) | pn) + 1u : 0u;
            hex[q][l] = ph; z[q][l] = pn;   // for now: the counts from the chunk's start
            ph += ref_isH(e[q][l], Ss, Se); pn += ref_isN(e[q][l], Ss, Se);
        }
    }
    C.runH += tot & 0xFFFFu; C.runN += tot >> 16;
    lscan_last4(kb, C.base);
    LFOR(l) {
        CSH_UNROLL
        for (int q = 0; q < 4; q++) {
            const uint32_t b = kb[q][l] ? kb[q][l] - 1u : 0u, blk = (e[q][l] >> 23) & 255u, nz = ref_isH(e[q][l], Ss, Se) | ref_isN(e[q][l], Ss, Se);
            const uint32_t h = hex[q][l] - (b >> 14), n = z[q][l] - (b & 0x3FFFu);
            hex[q][l] = h;
            z[q][l] = nz ? (e[q][l] & 127u) - Ss - h - n : 0u;   // <= 62
            const uint32_t key = ((blk + 1u) << 6) | z[q][l];
            zp[q][l] = ref_isN(e[q][l], Ss, Se) ? key : 0u;
            if (WITH_ZQ) zq[q][l] = nz ? key : 0u;
        }
    }
    lscan_last4(zp, C.prevN);
    if (WITH_ZQ) lscan_last4(zq, C.prevNZ);
    LFOR(l) {
        CSH_UNROLL
        for (int q = 0; q < 4; q++) {
            const uint32_t blk = (e[q][l] >> 23) & 255u;
            zp[q][l] = ref_same(zp[q][l], blk);
            if (WITH_ZQ) zq[q][l] = ref_same(zq[q][l], blk);
        }
    }
}
// one step's tokens, behind ref_step<true>: per entry its ZRLs and its tokens (zq <- ZRLs | tokens << 8), the key of the block's last emitting entry in front
// of it (curc: carried across the steps of a chunk), a wave scan of the counts, and the token words at tk[at ...] in list order -- none at `limit` or behind it.
// lastn / nh: the chunk's blocks' last N (k << 6 | hex) and H entries, in LDS.  Returns the step's number of tokens.  Pass 2 of k_list_refine<true> stores
// them in the token pool; k_list_refine_pack in an LDS buffer it turns into bits at once: the same words either way
template <class TL, class TN>
__device__ __forceinline__ static uint32_t ref_step_tokens(const LV<uint32_t> (&e)[4], const LV<uint32_t> (&hex)[4], const LV<uint32_t> (&z)[4], const LV<uint32_t> (&zp)[4], LV<uint32_t> (&zq)[4],
                                                           uint32_t Ss, uint32_t Se, const TL *lastn, const TN *nh, uint32_t &curc, uint32_t *tk, uint32_t at, uint32_t limit) {
    LV<uint32_t> cur[4], nt;
    LFOR(l) {
        uint32_t s = 0;
        CSH_UNROLL
        for (int q = 0; q < 4; q++) {
            const uint32_t v = e[q][l], blk = (v >> 23) & 255u, lastk = uint32_t(lastn[blk]) >> 6, isN = ref_isN(v, Ss, Se);
            uint32_t nz = 0, n = 0;
            if ((isN | ref_isH(v, Ss, Se)) && (v & 127u) <= lastk) { nz = ((z[q][l] - zp[q][l]) >> 4) - ((zq[q][l] - zp[q][l]) >> 4); n = nz + isN; }
            cur[q][l] = n ? ((blk + 1u) << 6) | hex[q][l] : 0u;
            if ((v & CSH_NZ_END) && lastk != Se) n = 1u;
            zq[q][l] = nz | (n << 8);
            s += n;
        }
        nt[l] = s;
    }
    lscan_last4(cur, curc);
    uint32_t tot;
    const LV<uint32_t> ex = lscan(nt, tot);
    LFOR(l) {
        uint32_t o = at + ex[l];
        CSH_UNROLL
        for (int q = 0; q < 4; q++) {
            const uint32_t v = e[q][l], blk = (v >> 23) & 255u, nz = zq[q][l] & 255u, n = zq[q][l] >> 8;
            if (!n) continue;
            const uint32_t cu = ref_same(cur[q][l], blk);
            if (v & CSH_NZ_END) {
                if (o < limit) tk[o] = TK_EOB | (blk << 3) | ((uint32_t(nh[blk]) - cu) << 16) | (cu << 22);
                o++;
                continue;
            }
            // the first token takes the correction bits since the block's last emitting entry, the others none
            uint32_t cnt = hex[q][l] - cu, from = cu;
            for (uint32_t t = 0; t < nz; t++) {
                if (o < limit) tk[o] = TK_REF | (blk << 3) | (cnt << 16) | (from << 22) | (1u << 28);
                o++; cnt = 0u; from = hex[q][l];
            }
            if (n > nz) {
                if (o < limit) tk[o] = TK_REF | (blk << 3) | (((z[q][l] - zp[q][l]) & 15u) << 11) | ((v & 128u) ? 0u : (1u << 15)) | (cnt << 16) | (from << 22);
                o++;
            }
        }
    }
    return tot;
}
// Pass 1 counts 17 symbols only -- (r << 4) | 1 for the sixteen runs and ZRL; the EOB runs are k_ac_runs' -- so the wave's histogram is 17 words a copy, not 256
// (CSH_RH_WORDS: run r at word r, ZRL at word 16): 512 bytes a wave instead of 4 KB.  ref_hist_flush is hist_flush for that form: symbol (r << 4) | 1 is word 1 of
// lane 4 r, ZRL word 0 of lane 60; every other symbol of the slot's row is written as zero, as before
#define CSH_RH_WORDS 32
__device__ __forceinline__ static void ref_hist_flush(uint32_t *hist, uint16_t *row, LV<uint32_t> (&freq)[4]) {
    LFOR(l) {
        uint32_t zrl = 0, run = 0;
        CSH_UNROLL
        for (int cpy = 0; cpy < 4; cpy++) {
            uint32_t *h = hist + CSH_RH_WORDS * cpy;
            if ((l & 3) == 0) { run += h[l >> 2]; h[l >> 2] = 0u; }
            if (l == 60) { zrl += h[16]; h[16] = 0u; }
        }
        uint2 o; o.x = (zrl & 0xFFFFu) | (run << 16); o.y = 0u;
        *reinterpret_cast<uint2 *>(row + 4 * l) = o;
        freq[0][l] += zrl; freq[1][l] += run;
    }
}
// TOKENS = false (CSH_REF_PACK, the default): the kernel stops after pass 1 -- it also stores every block's last N (lastn[], indexed like corr[]), and
// k_list_refine_pack below derives the events again once the tables exist; no token, no reservation, no token region
template <bool TOKENS>
__global__ void __launch_bounds__(256, 6) k_list_refine(EncCtx c) {   // (six waves per SIMD asked for: <false> takes 65 VGPRs and holds seven, <true> 80 and six; 18 KB of LDS per workgroup
                                                                      // would allow eight -- an eighth for <false>, at 64 VGPRs, measured no gain)
    CSH_SHARED uint32_t s_hist[4][4][CSH_RH_WORDS];   // four copies, lane & 3 (k_list_stats); 17 words of each are used
    CSH_SHARED uint32_t s_lastn[4][256];     // per block: its last N, k << 6 | hex (0: no N)
    CSH_SHARED uint32_t s_nh[4][256];        // per block: its H entries
    CSH_SHARED uint32_t s_corr[4][256][2];   // per block: its correction word, high half first
    const int wv = int(uni(uint32_t(lwave())));   // (said to be wave-uniform: the run's records are then scalar loads into SGPRs, not a copy per lane in VGPRs)
    const uint32_t idx = blockIdx.x * 4u + uint32_t(wv);
    if (idx >= c.nref_runs) return;
    const uint32_t cs0 = c.ref_runs[idx];
    const SlotRec r = c.slots[cs0];
    if (c.work_active && !c.work_active[r.work]) return;
    const uint32_t nrun = run_chunks(c, r);
    const uint64_t lbase = c.nzlists[r.nzlist].base;
    ListSlot nx = list_chunk(c, lbase, r.nzrec);
    TokRegion rg;
    rg.base = 0; rg.cap = 0; rg.pad = 0;
    if (TOKENS) rg = c.regions[r.region];
    uint32_t *hist = &s_hist[wv][0][0], *lastn = s_lastn[wv], *nh = s_nh[wv], *corr = &s_corr[wv][0][0];
    LFOR(l) for (int i = l; i < 4 * CSH_RH_WORDS; i += 64) hist[i] = 0u;   // (a chunk's flush leaves it at zero for the next)
    const uint32_t Ss = r.Ss, Se = r.Se;
    LV<uint32_t> freq[4];   // the run's count of symbols 4 l .. 4 l + 3 (k_list_stats)
    LFOR(l) { freq[0][l] = 0u; freq[1][l] = 0u; freq[2][l] = 0u; freq[3][l] = 0u; }
    for (uint32_t ci = 0; ci < nrun; ci++) {
        // (the next chunk's record is asked for now; its entries are not -- pass 2 needs the registers they would wait in)
        const ListSlot ls = nx;
        if (ci + 1u < nrun) nx = list_chunk(c, lbase, r.nzrec + ci + 1u);
        const uint32_t cs = cs0 + ci, j = r.j + ci, unit0 = r.unit0 + 256u * ci, corr0 = r.corr0 + 256u * ci, hist_row = r.hist_row + ci * uint32_t(r.ntables);
        const uint32_t left = r.nunits_work - 256u * j, nun = left < 256u ? left : 256u;
        CSP_WAVE_SYNC();   // (pass 2 of the chunk before has read lastn and nh)
        LFOR(l) for (int i = l; i < 256; i += 64) { lastn[i] = 0u; nh[i] = 0u; corr[2 * i] = 0u; corr[2 * i + 1] = 0u; }
        CSP_WAVE_SYNC();
        // ---- pass 1
        RefCarry C;
        C.runH = C.runN = C.base = C.prevN = C.prevNZ = 0u;
        LV<uint32_t> ntok;
        LFOR(l) ntok[l] = 0u;
        {
        LV<uint32_t> x[4];   // the next step's entries, asked for a step ahead
        LFOR(l) list_load4(ls, 4u * uint32_t(l), x[0][l], x[1][l], x[2][l], x[3][l]);
        for (uint32_t g0 = 0; g0 < ls.n; g0 += 256) {
            LV<uint32_t> e[4], hex[4], z[4], zp[4], zq[4];
            LFOR(l) { e[0][l] = x[0][l]; e[1][l] = x[1][l]; e[2][l] = x[2][l]; e[3][l] = x[3][l]; }
            if (g0 + 256u < ls.n) LFOR(l) list_load4(ls, g0 + 256u + 4u * uint32_t(l), x[0][l], x[1][l], x[2][l], x[3][l]);
            ref_step<false>(e, Ss, Se, C, hex, z, zp, zq);
            LFOR(l) {
                uint32_t *h = hist + CSH_RH_WORDS * (l & 3);
                CSH_UNROLL
                for (int q = 0; q < 4; q++) {
                    const uint32_t v = e[q][l], blk = (v >> 23) & 255u;
                    if (ref_isH(v, Ss, Se)) {
                        atomicMax(&nh[blk], hex[q][l] + 1u);
                        if (v & 0x100u) atomicOr(&corr[2u * blk + (hex[q][l] >> 5)], 0x80000000u >> (hex[q][l] & 31u));
                    } else if (ref_isN(v, Ss, Se)) {
                        const uint32_t zr = z[q][l] - zp[q][l];
                        atomicMax(&lastn[blk], ((v & 127u) << 6) | hex[q][l]);
                        atomicAdd(&h[zr & 15u], 1u);            // symbol (zr & 15) << 4 | 1
                        if (zr >> 4) atomicAdd(&h[16], zr >> 4);   // ZRL
                        ntok[l] += 1u + (zr >> 4);
                    }
                }
            }
        }
        }
        CSP_WAVE_SYNC();
        // the blocks' ends: EOB tokens, tails, correction words, flags (lane = block bit, so the chunk's flags ARE four words of the scan's bit vectors)
        for (uint32_t w4 = 0; w4 < 4; w4++) {
            LFOR(l) {
                const uint32_t i = 64u * w4 + uint32_t(l);
                if (i < nun) {
                    const uint32_t ln = lastn[i];
                    if (ls.n && (ln >> 6) != Se) ntok[l] += 1u;   // (no entries: the list had no room, the run is repeated)
                    c.tail[unit0 + i] = uint8_t(nh[i] - (ln & 63u));   // the H entries behind the last N; all of them if there is no N
                    c.corr[corr0 + i] = (uint64_t(corr[2u * i]) << 32) | corr[2u * i + 1u];
                    if (!TOKENS) c.lastn[corr0 + i] = uint16_t(ln);   // k << 6 | hex, k <= 63: the block's H entries are tail + (lastn & 63)
                }
            }
            const uint64_t ms = lballot([&](int b) { const uint32_t i = 64u * w4 + uint32_t(b); return i < nun && lastn[i] != 0u; });
            const uint64_t me = lballot([&](int b) { const uint32_t i = 64u * w4 + uint32_t(b); return i < nun && (lastn[i] >> 6) != Se; });
            LFOR(l) if (l == 0 && j * 4u + w4 < ((r.nunits_work + 63u) >> 6)) { c.sym_bits[r.word_base + j * 4u + w4] = ms; c.eob_bits[r.word_base + j * 4u + w4] = me; }
        }
        const uint32_t total = lsum32(ntok);
        ref_hist_flush(hist, c.slot_hist + size_t(hist_row) * 256u, freq);
        LFOR(l) if (l == 0) c.slot_raw[cs] = C.runN + C.runH;   // a sign bit per new coefficient, a correction bit per old one
        if (c.stats_only || !TOKENS) continue;   // (nothing is written to the pool)
        // ---- room in the pool: one atomic add on the region's cursor
        uint32_t rel = 0;
        LFOR(l) if (l == 0) rel = atomicAdd(&c.tok_cursor[r.region], total);
        rel = uni(rel);
        const bool ok = uint64_t(rel) + total <= rg.cap;
        LFOR(l) {
            if (l < 4) { c.tok_off[cs * 4u + uint32_t(l)] = rg.base + rel; c.chunk_ntok[cs * 4u + uint32_t(l)] = (ok && l == 0) ? total : 0u; }
            if (l == 0 && !ok) c.overflow[1] = 1;
        }
        if (!ok) continue;
        uint32_t *tk = c.tokens + rg.base + rel;
        // (both passes derive the counts from the same entries, so pass 2 writes exactly `total` tokens: `o < total` below cannot fail -- it is there so that a
        // disagreement could never store outside the reserved room; the emulation build stops on one instead of dropping tokens)
        // ---- pass 2: the tokens
        C.runH = C.runN = C.base = C.prevN = C.prevNZ = 0u;
        uint32_t curc = 0, at = 0;
        for (uint32_t g0 = 0; g0 < ls.n; g0 += 256) {
            LV<uint32_t> e[4], hex[4], z[4], zp[4], zq[4];
            LFOR(l) list_load4(ls, g0 + 4u * uint32_t(l), e[0][l], e[1][l], e[2][l], e[3][l]);
            ref_step<true>(e, Ss, Se, C, hex, z, zp, zq);
            at += ref_step_tokens(e, hex, z, zp, zq, Ss, Se, lastn, nh, curc, tk, at, total);
        }
#ifdef CSH_EMUL
        if (at != total) { fprintf(stderr, "k_list_refine: pass 2 made %u tokens, pass 1 counted %u\n", at, total); abort(); }
#endif
    }
    freq_flush(c.tables[r.table_base].freq, freq);
}

// ---- pack of the refinement scans, from the lists (CSH_REF_PACK): ONE WAVE per run of (scan, chunk) slots, k_list_pack's shape -- the run's table staged once,
// position, window and code table carried across the chunk edges inside the run, only the run's first and last word ORed into the pool, the byte fill behind
// the scan's last chunk.  Per chunk the blocks' EOBRUN values, correction words, last N (k_list_refine<false> stored it) and H counts (tail + hex of the last N)
// go into LDS; then every step of 256 entries is pass 2 of k_list_refine<true> over again -- ref_step<true> and ref_step_tokens, the same statements -- only
// that the token words go into an LDS buffer of the wave, in list order, and are turned into bits at once, 64 tokens a sub-step, one per lane, through
// token_main<2> / token_pieces<2> (tok_bits.h: the one statement of what a token emits, k_pack's too).  Most entries of a refinement scan emit nothing (an H
// entry's correction bit rides behind the block's next token): the tokens are the dense form of the step, and the bit work is done on them, not per entry.
// Tokens of a step.  Per block: one per N entry, at most 3 ZRLs (z <= 62), one EOB -- at most N + 4 for at least N + 1 entries (its END), and N + 4 > N + 1
// needs an N: at least 2 entries.  So a block inside the step has at most 2.5 tokens per entry, the two blocks cut by the step's edges at most 3 + 1 more
// than their entries: 256 x 2.5 + 8 = 648 tokens at most (CSH_RP_STEP_TOKENS).  The buffer holds a ROUND of 256 of them: a step with more -- ZRLs must outnumber
// its H entries for that, which pictures seldom do -- is derived again, from the carries it started with and its entries out of the L2, once per further round,
// and ref_step_tokens keeps the round's tokens only (its `at` is minus the round's first token: the others fall outside `limit`).  At most three rounds a step.
// Bits of a sub-step.  A token emits a symbol of at most 16 bits and a sign bit or at most 14 run bits, then at most 63 correction bits: 30 + 63 = 93 bits --
// 3 ZRLs, a symbol, a sign bit and 63 correction bits of one entry are 4 of these tokens.  A sub-step is 64 tokens, one per lane: 64 x 93 = 5 952 bits = 186
// words.  (Small on purpose: the kernel waits on its chain of wave scans, so what counts is how many waves a SIMD holds, and LDS decides that -- 5.4 KB a wave
// with the 32-code table of tok_bits.h and the round of 256 tokens, 21.5 KB a workgroup, seven workgroups per CU.)
#define CSH_RP_STEP_TOKENS 648   // a step of 256 entries makes at most this many tokens (see above)
#define CSH_RP_TOKENS 256   // the wave's token buffer, in LDS words: one round of a step's tokens
#define CSH_RP_SUB 64       // tokens per sub-step
#define CSH_RP_WORDS 256    // the window of the bit stream, per wave, in LDS words (a sub-step of 64 tokens adds at most 186, see above)
#define CSH_RP_STEP 192     // slide when fewer words than this are left behind the complete ones: 1 partial word + 186 + the word lor_bits may touch behind its own
__global__ void __launch_bounds__(256, 7) k_list_refine_pack(EncCtx c) {   // (seven waves per SIMD: what its 21.5 KB of LDS per workgroup allow)
    CSH_SHARED alignas(16) uint32_t s_win[4][CSH_RP_WORDS];
    CSH_SHARED uint32_t s_lut[4][CSH_REF_CODES];
    CSH_SHARED uint64_t s_corr[4][256];
    CSH_SHARED uint16_t s_eob[4][256];
    CSH_SHARED uint16_t s_lastn[4][256];   // per block: its last N, k << 6 | hex (0: no N)
    CSH_SHARED uint8_t s_nh[4][256];       // per block: its H entries
    CSH_SHARED uint32_t s_tok[4][CSH_RP_TOKENS];
    const int wv = int(uni(uint32_t(lwave())));   // (said to be wave-uniform: the run's records are then scalar loads into SGPRs, not a copy per lane in VGPRs)
    const uint32_t idx = blockIdx.x * 4u + uint32_t(wv);
    if (idx >= c.nref_runs) return;
    const uint32_t cs0 = c.ref_runs[idx];
    const SlotRec r = c.slots[cs0];
    if (c.work_active && !c.work_active[r.work]) return;
    const ScanWork &w = c.work[r.work];
    if (w.no_room) { LFOR(l) if (l == 0) c.status[w.image] = 20200; return; }   // decided per scan by k_scan_place
    const uint32_t nrun = run_chunks(c, r);
    const uint64_t lbase = c.nzlists[r.nzlist].base;
    ListSlot nx = list_chunk(c, lbase, r.nzrec);
    // the run's place: from bit raw_bit0 of the raw pool on; the scan's last chunk (the last of its run) also carries the 1-bits that fill the last byte
    const uint64_t scan0 = c.chunk_off[r.first_chunk];
    const uint64_t raw_bit0 = w.raw_off * 8 + (c.chunk_off[cs0] - scan0);
    uint32_t pad = 0;
    if (r.j + nrun == r.nch) { const uint64_t total = c.chunk_off[r.first_chunk + r.nch] - scan0; pad = uint32_t((8 - (total & 7)) & 7); }
    uint32_t *buf = s_win[wv], *lut = s_lut[wv];
    uint64_t *corr = s_corr[wv];
    uint16_t *eobrun = s_eob[wv], *lastn = s_lastn[wv];
    uint8_t *nh = s_nh[wv];
    uint32_t *tok = s_tok[wv];
    LFOR(l) {
        if (l < CSH_REF_CODES) lut[l] = c.tables[r.table_base].lut[((uint32_t(l) & 15u) << 4) | (uint32_t(l) >> 4)];   // the symbol whose ref_code_index is l
        uint4 zero; zero.x = zero.y = zero.z = zero.w = 0u;
        for (int i = 4 * l; i < CSH_RP_WORDS; i += 256) *reinterpret_cast<uint4 *>(buf + i) = zero;
    }
    CSP_WAVE_SYNC();
    TokenCtx x;   // the chunk's, out of LDS
    x.lut = lut; x.lut_stride = CSH_REF_CODES; x.eobrun = eobrun; x.corr = corr;   // (the 32-code table: token_main / token_pieces <2, true>)
    uint32_t *out = c.raw + (raw_bit0 >> 5);        // word 0 of the frame below
    uint64_t pos = raw_bit0 & 31u;                   // next bit, in the frame whose word 0 is the run's first word in the pool
    uint32_t ww = 0;                                 // first word of the window
    bool first_flush = true;
    const uint32_t Ss = r.Ss, Se = r.Se;
    for (uint32_t ci = 0; ci < nrun; ci++) {
        const ListSlot ls = nx;
        const bool more = ci + 1u < nrun;
        if (more) nx = list_chunk(c, lbase, r.nzrec + ci + 1u);
#ifdef CSH_EMUL
        {   // (where a pool had no room the pass is repeated and its sizes are not of these lists: even then a run never gets ahead of its sized place -- DESIGN 4.1)
            const uint64_t want = (raw_bit0 & 31u) + (c.chunk_off[cs0 + ci] - c.chunk_off[cs0]);
            if (c.overflow[1] ? pos > want : pos != want) { fprintf(stderr, "k_list_refine_pack: chunk %u of a run does not start where the one before it ended\n", ci); abort(); }
        }
#endif
        CSP_WAVE_SYNC();   // (the steps of the chunk before have read what was staged for it)
        {
            const uint32_t u0 = r.unit0 + 256u * ci, corr0 = r.corr0 + 256u * ci, left = r.nunits_work - 256u * (r.j + ci), nun = left < 256u ? left : 256u;
            LFOR(l) for (int i = l; i < 256; i += 64) {
                const bool in = uint32_t(i) < nun;
                const uint32_t ln = in ? uint32_t(c.lastn[corr0 + uint32_t(i)]) : 0u;
                eobrun[i] = in ? c.eobrun[u0 + uint32_t(i)] : uint16_t(0);
                corr[i] = in ? c.corr[corr0 + uint32_t(i)] : uint64_t(0);
                lastn[i] = uint16_t(ln);
                nh[i] = in ? uint8_t(uint32_t(c.tail[u0 + uint32_t(i)]) + (ln & 63u)) : uint8_t(0);
            }
        }
        CSP_WAVE_SYNC();
        LV<uint32_t> xn[4];   // the next step's entries, asked for a step ahead
        LFOR(l) list_load4(ls, 4u * uint32_t(l), xn[0][l], xn[1][l], xn[2][l], xn[3][l]);
        RefCarry C;
        C.runH = C.runN = C.base = C.prevN = C.prevNZ = 0u;
        uint32_t curc = 0;
        for (uint32_t g0 = 0; g0 < ls.n; g0 += 256) {
            const RefCarry C0 = C;   // what the step starts with: a further round derives it again from here
            const uint32_t curc0 = curc;
            for (uint32_t t0 = 0;; t0 += CSH_RP_TOKENS) {   // the rounds: tokens t0 .. t0 + CSH_RP_TOKENS - 1 of the step (one round, but for a step of many ZRLs)
            uint32_t ntok;
            {
                LV<uint32_t> e[4], hex[4], z[4], zp[4], zq[4];
                if (t0 == 0u) {
                    LFOR(l) { e[0][l] = xn[0][l]; e[1][l] = xn[1][l]; e[2][l] = xn[2][l]; e[3][l] = xn[3][l]; }
                    if (g0 + 256u < ls.n) LFOR(l) list_load4(ls, g0 + 256u + 4u * uint32_t(l), xn[0][l], xn[1][l], xn[2][l], xn[3][l]);
                } else {
                    C = C0; curc = curc0;
                    LFOR(l) list_load4(ls, g0 + 4u * uint32_t(l), e[0][l], e[1][l], e[2][l], e[3][l]);
                }
                ref_step<true>(e, Ss, Se, C, hex, z, zp, zq);
                ntok = ref_step_tokens(e, hex, z, zp, zq, Ss, Se, lastn, nh, curc, tok, 0u - t0, uint32_t(CSH_RP_TOKENS));
            }
#ifdef CSH_EMUL
            if (ntok > CSH_RP_STEP_TOKENS) { fprintf(stderr, "k_list_refine_pack: a step of %u tokens\n", ntok); abort(); }
#endif
            CSP_WAVE_SYNC();
            // the round's tokens, 64 at a time, one per lane: the one-piece form first, the three pieces for the whole sub-step where a lane needs them
            const uint32_t nround = ntok - t0 < uint32_t(CSH_RP_TOKENS) ? ntok - t0 : uint32_t(CSH_RP_TOKENS);
            for (uint32_t s0 = 0; s0 < nround; s0 += CSH_RP_SUB) {
                LV<uint32_t> t, pv[3], pn[3], slow, len;
                LFOR(l) {
                    const uint32_t i = s0 + uint32_t(l);
                    t[l] = i < nround ? tok[i] : uint32_t(TK_RAW);   // (an empty RAW token emits nothing)
                    uint32_t v, n;
                    slow[l] = token_main<2, true>(t[l], x, v, n) ? 0u : 1u;
                    pv[0][l] = v; pn[0][l] = n; pv[1][l] = 0u; pn[1][l] = 0u; pv[2][l] = 0u; pn[2][l] = 0u;
                }
                if (lballot([&](int b) { return slow[b] != 0u; })) {
                    LFOR(l) {
                        const Pieces p = token_pieces<2, true>(t[l], x);
                        CSH_UNROLL
                        for (int k = 0; k < 3; k++) { pv[k][l] = p.v[k]; pn[k][l] = p.n[k]; }
                    }
                }
                LFOR(l) len[l] = pn[0][l] + pn[1][l] + pn[2][l];
                uint32_t tot;
                const LV<uint32_t> ex = lscan(len, tot);
                LFOR(l) {
                    uint64_t at = pos + ex[l] - uint64_t(ww) * 32u;    // bit position inside the window
                    CSH_UNROLL
                    for (int k = 0; k < 3; k++) if (pn[k][l]) { lor_bits(buf, at, pv[k][l], pn[k][l]); at += pn[k][l]; }
                }
                pos += tot;
                // slide the window when another sub-step's worth of bits might not fit any more
                const uint32_t done = uint32_t(pos >> 5) - ww;   // complete words in the window
                if (done > CSH_RP_WORDS - CSH_RP_STEP) {
                    CSP_WAVE_SYNC();
                    LFOR(l) for (uint32_t q = uint32_t(l); q < done; q += 64) {
                        const uint32_t v = buf[q];
                        if (first_flush && q == 0) { if (v) atomicOr(out + ww, v); } else out[ww + q] = v;
                    }
                    const uint32_t partial = buf[done];
                    CSP_WAVE_SYNC();
                    LFOR(l) for (int q = l; q < CSH_RP_WORDS; q += 64) buf[q] = (q == 0) ? partial : 0u;
                    CSP_WAVE_SYNC();
                    ww += done; first_flush = false;
                }
            }
            CSP_WAVE_SYNC();   // (the next round or step writes its tokens over these)
            if (t0 + uint32_t(CSH_RP_TOKENS) >= ntok) break;
            }
        }
    }
    // the byte fill of the scan's last chunk, behind the run's last token (the window has room for a sub-step, and the window is zero behind `pos`)
    if (pad) { LFOR(l) if (l == 0) lor_bits(buf, pos - uint64_t(ww) * 32u, (1u << pad) - 1u, pad); pos += pad; }
#ifdef CSH_EMUL
    {
        const uint64_t want = (raw_bit0 & 31u) + (c.chunk_off[cs0 + nrun] - c.chunk_off[cs0]) + pad;
        if (c.overflow[1] ? pos > want : pos != want) { fprintf(stderr, "k_list_refine_pack: a run does not end where its sizes say\n"); abort(); }
    }
#endif
    CSP_WAVE_SYNC();
    const uint32_t last = uint32_t((pos + 31) >> 5) - ww;   // words in the window that carry bits
    LFOR(l) for (uint32_t q = uint32_t(l); q < last; q += 64) {
        const uint32_t v = buf[q];
        if ((first_flush && q == 0) || q == last - 1) { if (v) atomicOr(out + ww + q, v); } else out[ww + q] = v;
    }
}

__global__ void k_reset_works(ScanWork *work, int nwork) {
    const int j = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= nwork) return;
    work[j].out_off = 0xFFFFFFFFu; work[j].raw_bytes = 0; work[j].hdr_bytes = 0; work[j].ff_bytes = 0; work[j].no_room = 0;
}

void launch_nzlist(hipStream_t st, const EncCtx &c) {
    if (!c.nnzchunks) return;
    if (c.nz_build) CSH_LAUNCH_PHASED(k_nzlist, 3, dim3(c.nnzchunks), dim3(2 * CSP_WAVE_THREADS), st, c);
    if (c.nz_filter) CSH_LAUNCH(k_nzfilter, dim3(c.nnzchunks), dim3(CSP_WAVE_THREADS), st, c);
}
// one wave per list run, four runs per workgroup
void launch_list_stats(hipStream_t st, const EncCtx &c) { if (c.nlist_runs) CSH_LAUNCH(k_list_stats, dim3((c.nlist_runs + 3) / 4), dim3(4 * CSP_WAVE_THREADS), st, c); }
void launch_list_refine(hipStream_t st, const EncCtx &c) {
    if (!c.nref_runs) return;
    if (c.ref_pack) CSH_LAUNCH(k_list_refine<false>, dim3((c.nref_runs + 3) / 4), dim3(4 * CSP_WAVE_THREADS), st, c);
    else CSH_LAUNCH(k_list_refine<true>, dim3((c.nref_runs + 3) / 4), dim3(4 * CSP_WAVE_THREADS), st, c);
}
void launch_list_refine_pack(hipStream_t st, const EncCtx &c) { if (c.nref_runs && c.ref_pack) CSH_LAUNCH(k_list_refine_pack, dim3((c.nref_runs + 3) / 4), dim3(4 * CSP_WAVE_THREADS), st, c); }
void launch_list_pack(hipStream_t st, const EncCtx &c) { if (c.nlist_runs) CSH_LAUNCH(k_list_pack, dim3((c.nlist_runs + 3) / 4), dim3(4 * CSP_WAVE_THREADS), st, c); }
// ---- the slots of the work items: one workgroup per work item, one lane per 256-unit chunk.  Under the scan search a 1080p image has ~3.9 k slots in 58 work
// items: built on the host they were 64 MB of records per 256 files to write and to upload in front of the first kernel (the boundary call paid ~15 ms of
// every 50 for them); the host only counts them now (batch_plan.cpp add_works).  Slots between the stages belong to no work item and stay zero.
__global__ void __launch_bounds__(64) k_make_slots(const ScanWork *works, uint32_t nworks, const EncScan *script, const NzList *nzlists, SlotRec *slots, uint32_t *slot_work, uint32_t *list_slots,
                                                   uint32_t *tok_slots, uint32_t *ref_slots, uint32_t *list_runs, uint32_t *ref_runs, uint32_t list_run) {
    const uint32_t wi = blockIdx.x;
    if (wi >= nworks) return;
    const ScanWork &w = works[wi];
    const EncScan &e = script[w.scan];
    const uint32_t nch = (w.nunits + 255u) / 256u;
    const bool prog_ac = e.Ss > 0 && !e.sequential, has_list = w.list != 0xFFFFFFFFu;
    const bool ref_list = has_list && prog_ac && e.Ah;   // a refinement scan coded from its list: k_list_refine, then k_list_refine_pack or (CSH_REF_PACK=0) k_pack over its tokens
    const bool listed = has_list && !ref_list;
    for (uint32_t j = threadIdx.x; j < nch; j += blockDim.x) {
        SlotRec r;
        r.work = wi; r.j = j; r.nch = nch; r.first_chunk = w.first_chunk; r.unit0 = w.unit_base + 256u * j;
        r.nun = w.nunits - 256u * j < 256u ? w.nunits - 256u * j : 256u; r.table_base = w.table_base; r.ntables = uint16_t(e.ntables);
        r.flags = uint16_t((prog_ac ? 1 : 0) | (prog_ac && e.Ah ? 2 : 0) | (listed ? 4 : 0) | (ref_list ? 8 : 0));
        r.hist_row = w.hist_row0 + j * uint32_t(e.ntables);
        r.word_base = w.word_base; r.unit_base = w.unit_base; r.nunits_work = w.nunits;
        r.Ss = uint8_t(e.Ss); r.Se = uint8_t(e.Se); r.Ah = uint8_t(e.Ah); r.Al = uint8_t(e.Al); r.corr0 = w.corr_base == 0xFFFFFFFFu ? 0u : w.corr_base + 256u * j;
        r.nzlist = has_list ? w.list : 0u; r.nzrec = has_list ? nzlists[w.list].chunk0 + j : 0u; r.region = ref_list ? w.region : 0u;
        slots[w.first_chunk + j] = r;
        slot_work[w.first_chunk + j] = wi;
        if (w.ls_base != 0xFFFFFFFFu) (listed ? list_slots : tok_slots)[w.ls_base + j] = w.first_chunk + j;   // (none: a refinement scan packed from its list)
        if (ref_list) ref_slots[w.rs_base + j] = w.first_chunk + j;
        // the list runs (k_list_stats, k_list_pack / k_list_refine): the first slot of every run of list_run chunks; the last run of a work item is as long as what is left
        if (listed && j % list_run == 0u) list_runs[w.lr_base + j / list_run] = w.first_chunk + j;
        if (ref_list && j % list_run == 0u) ref_runs[w.rr_base + j / list_run] = w.first_chunk + j;
    }
}
// the scan search re-points work items to the lists of the point transform it chose (scan_search.cpp search_decide): their slots follow
__global__ void __launch_bounds__(64) k_rebind_slots(const ScanWork *works, uint32_t nworks, const NzList *nzlists, SlotRec *slots) {
    const uint32_t wi = blockIdx.x;
    if (wi >= nworks) return;
    const ScanWork &w = works[wi];
    if (w.list == 0xFFFFFFFFu) return;
    const uint32_t nch = (w.nunits + 255u) / 256u, chunk0 = nzlists[w.list].chunk0;
    for (uint32_t j = threadIdx.x; j < nch; j += blockDim.x) { slots[w.first_chunk + j].nzlist = w.list; slots[w.first_chunk + j].nzrec = chunk0 + j; }
}
void launch_rebind_slots(hipStream_t st, const ScanWork *works, uint32_t nworks, const NzList *nzlists, SlotRec *slots) {
    if (nworks) CSH_LAUNCH(k_rebind_slots, dim3(nworks), dim3(64), st, works, nworks, nzlists, slots);
}
void launch_make_slots(hipStream_t st, const ScanWork *works, uint32_t nworks, const EncScan *script, const NzList *nzlists, SlotRec *slots, uint32_t *slot_work, uint32_t *list_slots,
                       uint32_t *tok_slots, uint32_t *ref_slots, uint32_t *list_runs, uint32_t *ref_runs, uint32_t list_run) {
    if (!nworks) return;
    CSH_LAUNCH(k_make_slots, dim3(nworks), dim3(64), st, works, nworks, script, nzlists, slots, slot_work, list_slots, tok_slots, ref_slots, list_runs, ref_runs, list_run);
}

void launch_reset_works(hipStream_t st, ScanWork *work, int nwork) { if (nwork) CSH_LAUNCH(k_reset_works, dim3((nwork + 255) / 256), dim3(256), st, work, nwork); }

}  // namespace csh
