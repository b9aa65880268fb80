// k_gif_lzw.hip -- GIF's one codec, both ways.
//
// Decode: one wave per input frame.  A code's width depends only on how many codes were read since the last clear code, so the bit position of the next 64
// codes is known before any of them is decoded: every lane reads one, a ballot finds the first clear / end / impossible code among them, and the codes in front
// of it are taken together.  Code j behind a clear code defines table entry clear + 1 + j with the code before it as its prefix; an entry's length and first
// byte come from its prefix, which may be an entry of the same step -- those chains are resolved by pointer jumping over the lanes (six rounds at most, none for
// a step whose prefixes are all older).  The strings' places in the output are an exclusive scan of their lengths; every lane writes its string back to front
// along the prefix chain.  The table (prefix, length, first and last byte of 4096 entries: 24 KB) lives in LDS.
//
// Encode: one wave per chunk of CSH_GIF_CHUNK pixels of an output frame.  A chunk is greedy LZW from an empty table and closes with the clear code the next
// chunk starts from (the last chunk: with the end code), so chunks do not depend on one another.  The dictionary is an open-addressed hash table of 8192 words
// in LDS; the wave probes 64 consecutive slots with one read and two ballots.  k_gif_layout scans the chunks' bit lengths and places the frames in their files,
// k_gif_merge shifts the chunks' bits together into 255-byte sub-blocks, k_gif_frame_head writes what stands around them.
// Under CSH_GIF=lossy (a distance D > 0) k_gif_near lists every table colour's neighbours within D and k_gif_lzw_encode_lossy codes the chunks instead: the
// match goes on with a neighbour of the next pixel's colour when the dictionary holds one.
#include "gif_kernels.h"
#include "wave.h"

namespace csg {

using csh::LV;
using csh::lballot;
using csh::lget;
using csh::lprev;
using csh::lscan;

// x[idx[l] & 63] into lane l
__device__ __forceinline__ static LV<uint32_t> lgather(const LV<uint32_t> &x, const LV<uint32_t> &idx) {
    LV<uint32_t> r;
#ifdef CSH_EMUL
    for (int j = 0; j < 64; j++) r.v[j] = x.v[idx.v[j] & 63u];
#else
    r.v = uint32_t(__shfl(int(x.v), int(idx.v & 63u), 64));
#endif
    return r;
}

// width of code j behind a clear code (j = 0: the first): the reader has clear + 1 + max(j, 1) codes when it reads it, and the width is the bit length of that count, 12 at most
__device__ __forceinline__ static uint32_t lzw_width(uint32_t j, uint32_t clear) {
    const uint32_t w = 32u - uint32_t(__clz(clear + 1u + (j ? j : 1u)));
    return w > 12u ? 12u : w;
}
// bits of the codes 0 .. i - 1 behind a clear code
__device__ __forceinline__ static uint64_t lzw_off(uint32_t i, uint32_t clear) {
    uint64_t bits = 0;
    for (uint32_t w = 3; w <= 12; w++) {   // codes of width w: clear + 1 + j in [2^(w-1), 2^w), open above at 12
        const int64_t lo = int64_t(1u << (w - 1)) - int64_t(clear) - 1, hi = w == 12 ? int64_t(i) : int64_t(1u << w) - int64_t(clear) - 1;
        const int64_t a = lo > 0 ? lo : 0, b = hi < int64_t(i) ? hi : int64_t(i);
        if (b > a) bits += uint64_t(b - a) * w;
    }
    return bits;
}

// row r of the data of an interlaced picture of h rows is row ... of the picture
__device__ __forceinline__ static uint32_t gif_deinterlace(uint32_t r, uint32_t h) {
    const uint32_t n1 = (h + 7) / 8, n2 = (h + 3) / 8, n3 = (h + 1) / 4;
    if (r < n1) return 8 * r;
    if (r < n1 + n2) return 8 * (r - n1) + 4;
    if (r < n1 + n2 + n3) return 4 * (r - n1 - n2) + 2;
    return 2 * (r - n1 - n2 - n3) + 1;
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_lzw_decode(const GifFrame *frames, const uint8_t *data, uint8_t *indices, uint32_t *status) {
    CSH_SHARED uint16_t s_prefix[4096];
    CSH_SHARED uint16_t s_len[4096];
    CSH_SHARED uint8_t s_first[4096];
    CSH_SHARED uint8_t s_last[4096];
    const GifFrame f = frames[blockIdx.x];
    const uint8_t *d = data + f.data_off;   // (the pool is padded: three bytes at any bit of the stream can be read)
    uint8_t *o = indices + f.idx_off;
    const uint32_t clear = 1u << f.mcs, npx = f.w * f.h;
    const bool interlaced = (f.flags & GIF_INTERLACED) != 0;
    LFOR(l) for (uint32_t c = uint32_t(l); c < clear; c += 64u) { s_prefix[c] = 0; s_len[c] = 1; s_first[c] = uint8_t(c); s_last[c] = uint8_t(c); }
    CSP_WAVE_SYNC();
    const uint64_t total_bits = uint64_t(f.data_len) * 8u;
    uint64_t bitpos = 0;
    uint32_t since = 0, prev = 0, out = 0, st = GIF_OK;   // since: codes read behind the last clear code (a stream need not start with one)
    while (out < npx) {
        const uint64_t off0 = lzw_off(since, clear);
        LV<uint32_t> c, wid;
        LFOR(l) {
            const uint32_t j = since + uint32_t(l), w = lzw_width(j, clear);
            const uint64_t p = bitpos + (lzw_off(j, clear) - off0);
            wid[l] = w;
            if (p + w > total_bits) c[l] = 0xFFFFu;   // the data ends here
            else { const uint8_t *q = d + (p >> 3); c[l] = ((uint32_t(q[0]) | (uint32_t(q[1]) << 8) | (uint32_t(q[2]) << 16)) >> uint32_t(p & 7u)) & ((1u << w) - 1u); }
        }
        const LV<uint32_t> pc = lprev(c, prev);
        // code j defines entry E = clear + 1 + j (from the second code on, while the table has room) and may be that entry itself (KwKwK), nothing beyond it
        const uint64_t stop = lballot([&](int l) { return c[l] == clear || c[l] == clear + 1u || c[l] == 0xFFFFu; });
        const uint64_t bad = lballot([&](int l) {
            const uint32_t j = since + uint32_t(l), E = clear + 1u + j;
            return c[l] != 0xFFFFu && (j == 0 ? c[l] > clear + 1u : (E < 4096u && c[l] > E));
        });
        const uint64_t ev = stop | bad;
        const uint32_t n = ev ? uint32_t(__ffsll((unsigned long long)ev)) - 1u : 64u;
        LV<uint32_t> dep, acc, fst;
        LFOR(l) {
            const uint32_t j = since + uint32_t(l), E = clear + 1u + j;
            const bool adds = uint32_t(l) < n && j >= 1u && E < 4096u;
            const int32_t m = int32_t(pc[l]) - int32_t(clear + 1u + since);   // the lane that defines the prefix, if one of this step does
            const bool inb = adds && m >= 0;
            dep[l] = inb ? uint32_t(m) : 64u;
            acc[l] = 1u + ((adds && !inb) ? uint32_t(s_len[pc[l]]) : 0u);
            fst[l] = (adds && !inb) ? uint32_t(s_first[pc[l]]) : 0u;
        }
        for (int r = 0; r < 6; r++) {
            if (!lballot([&](int l) { return dep[l] < 64u; })) break;
            const LV<uint32_t> da = lgather(acc, dep), df = lgather(fst, dep), dd = lgather(dep, dep);
            LFOR(l) if (dep[l] < 64u) { acc[l] += da[l]; fst[l] = df[l]; dep[l] = dd[l]; }
        }
        LFOR(l) {
            const uint32_t j = since + uint32_t(l), E = clear + 1u + j;
            if (uint32_t(l) < n && j >= 1u && E < 4096u) { s_prefix[E] = uint16_t(pc[l]); s_len[E] = uint16_t(acc[l]); s_first[E] = uint8_t(fst[l]); }
        }
        CSP_WAVE_SYNC();
        LFOR(l) {   // the entry's last byte is the first byte of the code that defines it
            const uint32_t j = since + uint32_t(l), E = clear + 1u + j;
            if (uint32_t(l) < n && j >= 1u && E < 4096u) s_last[E] = s_first[c[l]];
        }
        CSP_WAVE_SYNC();
        LV<uint32_t> slen;
        LFOR(l) slen[l] = uint32_t(l) < n ? uint32_t(s_len[c[l]]) : 0u;
        uint32_t total;
        const LV<uint32_t> pos = lscan(slen, total);
        LFOR(l) {
            uint32_t code = c[l], p = out + pos[l] + slen[l];
            for (uint32_t k = 0; k < slen[l]; k++) {   // surplus data is left unwritten
                p--;
                if (p < npx) {
                    const uint32_t row = p / f.w, x = p - row * f.w;
                    o[size_t(interlaced ? gif_deinterlace(row, f.h) : row) * f.w + x] = code >= clear ? s_last[code] : uint8_t(code);
                }
                if (code >= clear) code = s_prefix[code];
            }
        }
        out += total; since += n;
        if (n) prev = lget(c, n - 1u);
        bitpos += lzw_off(since, clear) - off0;
        if (n < 64u) {
            if ((bad >> n) & 1u) { st = GIF_BAD_CODE; break; }
            if (lget(c, n) != clear) break;   // the end code, or no data left
            bitpos += lget(wid, n); since = 0;
        }
    }
    if (st == GIF_OK && out < npx) st = GIF_SHORT;
    LFOR(l) if (l == 0) status[blockIdx.x] = st;
}

void launch_gif_lzw_decode(hipStream_t st, const GifFrame *frames, uint32_t nframes, const uint8_t *data, uint8_t *indices, uint32_t *status) {
    if (!nframes) return;
    CSH_LAUNCH(k_gif_lzw_decode, dim3(nframes), dim3(CSP_WAVE_THREADS), st, frames, data, indices, status);
}

// ------------------------------------------------------------------------------------------------ the coder
enum : uint32_t { ENC_SLOTS = 8192, ENC_EMPTY = 0xFFFFFFFFu };   // a slot: (prefix code << 8 | byte) << 12 | code

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_lzw_encode(const GifFrame *frames, const GifChunk *chunks, const uint8_t *pack, uint8_t *cbuf, uint32_t *cbits, uint32_t chunk_px) {
    CSH_SHARED uint32_t s_tab[ENC_SLOTS];
    const GifChunk ck = chunks[blockIdx.x];
    const GifFrame f = frames[ck.frame];
    const uint32_t npx = f.ow * f.oh, p0 = ck.index * chunk_px, n = npx - p0 < chunk_px ? npx - p0 : chunk_px;
    const uint8_t *px = pack + f.out_off + p0;
    uint32_t *dst = reinterpret_cast<uint32_t *>(cbuf + ck.buf_off);
    const uint32_t clear = 1u << f.omcs;
    uint32_t width = f.omcs + 1u, next = clear + 2u, nb = 0, words = 0;
    uint64_t acc = 0;
    auto emit = [&](uint32_t code) {
        acc |= uint64_t(code) << nb; nb += width;
        if (nb >= 32u) { LFOR(l) if (l == 0) dst[words] = uint32_t(acc); words++; acc >>= 32; nb -= 32u; }
    };
    auto wipe = [&]() {
        CSP_WAVE_SYNC();
        LFOR(l) for (uint32_t s = uint32_t(l); s < ENC_SLOTS; s += 64u) s_tab[s] = ENC_EMPTY;
        CSP_WAVE_SYNC();
    };
    // what follows every code: an entry while fewer than 4096 codes exist (the width follows the count), else a clear code and an empty table
    auto after_code = [&](uint32_t slot, uint32_t key, bool insert) {
        if (next < 4096u) {
            if (insert) { LFOR(l) if (l == 0) s_tab[slot] = (key << 12) | next; CSP_WAVE_SYNC(); }
            next++;
            if (next > (1u << width) && width < 12u) width++;
        } else { emit(clear); if (insert) wipe(); width = f.omcs + 1u; next = clear + 2u; }
    };
    wipe();
    if (ck.index == 0) emit(clear);
    uint32_t cur = 0;
    bool have = false;
    for (uint32_t base = 0; base < n; base += 64u) {
        LV<uint32_t> pv;
        LFOR(l) pv[l] = base + uint32_t(l) < n ? uint32_t(px[base + uint32_t(l)]) : 0u;
        const uint32_t cnt = n - base < 64u ? n - base : 64u;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t b = lget(pv, j);
            if (!have) { cur = b; have = true; continue; }
            const uint32_t key = (cur << 8) | b;
            uint32_t h = (key * 2654435761u) >> 19, slot = 0;
            bool found = false;
            for (;;) {   // 64 slots a step; the table is at most half full, so an empty slot ends the search
                LV<uint32_t> sv;
                LFOR(l) sv[l] = s_tab[(h + uint32_t(l)) & (ENC_SLOTS - 1u)];
                const uint64_t hit = lballot([&](int l) { return sv[l] != ENC_EMPTY && (sv[l] >> 12) == key; });
                if (hit) { cur = lget(sv, uint32_t(__ffsll((unsigned long long)hit)) - 1u) & 0xFFFu; found = true; break; }
                const uint64_t empty = lballot([&](int l) { return sv[l] == ENC_EMPTY; });
                if (empty) { slot = (h + uint32_t(__ffsll((unsigned long long)empty)) - 1u) & (ENC_SLOTS - 1u); break; }
                h += 64u;
            }
            if (found) continue;
            emit(cur);
            after_code(slot, key, true);
            cur = b;
        }
    }
    emit(cur);
    after_code(0, 0, false);
    emit(ck.index + 1u == f.nchunks ? clear + 1u : clear);
    const uint32_t bits = words * 32u + nb;
    LFOR(l) if (l == 0) { if (nb) dst[words] = uint32_t(acc); cbits[blockIdx.x] = bits; }
}

void launch_gif_lzw_encode(hipStream_t st, const GifFrame *frames, const GifChunk *chunks, uint32_t nchunks, const uint8_t *pack, uint8_t *cbuf, uint32_t *cbits, uint32_t chunk_px) {
    if (!nchunks) return;
    CSH_LAUNCH(k_gif_lzw_encode, dim3(nchunks), dim3(CSP_WAVE_THREADS), st, frames, chunks, pack, cbuf, cbits, chunk_px);
}

// ------------------------------------------------------------------------------------------------ the lossy coder (CSH_GIF=lossy, D > 0)
// A colour table's candidate rows.  One wave per (table, index b); lane l holds the entries c = l, 64 + l, 128 + l, 192 + l as keys distance^2 << 8 | c (26 bits:
// 3 * 255^2 < 2^18).  An entry that is b itself, stands at or behind the table's n, repeats a lower entry's colour or lies further than D from b has no key; a row
// whose b is such an entry holds b alone.  A key's place in the row is the number of smaller keys -- the keys carry the index, so no two are equal -- and the first
// 63 are kept behind b.  The rows were zeroed by the host.
enum : uint32_t { NEAR_NONE = 0xFFFFFFFFu };
__device__ __forceinline__ static uint32_t rgb_dist2(uint32_t a, uint32_t b) {
    const int32_t dr = int32_t(a & 255u) - int32_t(b & 255u), dg = int32_t((a >> 8) & 255u) - int32_t((b >> 8) & 255u), db = int32_t((a >> 16) & 255u) - int32_t((b >> 16) & 255u);
    return uint32_t(dr * dr + dg * dg + db * db);
}
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_near(const uint32_t *tables, const uint8_t *canon, const uint32_t *table_n, uint32_t dist, uint8_t *cand, uint8_t *count) {
    CSH_SHARED uint32_t s_key[256];
    const uint32_t t = blockIdx.x >> 8, b = blockIdx.x & 255u, n = table_n[t];
    const uint32_t *tb = tables + size_t(t) * 256u;
    const uint8_t *cn = canon + size_t(t) * 256u;
    uint8_t *row = cand + (size_t(t) * 256u + b) * GIF_NEAR_ROW;
    const bool listed = b < n && cn[b] == b;
    const uint32_t cb = tb[b], d2max = dist * dist;
    LV<uint32_t> key[4];
    LFOR(l) {
        CSH_UNROLL
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t c = q * 64u + uint32_t(l), d2 = rgb_dist2(tb[c], cb);
            key[q][l] = (listed && c != b && c < n && cn[c] == c && d2 <= d2max) ? ((d2 << 8) | c) : uint32_t(NEAR_NONE);
            s_key[c] = key[q][l];
        }
    }
    CSP_WAVE_SYNC();
    uint32_t total = 0;
    for (uint32_t q = 0; q < 4; q++) total += csh::popc64(lballot([&](int l) { return key[q][l] != NEAR_NONE; }));
    LFOR(l) {
        uint32_t rank[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < 256u; j++) {
            const uint32_t k = s_key[j];   // (no key is below a smaller one: NEAR_NONE is the largest word)
            CSH_UNROLL
            for (uint32_t q = 0; q < 4; q++) rank[q] += k < key[q][l] ? 1u : 0u;
        }
        CSH_UNROLL
        for (uint32_t q = 0; q < 4; q++) if (key[q][l] != NEAR_NONE && rank[q] < GIF_NEAR_ROW - 1u) row[1u + rank[q]] = uint8_t(key[q][l] & 255u);
        if (l == 0) { row[0] = uint8_t(b); count[size_t(t) * 256u + b] = uint8_t(1u + (total < GIF_NEAR_ROW - 1u ? total : GIF_NEAR_ROW - 1u)); }
    }
}
void launch_gif_near(hipStream_t st, const uint32_t *tables, const uint8_t *canon, const uint32_t *table_n, uint32_t ntables, uint32_t dist, uint8_t *cand, uint8_t *count) {
    for (uint32_t t0 = 0; t0 < ntables; t0 += 1u << 20) {   // (a grid's x stays below 2^31)
        const uint32_t nt = ntables - t0 < (1u << 20) ? ntables - t0 : (1u << 20);
        CSH_LAUNCH(k_gif_near, dim3(nt * 256u), dim3(CSP_WAVE_THREADS), st, tables + size_t(t0) * 256u, canon + size_t(t0) * 256u, table_n + t0, dist, cand + size_t(t0) * 256u * GIF_NEAR_ROW, count + size_t(t0) * 256u);
    }
}

// One wave per chunk, as k_gif_lzw_encode, over the same hash words; the wave's lanes take the candidates of the next pixel b instead of 64 neighbouring slots.
// Lane l looks (cur, cand(b)[l]) up along its own linear-probe chain -- the exact coder fills the first empty slot from the hash on, so a chain ends on the key or
// on an empty slot --, one ballot finds the first candidate the dictionary holds, and the match goes on with it: the decoder shows that colour, which lies within
// D of b's.  A candidate equal to the frame's transparent index is skipped, and a transparent b (or one behind the table) has no candidate but itself: alpha is
// never touched.  With no hit the code is sent and (cur, b), the exact pixel, goes where lane 0's chain ended.  The coder sends no more codes than the exact one
// would for the pixels it shows, so gif_chunk_cap bounds the chunk.  LDS: the table (32 KB) and the frame's rows (16 KB + 256 B): three workgroups a CU.
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_lzw_encode_lossy(const GifFrame *frames, const GifChunk *chunks, const uint8_t *pack, const uint8_t *cand, const uint8_t *count, uint8_t *cbuf, uint32_t *cbits,
                                                                            uint32_t chunk_px) {
    CSH_SHARED uint32_t s_tab[ENC_SLOTS];
    CSH_SHARED uint32_t s_rows[256u * GIF_NEAR_ROW / 4u];
    CSH_SHARED uint32_t s_count[256u / 4u];
    const GifChunk ck = chunks[blockIdx.x];
    const GifFrame f = frames[ck.frame];
    const uint32_t npx = f.ow * f.oh, p0 = ck.index * chunk_px, n = npx - p0 < chunk_px ? npx - p0 : chunk_px;
    const uint8_t *px = pack + f.out_off + p0;
    uint32_t *dst = reinterpret_cast<uint32_t *>(cbuf + ck.buf_off);
    const uint32_t clear = 1u << f.omcs;
    uint32_t width = f.omcs + 1u, next = clear + 2u, nb = 0, words = 0;
    uint64_t acc = 0;
    auto emit = [&](uint32_t code) {
        acc |= uint64_t(code) << nb; nb += width;
        if (nb >= 32u) { LFOR(l) if (l == 0) dst[words] = uint32_t(acc); words++; acc >>= 32; nb -= 32u; }
    };
    auto wipe = [&]() {
        CSP_WAVE_SYNC();
        LFOR(l) for (uint32_t s = uint32_t(l); s < ENC_SLOTS; s += 64u) s_tab[s] = ENC_EMPTY;
        CSP_WAVE_SYNC();
    };
    auto after_code = [&](uint32_t slot, uint32_t key, bool insert) {
        if (next < 4096u) {
            if (insert) { LFOR(l) if (l == 0) s_tab[slot] = (key << 12) | next; CSP_WAVE_SYNC(); }
            next++;
            if (next > (1u << width) && width < 12u) width++;
        } else { emit(clear); if (insert) wipe(); width = f.omcs + 1u; next = clear + 2u; }
    };
    {   // the rows of the frame's table (the pools are word-aligned: a table's rows are 16 KB, its counts 256 bytes)
        const uint32_t *gr = reinterpret_cast<const uint32_t *>(cand + size_t(f.pal) * 256u * GIF_NEAR_ROW), *gc = reinterpret_cast<const uint32_t *>(count + size_t(f.pal) * 256u);
        LFOR(l) {
            for (uint32_t i = uint32_t(l); i < 256u * GIF_NEAR_ROW / 4u; i += 64u) s_rows[i] = gr[i];
            s_count[l] = gc[l];
        }
    }
    const uint8_t *rows = reinterpret_cast<const uint8_t *>(s_rows), *counts = reinterpret_cast<const uint8_t *>(s_count);
    wipe();
    if (ck.index == 0) emit(clear);
    uint32_t cur = 0;
    bool have = false;
    for (uint32_t base = 0; base < n; base += 64u) {
        LV<uint32_t> pv;
        LFOR(l) pv[l] = base + uint32_t(l) < n ? uint32_t(px[base + uint32_t(l)]) : 0u;
        const uint32_t cnt = n - base < 64u ? n - base : 64u;
        for (uint32_t j = 0; j < cnt; j++) {
            const uint32_t b = lget(pv, j);
            if (!have) { cur = b; have = true; continue; }
            const uint32_t nc = b == f.transparent ? 1u : uint32_t(counts[b]);
            LV<uint32_t> found, slot;
            LFOR(l) {
                const uint32_t c = rows[b * GIF_NEAR_ROW + uint32_t(l)];
                found[l] = ENC_EMPTY; slot[l] = 0u;
                if (uint32_t(l) < nc && (l == 0 || c != f.transparent)) {
                    const uint32_t key = (cur << 8) | c;
                    uint32_t h = (key * 2654435761u) >> 19, sv;
                    for (;;) {   // the table is at most half full: an empty slot ends the chain
                        sv = s_tab[h & (ENC_SLOTS - 1u)];
                        if (sv == ENC_EMPTY || (sv >> 12) == key) break;
                        h++;
                    }
                    found[l] = sv; slot[l] = h & (ENC_SLOTS - 1u);
                }
            }
            const uint64_t hit = lballot([&](int l) { return found[l] != ENC_EMPTY; });
            if (hit) { cur = lget(found, uint32_t(__ffsll((unsigned long long)hit)) - 1u) & 0xFFFu; continue; }
            emit(cur);
            after_code(lget(slot, 0u), (cur << 8) | b, true);
            cur = b;
        }
    }
    emit(cur);
    after_code(0, 0, false);
    emit(ck.index + 1u == f.nchunks ? clear + 1u : clear);
    const uint32_t bits = words * 32u + nb;
    LFOR(l) if (l == 0) { if (nb) dst[words] = uint32_t(acc); cbits[blockIdx.x] = bits; }
}
void launch_gif_lzw_encode_lossy(hipStream_t st, const GifFrame *frames, const GifChunk *chunks, uint32_t nchunks, const uint8_t *pack, const uint8_t *cand, const uint8_t *count, uint8_t *cbuf,
                                 uint32_t *cbits, uint32_t chunk_px) {
    if (!nchunks) return;
    CSH_LAUNCH(k_gif_lzw_encode_lossy, dim3(nchunks), dim3(CSP_WAVE_THREADS), st, frames, chunks, pack, cand, count, cbuf, cbits, chunk_px);
}

// one lane per file: the chunks' bit offsets inside their frame, the frames' places inside their file, the file's size
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_layout(const GifFile *files, uint32_t nfiles, const GifFrame *frames, const uint32_t *cbits, uint64_t *cstart, GifPlace *place, uint64_t *file_bytes) {
    LFOR(l) {
        const uint32_t fi = blockIdx.x * 64u + uint32_t(l);
        if (fi < nfiles) {
            const GifFile F = files[fi];
            uint64_t pos = 0;
            for (uint32_t k = 0; k < F.nframes; k++) {
                const GifFrame &f = frames[F.first + k];
                uint64_t bits = 0;
                for (uint32_t c = 0; c < f.nchunks; c++) { cstart[f.first_chunk + c] = bits; bits += cbits[f.first_chunk + c]; }
                const uint64_t D = (bits + 7u) / 8u;
                place[F.first + k].pos = pos; place[F.first + k].data_bytes = D;
                pos += f.head_len + D + (D + 254u) / 255u + 1u;
            }
            file_bytes[fi] = pos + 1u;
        }
    }
}
void launch_gif_layout(hipStream_t st, const GifFile *files, uint32_t nfiles, const GifFrame *frames, const uint32_t *cbits, uint64_t *cstart, GifPlace *place, uint64_t *file_bytes) {
    if (!nfiles) return;
    CSH_LAUNCH(k_gif_layout, dim3((nfiles + 63u) / 64u), dim3(CSP_WAVE_THREADS), st, files, nfiles, frames, cbits, cstart, place, file_bytes);
}

// one wave per frame: the head bytes, the sub-blocks' length bytes, the block terminator, the file's trailer behind its last frame
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_frame_head(const GifFile *files, const GifFrame *frames, const uint32_t *frame_file, const uint8_t *heads, const GifPlace *place, uint8_t *out) {
    const uint32_t i = blockIdx.x;
    const GifFrame f = frames[i];
    const GifFile F = files[frame_file[i]];
    if (i >= F.first + F.nframes) return;   // a file that takes no part in the coding has no frames here
    const GifPlace pl = place[i];
    uint8_t *dst = out + F.out_off + pl.pos, *sub = dst + f.head_len;
    const uint64_t D = pl.data_bytes, nsub = (D + 254u) / 255u;
    LFOR(l) {
        for (uint32_t b = uint32_t(l); b < f.head_len; b += 64u) dst[b] = heads[f.head_off + b];
        for (uint64_t j = uint64_t(l); j < nsub; j += 64u) sub[j * 256u] = uint8_t(D - 255u * j < 255u ? D - 255u * j : 255u);
        if (l == 0) { sub[D + nsub] = 0; if (i + 1u == F.first + F.nframes) sub[D + nsub + 1u] = 0x3B; }
    }
}
void launch_gif_frame_head(hipStream_t st, const GifFile *files, const GifFrame *frames, const uint32_t *frame_file, uint32_t nframes, const uint8_t *heads, const GifPlace *place, uint8_t *out) {
    if (!nframes) return;
    CSH_LAUNCH(k_gif_frame_head, dim3(nframes), dim3(CSP_WAVE_THREADS), st, files, frames, frame_file, heads, place, out);
}

// eight bits of a chunk's stream from bit s on; bits past the chunk's length L read as 0
__device__ __forceinline__ static uint32_t chunk_bits8(const uint8_t *src, uint64_t s, uint64_t L) {
    if (s >= L) return 0u;
    const uint32_t w = uint32_t(src[s >> 3]) | (uint32_t(src[(s >> 3) + 1u]) << 8);
    uint32_t v = (w >> uint32_t(s & 7u)) & 0xFFu;
    if (L - s < 8u) v &= (1u << uint32_t(L - s)) - 1u;
    return v;
}
// one wave per chunk: the bytes of the frame's stream that begin inside the chunk (chunk 0: from byte 0), a lane a byte.  The last of them may end in the next
// chunk, whose first bits are fetched too.  No byte spans three chunks: a chunk that is not its frame's last holds CSH_GIF_CHUNK >= 1024 pixels, dozens of codes at the
// least; only the last chunk can be shorter than a byte (one pixel: a code and the end code, six bits at code size 2), and then it may own no byte at all --
// the chunk in front of it fetches all of it.
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_merge(const GifFile *files, const GifFrame *frames, const uint32_t *frame_file, const GifChunk *chunks, const uint8_t *cbuf, const uint32_t *cbits,
                                                                 const uint64_t *cstart, const GifPlace *place, uint8_t *out) {
    const uint32_t c = blockIdx.x;
    const GifChunk ck = chunks[c];
    const GifFrame &f = frames[ck.frame];
    const GifFile F = files[frame_file[ck.frame]];
    const uint64_t B = cstart[c], L = cbits[c], Bn = B + L;
    const bool has_next = ck.index + 1u < f.nchunks;
    const uint8_t *src = cbuf + ck.buf_off, *nsrc = has_next ? cbuf + chunks[c + 1u].buf_off : src;
    const uint64_t Ln = has_next ? cbits[c + 1u] : 0u;
    uint8_t *sub = out + F.out_off + place[ck.frame].pos + f.head_len;
    const uint64_t first = (B + 7u) / 8u, last = (Bn - 1u) / 8u;
    LFOR(l) {
        for (uint64_t d = first + uint64_t(l); d <= last; d += 64u) {
            uint32_t v = chunk_bits8(src, 8u * d - B, L);
            if (8u * d + 8u > Bn && has_next) v |= (chunk_bits8(nsrc, 0, Ln) << uint32_t(Bn - 8u * d)) & 0xFFu;
            sub[d + d / 255u + 1u] = uint8_t(v);
        }
    }
}
void launch_gif_merge(hipStream_t st, const GifFile *files, const GifFrame *frames, const uint32_t *frame_file, const GifChunk *chunks, uint32_t nchunks, const uint8_t *cbuf, const uint32_t *cbits,
                      const uint64_t *cstart, const GifPlace *place, uint8_t *out) {
    if (!nchunks) return;
    CSH_LAUNCH(k_gif_merge, dim3(nchunks), dim3(CSP_WAVE_THREADS), st, files, frames, frame_file, chunks, cbuf, cbits, cstart, place, out);
}

}  // namespace csg
