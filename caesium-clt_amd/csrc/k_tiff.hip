// k_tiff.hip -- TIFF's byte codecs, both ways, and the assembly of the output files.  A segment (one strip or one tile) is a byte-aligned stream of
// its own, so everything here is one wave per segment or per row, as in k_gif_lzw.hip.
//
// LZW decode (TIFF 6.0 section 13): k_gif_lzw_decode's scheme with TIFF's conventions -- codes are packed from the high bit down, Clear is 256, EOI 257, the first
// entry 258, and the width changes one code early: the code read while the table holds n entries is as wide as n + 1 is long, 12 bits at most.  The width depends
// only on how many codes were read since the last Clear, so the bit position of the next 64 codes is known before any is decoded: every lane reads one, a ballot
// finds the first Clear / EOI / impossible code, the codes in front of it are taken together; entries defined in the same step are resolved by pointer jumping over
// the lanes, the strings' places are an exclusive scan of their lengths.  LDS: the table (prefix, length, first and last byte of 4096 entries), 24 KB a wave: six
// workgroups a CU (160 KB).
// PackBits decode: the headers chain, so the wave walks them together (every lane reads the same header) and its lanes copy or fill the packet's bytes.
// Predictor 2: a wave a row.  The undo is a prefix sum with a stride of one pixel: windows of as many whole pixels as fit the 64 lanes are scanned by doubling
// (stride, 2 stride, ...) and take the last pixel of the window before as carry.  The forward direction is a subtraction per sample.
// LZW encode: one wave per (segment, predictor variant), greedy longest match from an empty table; k_gif_lzw_encode's dictionary -- an open-addressed hash table of
// 8192 words in LDS, probed 64 slots at a time.  32 KB a wave: five workgroups a CU.
// PackBits encode: a wave a row, lanes a byte: a byte belongs to a run of three or more equal bytes if it stands in three equal bytes, which it sees from its two
// neighbours either side; pieces (a run of >= 3, or everything between two such runs) start where that changes or a run's byte changes, packets every 128 bytes
// of a piece; a scan of what each byte contributes places the packets, and the lane at a packet's last byte writes its header.  The rows are sized first, a wave a segment
// scans the sizes into the rows' places, then the rows are written.
// k_tiff_layout places the segments, the value blocks and the IFDs in their files (a lane a file) and picks the predictor variant of every page;
// k_tiff_gather copies them there; k_tiff_patch writes the offsets that depend on the places.
#include "tiff_kernels.h"
#include "wave.h"

namespace cst {

using csh::LV;
using csh::lballot;
using csh::lget;
using csh::lprev;
using csh::lscan;
using csh::lsum32;

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
// lane l gets the value of lane l - d (d wave-uniform, 1..63), the lanes below d get 0
__device__ __forceinline__ static LV<uint32_t> lshift_up(const LV<uint32_t> &x, uint32_t d) {
    LV<uint32_t> r;
#ifdef CSH_EMUL
    for (int j = 0; j < 64; j++) r.v[j] = uint32_t(j) >= d ? x.v[uint32_t(j) - d] : 0u;
#else
    const uint32_t t = uint32_t(__shfl_up(int(x.v), d, 64));
    r.v = (threadIdx.x & 63u) >= d ? t : 0u;
#endif
    return r;
}
// n bytes, the lanes side by side; 16 at a time where both ends allow it
__device__ __forceinline__ static void wave_copy(uint8_t *dst, const uint8_t *src, uint64_t n) {
    uint64_t done = 0;
    if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0) {
        const uint64_t q = n / 16u;
        LFOR(l) for (uint64_t i = uint64_t(l); i < q; i += 64u) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
        done = q * 16u;
    }
    LFOR(l) for (uint64_t i = done + uint64_t(l); i < n; i += 64u) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------ LZW decode
// width of code j behind a Clear (j = 0: the first): the table holds 258 + max(j - 1, 0) entries when it is read, and the width is the bit length of that count + 1
__device__ __forceinline__ static uint32_t tlzw_width(uint32_t j) {
    const uint32_t w = 32u - uint32_t(__clz(258u + (j ? j : 1u)));
    return w > 12u ? 12u : w;
}
// bits of the codes 0 .. i - 1 behind a Clear: 254 codes of 9 bits, 512 of 10, 1024 of 11, the rest 12
__device__ __forceinline__ static uint64_t tlzw_off(uint32_t i) {
    const uint64_t a = i < 254u ? i : 254u, b = i < 254u ? 0u : (i - 254u < 512u ? i - 254u : 512u), c = i < 766u ? 0u : (i - 766u < 1024u ? i - 766u : 1024u), d = i < 1790u ? 0u : i - 1790u;
    return a * 9u + b * 10u + c * 11u + d * 12u;
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_lzw_decode(const TiffSeg *segs, const uint32_t *which, const uint8_t *data, uint8_t *dec, uint32_t *status) {
    CSH_SHARED uint16_t s_prefix[4096];
    CSH_SHARED uint16_t s_len[4096];
    CSH_SHARED uint8_t s_first[4096];
    CSH_SHARED uint8_t s_last[4096];
    const uint32_t si = which[blockIdx.x];
    const TiffSeg f = segs[si];
    const uint8_t *d = data + f.data_off;   // (the pool is padded: three bytes at any bit of the stream can be read)
    uint8_t *o = dec + f.dec_off;
    const uint32_t clear = 256u, npx = f.dec_len;
    LFOR(l) for (uint32_t c = uint32_t(l); c < clear; c += 64u) { s_prefix[c] = 0; s_len[c] = 1; s_first[c] = uint8_t(c); s_last[c] = uint8_t(c); }
    CSP_WAVE_SYNC();
    const uint64_t total_bits = uint64_t(f.data_len) * 8u;
    uint64_t bitpos = 0;
    uint32_t since = 0, prev = 0, out = 0, st = TIFF_OK;   // since: codes read behind the last Clear (a segment need not start with one)
    while (out < npx) {
        const uint64_t off0 = tlzw_off(since);
        LV<uint32_t> c, wid;
        LFOR(l) {
            const uint32_t j = since + uint32_t(l), w = tlzw_width(j);
            const uint64_t p = bitpos + (tlzw_off(j) - off0);
            wid[l] = w;
            if (p + w > total_bits) c[l] = 0xFFFFu;   // the data ends here
            else { const uint8_t *q = d + (p >> 3); c[l] = (((uint32_t(q[0]) << 16) | (uint32_t(q[1]) << 8) | uint32_t(q[2])) >> (24u - uint32_t(p & 7u) - w)) & ((1u << w) - 1u); }
        }
        const LV<uint32_t> pc = lprev(c, prev);
        // code j defines entry E = 257 + j (from the second code on, while the table has room) and may be that entry itself (KwKwK), nothing beyond it
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
            uint32_t code = c[l];
            uint64_t p = uint64_t(out) + pos[l] + slen[l];
            for (uint32_t k = 0; k < slen[l]; k++) {   // surplus data is left unwritten
                p--;
                if (p < npx) o[p] = code >= clear ? s_last[code] : uint8_t(code);
                if (code >= clear) code = s_prefix[code];
            }
        }
        out = uint64_t(out) + total > npx ? npx : out + total;
        since += n;
        if (n) prev = lget(c, n - 1u);
        bitpos += tlzw_off(since) - off0;
        if (n < 64u) {
            if ((bad >> n) & 1u) { if (out < npx) st = TIFF_BAD_CODE; break; }   // (behind a full segment it is surplus, whatever it reads as)
            if (lget(c, n) != clear) break;   // EOI, or no data left
            bitpos += lget(wid, n); since = 0;
        }
    }
    if (st == TIFF_OK && out < npx) st = TIFF_SHORT;
    LFOR(l) if (l == 0) status[si] = st;
}
void launch_tiff_lzw_decode(hipStream_t st, const TiffSeg *segs, const uint32_t *which, uint32_t n, const uint8_t *data, uint8_t *dec, uint32_t *status) {
    if (!n) return;
    CSH_LAUNCH(k_tiff_lzw_decode, dim3(n), dim3(CSP_WAVE_THREADS), st, segs, which, data, dec, status);
}

// ------------------------------------------------------------------------------------------------ PackBits decode, plain copies
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_packbits_decode(const TiffSeg *segs, const uint32_t *which, const uint8_t *data, uint8_t *dec, uint32_t *status) {
    const uint32_t si = which[blockIdx.x];
    const TiffSeg f = segs[si];
    const uint8_t *d = data + f.data_off;
    uint8_t *o = dec + f.dec_off;
    uint32_t pos = 0, out = 0, st = TIFF_OK;
    while (out < f.dec_len) {
        if (pos >= f.data_len) { st = TIFF_SHORT; break; }
        const uint32_t h = csh::uni(d[pos]);
        if (h == 128u) { pos++; continue; }   // the no-op header
        const bool literal = h < 128u;
        const uint32_t n = literal ? h + 1u : 257u - h, need = literal ? 1u + n : 2u;
        if (uint64_t(pos) + need > f.data_len) { st = TIFF_SHORT; break; }
        if (n > f.dec_len - out) { st = TIFF_BAD_CODE; break; }   // a packet may not cross the end of the segment (a row's end it may: libtiff does not look either)
        const uint8_t fill = d[pos + 1u];
        LFOR(l) for (uint32_t k = uint32_t(l); k < n; k += 64u) o[out + k] = literal ? d[pos + 1u + k] : fill;
        pos += need; out += n;
    }
    LFOR(l) if (l == 0) status[si] = st;
}
void launch_tiff_packbits_decode(hipStream_t st, const TiffSeg *segs, const uint32_t *which, uint32_t n, const uint8_t *data, uint8_t *dec, uint32_t *status) {
    if (!n) return;
    CSH_LAUNCH(k_tiff_packbits_decode, dim3(n), dim3(CSP_WAVE_THREADS), st, segs, which, data, dec, status);
}

// a wave takes PLACE_SLICE bytes of a segment (blockIdx.y: which): an input of one huge strip is copied by many waves
enum : uint32_t { PLACE_SLICE = 65536 };
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_place(const TiffSeg *segs, const uint32_t *which, const uint8_t *src, const uint64_t *scratch_off, uint8_t *dec, uint32_t *status) {
    const uint32_t si = which[blockIdx.x];
    const TiffSeg f = segs[si];
    const uint32_t n = (scratch_off || f.data_len > f.dec_len) ? f.dec_len : f.data_len;   // (an inflated segment is whole: the inflate kernels left the status)
    if (!scratch_off && blockIdx.y == 0) LFOR(l) if (l == 0) status[si] = f.data_len < f.dec_len ? uint32_t(TIFF_SHORT) : uint32_t(TIFF_OK);
    const uint64_t from = uint64_t(blockIdx.y) * PLACE_SLICE;
    if (from >= n) return;
    const uint8_t *s = src + (scratch_off ? scratch_off[blockIdx.x] : f.data_off);
    wave_copy(dec + f.dec_off + from, s + from, n - from < PLACE_SLICE ? n - from : uint64_t(PLACE_SLICE));
}
void launch_tiff_place(hipStream_t st, const TiffSeg *segs, const uint32_t *which, uint32_t n, uint32_t max_len, const uint8_t *src, const uint64_t *scratch_off, uint8_t *dec, uint32_t *status) {
    if (!n) return;
    const uint32_t slices = max_len ? (max_len + PLACE_SLICE - 1u) / PLACE_SLICE : 1u;   // (a segment decodes to at most 2^31 bytes: 32768 slices)
    CSH_LAUNCH(k_tiff_place, dim3(n, slices), dim3(CSP_WAVE_THREADS), st, segs, which, src, scratch_off, dec, status);
}

// ------------------------------------------------------------------------------------------------ Predictor 2
__device__ __forceinline__ static uint32_t sample_get(const uint8_t *p, uint32_t i, uint32_t pred) {
    if (pred == TIFF_PRED_8) return p[i];
    const uint32_t a = p[2u * i], b = p[2u * i + 1u];
    return pred == TIFF_PRED_16LE ? a | (b << 8) : (a << 8) | b;
}
__device__ __forceinline__ static void sample_put(uint8_t *p, uint32_t i, uint32_t pred, uint32_t v) {
    if (pred == TIFF_PRED_8) { p[i] = uint8_t(v); return; }
    p[2u * i] = uint8_t(pred == TIFF_PRED_16LE ? v : v >> 8); p[2u * i + 1u] = uint8_t(pred == TIFF_PRED_16LE ? v >> 8 : v);
}
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_unpredict(const TiffSeg *segs, const uint32_t *row_seg, uint8_t *dec) {
    const TiffSeg f = segs[row_seg[blockIdx.x]];
    uint8_t *p = dec + f.dec_off + uint64_t(blockIdx.x - f.row_base) * f.rowbytes;
    const uint32_t m = f.rowbytes / (f.pred == TIFF_PRED_8 ? 1u : 2u), stride = f.spp, W = (64u / stride) * stride, mask = f.pred == TIFF_PRED_8 ? 0xFFu : 0xFFFFu;
    LV<uint32_t> before, from;   // the window before, summed; the lane of its last pixel that holds this lane's sample
    LFOR(l) { before[l] = 0; from[l] = W - stride + uint32_t(l) % stride; }
    for (uint32_t base = 0; base < m; base += W) {
        LV<uint32_t> v;
        LFOR(l) v[l] = (uint32_t(l) < W && base + uint32_t(l) < m) ? sample_get(p, base + uint32_t(l), f.pred) : 0u;
        for (uint32_t d = stride; d < W; d <<= 1) { const LV<uint32_t> t = lshift_up(v, d); LFOR(l) v[l] += t[l]; }
        const LV<uint32_t> carry = lgather(before, from);
        LFOR(l) {
            v[l] = (v[l] + carry[l]) & mask;
            if (uint32_t(l) < W && base + uint32_t(l) < m) sample_put(p, base + uint32_t(l), f.pred, v[l]);
        }
        before = v;
    }
}
void launch_tiff_unpredict(hipStream_t st, const TiffSeg *segs, const uint32_t *row_seg, uint32_t nrows, uint8_t *dec) {
    if (!nrows) return;
    CSH_LAUNCH(k_tiff_unpredict, dim3(nrows), dim3(CSP_WAVE_THREADS), st, segs, row_seg, dec);
}
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_predict(const TiffOut *outs, const uint32_t *row_out, const uint8_t *dec, uint8_t *pred) {
    const TiffOut f = outs[row_out[blockIdx.x]];
    if (f.pred == TIFF_PRED_NONE) return;
    const uint64_t at = f.src_off + uint64_t(blockIdx.x - f.row_base) * f.rowbytes;
    const uint8_t *p = dec + at;
    uint8_t *q = pred + at;
    const uint32_t m = f.rowbytes / (f.pred == TIFF_PRED_8 ? 1u : 2u);
    LFOR(l) for (uint32_t i = uint32_t(l); i < m; i += 64u) sample_put(q, i, f.pred, sample_get(p, i, f.pred) - (i >= f.spp ? sample_get(p, i - f.spp, f.pred) : 0u));
}
void launch_tiff_predict(hipStream_t st, const TiffOut *outs, const uint32_t *row_out, uint32_t nrows, const uint8_t *dec, uint8_t *pred) {
    if (!nrows) return;
    CSH_LAUNCH(k_tiff_predict, dim3(nrows), dim3(CSP_WAVE_THREADS), st, outs, row_out, dec, pred);
}

// ------------------------------------------------------------------------------------------------ LZW encode
enum : uint32_t { ENC_SLOTS = 8192, ENC_EMPTY = 0xFFFFFFFFu };   // a slot: (prefix code << 8 | byte) << 12 | code

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_lzw_encode(const TiffOut *outs, uint32_t nouts, const uint8_t *dec, const uint8_t *pred, uint8_t *cbuf, uint32_t *cbytes) {
    CSH_SHARED uint32_t s_tab[ENC_SLOTS];
    const uint32_t variant = blockIdx.y;
    const TiffOut f = outs[blockIdx.x];
    if (variant && f.pred == TIFF_PRED_NONE) return;
    const uint8_t *px = (variant ? pred : dec) + f.src_off;
    const uint32_t n = f.len;
    uint32_t *dst = reinterpret_cast<uint32_t *>(cbuf + f.buf_off + uint64_t(variant) * f.cap);
    uint32_t width = 9u, next = 258u, nb = 0, words = 0;
    uint64_t acc = 0;
    auto emit = [&](uint32_t code) {   // from the high bit down: a word is stored with its first byte in front
        acc = (acc << width) | code; nb += width;
        if (nb >= 32u) { nb -= 32u; LFOR(l) if (l == 0) dst[words] = __builtin_bswap32(uint32_t(acc >> nb)); words++; acc &= (uint64_t(1) << nb) - 1u; }
    };
    auto wipe = [&]() {
        CSP_WAVE_SYNC();
        LFOR(l) for (uint32_t s = uint32_t(l); s < ENC_SLOTS; s += 64u) s_tab[s] = ENC_EMPTY;
        CSP_WAVE_SYNC();
    };
    // what follows every code: the entry `next` (the width follows the count, one code early); right behind entry 4094 a Clear and an empty table
    auto after_code = [&](uint32_t slot, uint32_t key, bool insert) {
        if (next < 4094u) {
            if (insert) { LFOR(l) if (l == 0) s_tab[slot] = (key << 12) | next; CSP_WAVE_SYNC(); }
            next++;
            if (next >= (1u << width) && width < 12u) width++;
        } else { emit(256u); if (insert) wipe(); width = 9u; next = 258u; }
    };
    wipe();
    emit(256u);
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
    if (have) { emit(cur); after_code(0, 0, false); }
    emit(257u);
    const uint32_t bytes = words * 4u + (nb + 7u) / 8u;
    LFOR(l) if (l == 0) { if (nb) dst[words] = __builtin_bswap32(uint32_t(acc << (32u - nb))); cbytes[variant * nouts + blockIdx.x] = bytes; }
}
void launch_tiff_lzw_encode(hipStream_t st, const TiffOut *outs, uint32_t nouts, const uint8_t *dec, const uint8_t *pred, uint8_t *cbuf, uint32_t *cbytes) {
    if (!nouts) return;   // (a batch holds at most 2^25 segments and as many rows: route_tiff.cpp cuts its groups so, and a grid's x stays below 2^31)
    CSH_LAUNCH(k_tiff_lzw_encode, dim3(nouts, 2), dim3(CSP_WAVE_THREADS), st, outs, nouts, dec, pred, cbuf, cbytes);
}

// ------------------------------------------------------------------------------------------------ PackBits encode
// One row of n bytes; dst == nullptr: the length alone.  Byte i is `rep` if it stands in three equal bytes in a row.  A piece starts at 0, where rep changes, and
// inside rep where the byte changes; a packet every 128 bytes of a piece.  A packet costs its header and, replicated, one byte, or, literal, its bytes.
__device__ __forceinline__ static uint32_t packbits_row(const uint8_t *b, uint32_t n, uint8_t *dst) {
    auto at = [&](int64_t i) -> int32_t { return (i < 0 || i >= int64_t(n)) ? -1 - int32_t(i & 1) : int32_t(b[i]); };   // (outside the row: equal to nothing)
    auto rep = [&](int64_t i) -> bool {
        const int32_t a = at(i - 2), c = at(i - 1), x = at(i), e = at(i + 1), g = at(i + 2);
        return (a == c && c == x) || (c == x && x == e) || (x == e && e == g);
    };
    auto piece = [&](int64_t i) -> bool { return i == 0 || rep(i) != rep(i - 1) || (rep(i) && at(i) != at(i - 1)); };
    uint32_t carry_start = 0, total = 0;   // the last piece start so far, + 1; bytes written so far
    for (uint32_t base = 0; base < n; base += 64u) {
        LV<uint32_t> key, r;
        LFOR(l) { const uint32_t i = base + uint32_t(l); r[l] = (i < n && rep(i)) ? 1u : 0u; key[l] = (i < n && piece(i)) ? i + 1u : 0u; }
        const LV<uint32_t> inc = csh::lmaxscan(key);
        LV<uint32_t> cost, ps;
        LFOR(l) {
            const uint32_t i = base + uint32_t(l);
            ps[l] = (inc[l] > carry_start ? inc[l] : carry_start) - 1u;   // the start of the piece byte i is in
            cost[l] = i >= n ? 0u : ((i - ps[l]) % 128u == 0u ? 2u : (r[l] ? 0u : 1u));
        }
        uint32_t sum;
        const LV<uint32_t> ex = lscan(cost, sum);
        if (dst) LFOR(l) {
            const uint32_t i = base + uint32_t(l);
            if (i < n) {
                const uint32_t o = total + ex[l], in_piece = i - ps[l], pk = i - in_piece % 128u;   // pk: the packet's first byte
                const bool first = in_piece % 128u == 0u;
                if (first || !r[l]) dst[first ? o + 1u : o] = b[i];
                const bool last = i + 1u == n || piece(int64_t(i) + 1) || (in_piece + 1u) % 128u == 0u;
                if (last) {
                    const uint32_t len = i - pk + 1u, ho = r[l] ? (i > pk ? o - 2u : o) : (i > pk ? o - 1u - (i - pk) : o);
                    dst[ho] = uint8_t(r[l] ? (len == 1u ? 0u : 257u - len) : len - 1u);
                }
            }
        }
        total += sum;
        const uint32_t last_key = csh::llast(inc);
        carry_start = last_key > carry_start ? last_key : carry_start;
    }
    return total;
}
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_packbits_size(const TiffOut *outs, const uint32_t *row_out, const uint8_t *dec, uint32_t *row_len) {
    const TiffOut f = outs[row_out[blockIdx.x]];
    const uint32_t len = packbits_row(dec + f.src_off + uint64_t(blockIdx.x - f.row_base) * f.rowbytes, f.rowbytes, nullptr);
    LFOR(l) if (l == 0) row_len[blockIdx.x] = len;
}
// a wave a segment: the rows' places in it, an exclusive scan of their lengths 64 at a time, and the segment's bytes
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_packbits_scan(const TiffOut *outs, const uint32_t *row_len, uint32_t *row_start, uint32_t *cbytes) {
    const TiffOut f = outs[blockIdx.x];
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < f.rows; k0 += 64u) {
        LV<uint32_t> v;
        LFOR(l) v[l] = k0 + uint32_t(l) < f.rows ? row_len[f.row_base + k0 + uint32_t(l)] : 0u;
        uint32_t sum;
        const LV<uint32_t> ex = lscan(v, sum);
        LFOR(l) if (k0 + uint32_t(l) < f.rows) row_start[f.row_base + k0 + uint32_t(l)] = carry + ex[l];
        carry += sum;
    }
    LFOR(l) if (l == 0) cbytes[blockIdx.x] = carry;
}
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_packbits_encode(const TiffOut *outs, const uint32_t *row_out, const uint8_t *dec, const uint32_t *row_start, uint8_t *cbuf) {
    const TiffOut f = outs[row_out[blockIdx.x]];
    (void)packbits_row(dec + f.src_off + uint64_t(blockIdx.x - f.row_base) * f.rowbytes, f.rowbytes, cbuf + f.buf_off + row_start[blockIdx.x]);
}
void launch_tiff_packbits_encode(hipStream_t st, const TiffOut *outs, const uint32_t *row_out, uint32_t nrows, uint32_t nouts, const uint8_t *dec, uint32_t *row_len, uint32_t *row_start, uint8_t *cbuf, uint32_t *cbytes) {
    if (!nrows) return;
    CSH_LAUNCH(k_tiff_packbits_size, dim3(nrows), dim3(CSP_WAVE_THREADS), st, outs, row_out, dec, row_len);
    CSH_LAUNCH(k_tiff_packbits_scan, dim3(nouts), dim3(CSP_WAVE_THREADS), st, outs, row_len, row_start, cbytes);
    CSH_LAUNCH(k_tiff_packbits_encode, dim3(nrows), dim3(CSP_WAVE_THREADS), st, outs, row_out, dec, row_start, cbuf);
}

// ------------------------------------------------------------------------------------------------ the files
__device__ __forceinline__ static void put32(uint8_t *p, uint32_t v, bool be) {
    for (uint32_t k = 0; k < 4u; k++) p[k] = uint8_t(v >> (be ? 24u - 8u * k : 8u * k));
}
__device__ __forceinline__ static uint32_t get32(const uint8_t *p, bool be) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4u; k++) v |= uint32_t(p[k]) << (be ? 24u - 8u * k : 8u * k);
    return v;
}
// one lane per file: behind the 8-byte header, page by page, the segments, then the values block and the IFD, each at an even offset; a page coded both ways takes
// the variant with the smaller sum of segment bytes, without the predictor on a tie
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_layout(const TiffFile *files, uint32_t nfiles, const TiffPage *pages, const TiffOut *outs, uint32_t nouts, const uint32_t *cbytes, int raw,
                                                                   uint64_t *seg_pos, uint32_t *seg_bytes, TiffPlace *place, uint64_t *file_bytes) {
    LFOR(l) {
        const uint32_t fi = blockIdx.x * 64u + uint32_t(l);
        if (fi < nfiles) {
            const TiffFile F = files[fi];
            uint64_t pos = 8;
            for (uint32_t k = 0; k < F.npages; k++) {
                const TiffPage &P = pages[F.first_page + k];
                uint32_t variant = 0;
                if (P.both) {
                    uint64_t s0 = 0, s1 = 0;
                    for (uint32_t o = P.first_out; o < P.first_out + P.nout; o++) { s0 += cbytes[o]; s1 += cbytes[nouts + o]; }
                    variant = s1 < s0 ? 1u : 0u;
                }
                for (uint32_t o = P.first_out; o < P.first_out + P.nout; o++) {
                    const uint32_t bytes = raw ? outs[o].len : cbytes[variant * nouts + o];
                    pos += pos & 1u;
                    seg_pos[o] = pos; seg_bytes[o] = bytes;
                    pos += bytes;
                }
                pos += pos & 1u;
                TiffPlace pl;
                pl.head_pos = pos; pl.next_ifd = 0; pl.variant = variant; pl.pad = 0;
                place[F.first_page + k] = pl;
                if (k) place[F.first_page + k - 1u].next_ifd = pos + P.head[variant].ifd_pos;
                pos += P.head[variant].len;
            }
            file_bytes[fi] = pos;
        }
    }
}
void launch_tiff_layout(hipStream_t st, const TiffFile *files, uint32_t nfiles, const TiffPage *pages, const TiffOut *outs, uint32_t nouts, const uint32_t *cbytes, int raw, uint64_t *seg_pos, uint32_t *seg_bytes,
                        TiffPlace *place, uint64_t *file_bytes) {
    if (!nfiles) return;
    CSH_LAUNCH(k_tiff_layout, dim3((nfiles + 63u) / 64u), dim3(CSP_WAVE_THREADS), st, files, nfiles, pages, outs, nouts, cbytes, raw, seg_pos, seg_bytes, place, file_bytes);
}

// one wave per output segment, then one per page: the segment's bytes (the variant the page took) and the page's values block and IFD to their places
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_gather(const TiffFile *files, const TiffPage *pages, const TiffOut *outs, uint32_t nouts, const uint8_t *dec, const uint8_t *cbuf, int raw,
                                                                   const uint8_t *heads, const uint64_t *seg_pos, const uint32_t *seg_bytes, const TiffPlace *place, uint8_t *out) {
    if (blockIdx.x < nouts) {
        const TiffOut f = outs[blockIdx.x];
        const TiffPlace pl = place[f.page];
        const uint8_t *src = raw ? dec + f.src_off : cbuf + f.buf_off + uint64_t(pl.variant) * f.cap;
        wave_copy(out + files[pages[f.page].file].out_off + seg_pos[blockIdx.x], src, seg_bytes[blockIdx.x]);
        return;
    }
    const uint32_t pg = blockIdx.x - nouts;
    const TiffPlace pl = place[pg];
    const TiffHead H = pages[pg].head[pl.variant];
    wave_copy(out + files[pages[pg].file].out_off + pl.head_pos, heads + H.off, H.len);
}
void launch_tiff_gather(hipStream_t st, const TiffFile *files, const TiffPage *pages, uint32_t npages, const TiffOut *outs, uint32_t nouts, const uint8_t *dec, const uint8_t *cbuf, int raw, const uint8_t *heads,
                        const uint64_t *seg_pos, const uint32_t *seg_bytes, const TiffPlace *place, uint8_t *out) {
    if (!npages) return;
    CSH_LAUNCH(k_tiff_gather, dim3(nouts + npages), dim3(CSP_WAVE_THREADS), st, files, pages, outs, nouts, dec, cbuf, raw, heads, seg_pos, seg_bytes, place, out);
}

// one wave per page, behind the gather: the blob's own offsets take the blob's place, the segments' offsets and byte counts go into their arrays, the next-IFD
// pointer into the IFD's last word; the file's first page writes the header
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_tiff_patch(const TiffFile *files, const TiffPage *pages, const uint32_t *relocs, const uint64_t *seg_pos, const uint32_t *seg_bytes, const TiffPlace *place,
                                                                  uint8_t *out) {
    const uint32_t pg = blockIdx.x;
    const TiffPage &P = pages[pg];
    const TiffFile F = files[P.file];
    const TiffPlace pl = place[pg];
    const TiffHead H = P.head[pl.variant];
    const bool be = F.big_endian != 0;
    uint8_t *file = out + F.out_off, *blob = file + pl.head_pos;
    LFOR(l) {
        for (uint32_t k = uint32_t(l); k < H.nreloc; k += 64u) { uint8_t *q = blob + relocs[H.reloc_first + k]; put32(q, get32(q, be) + uint32_t(pl.head_pos), be); }
        for (uint32_t k = uint32_t(l); k < P.nout; k += 64u) { put32(blob + H.off_pos + 4u * k, uint32_t(seg_pos[P.first_out + k]), be); put32(blob + H.cnt_pos + 4u * k, seg_bytes[P.first_out + k], be); }
        if (l == 0) {
            put32(blob + H.len - 4u, uint32_t(pl.next_ifd), be);
            if (pg == F.first_page) { file[0] = file[1] = be ? 'M' : 'I'; file[2] = be ? 0 : 42; file[3] = be ? 42 : 0; put32(file + 4, uint32_t(pl.head_pos + H.ifd_pos), be); }
        }
    }
}
void launch_tiff_patch(hipStream_t st, const TiffFile *files, const TiffPage *pages, uint32_t npages, const uint32_t *relocs, const uint64_t *seg_pos, const uint32_t *seg_bytes, const TiffPlace *place, uint8_t *out) {
    if (!npages) return;
    CSH_LAUNCH(k_tiff_patch, dim3(npages), dim3(CSP_WAVE_THREADS), st, files, pages, relocs, seg_pos, seg_bytes, place, out);
}

}  // namespace cst
