// k_vp8l_refs.hip -- lossless WebP OUTPUT with the format's LZ77 backward references and colour cache (CSH_VP8L=refs).  The front end is
// k_vp8l_enc.hip's (subtract-green, the per-block predictor, the residual ARGB image); everything here works on that residual image in the scan order the
// format codes it, cut into CHUNKS of VP8L_CHUNK positions.  A chunk is a unit of scheduling, not of the format: the stream is one piece, a copy may reach
// back past its chunk's start, and only the parse restarts (and cuts a copy) at a chunk's end.
//   k_vp8l_match       one wave per chunk, one lane per pixel: per position the longest copy among the fixed distances 1, 2, width - 1, width, width + 1 (for a
//                      fixed distance d, len_d(i) = px[i] == px[i - d] ? 1 + len_d(i + 1) : 0 -- a segmented reverse scan, done with ballots) and one hashed
//                      candidate, the NEAREST earlier position whose next three pixels hash alike: an LDS table of positions updated with atomicMax, so it is
//                      defined by position and never by which lane's store landed last
//   k_vp8l_parse       one wave per chunk: the greedy walk over a group of 64 positions is a chain of readlanes; every position becomes a token or nothing
//   k_vp8l_cache_*     "pixel i hits the cache" = the nearest earlier pixel with the same slot has the same ARGB: the last pixel per slot of every chunk (last),
//                      an exclusive scan of those over the chunks (scan), then the same previous-occurrence query inside the chunk (hits) -- for every cache size
//                      tried at once
//   k_vp8l_refs_hist   symbol counts of every cache size
//   k_vp8l_refs_codes  one wave per picture: the cache size by estimated cost, the five codes (the green alphabet is up to 256 + 24 + 1024 symbols: the heap of
//                      png_codes.h code_lengths over LDS arrays instead of scratch), the EXACT size of the stream and of the plain coder's: the smaller is written
//   k_vp8l_pack_refs   one wave per picture: the tokens through the LDS bit window, placed by a scan of their bit lengths
#include "vp8l_refs.h"

namespace csw {


// ---- candidates
struct MatchLds { uint32_t table[1u << VP8L_HASH_BITS]; };   // hash -> the last position that has it, plus one

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_match(const Vp8lImg *imgs, const uint32_t *work, uint64_t *toks) {
    CSH_SHARED MatchLds S;
    const Vp8lImg im = imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    const uint32_t *px = work + im.res_off;
    uint64_t *tok = toks + im.tok_off;
    const uint32_t N = im.width * im.height, start = blockIdx.x * VP8L_CHUNK, end = N - start < VP8L_CHUNK ? N : start + VP8L_CHUNK;
    // the hashed candidate: positions enter the table in scan order, VP8L_WARM of them in front of the chunk first
    LFOR(l) for (uint32_t i = uint32_t(l); i < (1u << VP8L_HASH_BITS); i += 64) S.table[i] = 0;
    CSP_WAVE_SYNC();
    for (uint32_t g0 = start > VP8L_WARM ? start - VP8L_WARM : 0u; g0 < start; g0 += 64) LFOR(l) {
        const uint32_t p = g0 + uint32_t(l);
        if (p + 3 <= N) atomicMax(&S.table[vp8l_hash3(px[p], px[p + 1], px[p + 2])], p + 1);
    }
    CSP_WAVE_SYNC();
    for (uint32_t g0 = start; g0 < end; g0 += 64) {
        LV<uint32_t> h, ok, cand;
        LFOR(l) {
            const uint32_t p = g0 + uint32_t(l);
            ok[l] = p < end && p + 3 <= N ? 1u : 0u;
            h[l] = ok[l] ? vp8l_hash3(px[p], px[p + 1], px[p + 2]) : 0u;
            cand[l] = ok[l] ? S.table[h[l]] : 0u;
        }
        const LV<int> prev = lprev_same(h, ok);   // a nearer one inside the group
        LFOR(l) {
            const uint32_t p = g0 + uint32_t(l);
            if (prev[l] >= 0) cand[l] = g0 + uint32_t(prev[l]) + 1;
            if (p < end) tok[p] = cand[l];   // read back by this lane in the pass below
        }
        CSP_WAVE_SYNC();
        LFOR(l) if (ok[l]) atomicMax(&S.table[h[l]], g0 + uint32_t(l) + 1);
        CSP_WAVE_SYNC();
    }
    // the fixed distances, backwards: nz[k] = the first position at or behind the group where the run of distance dv[k] breaks.  The pass starts
    // VP8L_MAX_LEN behind the chunk's end: a run that reaches that far is at the cap whatever follows.
    const uint32_t hi = N - end < VP8L_MAX_LEN ? N : end + VP8L_MAX_LEN;
    const uint32_t w = im.width;
    uint32_t dv[5] = {1u, w, w + 1u, w - 1u, 2u};   // ties go to the first
    for (int k = 1; k < 5; k++) for (int j = 0; j < k; j++) if (dv[k] == dv[j]) dv[k] = 0;
    uint32_t nz[5] = {hi, hi, hi, hi, hi};
    for (uint32_t gi = (hi - start + 63) / 64; gi-- > 0;) {
        const uint32_t g0 = start + gi * 64;
        LV<uint32_t> me, blen, bdist;
        LFOR(l) { const uint32_t p = g0 + uint32_t(l); me[l] = p < hi ? px[p] : 0u; blen[l] = 0; bdist[l] = 0; }
        for (int k = 0; k < 5; k++) {
            const uint32_t d = dv[k];
            if (!d) continue;
            const uint64_t brk = ~csp::lballot([&](int l) { const uint32_t p = g0 + uint32_t(l); return p < hi && p >= d && px[p - d] == me[l]; });
            LFOR(l) {
                const uint64_t m = brk >> l;
                uint32_t len = m ? uint32_t(__ffsll(static_cast<unsigned long long>(m)) - 1) : nz[k] - (g0 + uint32_t(l));
                if (len > VP8L_MAX_LEN) len = VP8L_MAX_LEN;
                if (len > blen[l]) { blen[l] = len; bdist[l] = d; }
            }
            if (brk) nz[k] = g0 + uint32_t(__ffsll(static_cast<unsigned long long>(brk)) - 1);
        }
        LFOR(l) {
            const uint32_t p = g0 + uint32_t(l);
            if (p >= end) continue;
            uint32_t bl = blen[l], bd = bdist[l];
            const uint32_t hc = uint32_t(tok[p]), maxl = N - p < VP8L_MAX_LEN ? N - p : uint32_t(VP8L_MAX_LEN);
            if (hc && bl < maxl) {
                const uint32_t d = p - (hc - 1);
                // worth walking only if it is not a fixed distance and agrees where it would have to get past the best so far
                if (d <= VP8L_WINDOW && d != dv[0] && d != dv[1] && d != dv[2] && d != dv[3] && d != dv[4] && px[p + bl] == px[p - d + bl]) {
                    uint32_t n = 0;
                    while (n < maxl && px[p + n] == px[p - d + n]) n++;
                    if (n > bl) { bl = n; bd = d; }
                }
            }
            if (bl < VP8L_MIN_MATCH) { bl = 0; bd = 0; }
            tok[p] = uint64_t(bl) | (uint64_t(bd) << 16);
        }
    }
}

// ---- the parse: greedy, from the chunk's first position; a copy is cut at the chunk's end
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_parse(const Vp8lImg *imgs, uint64_t *toks) {
    const Vp8lImg im = imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    uint64_t *tok = toks + im.tok_off;
    const uint32_t N = im.width * im.height, start = blockIdx.x * VP8L_CHUNK, end = N - start < VP8L_CHUNK ? N : start + VP8L_CHUNK;
    uint32_t next = start;   // the next token's position (wave-uniform)
    for (uint32_t g0 = start; g0 < end; g0 += 64) {
        LV<uint32_t> len, dist;
        LFOR(l) {
            const uint32_t p = g0 + uint32_t(l);
            const uint64_t c = p < end ? tok[p] : 0ull;
            len[l] = uint32_t(c) & 0xFFFFu; dist[l] = uint32_t(c >> 16);
            if (p < end && len[l] > end - p) len[l] = end - p;
            if (len[l] < VP8L_MIN_MATCH) { len[l] = 1; dist[l] = 0; }
        }
        uint64_t starts = 0;
        while (next < g0 + 64 && next < end) {
            const int j = int(next - g0);
            starts |= 1ull << j;
            next += lget(len, j);
        }
        LFOR(l) {
            const uint32_t p = g0 + uint32_t(l);
            if (p < end) tok[p] = (starts >> l) & 1u ? VP8L_TOKEN | uint64_t(len[l]) | (uint64_t(dist[l]) << 16) : 0ull;
        }
    }
}

// ---- the colour cache.  An entry of a table: (order << 32) | ARGB, order 0 = never written, 1 = written in front of the chunk, p - start + 2 = by position p
struct CacheLds { unsigned long long t[VP8L_CACHE_STATE]; };

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_cache_last(const Vp8lImg *imgs, const uint32_t *work, uint64_t *cst) {
    CSH_SHARED CacheLds S;
    const Vp8lImg im = imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    const uint32_t *px = work + im.res_off;
    const uint32_t N = im.width * im.height, start = blockIdx.x * VP8L_CHUNK, end = N - start < VP8L_CHUNK ? N : start + VP8L_CHUNK;
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_CACHE_STATE; i += 64) S.t[i] = 0;
    CSP_WAVE_SYNC();
    for (uint32_t g0 = start; g0 < end; g0 += 64) LFOR(l) {
        const uint32_t p = g0 + uint32_t(l);
        if (p >= end) continue;
        const uint32_t v = px[p];
        for (uint32_t o = 1; o < VP8L_NOPT; o++)
            atomicMax(&S.t[vp8l_state_off(o) + vp8l_slot(v, vp8l_cache_bits(o))], (static_cast<unsigned long long>(p - start + 2) << 32) | v);
    }
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_CACHE_STATE; i += 64) cst[im.cst_off + uint64_t(blockIdx.x) * VP8L_CACHE_STATE + i] = S.t[i];
}
// one lane per slot: what the chunks in front of each chunk left there
__global__ void __launch_bounds__(256) k_vp8l_cache_scan(const Vp8lImg *imgs, uint64_t *cst) {
    const Vp8lImg im = imgs[blockIdx.y];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= VP8L_CACHE_STATE) return;
    uint64_t carry = 0;
    for (uint32_t c = 0; c < im.nchunk; c++) {
        uint64_t *e = &cst[im.cst_off + uint64_t(c) * VP8L_CACHE_STATE + i];
        const uint64_t cur = *e;
        *e = carry;
        if (cur) carry = (1ull << 32) | uint32_t(cur);
    }
}
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_cache_hits(const Vp8lImg *imgs, const uint32_t *work, const uint64_t *cst, uint8_t *hits) {
    CSH_SHARED CacheLds S;
    const Vp8lImg im = imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    const uint32_t *px = work + im.res_off;
    uint8_t *hit = hits + im.hit_off;
    const uint32_t N = im.width * im.height, start = blockIdx.x * VP8L_CHUNK, end = N - start < VP8L_CHUNK ? N : start + VP8L_CHUNK;
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_CACHE_STATE; i += 64) S.t[i] = cst[im.cst_off + uint64_t(blockIdx.x) * VP8L_CACHE_STATE + i];
    CSP_WAVE_SYNC();
    for (uint32_t g0 = start; g0 < end; g0 += 64) {
        LV<uint32_t> v, active, mask;
        LFOR(l) { const uint32_t p = g0 + uint32_t(l); active[l] = p < end ? 1u : 0u; v[l] = active[l] ? px[p] : 0u; mask[l] = 0; }
        for (uint32_t o = 1; o < VP8L_NOPT; o++) {
            LV<uint32_t> slot;
            LV<unsigned long long> cur;
            LFOR(l) { slot[l] = vp8l_slot(v[l], vp8l_cache_bits(o)); cur[l] = S.t[vp8l_state_off(o) + slot[l]]; }
            const LV<int> prev = lprev_same(slot, active);
            const LV<uint32_t> pv = lshfl(v, prev);
            LFOR(l) {
                const bool h = prev[l] >= 0 ? pv[l] == v[l] : (cur[l] != 0 && uint32_t(cur[l]) == v[l]);
                if (active[l] && h) mask[l] |= 1u << o;
            }
            CSP_WAVE_SYNC();
            LFOR(l) if (active[l]) atomicMax(&S.t[vp8l_state_off(o) + slot[l]], (static_cast<unsigned long long>(g0 + uint32_t(l) - start + 2) << 32) | v[l]);
            CSP_WAVE_SYNC();
        }
        LFOR(l) if (active[l]) hit[g0 + uint32_t(l)] = uint8_t(mask[l]);
    }
}

// ---- statistics of every option: a pixel that hits the option's cache is a cache symbol, any other single pixel four literals; copies count alike in all
__global__ void __launch_bounds__(256) k_vp8l_refs_hist(const Vp8lImg *imgs, const uint32_t *work, const uint64_t *toks, const uint8_t *hits, uint32_t *hist) {
    CSH_SHARED uint32_t h[VP8L_NOPT * VP8L_HIST];
    const Vp8lImg &im = imgs[blockIdx.y];
    const uint32_t N = im.width * im.height, i0 = blockIdx.x * VP8L_CHUNK;
    CSH_PHASE_LOOP(3) {
        if (blockIdx.x >= im.nchunk) continue;
        if (phase == 0) { for (uint32_t i = threadIdx.x; i < VP8L_NOPT * VP8L_HIST; i += 256) h[i] = 0; continue; }
        if (phase == 1) {
            for (uint32_t k = threadIdx.x; k < VP8L_CHUNK; k += 256) {
                const uint32_t i = i0 + k;
                if (i >= N) break;
                const uint64_t t = toks[im.tok_off + i];
                if (!(t & VP8L_TOKEN)) continue;
                const uint32_t dist = uint32_t(t >> 16);
                if (dist) {
                    uint32_t ls, ds, ne, ex;
                    vp8l_prefix(uint32_t(t) & 0xFFFFu, ls, ne, ex);
                    vp8l_prefix(vp8l_dist_code(dist, im.width), ds, ne, ex);
                    for (uint32_t o = 0; o < VP8L_NOPT; o++) { atomicAdd(&h[o * VP8L_HIST + 256 + ls], 1u); atomicAdd(&h[o * VP8L_HIST + VP8L_GREEN_MAX + 768 + ds], 1u); }
                    continue;
                }
                const uint32_t v = work[im.res_off + i], hm = hits[im.hit_off + i];
                for (uint32_t o = 0; o < VP8L_NOPT; o++) {
                    uint32_t *ho = h + o * VP8L_HIST;
                    if ((hm >> o) & 1u) { atomicAdd(&ho[280 + vp8l_slot(v, vp8l_cache_bits(o))], 1u); continue; }
                    atomicAdd(&ho[(v >> 8) & 255u], 1u); atomicAdd(&ho[VP8L_GREEN_MAX + ((v >> 16) & 255u)], 1u);
                    atomicAdd(&ho[VP8L_GREEN_MAX + 256 + (v & 255u)], 1u); atomicAdd(&ho[VP8L_GREEN_MAX + 512 + (v >> 24)], 1u);
                }
            }
            continue;
        }
        for (uint32_t i = threadIdx.x; i < VP8L_NOPT * VP8L_HIST; i += 256) if (h[i]) atomicAdd(&hist[uint64_t(blockIdx.y) * (VP8L_NOPT * VP8L_HIST) + i], h[i]);
    }
}


struct CodesLds {
    CodeWs ws;
    uint8_t len[9][288];        // the chosen option's red, blue, alpha, distance (1 .. 4); the plain coder's green, red, blue, alpha (5 .. 8)
    uint8_t glen[VP8L_GREEN_MAX];
    uint32_t gh[288];           // the plain green histogram widened to its alphabet
    unsigned long long bits[9];
};
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_refs_codes(const Vp8lImg *imgs, int nimg, const uint32_t *hist_plain, const uint32_t *hist, uint8_t *lens, uint32_t *pick) {
    CSH_SHARED CodesLds S;
    const int image = blockIdx.x;
    if (image >= nimg) return;
    const uint32_t *hp = hist_plain + uint64_t(image) * 1024u, *hr = hist + uint64_t(image) * (VP8L_NOPT * VP8L_HIST);
    // the option: the entropy of its five alphabets plus six bits per symbol in use for the description (the copies' extra bits are the same in all)
    uint64_t best = ~0ull;
    uint32_t opt = 0;
    for (uint32_t o = 0; o < VP8L_NOPT; o++) {
        const uint32_t *ho = hr + o * VP8L_HIST;
        uint64_t est = 0;
        for (int c = 0; c < 5; c++) {
            const uint32_t *f = ho + vp8l_hist_off(c), n = vp8l_alphabet(c, o);
            LV<uint64_t> part;
            LFOR(l) { part[l] = 0; for (uint32_t i = uint32_t(l); i < n; i += 64) part[l] += f[i]; }
            const uint64_t total = csp::lsum(part);
            LV<uint64_t> used;
            LFOR(l) { part[l] = 0; used[l] = 0; for (uint32_t i = uint32_t(l); i < n; i += 64) if (f[i]) { part[l] += uint64_t(f[i]) * bits16(f[i], total); used[l]++; } }
            est += csp::lsum(part) + 96ull * csp::lsum(used);
        }
        if (est < best) { best = est; opt = o; }
    }
    const uint32_t *hc = hr + opt * VP8L_HIST;
    LFOR(l) for (int i = l; i < 288; i += 64) S.gh[i] = i < 256 ? hp[i] : 0u;
    CSP_WAVE_SYNC();
    // the codes, one lane each: lane 0 the wide one; a code with one symbol costs no bits (code_lengths always codes two)
    LFOR(l) if (l < 9) {
        const int code = l < 5 ? l : l - 5;
        const uint32_t n = l < 5 ? vp8l_alphabet(code, opt) : (l == 5 ? 280u : 256u);
        const uint32_t *f = l < 5 ? hc + vp8l_hist_off(code) : (l == 5 ? S.gh : l == 8 ? hp + 768u : hp + 256u * uint32_t(l - 5));
        uint8_t *len = l == 0 ? S.glen : S.len[l];
        if (l == 0) code_lengths_wide(f, int(n), 15, len, S.ws); else csp::code_lengths(f, int(n), 15, len);
        const Vp8lCodeUse u = vp8l_code_use([&](int i) { return f[i]; }, int(n));
        if (u.nused <= 1) for (uint32_t i = 0; i < n; i++) len[i] = 0;
        unsigned long long b = l < 5 ? vp8l_refs_desc_bits(len, int(n), u) : vp8l_code_desc_bits(u);
        for (uint32_t i = 0; i < n; i++) b += static_cast<unsigned long long>(f[i]) * len[i];
        if (l == 0) for (uint32_t s = 0; s < 24; s++) b += static_cast<unsigned long long>(f[256 + s]) * vp8l_prefix_extra(s);
        if (l == 4) for (uint32_t s = 0; s < 40; s++) b += static_cast<unsigned long long>(f[s]) * vp8l_prefix_extra(s);
        S.bits[l] = b;
        if (l < 5) { uint8_t *o = lens + uint64_t(image) * VP8L_LENS + uint32_t(l) * VP8L_GREEN_MAX; for (uint32_t i = 0; i < n; i++) o[i] = len[i]; }
    }
    CSP_WAVE_SYNC();
    LFOR(l) if (l == 0) {
        // behind the common head: the cache's bit (and its size), "no meta prefix image", the descriptions, the symbols
        const unsigned long long refs = (opt ? 5u : 1u) + 1u + S.bits[0] + S.bits[1] + S.bits[2] + S.bits[3] + S.bits[4];
        const unsigned long long plain = 1u + 1u + S.bits[5] + S.bits[6] + S.bits[7] + S.bits[8] + 4u;
        const unsigned long long cap = 0xFFFFFFFFull;
        pick[4 * image] = refs < plain ? 1u : 0u; pick[4 * image + 1] = opt;
        pick[4 * image + 2] = uint32_t(refs < cap ? refs : cap); pick[4 * image + 3] = uint32_t(plain < cap ? plain : cap);
    }
}

// ---- one wave per picture
struct PackRefsLds {
    uint8_t glen[VP8L_GREEN_MAX], len[4][256];   // green; red, blue, alpha, distance
    uint16_t gcode[VP8L_GREEN_MAX], code[4][256];
    uint8_t mlen[288];
    uint16_t mcode[288];
    uint32_t mh[288];
    uint32_t win[160];
    Vp8lCodeUse use[6];
    Vp8lDescLds desc;
    Vp8lPalCodes pal;   // a palette candidate's head (CSH_VP8L=palette)
};
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_pack_refs(const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const uint64_t *toks, const uint8_t *hits,
                                                                     const uint32_t *hist, const uint8_t *lens, const uint32_t *pick, uint8_t *outp, uint32_t *file_len, uint32_t *status) {
    CSH_SHARED PackRefsLds S;
    const int image = blockIdx.x;
    if (image >= nimg || pick[4 * image] != 1u) return;
    const Vp8lImg im = imgs[image];
    uint8_t *file = outp + im.out_off;
    const uint32_t opt = pick[4 * image + 1], cbits = vp8l_cache_bits(opt);
    const uint32_t *hc = hist + uint64_t(image) * (VP8L_NOPT * VP8L_HIST) + opt * VP8L_HIST;
    const uint8_t *ln = lens + uint64_t(image) * VP8L_LENS;
    const uint32_t nblk = im.bw * im.bh;
    LFOR(l) for (int i = l; i < 288; i += 64) S.mh[i] = 0;
    LFOR(l) for (int i = l; i < 160; i += 64) S.win[i] = 0;
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_GREEN_MAX; i += 64) S.glen[i] = ln[i];
    LFOR(l) for (uint32_t i = uint32_t(l); i < 4 * 256; i += 64) S.len[i >> 8][i & 255u] = ln[((i >> 8) + 1) * VP8L_GREEN_MAX + (i & 255u)];
    CSP_WAVE_SYNC();
    for (uint32_t b0 = 0; b0 < nblk; b0 += 64) LFOR(l) if (b0 + uint32_t(l) < nblk) atomicAdd(&S.mh[modes[im.mode_off + b0 + uint32_t(l)]], 1u);
    CSP_WAVE_SYNC();
    LFOR(l) if (l < 6) {
        if (l == 5) {   // the predictor modes' code, as the plain coder makes it
            csp::code_lengths(S.mh, 280, 15, S.mlen);
            const Vp8lCodeUse u = vp8l_code_use([&](int i) { return S.mh[i]; }, 280);
            if (u.nused <= 1) for (int i = 0; i < 280; i++) S.mlen[i] = 0;
            csp::canonical(S.mlen, 280, S.mcode);
            S.use[5] = u;
        } else {
            const uint32_t n = vp8l_alphabet(l, opt);
            const uint32_t *f = hc + vp8l_hist_off(l);
            S.use[l] = vp8l_code_use([&](int i) { return f[i]; }, int(n));
            if (l == 0) csp::canonical(S.glen, int(n), S.gcode); else csp::canonical(S.len[l - 1], int(n), S.code[l - 1]);
        }
    }
    CSP_WAVE_SYNC();
    Vp8lPut P;
    P.begin(S.win, file + 20);
    if (im.pal) { vp8l_pal_codes(im.pal + 512, S.pal); P.head_palette(im, S.pal, S.desc); }   // the bundled indices of picture im.parent: width is the packed width
    else P.head(im, modes, S.mlen, S.mcode, S.use[5]);
    if (cbits) P.put1(1u | (uint64_t(cbits) << 1), 5); else P.put1(0, 1);   // the picture's colour cache
    P.put1(0, 1);                                                              // no meta prefix image
    P.code_runs(S.glen, int(vp8l_alphabet(0, opt)), S.use[0], S.desc);
    for (int c = 1; c < 5; c++) P.code_runs(S.len[c - 1], int(vp8l_alphabet(c, opt)), S.use[c], S.desc);
    // one wave walks the picture, so a group's loads are its latency: token, residual and hit byte are asked for together, and a group ahead of the bits
    const uint32_t N = im.width * im.height;
    LV<uint64_t> tn; LV<uint32_t> vn, hn;
    LFOR(l) { const uint32_t i = uint32_t(l); tn[l] = i < N ? toks[im.tok_off + i] : 0ull; vn[l] = i < N ? work[im.res_off + i] : 0u; hn[l] = i < N ? hits[im.hit_off + i] : 0u; }
    for (uint32_t i0 = 0; i0 < N; i0 += 64) {
        LV<uint64_t> val; LV<uint32_t> nb;
        LFOR(l) {
            const uint64_t t = tn[l];
            const uint32_t v = vn[l], hm = hn[l];
            const uint32_t j = i0 + 64u + uint32_t(l);
            tn[l] = j < N ? toks[im.tok_off + j] : 0ull; vn[l] = j < N ? work[im.res_off + j] : 0u; hn[l] = j < N ? hits[im.hit_off + j] : 0u;
            nb[l] = 0; val[l] = 0;
            if (!(t & VP8L_TOKEN)) continue;
            const uint32_t dist = uint32_t(t >> 16);
            if (dist) {   // length prefix, its extra bits, distance prefix, its extra bits: 15 + 10 + 15 + 18 at the most
                uint32_t ls, lne, lex, ds, dne, dex;
                vp8l_prefix(uint32_t(t) & 0xFFFFu, ls, lne, lex);
                vp8l_prefix(vp8l_dist_code(dist, im.width), ds, dne, dex);
                const uint32_t lg = S.glen[256 + ls], ld = S.len[3][ds];
                val[l] = uint64_t(S.gcode[256 + ls]) | (uint64_t(lex) << lg) | (uint64_t(S.code[3][ds]) << (lg + lne)) | (uint64_t(dex) << (lg + lne + ld));
                nb[l] = lg + lne + ld + dne;
                continue;
            }
            if (opt && ((hm >> opt) & 1u)) { const uint32_t s = 280 + vp8l_slot(v, cbits); val[l] = S.gcode[s]; nb[l] = S.glen[s]; continue; }
            const uint32_t g = (v >> 8) & 255u, r = (v >> 16) & 255u, b = v & 255u, a = v >> 24;
            const uint32_t lg = S.glen[g], lr = S.len[0][r], lb = S.len[1][b], la = S.len[2][a];
            nb[l] = lg + lr + lb + la;
            val[l] = uint64_t(S.gcode[g]) | (uint64_t(S.code[0][r]) << lg) | (uint64_t(S.code[1][b]) << (lg + lr)) | (uint64_t(S.code[2][a]) << (lg + lr + lb));
        }
        P.bo.put(val, nb);
    }
    P.finish(im, file, im.pal ? int(im.parent) : image, file_len, status);
}

void launch_vp8l_refs_stages(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &R) {
    const unsigned max_chunks = unsigned((max_pixels + VP8L_CHUNK - 1) / VP8L_CHUNK);
    launch_vp8l_front(st, imgs, nimg, max_blocks, max_pixels, work, modes, hist);
    CSH_LAUNCH(k_vp8l_match, dim3(max_chunks, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, work, R.tok);
    CSH_LAUNCH(k_vp8l_parse, dim3(max_chunks, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, R.tok);
    CSH_LAUNCH(k_vp8l_cache_last, dim3(max_chunks, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, work, R.cst);
    CSH_LAUNCH(k_vp8l_cache_scan, dim3((VP8L_CACHE_STATE + 255) / 256, unsigned(nimg)), dim3(256), st, imgs, R.cst);
    CSH_LAUNCH(k_vp8l_cache_hits, dim3(max_chunks, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, work, R.cst, R.hit);
    CSH_LAUNCH_PHASED(k_vp8l_refs_hist, 3, dim3(max_chunks, unsigned(nimg)), dim3(256), st, imgs, work, R.tok, R.hit, R.hist);
    CSH_LAUNCH(k_vp8l_refs_codes, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, nimg, hist, R.hist, R.lens, R.pick);
}
void launch_vp8l_token_stages(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, const uint32_t *work, const uint32_t *hist, const Vp8lRefs &R) {
    const unsigned max_chunks = unsigned((max_pixels + VP8L_CHUNK - 1) / VP8L_CHUNK);
    CSH_LAUNCH(k_vp8l_parse, dim3(max_chunks, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, R.tok);
    CSH_LAUNCH_PHASED(k_vp8l_refs_hist, 3, dim3(max_chunks, unsigned(nimg)), dim3(256), st, imgs, work, R.tok, R.hit, R.hist);
    CSH_LAUNCH(k_vp8l_refs_codes, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, nimg, hist, R.hist, R.lens, R.pick);
}
void launch_vp8l_refs_packs(hipStream_t st, const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const uint32_t *hist, const Vp8lRefs &R, uint8_t *out, uint32_t *file_len,
                            uint32_t *status) {
    CSH_LAUNCH(k_vp8l_pack_refs, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, nimg, work, modes, R.tok, R.hit, R.hist, R.lens, R.pick, out, file_len, status);
    launch_vp8l_pack_plain(st, imgs, nimg, work, modes, hist, R.pick, out, file_len, status);
}
void launch_vp8l_encode_refs(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &R,
                             uint8_t *out, uint32_t *file_len, uint32_t *status) {
    if (!nimg) return;
    launch_vp8l_refs_stages(st, imgs, nimg, max_blocks, max_pixels, work, modes, hist, R);
    launch_vp8l_refs_packs(st, imgs, nimg, work, modes, hist, R, out, file_len, status);
}

}  // namespace csw
