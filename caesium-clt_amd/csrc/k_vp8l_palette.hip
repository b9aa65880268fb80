// k_vp8l_palette.hip -- lossless WebP OUTPUT with the format's colour-indexing transform (CSH_VP8L=palette).  A picture with at most 256 distinct ARGB
// values gets, beside its own record, a CANDIDATE record: its pixels as indices into the sorted palette, 8 / 4 / 2 / 1 of them bundled into the green byte of a
// packed pixel (2 / 4 / 16 / 256 colours), no subtract-green and no predictor.  The stages of k_vp8l_refs.hip run over the candidate as over any picture -- it is
// narrower, that is all -- and the smallest of the picture's plain stream, its refs stream and the candidate's (with or without copies) is written.
//   k_vp8l_pal_count   one wave per VP8L_PAL_STRIP pixels: the strip's distinct values in an LDS hash table, left as soon as there are 257 (a photograph leaves
//                      after a few hundred pixels), then merged into the picture's table with compare-and-swap.  Every probe sequence is at most the table's length;
//                      a lane never waits for another's store: a slot holds 0 or, for good, one value
//   k_vp8l_pal_sort    one wave per candidate: the table's values ascending by rank (the palette is defined by value, never by who inserted first), the palette's
//                      sub-image (entry minus predecessor) and its counts
//   k_vp8l_pal_index   one lane per packed pixel: binary search over the palette in LDS, the indices bundled lowest position in the lowest bits
//   k_vp8l_pal_choose  one wave per candidate, behind k_vp8l_refs_codes: the exact bits of the three streams; pick leaves one writer
#include "vp8l_pack.h"

namespace csw {

__device__ __forceinline__ static uint32_t vp8l_argb(const Vp8lImg &im, uint64_t i) {   // pixel i as the coder forms it, before subtract-green (k_vp8l_enc.hip sg_pixel)
    const uint32_t pick = im.channels >= VP8L_ALPHA_OF ? im.channels - VP8L_ALPHA_OF : 0u, nc = pick ? pick : im.channels;
    const uint8_t *p = im.rgb + i * nc;
    if (pick) return 0xFF000000u | (uint32_t(p[nc - 1]) * 0x010101u);
    if (nc <= 2) return (nc == 2 ? uint32_t(p[1]) << 24 : 0xFF000000u) | (uint32_t(p[0]) * 0x010101u);
    return (nc == 4 ? uint32_t(p[3]) << 24 : 0xFF000000u) | (uint32_t(p[0]) << 16) | (uint32_t(p[1]) << 8) | p[2];
}

// v into an open-addressed table of VP8L_PAL_SLOTS entries: 1 = it is new, 0 = it was there, 2 = the table is full.  At most VP8L_PAL_SLOTS probes.
// PEEK: look before the compare-and-swap (an entry never changes once it is set, so what a plain load sees is either final or empty)
template <bool PEEK>
__device__ __forceinline__ static uint32_t pal_insert(unsigned long long *t, uint32_t v) {
    const unsigned long long key = (1ull << 32) | v;
    uint32_t s = (v * 0x9E3779B1u) >> 22;
    static_assert(VP8L_PAL_SLOTS == 1u << 10, "the hash keeps ten bits");
    for (uint32_t k = 0; k < VP8L_PAL_SLOTS; k++, s = (s + 1u) & (VP8L_PAL_SLOTS - 1u)) {
        if (PEEK) { const unsigned long long cur = t[s]; if (cur == key) return 0u; if (cur) continue; }
        const unsigned long long old = atomicCAS(&t[s], 0ull, key);
        if (!old) return 1u;
        if (old == key) return 0u;
    }
    return 2u;
}

struct PalCountLds { unsigned long long t[VP8L_PAL_SLOTS]; };

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_pal_count(const Vp8lImg *imgs, unsigned long long *tabs, uint32_t *count) {
    CSH_SHARED PalCountLds S;
    const Vp8lImg im = imgs[blockIdx.y];
    const uint64_t N = uint64_t(im.width) * im.height, start = uint64_t(blockIdx.x) * VP8L_PAL_STRIP, end = N - start < VP8L_PAL_STRIP ? N : start + VP8L_PAL_STRIP;
    if (start >= N) return;
    if (csp::coherent_load(&count[blockIdx.y]) > VP8L_PAL_MAX) return;   // another strip has seen too many already
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_PAL_SLOTS; i += 64) S.t[i] = 0;
    CSP_WAVE_SYNC();
    uint32_t n = 0;   // the strip's distinct values so far (wave-uniform); at most VP8L_PAL_MAX + 64 enter the table, so it never fills
    for (uint64_t g0 = start; g0 < end && n <= VP8L_PAL_MAX; g0 += 64) {
        LV<uint32_t> r;
        LFOR(l) { const uint64_t p = g0 + uint32_t(l); r[l] = p < end ? pal_insert<true>(S.t, vp8l_argb(im, p)) : 0u; }
        n += uint32_t(__popcll(static_cast<unsigned long long>(csp::lballot([&](int l) { return r[l] == 1u; }))));
        if (csp::lballot([&](int l) { return r[l] == 2u; })) n = VP8L_PAL_MAX + 1;
    }
    CSP_WAVE_SYNC();
    if (n > VP8L_PAL_MAX) { LFOR(l) if (l == 0) atomicAdd(&count[blockIdx.y], VP8L_PAL_MAX + 1u); return; }
    // the strip's values into the picture's table: the count grows by what is new there.  A full table (other strips brought more than 1024 values) counts as too many
    unsigned long long *tab = tabs + uint64_t(blockIdx.y) * VP8L_PAL_SLOTS;
    LV<uint64_t> add;
    LFOR(l) {
        add[l] = 0;
        for (uint32_t i = uint32_t(l); i < VP8L_PAL_SLOTS; i += 64) {
            const unsigned long long e = S.t[i];
            if (!e) continue;
            const uint32_t r = pal_insert<false>(tab, uint32_t(e));
            add[l] += r == 1u ? 1u : r == 2u ? VP8L_PAL_MAX + 1u : 0u;
        }
    }
    const uint64_t total = csp::lsum(add);
    LFOR(l) if (l == 0 && total) atomicAdd(&count[blockIdx.y], uint32_t(total));
}

struct PalSortLds { uint32_t v[VP8L_PAL_MAX], s[VP8L_PAL_MAX], n, h[VP8L_PAL_HIST]; };

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_pal_sort(const Vp8lImg *imgs, int nparent, const unsigned long long *tabs, uint32_t *pal) {
    CSH_SHARED PalSortLds S;
    const Vp8lImg im = imgs[nparent + int(blockIdx.x)];
    const unsigned long long *tab = tabs + uint64_t(im.parent) * VP8L_PAL_SLOTS;
    uint32_t *out = pal + uint64_t(blockIdx.x) * VP8L_PAL_BLOCK;   // = im.pal
    LFOR(l) { if (l == 0) S.n = 0; for (uint32_t i = uint32_t(l); i < VP8L_PAL_HIST; i += 64) S.h[i] = 0; }
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_PAL_SLOTS; i += 64) {
        const unsigned long long e = tab[i];
        if (!e) continue;
        const uint32_t k = atomicAdd(&S.n, 1u);   // any order: the ranks below put them in place
        if (k < VP8L_PAL_MAX) S.v[k] = uint32_t(e);
    }
    CSP_WAVE_SYNC();
    const uint32_t n = S.n < im.pal_n ? S.n : im.pal_n;   // (equal: the host made the record from this table's count)
    LFOR(l) for (uint32_t i = uint32_t(l); i < n; i += 64) {
        const uint32_t me = S.v[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; j++) rank += S.v[j] < me ? 1u : 0u;   // the values are distinct
        S.s[rank] = me;
    }
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_PAL_MAX; i += 64) {
        const uint32_t cur = i < n ? S.s[i] : 0u, d = i < n ? lsub(cur, i ? S.s[i - 1] : 0u) : 0u;
        out[i] = cur; out[256 + i] = d;
        if (i >= n) continue;
        atomicAdd(&S.h[(d >> 8) & 255u], 1u); atomicAdd(&S.h[288 + ((d >> 16) & 255u)], 1u); atomicAdd(&S.h[288 + 256 + (d & 255u)], 1u); atomicAdd(&S.h[288 + 512 + (d >> 24)], 1u);
    }
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_PAL_HIST; i += 64) out[512 + i] = S.h[i];
}

// the candidate's pixels: per packed pixel 1 << bits indices of 8 >> bits bits each, the row's last one filled with zero bits
__global__ void __launch_bounds__(256) k_vp8l_pal_index(const Vp8lImg *imgs, int nparent, uint32_t *work) {
    CSH_SHARED uint32_t sp[VP8L_PAL_MAX];
    const Vp8lImg &im = imgs[nparent + int(blockIdx.y)];
    const uint32_t N = im.width * im.height, i0 = blockIdx.x * VP8L_CHUNK;
    const uint32_t bits = vp8l_pal_bits(im.pal_n), per = 1u << bits, each = 8u >> bits;
    CSH_PHASE_LOOP(2) {
        if (i0 >= N) continue;
        if (phase == 0) { if (threadIdx.x < VP8L_PAL_MAX) sp[threadIdx.x] = threadIdx.x < im.pal_n ? im.pal[threadIdx.x] : 0xFFFFFFFFu; continue; }
        for (uint32_t k = threadIdx.x; k < VP8L_CHUNK; k += 256) {
            const uint32_t i = i0 + k;
            if (i >= N) break;
            const uint32_t y = i / im.width, xp = i - y * im.width;
            uint32_t g = 0;
            for (uint32_t j = 0; j < per; j++) {
                const uint32_t x = xp * per + j;
                if (x >= im.src_width) break;
                const uint32_t v = vp8l_argb(im, uint64_t(y) * im.src_width + x);
                uint32_t lo = 0;   // the last entry <= v: v itself
                for (uint32_t step = VP8L_PAL_MAX / 2; step; step >>= 1) if (lo + step < im.pal_n && sp[lo + step] <= v) lo += step;
                g |= lo << (j * each);
            }
            work[im.res_off + i] = 0xFF000000u | (g << 8);
        }
    }
}

struct PalChooseLds { Vp8lPalCodes pal; uint32_t mh[288]; uint8_t mlen[288]; };

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_pal_choose(const Vp8lImg *imgs, int nparent, const uint8_t *modes, uint32_t *pick) {
    CSH_SHARED PalChooseLds S;
    const uint32_t c = uint32_t(nparent) + blockIdx.x;
    const Vp8lImg im = imgs[c], par = imgs[im.parent];
    // the picture's head behind the sizes, as Vp8lPut::head writes it: two transforms (3 + 6), the mode image ("no cache", its code, four codes of one symbol, the
    // modes), "no further transform"
    const uint32_t nblk = par.bw * par.bh;
    LFOR(l) for (int i = l; i < 288; i += 64) S.mh[i] = 0;
    CSP_WAVE_SYNC();
    for (uint32_t b0 = 0; b0 < nblk; b0 += 64) LFOR(l) if (b0 + uint32_t(l) < nblk) atomicAdd(&S.mh[modes[par.mode_off + b0 + uint32_t(l)]], 1u);
    CSP_WAVE_SYNC();
    vp8l_pal_codes(im.pal + 512, S.pal);
    LFOR(l) if (l == 0) {
        csp::code_lengths(S.mh, 280, 15, S.mlen);
        const Vp8lCodeUse u = vp8l_code_use([&](int i) { return S.mh[i]; }, 280);
        unsigned long long head = 3u + 6u + 1u + vp8l_code_desc_bits(u) + 16u + 1u;
        if (u.nused > 1) for (int i = 0; i < 280; i++) head += static_cast<unsigned long long>(S.mh[i]) * S.mlen[i];
        const uint32_t *pp = pick + 4 * im.parent, *pc = pick + 4 * c;
        const unsigned long long mine = head + (pp[0] ? pp[2] : pp[3]);
        const unsigned long long cand = vp8l_pal_head_bits(S.pal) + (pc[0] ? pc[2] : pc[3]);
        // a tie goes to the stream that exists without the palette
        if (cand < mine) pick[4 * im.parent] = 2u; else pick[4 * c] = 2u;
    }
}

void launch_vp8l_pal_count(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, unsigned long long *tabs, uint32_t *count) {
    if (!nimg) return;
    CSH_LAUNCH(k_vp8l_pal_count, dim3(unsigned((max_pixels + VP8L_PAL_STRIP - 1) / VP8L_PAL_STRIP), unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, tabs, count);
}

// max_tiles != 0: CSH_VP8L=groups; far: CSH_VP8L=far
static void encode_palette(hipStream_t st, const Vp8lImg *imgs, int nparent, int ncand, uint32_t max_blocks, uint64_t max_pixels, uint64_t max_packed, uint32_t max_tiles,
                           const unsigned long long *tabs, uint32_t *pal, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &R, const Vp8lFar *far, uint8_t *out, uint32_t *file_len,
                           uint32_t *status) {
    const int nimg = nparent + ncand;
    if (!nimg) return;
    if (ncand) {
        CSH_LAUNCH(k_vp8l_pal_sort, dim3(unsigned(ncand)), dim3(CSP_WAVE_THREADS), st, imgs, nparent, tabs, pal);
        CSH_LAUNCH_PHASED(k_vp8l_pal_index, 2, dim3(unsigned((max_packed + VP8L_CHUNK - 1) / VP8L_CHUNK), unsigned(ncand)), dim3(256), st, imgs, nparent, work);
    }
    launch_vp8l_refs_stages(st, imgs, nimg, max_blocks, max_pixels, work, modes, hist, R);
    if (max_tiles) launch_vp8l_group_stages(st, imgs, nparent, max_tiles, work, R);   // in front of the palette's choice: it compares with the picture's best
    if (far) launch_vp8l_far_stages(st, imgs, nparent, nimg, max_pixels, max_tiles, work, hist, R, *far);   // every record's better token set, in the first set's pools
    if (ncand) CSH_LAUNCH(k_vp8l_pal_choose, dim3(unsigned(ncand)), dim3(CSP_WAVE_THREADS), st, imgs, nparent, modes, R.pick);
    launch_vp8l_refs_packs(st, imgs, nimg, work, modes, hist, R, out, file_len, status);
    launch_vp8l_pack_candidates(st, imgs, nparent, nimg, work, modes, hist, R.pick, out, file_len, status);
    if (max_tiles) launch_vp8l_pack_groups(st, imgs, nparent, work, modes, R, out, file_len, status);
}
void launch_vp8l_encode_palette(hipStream_t st, const Vp8lImg *imgs, int nparent, int ncand, uint32_t max_blocks, uint64_t max_pixels, uint64_t max_packed, const unsigned long long *tabs,
                                uint32_t *pal, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &R, uint8_t *out, uint32_t *file_len, uint32_t *status) {
    encode_palette(st, imgs, nparent, ncand, max_blocks, max_pixels, max_packed, 0u, tabs, pal, work, modes, hist, R, nullptr, out, file_len, status);
}
void launch_vp8l_encode_groups(hipStream_t st, const Vp8lImg *imgs, int nparent, int ncand, uint32_t max_blocks, uint64_t max_pixels, uint64_t max_packed, uint32_t max_tiles,
                               const unsigned long long *tabs, uint32_t *pal, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &R, uint8_t *out, uint32_t *file_len, uint32_t *status) {
    encode_palette(st, imgs, nparent, ncand, max_blocks, max_pixels, max_packed, max_tiles, tabs, pal, work, modes, hist, R, nullptr, out, file_len, status);
}
void launch_vp8l_encode_far(hipStream_t st, const Vp8lImg *imgs, int nparent, int ncand, uint32_t max_blocks, uint64_t max_pixels, uint64_t max_packed, uint32_t max_tiles,
                            const unsigned long long *tabs, uint32_t *pal, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &R, const Vp8lFar &far, uint8_t *out, uint32_t *file_len,
                            uint32_t *status) {
    encode_palette(st, imgs, nparent, ncand, max_blocks, max_pixels, max_packed, max_tiles, tabs, pal, work, modes, hist, R, &far, out, file_len, status);
}

}  // namespace csw
