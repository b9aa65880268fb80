// vp8l_pack.h -- what the two pack kernels of the lossless WebP coder share (k_vp8l_enc.hip: literals only; k_vp8l_refs.hip: backward references and a
// colour cache): fields and prefix-code descriptions through the LDS bit window of png_codes.h, the stream's head up to the predictor's mode image, the
// RIFF framing.  One wave per picture.
#pragma once
#include "webp_kernels.h"
#include "png_codes.h"

namespace csw {

using csp::LV;

__device__ __forceinline__ static uint32_t lsub(uint32_t a, uint32_t b) {   // per-channel a - b mod 256
    return (((a | 0x00FF00FFu) - (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a | 0xFF00FF00u) - (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
__device__ __forceinline__ static uint32_t rev4(uint32_t v) { return ((v & 1u) << 3) | ((v & 2u) << 1) | ((v & 4u) >> 1) | ((v & 8u) >> 3); }

// one prefix code as the stream describes it: symbols with a non-zero count, the first two of them, the highest
struct Vp8lCodeUse { uint32_t nused, sym0, sym1, last; };
template <class F>
__device__ __forceinline__ static Vp8lCodeUse vp8l_code_use(F freq, int n) {
    Vp8lCodeUse u = {0, 0, 0, 0};
    for (int i = 0; i < n; i++) if (freq(i)) { if (u.nused == 0) u.sym0 = uint32_t(i); else if (u.nused == 1) u.sym1 = uint32_t(i); u.nused++; u.last = uint32_t(i); }
    return u;
}
// bits of a code's description (Vp8lPut::code)
__device__ __forceinline__ static uint32_t vp8l_code_desc_bits(const Vp8lCodeUse &u) {
    if (u.nused <= 2) return 3u + (u.sym0 > 1 ? 8u : 1u) + (u.nused == 2 ? 8u : 0u);
    return 1u + 4u + 42u + 15u + 14u + 4u * (u.last + 1u);
}

// ---- the description the refs coder writes: a real code-length code.  The lengths of an alphabet as code-length symbols: 0..15 a length, 16 repeats the last
// non-zero length (8 at the start) 3..6 times, 17 / 18 a run of 3..10 / 11..138 zeros; emit(symbol, value of its extra bits)
template <class F>
__device__ __forceinline__ static void vp8l_length_runs(const uint8_t *len, int n, F emit) {
    int prev = 8;
    for (int i = 0; i < n;) {
        const int v = len[i];
        int r = 1;
        while (i + r < n && len[i + r] == v) r++;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int k = r < 138 ? r : 138; emit(18u, uint32_t(k - 11)); r -= k; }
            if (r >= 3) { emit(17u, uint32_t(r - 3)); r = 0; }
            while (r-- > 0) emit(0u, 0u);
        } else {
            if (v != prev) { emit(uint32_t(v), 0u); r--; prev = v; }
            while (r >= 3) { const int k = r < 6 ? r : 6; emit(16u, uint32_t(k - 3)); r -= k; }
            while (r-- > 0) emit(uint32_t(v), 0u);
        }
    }
}
__device__ __forceinline__ static uint32_t vp8l_length_extra(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }
__device__ __forceinline__ static uint32_t vp8l_length_order(int i) {   // the order the stream lists the code-length code's own lengths in
    const uint8_t order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    return order[i];
}
struct Vp8lLengthCode { uint8_t cl[19]; uint16_t cc[19]; uint32_t ncl; };   // lengths (at most 7), codes, how many of the lengths are listed
__device__ __forceinline__ static bool vp8l_simple_code(const Vp8lCodeUse &u) { return u.nused <= 2 && u.last < 256; }   // (a simple code's symbols are 8-bit fields)
// the code-length code of all n lengths (the stream gives no count, so the zeros behind the last symbol in use are runs too); returns the description's bits
__device__ static uint32_t vp8l_length_code(const uint8_t *len, int n, Vp8lLengthCode &L) {
    uint32_t h[19], extra = 0;
    for (int i = 0; i < 19; i++) h[i] = 0;
    vp8l_length_runs(len, n, [&](uint32_t s, uint32_t) { h[s]++; extra += vp8l_length_extra(s); });
    csp::code_lengths(h, 19, 7, L.cl);
    csp::canonical(L.cl, 19, L.cc);
    L.ncl = 19;
    while (L.ncl > 4 && L.cl[vp8l_length_order(int(L.ncl) - 1)] == 0) L.ncl--;
    uint32_t bits = 1u + 4u + 3u * L.ncl + 1u + extra;
    for (int i = 0; i < 19; i++) bits += h[i] * L.cl[i];
    return bits;
}
__device__ __forceinline__ static uint32_t vp8l_refs_desc_bits(const uint8_t *len, int n, const Vp8lCodeUse &u) {
    if (vp8l_simple_code(u)) return vp8l_code_desc_bits(u);
    Vp8lLengthCode L;
    return vp8l_length_code(len, n, L);
}
struct Vp8lDescLds { Vp8lLengthCode L; uint32_t ntok; uint16_t tok[VP8L_GREEN_MAX]; };   // the pack kernel's room for one description: symbol | extra << 8

// ---- the palette's sub-image (CSH_VP8L=palette): its four codes from its counts (VP8L_PAL_HIST), one lane each, and the exact bits of its descriptions and pixels
struct Vp8lPalCodes { uint8_t len[4][288]; uint16_t code[4][288]; Vp8lCodeUse use[4]; uint32_t bits[4]; };
__device__ __forceinline__ static int vp8l_pal_alphabet(int c) { return c == 0 ? 280 : 256; }
__device__ __forceinline__ static void vp8l_pal_codes(const uint32_t *hist, Vp8lPalCodes &C) {
    LFOR(l) if (l < 4) {
        const int n = vp8l_pal_alphabet(l);
        const uint32_t *f = hist + (l == 0 ? 0 : 288 + 256 * (l - 1));
        csp::code_lengths(f, n, 15, C.len[l]);
        const Vp8lCodeUse u = vp8l_code_use([&](int i) { return f[i]; }, n);
        if (u.nused <= 1) for (int i = 0; i < n; i++) C.len[l][i] = 0;   // a code with one symbol costs no bits
        csp::canonical(C.len[l], n, C.code[l]);
        uint32_t b = vp8l_refs_desc_bits(C.len[l], n, u);
        for (int i = 0; i < n; i++) b += f[i] * C.len[l][i];
        C.use[l] = u; C.bits[l] = b;
    }
    CSP_WAVE_SYNC();
}
// bits of a candidate's head behind the sizes: the transform (1 + 2 + 8), the sub-image ("no cache", five descriptions, the entries), "no further transform"
__device__ __forceinline__ static uint32_t vp8l_pal_head_bits(const Vp8lPalCodes &C) { return 11u + 1u + C.bits[0] + C.bits[1] + C.bits[2] + C.bits[3] + 4u + 1u; }

struct Vp8lPut {
    csp::BitOut bo;
    __device__ __forceinline__ void begin(uint32_t *win, uint8_t *out) { bo.win = win; bo.out = out; bo.bitpos = 0; bo.wbase = 0; }
    __device__ __forceinline__ void put1(uint64_t v, uint32_t n) {   // one field, from the first lane
        LV<uint64_t> val; LV<uint32_t> nb;
        LFOR(l) { val[l] = l == 0 ? v : 0ull; nb[l] = l == 0 ? n : 0u; }
        bo.put(val, nb);
    }
    // a code with one or two symbols is written as such (8-bit symbol fields); any other the long way: the code-length code gives the lengths
    // 0..15 four bits each and the run-length symbols 16..18 none, the lengths are cut behind the last symbol in use
    __device__ __forceinline__ void code(const uint8_t *len, const Vp8lCodeUse &u) {
        if (u.nused <= 2) {
            const uint64_t two = u.nused == 2 ? 1 : 0, wide = u.sym0 > 1 ? 1 : 0;   // the first symbol's field is one bit wide when that is enough
            const uint32_t w0 = wide ? 8u : 1u;
            put1(1ull | (two << 1) | (wide << 2) | (uint64_t(u.sym0) << 3) | (two ? uint64_t(u.sym1) << (3 + w0) : 0ull), 3 + w0 + (two ? 8u : 0u));
            return;
        }
        put1(0, 1);          // not a simple code
        put1(15, 4);         // 19 code-length code lengths follow, in the format's order 17 18 0 1 2 3 4 5 16 6 .. 15
        put1((4ull << 6) | (4ull << 9) | (4ull << 12) | (4ull << 15) | (4ull << 18) | (4ull << 21) | (4ull << 27) | (4ull << 30) | (4ull << 33) | (4ull << 36) | (4ull << 39), 42);   // 14 of the 19
        put1(4ull | (4ull << 3) | (4ull << 6) | (4ull << 9) | (4ull << 12), 15);                                                                                                   // symbols 11 .. 15
        const int n = int(u.last) + 1;   // >= 3 here
        put1(1ull | (4ull << 1) | (uint64_t(n - 2) << 4), 14);   // the number of lengths that follow: a 10-bit field (2 + 2 * 4), holding n - 2
        for (int i0 = 0; i0 < n; i0 += 64) {
            LV<uint64_t> val; LV<uint32_t> nb;
            LFOR(l) { const int i = i0 + l; nb[l] = i < n ? 4u : 0u; val[l] = i < n ? rev4(len[i]) : 0u; }
            bo.put(val, nb);
        }
    }
    // the refs coder's description of a code over n symbols
    __device__ __forceinline__ void code_runs(const uint8_t *len, int n, const Vp8lCodeUse &u, Vp8lDescLds &D) {
        if (vp8l_simple_code(u)) { code(len, u); return; }
        LFOR(l) if (l == 0) {
            vp8l_length_code(len, n, D.L);
            uint32_t k = 0;
            vp8l_length_runs(len, n, [&](uint32_t s, uint32_t e) { D.tok[k++] = uint16_t(s | (e << 8)); });
            D.ntok = k;
        }
        CSP_WAVE_SYNC();
        put1(0ull | (uint64_t(D.L.ncl - 4) << 1), 5);   // not a simple code; the number of code-length code lengths
        {
            LV<uint64_t> val; LV<uint32_t> nb;
            LFOR(l) { const bool in = uint32_t(l) < D.L.ncl; nb[l] = in ? 3u : 0u; val[l] = in ? D.L.cl[vp8l_length_order(l)] : 0u; }
            bo.put(val, nb);
        }
        put1(0, 1);          // every length of the alphabet follows
        const uint32_t ntok = D.ntok;
        for (uint32_t i0 = 0; i0 < ntok; i0 += 64) {
            LV<uint64_t> val; LV<uint32_t> nb;
            LFOR(l) {
                const uint32_t i = i0 + uint32_t(l), t = i < ntok ? D.tok[i] : 0u, sym = t & 255u;
                nb[l] = i < ntok ? D.L.cl[sym] + vp8l_length_extra(sym) : 0u;
                val[l] = uint64_t(D.L.cc[sym]) | (uint64_t(t >> 8) << D.L.cl[sym]);
            }
            bo.put(val, nb);
        }
        CSP_WAVE_SYNC();
    }
    __device__ __forceinline__ void single() { put1(1 | (0 << 1) | (0 << 2) | (0 << 3), 4); }   // simple code, one symbol, 1-bit symbol field, symbol 0
    // signature, sizes, the two transforms with the predictor's mode image (its code: mlen / mcode / mu), "no further transform"
    __device__ __forceinline__ void head(const Vp8lImg &im, const uint8_t *modes, const uint8_t *mlen, const uint16_t *mcode, const Vp8lCodeUse &mu) {
        const uint32_t nblk = im.bw * im.bh;
        put1(0x2F, 8);
        const bool has_alpha = im.channels == 2 || im.channels == 4;
        put1(uint64_t(im.width - 1) | (uint64_t(im.height - 1) << 14) | (uint64_t(has_alpha ? 1 : 0) << 28) | (0ull << 29), 32);   // sizes, alpha_is_used (a hint), version 0
        put1(1 | (2u << 1), 3);                      // a transform follows: subtract green
        put1(1 | (0u << 1) | (2u << 3), 6);          // a transform follows: predictor, block side 1 << (2 + 2)
        put1(0, 1);                                   // the mode image: no colour cache
        code(mlen, mu); single(); single(); single(); single();
        for (uint32_t b0 = 0; b0 < nblk; b0 += 64) {
            LV<uint64_t> val; LV<uint32_t> nb;
            LFOR(l) {
                const uint32_t b = b0 + uint32_t(l);
                const uint32_t m = b < nblk ? modes[im.mode_off + b] : 0u;
                nb[l] = b < nblk ? mlen[m] : 0u; val[l] = mcode[m];
            }
            bo.put(val, nb);
        }
        put1(0, 1);                                   // no further transform
    }
    // a candidate's head: signature, the PICTURE's sizes, the colour-indexing transform with its palette as a sub-image, "no further transform"
    __device__ __forceinline__ void head_palette(const Vp8lImg &im, const Vp8lPalCodes &C, Vp8lDescLds &D) {
        put1(0x2F, 8);
        const bool has_alpha = im.channels == 2 || im.channels == 4;
        put1(uint64_t(im.src_width - 1) | (uint64_t(im.height - 1) << 14) | (uint64_t(has_alpha ? 1 : 0) << 28) | (0ull << 29), 32);
        put1(1 | (3u << 1) | (uint64_t(im.pal_n - 1) << 3), 11);   // a transform follows: colour indexing, the number of colours minus one
        put1(0, 1);                                                 // the sub-image: no colour cache
        for (int c = 0; c < 4; c++) code_runs(C.len[c], vp8l_pal_alphabet(c), C.use[c], D);
        single();                                                   // green, red, blue, alpha, distance
        const uint32_t *sub = im.pal + 256;
        for (uint32_t i0 = 0; i0 < im.pal_n; i0 += 64) {
            LV<uint64_t> val; LV<uint32_t> nb;
            LFOR(l) {
                const uint32_t i = i0 + uint32_t(l), v = i < im.pal_n ? sub[i] : 0u;
                const uint32_t g = (v >> 8) & 255u, r = (v >> 16) & 255u, b = v & 255u, a = v >> 24;
                const uint32_t lg = C.len[0][g], lr = C.len[1][r], lb = C.len[2][b], la = C.len[3][a];
                nb[l] = i < im.pal_n ? lg + lr + lb + la : 0u;
                val[l] = uint64_t(C.code[0][g]) | (uint64_t(C.code[1][r]) << lg) | (uint64_t(C.code[2][b]) << (lg + lr)) | (uint64_t(C.code[3][a]) << (lg + lr + lb));
            }
            bo.put(val, nb);
        }
        put1(0, 1);                                                 // no further transform
    }
    // the last bits, then the RIFF framing in front of the payload (which starts at file + 20).  image: the picture's entry (a candidate's: its parent's)
    __device__ __forceinline__ void finish(const Vp8lImg &im, uint8_t *file, int image, uint32_t *file_len, uint32_t *status) {
        const uint64_t payload = (bo.bitpos + 7) >> 3;
        bo.finish();
        CSP_WAVE_SYNC();
        const uint64_t padded = payload + (payload & 1u), total = 20 + padded;
        LFOR(l) if (l == 0) {
            if (total > im.out_cap) { status[image] = 1; file_len[image] = 0; }
            else {
                if (payload & 1u) file[20 + payload] = 0;
                const uint8_t hd[20] = {'R', 'I', 'F', 'F', uint8_t(total - 8), uint8_t((total - 8) >> 8), uint8_t((total - 8) >> 16), uint8_t((total - 8) >> 24), 'W', 'E', 'B', 'P',
                                        'V', 'P', '8', 'L', uint8_t(payload), uint8_t(payload >> 8), uint8_t(payload >> 16), uint8_t(payload >> 24)};
                for (int k = 0; k < 20; k++) file[k] = hd[k];
                status[image] = 0; file_len[image] = uint32_t(total);
            }
        }
    }
};

}  // namespace csw
