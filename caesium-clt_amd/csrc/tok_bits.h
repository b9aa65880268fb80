// tok_bits.h -- tokens -> bits: THE statement of what a token puts into the stream.  Shared by the token packer (k_entropy.hip k_pack) and by the packer of the
// refinement scans coded from the lists (k_aclist.hip k_list_refine_pack), whose token words live in an LDS buffer of the wave for one step and never reach the pool.
// A token is one u32; bits 0-2 are its kind (kernels.h TK_*), the fields of every kind are read below and nowhere else.
#pragma once
#include "kernels.h"

namespace csh {

// What one token puts into the stream: at most three pieces of at most 32 bits, in order (piece i: the n[i] low bits of v[i]).
struct Pieces { uint32_t v[3], n[3]; };
struct TokenCtx {                 // what the packer kernels know about the slot their tokens belong to
    const uint32_t *lut;          // the scan's tables: lut[t * lut_stride + s] = size << 16 | code   (DevEncTable::lut in HBM, or its copy in LDS)
    uint32_t lut_stride;
    const uint16_t *eobrun;       // of the chunk's units
    const uint64_t *corr;         // of the chunk's units (refinement scans)
};
#define CSH_LUT_STRIDE uint32_t(sizeof(DevEncTable) / 4)
__device__ __forceinline__ static void corr_pieces(Pieces &p, uint64_t corr, uint32_t t) {
    const uint32_t cnt = (t >> 16) & 63u, cur = (t >> 22) & 63u;
    if (!cnt) return;
    const uint64_t bits = (corr << cur) >> (64u - cnt);   // cnt >= 1, cur + cnt <= 63
    if (cnt > 32) { p.v[1] = uint32_t(bits >> 32); p.n[1] = cnt - 32; p.v[2] = uint32_t(bits); p.n[2] = 32; }
    else { p.v[2] = uint32_t(bits); p.n[2] = cnt; }
}
// A refinement scan's alphabet is 32 symbols -- EOB0 .. EOB14 (n << 4), ZRL (0xF0), and (r << 4) | 1 for r = 0 .. 15 -- so a packer that meets nothing else may
// stage those 32 codes alone (REF32: x.lut is then that table, 128 bytes instead of 1 KB): symbol s stands at ref_code_index(s) -- EOBn at n, ZRL at 15, run r at 16 + r
#define CSH_REF_CODES 32
__device__ __forceinline__ static uint32_t ref_code_index(uint32_t s) { return (s >> 4) | ((s & 1u) << 4); }
template <bool REF32>
__device__ __forceinline__ static uint32_t ref_code(const TokenCtx &x, uint32_t s) { return x.lut[REF32 ? ref_code_index(s) : s]; }
// MODE names what the scan's tokens can be, so that a wave does not walk through the code of kinds it cannot meet:
// 0 anything, 1 first-pass AC scan (ACF, EOB), 2 refinement scan (REF, EOB, empty RAW), 3 DC or sequential-mode scan (SYM, RAW)
// REF32 (MODE 2 only): the look-ups of the REF and EOB tokens go through the 32-entry table above
template <int MODE = 0, bool REF32 = false>
__device__ __forceinline__ static Pieces token_pieces(uint32_t t, const TokenCtx &x) {
    static_assert(!REF32 || MODE == 2, "the 32-entry table holds a refinement scan's codes only");
    Pieces p;
    p.v[0] = p.v[1] = p.v[2] = 0; p.n[0] = p.n[1] = p.n[2] = 0;
    uint32_t kind = t & 7u;
    if (MODE == 1) { if (kind == TK_RAW) return p; kind = kind == TK_ACF ? uint32_t(TK_ACF) : uint32_t(TK_EOB); }   // RAW: the empty token behind a segment's end
    if (MODE == 2) { if (kind == TK_RAW) return p; kind = kind == TK_REF ? uint32_t(TK_REF) : uint32_t(TK_EOB); }
    if (MODE == 3) kind = kind == TK_SYM ? uint32_t(TK_SYM) : uint32_t(TK_RAW);
    if (kind == TK_SYM) {
        const uint32_t e = x.lut[((t >> 11) & 3u) * x.lut_stride + ((t >> 3) & 255u)], nr = (t >> 13) & 15u;
        p.v[0] = ((e & 0xFFFFu) << nr) | (t >> 17); p.n[0] = (e >> 16) + nr;            // <= 16 + 15 bits
    } else if (kind == TK_RAW) { p.v[0] = t >> 17; p.n[0] = (t >> 13) & 15u; }
    else if (kind == TK_ACF) {
        const uint32_t r = (t >> 3) & 63u, nb = (t >> 9) & 15u, zr = r >> 4;
        if (zr) {
            const uint32_t z = x.lut[0xF0], zc = z & 0xFFFFu, zl = z >> 16;
            p.v[0] = zc; p.n[0] = zl;
            if (zr > 1) { p.v[0] = (zc << zl) | zc; p.n[0] = 2 * zl; }
            if (zr > 2) { p.v[1] = zc; p.n[1] = zl; }
        }
        const uint32_t e = x.lut[((r & 15u) << 4) | nb];
        p.v[2] = ((e & 0xFFFFu) << nb) | ((t >> 13) & 0xFFFFu); p.n[2] = (e >> 16) + nb;   // <= 16 + 15 bits
    } else if (kind == TK_REF) {
        const uint32_t unit = (t >> 3) & 255u;
        if (t & (1u << 28)) { const uint32_t e = ref_code<REF32>(x, 0xF0u); p.v[0] = e & 0xFFFFu; p.n[0] = e >> 16; }
        else { const uint32_t e = ref_code<REF32>(x, (((t >> 11) & 15u) << 4) | 1u); p.v[0] = ((e & 0xFFFFu) << 1) | ((t >> 15) & 1u); p.n[0] = (e >> 16) + 1; }
        if ((t >> 16) & 63u) corr_pieces(p, x.corr[unit], t);
    } else {   // TK_EOB
        const uint32_t unit = (t >> 3) & 255u;
        const uint32_t run = x.eobrun[unit];
        if (run) {
            const uint32_t nb = 31u - uint32_t(__clz(run));
            const uint32_t e = ref_code<REF32>(x, nb << 4);
            p.v[0] = ((e & 0xFFFFu) << nb) | (run & ((1u << nb) - 1u)); p.n[0] = (e >> 16) + nb;   // <= 16 + 14 bits
        }
        if ((t >> 16) & 63u) corr_pieces(p, x.corr[unit], t);
    }
    return p;
}
// the common case of token_pieces: everything a token emits fits ONE piece of at most 32 bits (no ZRL in front of a first-pass coefficient,
// symbol + sign + correction bits of a refinement event within 32 bits).  Returns false when it does not: the caller then takes the
// three-piece form for the whole step.
template <int MODE, bool REF32 = false>
__device__ __forceinline__ static bool token_main(uint32_t t, const TokenCtx &x, uint32_t &v, uint32_t &n) {
    static_assert(!REF32 || MODE == 2, "the 32-entry table holds a refinement scan's codes only");
    v = 0; n = 0;
    const uint32_t kind = t & 7u;
    if (kind == TK_RAW) { v = t >> 17; n = (t >> 13) & 15u; return true; }
    if (MODE == 3) {   // SYM
        const uint32_t e = x.lut[((t >> 11) & 3u) * x.lut_stride + ((t >> 3) & 255u)], nr = (t >> 13) & 15u;
        v = ((e & 0xFFFFu) << nr) | (t >> 17); n = (e >> 16) + nr;
        return true;
    }
    if (MODE == 1 && kind == TK_ACF) {
        const uint32_t r = (t >> 3) & 63u, nb = (t >> 9) & 15u;
        if (r >> 4) return false;
        const uint32_t e = x.lut[(r << 4) | nb];
        v = ((e & 0xFFFFu) << nb) | ((t >> 13) & 0xFFFFu); n = (e >> 16) + nb;
        return true;
    }
    const uint32_t unit = (t >> 3) & 255u, cnt = (t >> 16) & 63u, cur = (t >> 22) & 63u;
    if (MODE == 2 && kind == TK_REF) {
        if (t & (1u << 28)) { const uint32_t e = ref_code<REF32>(x, 0xF0u); v = e & 0xFFFFu; n = e >> 16; }
        else { const uint32_t e = ref_code<REF32>(x, (((t >> 11) & 15u) << 4) | 1u); v = ((e & 0xFFFFu) << 1) | ((t >> 15) & 1u); n = (e >> 16) + 1; }
    } else {   // EOB
        const uint32_t run = x.eobrun[unit];
        if (run) {
            const uint32_t nb = 31u - uint32_t(__clz(run));
            const uint32_t e = ref_code<REF32>(x, nb << 4);
            v = ((e & 0xFFFFu) << nb) | (run & ((1u << nb) - 1u)); n = (e >> 16) + nb;
        }
    }
    if (MODE == 2 && cnt) {
        if (n + cnt > 32) return false;
        const uint32_t bits = uint32_t((x.corr[unit] << cur) >> (64u - cnt));
        v = (n ? (v << cnt) : 0u) | bits; n += cnt;
    }
    return true;
}

}  // namespace csh
