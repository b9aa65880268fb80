// vp8l_refs.h -- what the kernels behind CSH_VP8L=refs share (k_vp8l_refs.hip: the stream with one set of codes; k_vp8l_groups.hip: the same tokens coded
// with a set of codes per group of tiles): lane helpers, the format's LZ77 numbers, the token word, the wide code construction and the cost unit.
#pragma once
#include "vp8l_pack.h"

namespace csw {

enum : uint32_t { VP8L_HASH_BITS = 12, VP8L_WARM = 3 * VP8L_CHUNK, VP8L_MIN_MATCH = 3 };
static_assert(VP8L_CHUNK % 64 == 0 && VP8L_WARM % VP8L_CHUNK == 0, "groups of 64 lanes never straddle a chunk");
#define VP8L_TOKEN (1ull << 63)   // a token starts here: bits 0-15 its length (1: one pixel), bits 16-47 the distance (0: no copy)

// ---- lanes
__device__ __forceinline__ static uint32_t lget(const LV<uint32_t> &x, int src) {   // lane src's value; src is wave-uniform
#ifdef CSH_EMUL
    return x.v[src];
#else
    return uint32_t(__builtin_amdgcn_readlane(int(x.v), __builtin_amdgcn_readfirstlane(src)));
#endif
}
__device__ __forceinline__ static LV<uint32_t> lshfl(const LV<uint32_t> &x, const LV<int> &src) {   // lane l gets lane src[l]'s value (src < 0: its own)
    LV<uint32_t> r;
#ifdef CSH_EMUL
    for (int j = 0; j < 64; j++) r.v[j] = x.v[src.v[j] < 0 ? j : src.v[j]];
#else
    r.v = uint32_t(__shfl(int(x.v), src.v < 0 ? int(threadIdx.x & 63u) : src.v, 64));
#endif
    return r;
}
// for every active lane the highest lower active lane with the same key, or -1: one round per distinct key
__device__ __forceinline__ static LV<int> lprev_same(const LV<uint32_t> &key, const LV<uint32_t> &active) {
    LV<int> prev;
    LFOR(l) prev[l] = -1;
    uint64_t rem = csp::lballot([&](int l) { return active[l] != 0; });
    while (rem) {
        const int leader = __ffsll(static_cast<unsigned long long>(rem)) - 1;
        const uint32_t k = lget(key, leader);
        const uint64_t m = csp::lballot([&](int l) { return active[l] != 0 && key[l] == k; });
        LFOR(l) if ((m >> l) & 1u) { const uint64_t below = m & csp::lanes_below(l); prev[l] = below ? 63 - __clzll(static_cast<unsigned long long>(below)) : -1; }
        rem &= ~m;
    }
    return prev;
}

// ---- the format's LZ77 numbers
// a length or a distance code v >= 1 -> prefix symbol, number of extra bits, their value
__device__ __forceinline__ static void vp8l_prefix(uint32_t v, uint32_t &sym, uint32_t &nextra, uint32_t &extra) {
    const uint32_t x = v - 1;
    if (x < 2) { sym = x; nextra = 0; extra = 0; return; }
    const uint32_t hb = 31u - uint32_t(__clz(x)), sb = (x >> (hb - 1)) & 1u;
    sym = 2 * hb + sb; nextra = hb - 1; extra = x & ((1u << nextra) - 1u);
}
__device__ __forceinline__ static uint32_t vp8l_prefix_extra(uint32_t sym) { return sym < 4 ? 0u : (sym - 2) >> 1; }
// the 120 short distance codes name positions (dx, dy) around the pixel, dy in 0..7, dx in -7..8, ordered by dx^2 + dy^2, then |dx|, then dx > 0 first (the
// specification's table); this is its inverse, indexed (dy << 4) | (8 - dx): the code minus one, 255 where there is none
struct Vp8lPlaneLut { uint8_t code[128]; };
constexpr Vp8lPlaneLut vp8l_make_plane_lut() {
    Vp8lPlaneLut t = {};
    for (int i = 0; i < 128; i++) t.code[i] = 255;
    int n = 0;
    for (int d2 = 1; d2 <= 113 && n < 120; d2++)
        for (int ax = 0; ax <= 8; ax++)
            for (int sgn = 0; sgn < 2; sgn++) {
                const int dx = sgn ? -ax : ax;
                if (sgn && ax == 0) continue;
                const int r = d2 - ax * ax;
                if (r < 0) continue;
                int dy = 0;
                while (dy * dy < r) dy++;
                if (dy * dy != r || dy > 7 || dx < -7 || dx > 8 || (dy == 0 && dx <= 0)) continue;
                t.code[(dy << 4) | (8 - dx)] = uint8_t(n++);
            }
    return t;
}
// pixel distance -> distance code (the nearer of the two positions that can name it; anything else is the distance plus 120)
__device__ __forceinline__ static uint32_t vp8l_dist_code(uint32_t dist, uint32_t width) {
    static constexpr Vp8lPlaneLut lut = vp8l_make_plane_lut();
    const uint32_t yo = dist / width, xo = dist - yo * width;
    if (xo <= 8 && yo < 8) return uint32_t(lut.code[yo * 16 + 8 - xo]) + 1u;
    if (xo + 8 > width && yo < 7) return uint32_t(lut.code[(yo + 1) * 16 + 8 + (width - xo)]) + 1u;
    return dist + 120u;
}
__device__ __forceinline__ static uint32_t vp8l_slot(uint32_t argb, uint32_t bits) { return (0x1E35A7BDu * argb) >> (32 - bits); }
__device__ __forceinline__ static uint32_t vp8l_state_off(uint32_t opt) { return opt == 1 ? 0u : opt == 2 ? 16u : 16u + 128u; }   // of option 1 .. 3 among VP8L_CACHE_STATE
__device__ __forceinline__ static uint32_t vp8l_hash3(uint32_t a, uint32_t b, uint32_t c) {
    return (((a * 0x9E3779B1u) ^ (b * 0x85EBCA6Bu) ^ (c * 0xC2B2AE35u)) * 0x27D4EB2Fu) >> (32 - VP8L_HASH_BITS);
}

// ---- codes
// png_codes.h code_lengths for an alphabet of up to VP8L_GREEN_MAX symbols: the same merges (the two least frequent, the larger index first on a tie; the merged
// tree in the first one's slot), the same limit by the bit-count adjustment, the same lengths -- with the arrays where the caller puts them (LDS)
struct CodeWs {
    unsigned long long heap[VP8L_GREEN_MAX];
    int16_t parent[2 * VP8L_GREEN_MAX], node_of_slot[VP8L_GREEN_MAX], idx[VP8L_GREEN_MAX], order[VP8L_GREEN_MAX];
    uint8_t depth[2 * VP8L_GREEN_MAX];
};
__device__ static void code_lengths_wide(const uint32_t *freq_in, int n, int limit, uint8_t *len_out, CodeWs &W) {
    int used = 0, m = 0;
    for (int i = 0; i < n; i++) used += freq_in[i] != 0;
    int forced = 2 - used;
    for (int i = 0; i < n; i++) {
        uint32_t f = freq_in[i];
        if (!f && forced > 0) { f = 1; forced--; }
        len_out[i] = 0;
        if (f) { W.heap[m] = (static_cast<unsigned long long>(f) << 16) | static_cast<unsigned long long>(0xFFFF - m); W.idx[m] = int16_t(i); W.node_of_slot[m] = int16_t(m); m++; }
    }
    auto sift_down = [&](int at, int size) {
        const unsigned long long v = W.heap[at];
        for (;;) {
            int ch = 2 * at + 1;
            if (ch >= size) break;
            if (ch + 1 < size && W.heap[ch + 1] < W.heap[ch]) ch++;
            if (W.heap[ch] >= v) break;
            W.heap[at] = W.heap[ch]; at = ch;
        }
        W.heap[at] = v;
    };
    for (int i = m / 2 - 1; i >= 0; i--) sift_down(i, m);
    int size = m, next = m;
    while (size > 1) {
        const unsigned long long k1 = W.heap[0];
        W.heap[0] = W.heap[--size]; sift_down(0, size);
        const unsigned long long k2 = W.heap[0];
        const int s1 = 0xFFFF - int(k1 & 0xFFFFu), s2 = 0xFFFF - int(k2 & 0xFFFFu);
        W.parent[W.node_of_slot[s1]] = int16_t(next); W.parent[W.node_of_slot[s2]] = int16_t(next);
        W.node_of_slot[s1] = int16_t(next++);
        W.heap[0] = (((k1 >> 16) + (k2 >> 16)) << 16) | (k1 & 0xFFFFu);
        sift_down(0, size);
    }
    W.depth[next - 1] = 0;
    for (int v = next - 2; v >= 0; v--) { const int d = W.depth[W.parent[v]] + 1; W.depth[v] = uint8_t(d > 63 ? 63 : d); }
    int bits[64], first[64];
    for (int i = 0; i < 64; i++) bits[i] = 0;
    for (int i = 0; i < m; i++) bits[W.depth[i]]++;
    { int at = 0; for (int cs = 0; cs < 64; cs++) { first[cs] = at; at += bits[cs]; } }
    for (int i = 63; i > limit; i--)
        while (bits[i] > 0) {
            int j = i - 2; while (bits[j] == 0) j--;
            bits[i] -= 2; bits[i - 1]++; bits[j + 1] += 2; bits[j]--;
        }
    for (int i = 0; i < m; i++) W.order[first[W.depth[i]]++] = int16_t(i);
    int l = 1;
    for (int r = 0; r < m; r++) { while (bits[l] == 0) l++; bits[l]--; len_out[W.idx[W.order[r]]] = uint8_t(l); }
}
__device__ __forceinline__ static uint32_t bits16(uint32_t c, uint64_t total) {   // 16 log2(total / c), c <= total
    const uint64_t q = (total << 8) / c;
    const uint32_t e = 63u - uint32_t(__clzll(static_cast<unsigned long long>(q)));
    return 16u * (e - 8u) + (uint32_t((q << 4) >> e) & 15u);
}
__device__ __forceinline__ static uint32_t vp8l_alphabet(int code, uint32_t opt) { return code == 0 ? 280u + (opt ? 1u << vp8l_cache_bits(opt) : 0u) : code == 4 ? 40u : 256u; }
__device__ __forceinline__ static uint32_t vp8l_hist_off(int code) { return code == 0 ? 0u : VP8L_GREEN_MAX + 256u * uint32_t(code - 1); }   // of a code's counts among VP8L_HIST

}  // namespace csw
