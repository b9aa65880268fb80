// k_vp8l_groups.hip -- lossless WebP OUTPUT with the format's meta prefix (entropy) image (CSH_VP8L=groups).  The match finder, the parse and the
// cache stages of k_vp8l_refs.hip stay as they are: the same tokens are coded once more, with up to VP8L_MAX_GROUPS sets of five prefix codes instead of one.  The
// picture is cut into tiles of (1 << bits)^2 pixels, every tile names its set (its GROUP) in the entropy image, and a symbol is coded with the group of the tile
// that holds its position -- a copy with the group of its first pixel.  The grouped stream is one more candidate: it is written where it is strictly smaller than
// the picture's refs stream and its plain stream.
//   k_vp8l_tile_feat     one workgroup per tile: the tile's tokens as VP8L_TILE_FEAT folded counts (magnitude classes of the literals, cache hits, copies)
//   k_vp8l_tile_cluster  one wave per picture: k-means by coding cost over the folded counts, for 2, 4 and 8 groups; a model in the same unit keeps one of them
//   k_vp8l_group_hist    one workgroup per tile: the exact counts of k_vp8l_refs_hist for the chosen option, into the tile's group
//   k_vp8l_group_codes   one wave per (picture, group): five codes, the exact bits of their descriptions and symbols
//   k_vp8l_group_choose  one wave per picture: the exact bits of the grouped stream against pick's two
//   k_vp8l_pack_groups   one wave per picture: k_vp8l_pack_refs' walk with every lane's tables looked up from its position's tile
// Every count is a sum and every choice is made by value and index (a tie goes to the lower group), so no lane's or wave's order shows in the bytes.
#include "vp8l_refs.h"

namespace csw {

enum : uint32_t {
    VP8L_FEAT_CLASSES = 15,               // per literal channel: |v| = 0, 1, 2, 3, then two classes per power of two up to 128
    VP8L_FEAT_CACHE = 60, VP8L_FEAT_COPY = 61, VP8L_FEAT_USED = 62,
    VP8L_CLUSTER_ROUNDS = 6,
    VP8L_START_VALUES = 4096,             // 64 x the mean magnitude class of a tile's positions, 0 .. 64 x 4 x 14
    VP8L_GROUP_ALLOW = 16 * 2400,         // the model's price of one more group's five descriptions, in 1/16 bit
};

// a channel's residual -> its magnitude class: the distance from 0 mod 256, geometric above 4
__device__ __forceinline__ static uint32_t vp8l_fold(uint32_t v) {
    const uint32_t m = v < 128 ? v : 256 - v;
    if (m < 2) return m;
    const uint32_t hb = 31u - uint32_t(__clz(m));
    return 2 * hb + ((m >> (hb - 1)) & 1u);
}
// the prefix code a folded class belongs to: 0 green (with the cache hits and the copies), 1 red, 2 blue, 3 alpha, 4 none
__device__ __forceinline__ static uint32_t vp8l_feat_code(uint32_t c) { return c < 60 ? c / VP8L_FEAT_CLASSES : c < VP8L_FEAT_USED ? 0u : 4u; }

struct TileBox { uint32_t x0, y0, w, h; };
__device__ __forceinline__ static TileBox vp8l_tile_box(const Vp8lImg &im, const Vp8lGroupImg &G, uint32_t tile) {
    const uint32_t side = 1u << G.bits, ty = tile / G.tw, tx = tile - ty * G.tw;
    TileBox b;
    b.x0 = tx << G.bits; b.y0 = ty << G.bits;
    b.w = im.width - b.x0 < side ? im.width - b.x0 : side; b.h = im.height - b.y0 < side ? im.height - b.y0 : side;
    return b;
}

// ---- tile features: the tokens of the option k_vp8l_refs_codes chose
__global__ void __launch_bounds__(256) k_vp8l_tile_feat(const Vp8lImg *imgs, const Vp8lGroupImg *gimgs, const uint32_t *work, const uint64_t *toks, const uint8_t *hits, const uint32_t *pick,
                                                        uint32_t *feat) {
    CSH_SHARED uint32_t h[VP8L_TILE_FEAT];
    const Vp8lImg &im = imgs[blockIdx.y];
    const Vp8lGroupImg &G = gimgs[blockIdx.y];
    const uint32_t tile = blockIdx.x;
    CSH_PHASE_LOOP(3) {
        if (!G.bits || tile >= G.ntile) continue;
        if (phase == 0) { if (threadIdx.x < VP8L_TILE_FEAT) h[threadIdx.x] = 0; continue; }
        if (phase == 1) {
            const uint32_t opt = pick[4 * blockIdx.y + 1];
            const TileBox b = vp8l_tile_box(im, G, tile);
            for (uint32_t k = threadIdx.x; k < b.w * b.h; k += 256) {
                const uint32_t yy = k / b.w, i = (b.y0 + yy) * im.width + b.x0 + (k - yy * b.w);
                const uint64_t t = toks[im.tok_off + i];
                if (!(t & VP8L_TOKEN)) continue;
                if (uint32_t(t >> 16)) { atomicAdd(&h[VP8L_FEAT_COPY], 1u); continue; }
                if ((hits[im.hit_off + i] >> opt) & 1u) { atomicAdd(&h[VP8L_FEAT_CACHE], 1u); continue; }
                const uint32_t v = work[im.res_off + i];
                atomicAdd(&h[vp8l_fold((v >> 8) & 255u)], 1u); atomicAdd(&h[VP8L_FEAT_CLASSES + vp8l_fold((v >> 16) & 255u)], 1u);
                atomicAdd(&h[2 * VP8L_FEAT_CLASSES + vp8l_fold(v & 255u)], 1u); atomicAdd(&h[3 * VP8L_FEAT_CLASSES + vp8l_fold(v >> 24)], 1u);
            }
            continue;
        }
        if (threadIdx.x < VP8L_TILE_FEAT) feat[(G.tile_off + tile) * VP8L_TILE_FEAT + threadIdx.x] = h[threadIdx.x];
    }
}

// ---- clustering
struct ClusterLds {
    uint32_t bucket[VP8L_START_VALUES];   // tiles per start value, then the tiles with a smaller one
    uint16_t val[VP8L_MAX_TILES];
    uint8_t lab[VP8L_MAX_TILES], best[VP8L_MAX_TILES];
    uint32_t cent[VP8L_MAX_GROUPS][VP8L_TILE_FEAT], cost[VP8L_MAX_GROUPS][VP8L_TILE_FEAT], ntiles[VP8L_MAX_GROUPS], map[VP8L_MAX_GROUPS];
};
// the groups' summed counts and tile counts from the labels, then the price of every class in every group: 16 log2(the code's total / the class's count), an empty
// class priced as count 1
__device__ static void cluster_centroids(ClusterLds &S, const uint8_t *lab, const uint32_t *F, uint32_t nt, uint32_t K) {
    LFOR(l) { for (uint32_t i = uint32_t(l); i < VP8L_MAX_GROUPS * VP8L_TILE_FEAT; i += 64) (&S.cent[0][0])[i] = 0; if (l < int(VP8L_MAX_GROUPS)) S.ntiles[l] = 0; }
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) {
        const uint32_t g = lab[t];
        atomicAdd(&S.ntiles[g], 1u);
        for (uint32_t c = 0; c < VP8L_FEAT_USED; c++) { const uint32_t v = F[uint64_t(t) * VP8L_TILE_FEAT + c]; if (v) atomicAdd(&S.cent[g][c], v); }
    }
    CSP_WAVE_SYNC();
    for (uint32_t g = 0; g < K; g++) {   // lane = class
        uint64_t tot[4];
        for (uint32_t a = 0; a < 4; a++) {
            LV<uint64_t> x;
            LFOR(l) x[l] = vp8l_feat_code(uint32_t(l)) == a ? S.cent[g][l] : 0u;
            tot[a] = csp::lsum(x);
        }
        LFOR(l) {
            const uint32_t a = vp8l_feat_code(uint32_t(l));
            const uint64_t t = a == 0 ? tot[0] : a == 1 ? tot[1] : a == 2 ? tot[2] : tot[3];
            const uint32_t c = S.cent[g][l];
            S.cost[g][l] = a < 4 ? bits16(c ? c : 1u, t ? t : 1u) : 0u;
        }
    }
    CSP_WAVE_SYNC();
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_tile_cluster(const Vp8lImg *imgs, int nimg, const Vp8lGroupImg *gimgs, const uint32_t *feat, uint8_t *label, unsigned long long *ginfo) {
    CSH_SHARED ClusterLds S;
    const int image = blockIdx.x;
    if (image >= nimg) return;
    const Vp8lImg im = imgs[image];
    const Vp8lGroupImg G = gimgs[image];
    unsigned long long *info = ginfo + uint64_t(image) * VP8L_GROUP_INFO;
    if (!G.bits) { LFOR(l) if (l == 0) info[0] = 0; return; }
    const uint32_t *F = feat + G.tile_off * VP8L_TILE_FEAT;
    const uint32_t nt = G.ntile;
    // the start: the tiles ranked by their mean magnitude class per position and cut into K quantiles; tiles of one value share a group
    LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_START_VALUES; i += 64) S.bucket[i] = 0;
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) {
        const TileBox b = vp8l_tile_box(im, G, t);
        uint32_t s = 0;
        for (uint32_t c = 0; c < 60; c++) s += (c % VP8L_FEAT_CLASSES) * F[uint64_t(t) * VP8L_TILE_FEAT + c];
        const uint32_t v = uint32_t((uint64_t(s) * 64u) / (b.w * b.h));
        S.val[t] = uint16_t(v < VP8L_START_VALUES ? v : VP8L_START_VALUES - 1);
        atomicAdd(&S.bucket[S.val[t]], 1u);
    }
    CSP_WAVE_SYNC();
    {   // exclusive prefix: a lane owns 64 values
        LV<uint32_t> own;
        LFOR(l) { uint32_t s = 0; for (uint32_t j = 0; j < 64; j++) s += S.bucket[64 * uint32_t(l) + j]; own[l] = s; }
        uint32_t total;
        const LV<uint32_t> off = csp::lscan(own, total);
        LFOR(l) { uint32_t s = off[l]; for (uint32_t j = 0; j < 64; j++) { const uint32_t c = S.bucket[64 * uint32_t(l) + j]; S.bucket[64 * uint32_t(l) + j] = s; s += c; } }
    }
    CSP_WAVE_SYNC();
    unsigned long long best_cost = ~0ull;
    uint32_t best_k = 0;
    for (uint32_t K = 2, logk = 1; K <= VP8L_MAX_GROUPS && K <= nt; K *= 2, logk++) {
        LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) S.lab[t] = uint8_t((uint64_t(S.bucket[S.val[t]]) * K) / nt);
        CSP_WAVE_SYNC();
        for (uint32_t round = 0;; round++) {
            cluster_centroids(S, S.lab, F, nt, K);
            if (round == VP8L_CLUSTER_ROUNDS) break;
            // a tile goes to the group that codes it in the fewest bits; a group without tiles takes none
            LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) {
                unsigned long long s[VP8L_MAX_GROUPS];
                for (uint32_t g = 0; g < VP8L_MAX_GROUPS; g++) s[g] = 0;
                for (uint32_t c = 0; c < VP8L_FEAT_USED; c++) {
                    const unsigned long long v = F[uint64_t(t) * VP8L_TILE_FEAT + c];
                    if (!v) continue;
                    CSH_UNROLL
                    for (uint32_t g = 0; g < VP8L_MAX_GROUPS; g++) s[g] += v * S.cost[g][c];
                }
                unsigned long long lo = ~0ull;
                uint32_t at = 0;
                CSH_UNROLL
                for (uint32_t g = 0; g < VP8L_MAX_GROUPS; g++) if (g < K && S.ntiles[g] && s[g] < lo) { lo = s[g]; at = g; }
                S.lab[t] = uint8_t(at);
            }
            CSP_WAVE_SYNC();
        }
        // the model: the groups' counts at their own prices, an allowance per group in use, the entropy image at log2 K bits per tile
        LV<uint64_t> part;
        LFOR(l) { part[l] = 0; for (uint32_t g = 0; g < K; g++) part[l] += uint64_t(S.cent[g][l]) * S.cost[g][l]; if (uint32_t(l) < K && S.ntiles[l]) part[l] += VP8L_GROUP_ALLOW; }
        const unsigned long long model = csp::lsum(part) + 16ull * logk * nt;
        if (model < best_cost) {   // a tie keeps the fewer groups
            best_cost = model; best_k = K;
            LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) S.best[t] = S.lab[t];
        }
        CSP_WAVE_SYNC();
    }
    // the groups in use, renumbered densely in their order
    LFOR(l) if (l < int(VP8L_MAX_GROUPS)) S.ntiles[l] = 0;
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) atomicAdd(&S.ntiles[S.best[t]], 1u);
    CSP_WAVE_SYNC();
    uint32_t ng = 0;
    for (uint32_t g = 0; g < VP8L_MAX_GROUPS; g++) ng += g < best_k && S.ntiles[g] ? 1u : 0u;
    LFOR(l) if (l < int(VP8L_MAX_GROUPS)) { uint32_t m = 0; for (int g = 0; g < l; g++) m += S.ntiles[g] ? 1u : 0u; S.map[l] = m; }
    CSP_WAVE_SYNC();
    if (ng < 2) ng = 0;
    if (ng) LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) label[G.tile_off + t] = uint8_t(S.map[S.best[t]]);
    LFOR(l) if (l == 0) info[0] = ng;
}

// ---- the exact counts, per group: the events of k_vp8l_refs_hist for the chosen option, a tile's all into its group
__global__ void __launch_bounds__(256) k_vp8l_group_hist(const Vp8lImg *imgs, const Vp8lGroupImg *gimgs, const uint32_t *work, const uint64_t *toks, const uint8_t *hits, const uint32_t *pick,
                                                         const uint8_t *label, const unsigned long long *ginfo, uint32_t *ghist) {
    CSH_SHARED uint32_t h[VP8L_HIST];
    const Vp8lImg &im = imgs[blockIdx.y];
    const Vp8lGroupImg &G = gimgs[blockIdx.y];
    const uint32_t tile = blockIdx.x;
    CSH_PHASE_LOOP(3) {
        if (!G.bits || tile >= G.ntile || !ginfo[uint64_t(blockIdx.y) * VP8L_GROUP_INFO]) continue;
        if (phase == 0) { for (uint32_t i = threadIdx.x; i < VP8L_HIST; i += 256) h[i] = 0; continue; }
        if (phase == 1) {
            const uint32_t opt = pick[4 * blockIdx.y + 1];
            const TileBox b = vp8l_tile_box(im, G, tile);
            for (uint32_t k = threadIdx.x; k < b.w * b.h; k += 256) {
                const uint32_t yy = k / b.w, i = (b.y0 + yy) * im.width + b.x0 + (k - yy * b.w);
                const uint64_t t = toks[im.tok_off + i];
                if (!(t & VP8L_TOKEN)) continue;
                const uint32_t dist = uint32_t(t >> 16);
                if (dist) {
                    uint32_t ls, ds, ne, ex;
                    vp8l_prefix(uint32_t(t) & 0xFFFFu, ls, ne, ex);
                    vp8l_prefix(vp8l_dist_code(dist, im.width), ds, ne, ex);
                    atomicAdd(&h[256 + ls], 1u); atomicAdd(&h[VP8L_GREEN_MAX + 768 + ds], 1u);
                    continue;
                }
                const uint32_t v = work[im.res_off + i];
                if ((hits[im.hit_off + i] >> opt) & 1u) { atomicAdd(&h[280 + vp8l_slot(v, vp8l_cache_bits(opt))], 1u); continue; }
                atomicAdd(&h[(v >> 8) & 255u], 1u); atomicAdd(&h[VP8L_GREEN_MAX + ((v >> 16) & 255u)], 1u);
                atomicAdd(&h[VP8L_GREEN_MAX + 256 + (v & 255u)], 1u); atomicAdd(&h[VP8L_GREEN_MAX + 512 + (v >> 24)], 1u);
            }
            continue;
        }
        uint32_t *out = ghist + (uint64_t(blockIdx.y) * VP8L_MAX_GROUPS + label[G.tile_off + tile]) * VP8L_HIST;
        for (uint32_t i = threadIdx.x; i < VP8L_HIST; i += 256) if (h[i]) atomicAdd(&out[i], h[i]);
    }
}

// ---- a group's five codes, as k_vp8l_refs_codes makes the picture's
struct GroupCodesLds {
    CodeWs ws;
    uint8_t len[5][288];
    uint8_t glen[VP8L_GREEN_MAX];
    unsigned long long bits[5];
};
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_group_codes(const uint32_t *pick, const uint32_t *ghist, uint8_t *glens, unsigned long long *ginfo) {
    CSH_SHARED GroupCodesLds S;
    const uint32_t g = blockIdx.x, image = blockIdx.y;
    unsigned long long *info = ginfo + uint64_t(image) * VP8L_GROUP_INFO;
    if (g >= info[0]) return;
    const uint32_t opt = pick[4 * image + 1];
    const uint32_t *hc = ghist + (uint64_t(image) * VP8L_MAX_GROUPS + g) * VP8L_HIST;
    LFOR(l) if (l < 5) {
        const uint32_t n = vp8l_alphabet(l, opt);
        const uint32_t *f = hc + vp8l_hist_off(l);
        uint8_t *len = l == 0 ? S.glen : S.len[l];
        if (l == 0) code_lengths_wide(f, int(n), 15, len, S.ws); else csp::code_lengths(f, int(n), 15, len);
        const Vp8lCodeUse u = vp8l_code_use([&](int i) { return f[i]; }, int(n));
        if (u.nused <= 1) for (uint32_t i = 0; i < n; i++) len[i] = 0;   // a code with one symbol costs no bits
        unsigned long long b = vp8l_refs_desc_bits(len, int(n), u);
        for (uint32_t i = 0; i < n; i++) b += static_cast<unsigned long long>(f[i]) * len[i];
        if (l == 0) for (uint32_t s = 0; s < 24; s++) b += static_cast<unsigned long long>(f[256 + s]) * vp8l_prefix_extra(s);
        if (l == 4) for (uint32_t s = 0; s < 40; s++) b += static_cast<unsigned long long>(f[s]) * vp8l_prefix_extra(s);
        S.bits[l] = b;
        uint8_t *o = glens + (uint64_t(image) * VP8L_MAX_GROUPS + g) * VP8L_LENS + uint32_t(l) * VP8L_GREEN_MAX;
        for (uint32_t i = 0; i < n; i++) o[i] = len[i];
    }
    CSP_WAVE_SYNC();
    LFOR(l) if (l == 0) info[1 + g] = S.bits[0] + S.bits[1] + S.bits[2] + S.bits[3] + S.bits[4];
}

// ---- the entropy image's own code, from the labels: what the choice counts is what the pack writes.  At least two groups are in use, so the code is never empty
struct LabelCode { uint32_t h[VP8L_MAX_GROUPS]; uint8_t len[VP8L_MAX_GROUPS]; uint16_t code[VP8L_MAX_GROUPS]; Vp8lCodeUse use; unsigned long long bits; };
__device__ static void vp8l_label_code(const uint8_t *lab, uint32_t nt, LabelCode &C) {
    LFOR(l) if (l < int(VP8L_MAX_GROUPS)) C.h[l] = 0;
    CSP_WAVE_SYNC();
    LFOR(l) for (uint32_t t = uint32_t(l); t < nt; t += 64) atomicAdd(&C.h[lab[t]], 1u);
    CSP_WAVE_SYNC();
    LFOR(l) if (l == 0) {
        csp::code_lengths(C.h, int(VP8L_MAX_GROUPS), 15, C.len);
        C.use = vp8l_code_use([&](int i) { return C.h[i]; }, int(VP8L_MAX_GROUPS));
        csp::canonical(C.len, int(VP8L_MAX_GROUPS), C.code);
        // the sub-image as Vp8lPut::head writes the predictor's: "no cache", the green code, four codes of one symbol, the tiles
        unsigned long long b = 1u + vp8l_code_desc_bits(C.use) + 16u;
        for (uint32_t i = 0; i < VP8L_MAX_GROUPS; i++) b += static_cast<unsigned long long>(C.h[i]) * C.len[i];
        C.bits = b;
    }
    CSP_WAVE_SYNC();
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_group_choose(int nimg, const Vp8lGroupImg *gimgs, const uint8_t *label, const unsigned long long *ginfo, uint32_t *pick) {
    CSH_SHARED LabelCode S;
    const int image = blockIdx.x;
    if (image >= nimg) return;
    const Vp8lGroupImg G = gimgs[image];
    const unsigned long long *info = ginfo + uint64_t(image) * VP8L_GROUP_INFO;
    const uint32_t ng = uint32_t(info[0]);
    if (!G.bits || !ng) return;
    vp8l_label_code(label + G.tile_off, G.ntile, S);
    LFOR(l) if (l == 0) {
        // behind the common head: the cache's bit (and its size), the meta prefix flag and the tile side, the entropy image, the groups
        unsigned long long total = (pick[4 * image + 1] ? 5u : 1u) + 1u + 3u + S.bits;
        for (uint32_t g = 0; g < ng; g++) total += info[1 + g];
        // a tie keeps the stream that exists without groups
        if (total < pick[4 * image + 2] && total < pick[4 * image + 3]) { pick[4 * image] = 3u; pick[4 * image + 2] = uint32_t(total); }
    }
}

// ---- one wave per picture whose grouped stream won
struct PackGroupsLds {
    uint8_t glen[VP8L_MAX_GROUPS][VP8L_GREEN_MAX], len[VP8L_MAX_GROUPS][4][256];   // green; red, blue, alpha, distance
    uint16_t gcode[VP8L_MAX_GROUPS][VP8L_GREEN_MAX], code[VP8L_MAX_GROUPS][4][256];
    uint8_t mlen[288];
    uint16_t mcode[288];
    uint32_t mh[288];
    uint32_t win[160];
    Vp8lCodeUse use[5 * VP8L_MAX_GROUPS + 1];
    Vp8lDescLds desc;
    LabelCode lc;
};
static_assert(sizeof(PackGroupsLds) <= 64 * 1024, "the groups' code tables stay in LDS");

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_pack_groups(const Vp8lImg *imgs, int nimg, const Vp8lGroupImg *gimgs, const uint32_t *work, const uint8_t *modes, const uint64_t *toks,
                                                                       const uint8_t *hits, const uint32_t *ghist, const uint8_t *glens, const uint8_t *label, const unsigned long long *ginfo,
                                                                       const uint32_t *pick, uint8_t *outp, uint32_t *file_len, uint32_t *status) {
    CSH_SHARED PackGroupsLds S;
    const int image = blockIdx.x;
    if (image >= nimg || pick[4 * image] != 3u) return;
    const Vp8lImg im = imgs[image];
    const Vp8lGroupImg G = gimgs[image];
    uint8_t *file = outp + im.out_off;
    const uint32_t opt = pick[4 * image + 1], cbits = vp8l_cache_bits(opt), ng = uint32_t(ginfo[uint64_t(image) * VP8L_GROUP_INFO]);
    const uint32_t *hg = ghist + uint64_t(image) * VP8L_MAX_GROUPS * VP8L_HIST;
    const uint8_t *ln = glens + uint64_t(image) * VP8L_MAX_GROUPS * VP8L_LENS;
    const uint8_t *lab = label + G.tile_off;
    const uint32_t nblk = im.bw * im.bh;
    LFOR(l) for (int i = l; i < 288; i += 64) S.mh[i] = 0;
    LFOR(l) for (int i = l; i < 160; i += 64) S.win[i] = 0;
    for (uint32_t g = 0; g < ng; g++) {
        LFOR(l) for (uint32_t i = uint32_t(l); i < VP8L_GREEN_MAX; i += 64) S.glen[g][i] = ln[g * VP8L_LENS + i];
        LFOR(l) for (uint32_t i = uint32_t(l); i < 4 * 256; i += 64) S.len[g][i >> 8][i & 255u] = ln[g * VP8L_LENS + ((i >> 8) + 1) * VP8L_GREEN_MAX + (i & 255u)];
    }
    CSP_WAVE_SYNC();
    for (uint32_t b0 = 0; b0 < nblk; b0 += 64) LFOR(l) if (b0 + uint32_t(l) < nblk) atomicAdd(&S.mh[modes[im.mode_off + b0 + uint32_t(l)]], 1u);
    CSP_WAVE_SYNC();
    LFOR(l) if (l <= int(5 * VP8L_MAX_GROUPS)) {
        if (l == int(5 * VP8L_MAX_GROUPS)) {   // the predictor modes' code, as the plain coder makes it
            csp::code_lengths(S.mh, 280, 15, S.mlen);
            const Vp8lCodeUse u = vp8l_code_use([&](int i) { return S.mh[i]; }, 280);
            if (u.nused <= 1) for (int i = 0; i < 280; i++) S.mlen[i] = 0;
            csp::canonical(S.mlen, 280, S.mcode);
            S.use[l] = u;
        } else if (uint32_t(l) / 5u < ng) {
            const uint32_t g = uint32_t(l) / 5u;
            const int c = l % 5;
            const uint32_t n = vp8l_alphabet(c, opt);
            const uint32_t *f = hg + g * VP8L_HIST + vp8l_hist_off(c);
            S.use[l] = vp8l_code_use([&](int i) { return f[i]; }, int(n));
            if (c == 0) csp::canonical(S.glen[g], int(n), S.gcode[g]); else csp::canonical(S.len[g][c - 1], int(n), S.code[g][c - 1]);
        }
    }
    CSP_WAVE_SYNC();
    vp8l_label_code(lab, G.ntile, S.lc);
    Vp8lPut P;
    P.begin(S.win, file + 20);
    P.head(im, modes, S.mlen, S.mcode, S.use[5 * VP8L_MAX_GROUPS]);
    if (cbits) P.put1(1u | (uint64_t(cbits) << 1), 5); else P.put1(0, 1);   // the picture's colour cache
    P.put1(1u | (uint64_t(G.bits - 2) << 1), 4);                              // a meta prefix image follows; its tile side
    P.put1(0, 1);                                                              // the entropy image: no colour cache
    P.code(S.lc.len, S.lc.use); P.single(); P.single(); P.single(); P.single();
    for (uint32_t t0 = 0; t0 < G.ntile; t0 += 64) {
        LV<uint64_t> val; LV<uint32_t> nb;
        LFOR(l) {
            const uint32_t t = t0 + uint32_t(l), g = t < G.ntile ? lab[t] : 0u;
            nb[l] = t < G.ntile ? S.lc.len[g] : 0u; val[l] = S.lc.code[g];
        }
        P.bo.put(val, nb);
    }
    for (uint32_t g = 0; g < ng; g++) {
        P.code_runs(S.glen[g], int(vp8l_alphabet(0, opt)), S.use[5 * g], S.desc);
        for (int c = 1; c < 5; c++) P.code_runs(S.len[g][c - 1], int(vp8l_alphabet(c, opt)), S.use[5 * g + uint32_t(c)], S.desc);
    }
    // the walk of k_vp8l_pack_refs; a token's tables are those of the tile that holds its position
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
            const uint32_t i = i0 + uint32_t(l), y = i / im.width, x = i - y * im.width;
            const uint32_t g = lab[(y >> G.bits) * G.tw + (x >> G.bits)];
            const uint32_t dist = uint32_t(t >> 16);
            if (dist) {   // length prefix, its extra bits, distance prefix, its extra bits: 15 + 10 + 15 + 18 at the most
                uint32_t ls, lne, lex, ds, dne, dex;
                vp8l_prefix(uint32_t(t) & 0xFFFFu, ls, lne, lex);
                vp8l_prefix(vp8l_dist_code(dist, im.width), ds, dne, dex);
                const uint32_t lg = S.glen[g][256 + ls], ld = S.len[g][3][ds];
                val[l] = uint64_t(S.gcode[g][256 + ls]) | (uint64_t(lex) << lg) | (uint64_t(S.code[g][3][ds]) << (lg + lne)) | (uint64_t(dex) << (lg + lne + ld));
                nb[l] = lg + lne + ld + dne;
                continue;
            }
            if (opt && ((hm >> opt) & 1u)) { const uint32_t s = 280 + vp8l_slot(v, cbits); val[l] = S.gcode[g][s]; nb[l] = S.glen[g][s]; continue; }
            const uint32_t gr = (v >> 8) & 255u, r = (v >> 16) & 255u, b = v & 255u, a = v >> 24;
            const uint32_t lg = S.glen[g][gr], lr = S.len[g][0][r], lb = S.len[g][1][b], la = S.len[g][2][a];
            nb[l] = lg + lr + lb + la;
            val[l] = uint64_t(S.gcode[g][gr]) | (uint64_t(S.code[g][0][r]) << lg) | (uint64_t(S.code[g][1][b]) << (lg + lr)) | (uint64_t(S.code[g][2][a]) << (lg + lr + lb));
        }
        P.bo.put(val, nb);
    }
    P.finish(im, file, image, file_len, status);
}

void launch_vp8l_group_stages(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_tiles, const uint32_t *work, const Vp8lRefs &R) {
    if (!nimg || !max_tiles) return;
    CSH_LAUNCH_PHASED(k_vp8l_tile_feat, 3, dim3(max_tiles, unsigned(nimg)), dim3(256), st, imgs, R.gimg, work, R.tok, R.hit, R.pick, R.feat);
    CSH_LAUNCH(k_vp8l_tile_cluster, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, nimg, R.gimg, R.feat, R.label, R.ginfo);
    CSH_LAUNCH_PHASED(k_vp8l_group_hist, 3, dim3(max_tiles, unsigned(nimg)), dim3(256), st, imgs, R.gimg, work, R.tok, R.hit, R.pick, R.label, R.ginfo, R.ghist);
    CSH_LAUNCH(k_vp8l_group_codes, dim3(VP8L_MAX_GROUPS, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, R.pick, R.ghist, R.glens, R.ginfo);
    CSH_LAUNCH(k_vp8l_group_choose, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, nimg, R.gimg, R.label, R.ginfo, R.pick);
}
void launch_vp8l_pack_groups(hipStream_t st, const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const Vp8lRefs &R, uint8_t *out, uint32_t *file_len, uint32_t *status) {
    if (!nimg) return;
    CSH_LAUNCH(k_vp8l_pack_groups, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, nimg, R.gimg, work, modes, R.tok, R.hit, R.ghist, R.glens, R.label, R.ginfo, R.pick, out, file_len, status);
}

}  // namespace csw
