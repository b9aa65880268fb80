// k_vp8l_far.hip -- lossless WebP OUTPUT with a match finder that sees the format's whole window (CSH_VP8L=far).  Everything CSH_VP8L=groups does
// stays as it is and gives every record (a picture, a palette candidate) its token set A.  Here the record gets a second set, B: k_vp8l_match's best fixed-distance
// copy, then a walk of up to VP8L_FAR_LINKS links of a hash chain over the WHOLE record.  The stages that depend on tokens (parse, counts, codes, the group
// stages) run once more over B's pools, and the record keeps the set whose best stream is smaller in exact bits: B only where it is strictly smaller, so a file
// is never larger than the groups mode's.
// The chain, prev[p] = the largest q < p whose next three pixels hash like p's (24 bits), is built without serial insertion: the positions are already ascending,
// so a STABLE least-significant-digit radix sort of the positions by their hash, three passes of 8 bits, leaves every bucket in position order and prev is the
// left neighbour with an equal hash.  Keys are recomputed from the pixels: only positions move (two arrays of one word per pixel, and one word per pixel of prev).
// A position in the inside of a flat run, px[p - 1] == px[p] == px[p + 1] == px[p + 2], gets no link and is no link's target (it does not enter the sort): the
// fixed distances 1 and width cover runs, and a flat area would otherwise put a million positions into one bucket.
//   k_vp8l_far_hist      one workgroup per block of 4096 entries: the pass's 256 digit counts (LDS), stored per (digit, block)
//   k_vp8l_far_scan      one wave per digit: the exclusive scan of the digit's counts over the blocks, and the digit's total
//   k_vp8l_far_scatter   one wave per block: a key's rank among the lanes before it with the same digit is a popcount of eight ballots; the digits' running
//                        places live in LDS and advance group by group, so the order inside a digit is the order of the entries
//   k_vp8l_far_link      prev from the sorted positions
//   k_vp8l_match_far     k_vp8l_match's scheduling (one wave per chunk, one lane per position) with the walk in place of the hashed candidate
//   k_vp8l_far_choose    per record: B's best exact bits against A's
//   k_vp8l_far_take      where B won: its tokens, counts, lengths, pick words and group pools over A's
// Every count is a sum, every place a scan of counts and every choice goes by value: no lane's, wave's or block's order shows in prev, in the tokens or in the bytes.
#include "vp8l_refs.h"

namespace csw {

static_assert(uint32_t(VP8L_FAR_BLOCK) == uint32_t(VP8L_CHUNK), "a record has as many sort blocks as chunks: Vp8lImg::nchunk and cst_off place its digit counts");

__device__ __forceinline__ static uint32_t vp8l_hash24(uint32_t a, uint32_t b, uint32_t c) {
    return (((a * 0x9E3779B1u) ^ (b * 0x85EBCA6Bu) ^ (c * 0xC2B2AE35u)) * 0x27D4EB2Fu) >> 8;
}
__device__ __forceinline__ static uint32_t far_key(const uint32_t *px, uint32_t p) { return vp8l_hash24(px[p], px[p + 1], px[p + 2]); }
// position p has a link and may be a link's target
__device__ __forceinline__ static bool far_linked(const uint32_t *px, uint32_t N, uint32_t p) {
    if (p + 3 > N) return false;
    return !(p >= 1 && px[p - 1] == px[p] && px[p] == px[p + 1] && px[p + 1] == px[p + 2]);
}
// a copy found through a link pays for its distance: at least this long (the fixed distances and CSH_VP8L=refs' own candidate keep VP8L_MIN_MATCH)
__device__ __forceinline__ static uint32_t far_min_len(uint32_t dist) { return VP8L_MIN_MATCH + (dist >= 4096u ? 1u : 0u) + (dist >= 65536u ? 1u : 0u); }

struct FarRec { const uint32_t *px; uint32_t *cnt, *tot; uint32_t N, nblk, nlive; };
__device__ __forceinline__ static FarRec far_rec(const Vp8lImg &im, uint32_t rec, const uint32_t *work, uint32_t *cnt, uint32_t *dtot, int pass) {
    FarRec r;
    r.px = work + im.res_off; r.N = im.width * im.height; r.nblk = im.nchunk;
    r.cnt = cnt + (im.cst_off / VP8L_CACHE_STATE) * 256u;   // the record's first chunk among all the chunks, 256 counts each: digit d's column is cnt + d * nblk
    r.tot = dtot + uint64_t(rec) * VP8L_FAR_TOT;
    r.nlive = pass ? r.tot[768] : 0u;                        // the positions with a link: pass 0 counts them
    return r;
}
// entry i of a pass: pass 0 reads the positions themselves and leaves out those without a link; the later passes read the live ones, in the order of the pass before
__device__ __forceinline__ static bool far_entry(const FarRec &r, const uint32_t *src, int pass, uint32_t i, uint32_t &p) {
    if (pass == 0) { p = i; return i < r.N && far_linked(r.px, r.N, i); }
    if (i >= r.nlive) return false;
    p = src[i];
    return true;
}

__global__ void __launch_bounds__(256) k_vp8l_far_hist(const Vp8lImg *imgs, const uint32_t *work, const uint32_t *srcs, uint32_t *cnt, uint32_t *dtot, uint32_t *prevs, int pass) {
    CSH_SHARED uint32_t h[256];
    const Vp8lImg &im = imgs[blockIdx.y];
    const FarRec r = far_rec(im, blockIdx.y, work, cnt, dtot, pass);
    const uint32_t *src = srcs + im.res_off;
    const uint32_t i0 = blockIdx.x * VP8L_FAR_BLOCK;
    CSH_PHASE_LOOP(3) {
        if (blockIdx.x >= r.nblk) continue;
        if (phase == 0) { h[threadIdx.x] = 0; continue; }
        if (phase == 1) {
            for (uint32_t k = threadIdx.x; k < VP8L_FAR_BLOCK; k += 256) {
                uint32_t p;
                if (pass == 0 && i0 + k < r.N) prevs[im.res_off + i0 + k] = VP8L_FAR_NONE;   // k_vp8l_far_link writes the links there are
                if (far_entry(r, src, pass, i0 + k, p)) atomicAdd(&h[(far_key(r.px, p) >> (8 * pass)) & 255u], 1u);
            }
            continue;
        }
        r.cnt[uint64_t(threadIdx.x) * r.nblk + blockIdx.x] = h[threadIdx.x];
    }
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_far_scan(const Vp8lImg *imgs, uint32_t *cnt, uint32_t *dtot, int pass) {
    const Vp8lImg im = imgs[blockIdx.y];
    const FarRec r = far_rec(im, blockIdx.y, cnt, cnt, dtot, 0);   // (no pixels here)
    uint32_t *col = r.cnt + uint64_t(blockIdx.x) * r.nblk;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < r.nblk; b0 += 64) {
        LV<uint32_t> x;
        LFOR(l) x[l] = b0 + uint32_t(l) < r.nblk ? col[b0 + uint32_t(l)] : 0u;
        uint32_t total;
        const LV<uint32_t> off = csp::lscan(x, total);
        LFOR(l) if (b0 + uint32_t(l) < r.nblk) col[b0 + uint32_t(l)] = carry + off[l];
        carry += total;
    }
    LFOR(l) if (l == 0) {
        r.tot[256 * pass + blockIdx.x] = carry;
        if (pass == 0) atomicAdd(&r.tot[768], carry);   // the live positions: a sum, zeroed by the caller
    }
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_far_scatter(const Vp8lImg *imgs, const uint32_t *work, const uint32_t *srcs, uint32_t *dsts, uint32_t *cnt, uint32_t *dtot, int pass) {
    CSH_SHARED uint32_t place[256];
    const Vp8lImg im = imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    const FarRec r = far_rec(im, blockIdx.y, work, cnt, dtot, pass);
    const uint32_t *src = srcs + im.res_off;
    uint32_t *dst = dsts + im.res_off;
    const uint32_t i0 = blockIdx.x * VP8L_FAR_BLOCK, *dt = r.tot + 256 * pass;
    {   // where this block's first key of every digit goes: the digits in front (a lane owns four), the blocks in front
        LV<uint32_t> own;
        LFOR(l) own[l] = dt[4 * l] + dt[4 * l + 1] + dt[4 * l + 2] + dt[4 * l + 3];
        uint32_t total;
        const LV<uint32_t> off = csp::lscan(own, total);
        LFOR(l) {
            uint32_t s = off[l];
            for (uint32_t j = 0; j < 4; j++) { const uint32_t d = 4u * uint32_t(l) + j; place[d] = s + r.cnt[uint64_t(d) * r.nblk + blockIdx.x]; s += dt[d]; }
        }
    }
    CSP_WAVE_SYNC();
    for (uint32_t g0 = i0; g0 < i0 + VP8L_FAR_BLOCK; g0 += 64) {
        LV<uint32_t> p, live, dig;
        LFOR(l) {
            uint32_t q = 0;
            live[l] = far_entry(r, src, pass, g0 + uint32_t(l), q) ? 1u : 0u;
            p[l] = q; dig[l] = live[l] ? (far_key(r.px, q) >> (8 * pass)) & 255u : 0u;
        }
        const uint64_t act = csp::lballot([&](int l) { return live[l] != 0; });
        if (!act) continue;
        LV<uint64_t> same;   // the live lanes with this lane's digit
        LFOR(l) same[l] = act;
        for (uint32_t bit = 0; bit < 8; bit++) {
            const uint64_t b = csp::lballot([&](int l) { return ((dig[l] >> bit) & 1u) != 0; });
            LFOR(l) same[l] &= (dig[l] >> bit) & 1u ? b : ~b;
        }
        LFOR(l) if (live[l]) dst[place[dig[l]] + uint32_t(__popcll(static_cast<unsigned long long>(same[l] & csp::lanes_below(l))))] = p[l];
        CSP_WAVE_SYNC();
        LFOR(l) if (live[l] && ((same[l] >> l) >> 1) == 0) place[dig[l]] += uint32_t(__popcll(static_cast<unsigned long long>(same[l])));   // the digit's last lane
        CSP_WAVE_SYNC();
    }
}

__global__ void __launch_bounds__(256) k_vp8l_far_link(const Vp8lImg *imgs, const uint32_t *work, const uint32_t *sorteds, const uint32_t *dtot, uint32_t *prevs) {
    const Vp8lImg &im = imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    const uint32_t *px = work + im.res_off, *sorted = sorteds + im.res_off;
    const uint32_t live = dtot[uint64_t(blockIdx.y) * VP8L_FAR_TOT + 768];
    for (uint32_t k = threadIdx.x; k < VP8L_FAR_BLOCK; k += 256) {
        const uint32_t i = blockIdx.x * VP8L_FAR_BLOCK + k;
        if (i >= live) break;
        const uint32_t p = sorted[i];
        if (i) { const uint32_t q = sorted[i - 1]; if (far_key(px, q) == far_key(px, p)) prevs[im.res_off + p] = q; }   // stable: q < p
    }
}

// ---- candidates: k_vp8l_match's fixed distances, restated (that kernel keeps its registers), then the chain
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_match_far(const Vp8lImg *imgs, const uint32_t *work, const uint32_t *prevs, uint64_t *toks) {
    const Vp8lImg im = imgs[blockIdx.y];
    if (blockIdx.x >= im.nchunk) return;
    const uint32_t *px = work + im.res_off, *prev = prevs + im.res_off;
    uint64_t *tok = toks + im.tok_off;
    const uint32_t N = im.width * im.height, start = blockIdx.x * VP8L_CHUNK, end = N - start < VP8L_CHUNK ? N : start + VP8L_CHUNK;
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
            const uint32_t maxl = N - p < VP8L_MAX_LEN ? N - p : uint32_t(VP8L_MAX_LEN);
            // the chain, nearest first: a link is one of the VP8L_FAR_LINKS whether it is walked or not; only a strictly longer copy replaces the best so far
            uint32_t q = p;
            for (uint32_t k = 0; k < VP8L_FAR_LINKS && bl < maxl; k++) {
                q = prev[q];
                if (q == VP8L_FAR_NONE) break;
                const uint32_t d = p - q;
                if (d > VP8L_WINDOW) break;
                if (d == dv[0] || d == dv[1] || d == dv[2] || d == dv[3] || d == dv[4]) continue;
                if (px[p + bl] != px[q + bl]) continue;   // it would have to get past the best so far
                uint32_t n = 0;
                while (n < maxl && px[p + n] == px[q + n]) n++;
                if (n > bl && n >= far_min_len(d)) { bl = n; bd = d; }
            }
            if (bl < VP8L_MIN_MATCH) { bl = 0; bd = 0; }
            tok[p] = uint64_t(bl) | (uint64_t(bd) << 16);
        }
    }
}

// ---- the choice, per record: the best of a set is the smaller of its refs (or grouped) stream and its plain stream, in exact bits behind the head
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_far_choose(int nimg, const uint32_t *pick_a, const uint32_t *pick_b, uint32_t *won) {
    const int image = blockIdx.x;
    if (image >= nimg) return;
    LFOR(l) if (l == 0) {
        const uint32_t a = min(pick_a[4 * image + 2], pick_a[4 * image + 3]), b = min(pick_b[4 * image + 2], pick_b[4 * image + 3]);
        won[image] = b < a ? 1u : 0u;   // a tie keeps the set that exists without the chain
    }
}

template <class T>
__device__ __forceinline__ static void far_copy(T *dst, const T *src, uint64_t n) { for (uint64_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i]; }

// grid.x: the record's chunks (its tokens), then one block more for everything that is kept per record
__global__ void __launch_bounds__(256) k_vp8l_far_take(const Vp8lImg *imgs, int nparent, const uint32_t *won, Vp8lRefs A, Vp8lRefs B) {
    const uint32_t image = blockIdx.y;
    const Vp8lImg &im = imgs[image];
    if (!won[image] || blockIdx.x > im.nchunk) return;
    if (blockIdx.x < im.nchunk) {
        const uint32_t N = im.width * im.height, start = blockIdx.x * VP8L_CHUNK, n = N - start < VP8L_CHUNK ? N - start : uint32_t(VP8L_CHUNK);
        far_copy(A.tok + im.tok_off + start, B.tok + im.tok_off + start, n);
        return;
    }
    far_copy(A.hist + uint64_t(image) * (VP8L_NOPT * VP8L_HIST), B.hist + uint64_t(image) * (VP8L_NOPT * VP8L_HIST), VP8L_NOPT * VP8L_HIST);
    far_copy(A.lens + uint64_t(image) * VP8L_LENS, B.lens + uint64_t(image) * VP8L_LENS, VP8L_LENS);
    far_copy(A.pick + 4 * uint64_t(image), B.pick + 4 * uint64_t(image), 4);
    if (int(image) >= nparent || !A.gimg || !A.gimg[image].bits) return;   // a candidate, or a picture of one tile: no grouped stream
    const Vp8lGroupImg &G = A.gimg[image];
    far_copy(A.label + G.tile_off, B.label + G.tile_off, G.ntile);
    far_copy(A.ghist + uint64_t(image) * VP8L_MAX_GROUPS * VP8L_HIST, B.ghist + uint64_t(image) * VP8L_MAX_GROUPS * VP8L_HIST, VP8L_MAX_GROUPS * VP8L_HIST);
    far_copy(A.glens + uint64_t(image) * VP8L_MAX_GROUPS * VP8L_LENS, B.glens + uint64_t(image) * VP8L_MAX_GROUPS * VP8L_LENS, VP8L_MAX_GROUPS * VP8L_LENS);
    far_copy(A.ginfo + uint64_t(image) * VP8L_GROUP_INFO, B.ginfo + uint64_t(image) * VP8L_GROUP_INFO, VP8L_GROUP_INFO);
}

void launch_vp8l_far_links(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, const uint32_t *work, const Vp8lFar &F) {
    if (!nimg) return;
    const unsigned max_chunks = unsigned((max_pixels + VP8L_CHUNK - 1) / VP8L_CHUNK);
    for (int pass = 0; pass < 3; pass++) {   // positions -> pos[0] -> pos[1] -> pos[0]
        const uint32_t *src = F.pos[(pass + 1) & 1];
        uint32_t *dst = F.pos[pass & 1];
        CSH_LAUNCH_PHASED(k_vp8l_far_hist, 3, dim3(max_chunks, unsigned(nimg)), dim3(256), st, imgs, work, src, F.cnt, F.dtot, F.prev, pass);
        CSH_LAUNCH(k_vp8l_far_scan, dim3(256, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, F.cnt, F.dtot, pass);
        CSH_LAUNCH(k_vp8l_far_scatter, dim3(max_chunks, unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, work, src, dst, F.cnt, F.dtot, pass);
    }
    CSH_LAUNCH(k_vp8l_far_link, dim3(max_chunks, unsigned(nimg)), dim3(256), st, imgs, work, static_cast<const uint32_t *>(F.pos[0]), static_cast<const uint32_t *>(F.dtot), F.prev);
}
void launch_vp8l_far_match(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, const uint32_t *work, const Vp8lFar &F) {
    if (!nimg) return;
    CSH_LAUNCH(k_vp8l_match_far, dim3(unsigned((max_pixels + VP8L_CHUNK - 1) / VP8L_CHUNK), unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, work, static_cast<const uint32_t *>(F.prev), F.B.tok);
}
void launch_vp8l_far_stages(hipStream_t st, const Vp8lImg *imgs, int nparent, int nimg, uint64_t max_pixels, uint32_t max_tiles, const uint32_t *work, const uint32_t *hist, const Vp8lRefs &A,
                            const Vp8lFar &F) {
    if (!nimg) return;
    launch_vp8l_far_links(st, imgs, nimg, max_pixels, work, F);
    launch_vp8l_far_match(st, imgs, nimg, max_pixels, work, F);
    launch_vp8l_token_stages(st, imgs, nimg, max_pixels, work, hist, F.B);
    if (max_tiles) launch_vp8l_group_stages(st, imgs, nparent, max_tiles, work, F.B);
    CSH_LAUNCH(k_vp8l_far_choose, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, nimg, static_cast<const uint32_t *>(A.pick), static_cast<const uint32_t *>(F.B.pick), F.won);
    CSH_LAUNCH(k_vp8l_far_take, dim3(unsigned((max_pixels + VP8L_CHUNK - 1) / VP8L_CHUNK) + 1u, unsigned(nimg)), dim3(256), st, imgs, nparent, static_cast<const uint32_t *>(F.won), A, F.B);
}

}  // namespace csw
