// k_gif_anim.hip -- GIF inputs: the canvases of a file from its decoded frames, what changed between them, and the output frames' index rectangles
// (DESIGN.md 8.3).  The shape is k_webp_anim.hip's: one wave takes GIF_TILE consecutive canvas pixels of one file, GIF_PX per lane, and walks the file's frames
// in order with the canvas in registers; pixels do not depend on one another, only the frame loop is serial.  A canvas is RGBA and starts as 0x00000000; a
// frame's pixel that is not its transparent index sets the canvas to its colour with alpha 255; the disposal method then acts on the frame's rectangle (2: cleared
// to 0x00000000 -- the background colour is not used, which is how browsers compose; 3: back to what it held before the frame).
//   GIF_WALK_STATS   per frame k > 0 two bounding boxes: C_k, where canvas k differs from canvas k - 1, and U_k, where canvas k - 1 is opaque and canvas k is not
//   GIF_WALK_PACK    the output frames' rectangles (the host made them from the boxes) as indices into each frame's own colour table
//   GIF_WALK_CANVAS  canvas `target` of one file, the tests' tap
#include "gif_kernels.h"
#include "wave.h"

namespace csg {

using csh::LV;
using csh::lballot;

enum : uint32_t { GIF_PX = 4, GIF_TILE = 64 * GIF_PX };

// the lowest index of colour c in the frame's table that is not the transparent index; GIF_NO_INDEX if the table does not hold the colour
__device__ static uint32_t gif_find_colour(const uint32_t *table, uint32_t n, uint32_t transparent, uint32_t c) {
    for (uint32_t i = 0; i < n; i++) if (table[i] == c && i != transparent) return i;
    return GIF_NO_INDEX;
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_gif_anim(int mode, const GifFile *files, const GifFrame *frames, const uint8_t *indices, const uint32_t *tables, const uint8_t *canon, uint32_t *stats,
                                                                uint32_t *file_flags, uint8_t *pool, uint32_t target) {
    const GifFile F = files[blockIdx.y];
    const uint32_t npx = F.cw * F.ch, base = blockIdx.x * GIF_TILE;
    if (base >= npx) return;
    // work: the canvas the next frame draws on (disposals applied); shown: the canvas the frame before showed; state: what the output's frames have painted
    LV<uint32_t> work[GIF_PX], shown[GIF_PX], state[GIF_PX], px[GIF_PX], py[GIF_PX];
    LFOR(l) {
        CSH_UNROLL
        for (uint32_t q = 0; q < GIF_PX; q++) {
            const uint32_t i = base + q * 64u + uint32_t(l);
            work[q][l] = shown[q][l] = state[q][l] = 0u;
            px[q][l] = i < npx ? i % F.cw : 0xFFFFFFFFu;   // a pixel past the canvas lies in no rectangle
            py[q][l] = i / F.cw;
        }
    }
    LV<uint32_t> flags;
    LFOR(l) flags[l] = 0u;
    const uint32_t last = mode == GIF_WALK_CANVAS ? (target < F.nframes ? target + 1u : F.nframes) : F.nframes;
    for (uint32_t k = 0; k < last; k++) {
        const GifFrame f = frames[F.first + k];
        const uint32_t *table = tables + size_t(f.pal) * 256u;
        const uint8_t *idx = indices + f.idx_off;
        LV<uint32_t> cur[GIF_PX], own[GIF_PX];   // canvas k; the index this frame painted the pixel with (GIF_NO_INDEX: it did not)
        LFOR(l) {
            CSH_UNROLL
            for (uint32_t q = 0; q < GIF_PX; q++) {
                const uint32_t x = px[q][l], y = py[q][l];
                uint32_t c = work[q][l], mine = GIF_NO_INDEX;
                const bool inside = x - f.x < f.w && y - f.y < f.h;
                if (inside) {
                    const uint32_t v = idx[size_t(y - f.y) * f.w + (x - f.x)];
                    if (v != f.transparent) { c = table[v]; mine = v; }
                }
                cur[q][l] = c; own[q][l] = mine;
                if (inside) work[q][l] = f.disposal == 2u ? 0u : f.disposal == 3u ? work[q][l] : c;
            }
        }
        if (mode == GIF_WALK_STATS && k > 0) {
            // most waves of most frames see no change: they leave here behind one ballot
            const uint64_t any = lballot([&](int l) { bool ch = false; for (uint32_t q = 0; q < GIF_PX; q++) ch |= cur[q][l] != shown[q][l]; return ch; });
            if (any) {
                LV<uint32_t> b[8];
                LFOR(l) {
                    b[0][l] = b[1][l] = b[4][l] = b[5][l] = 0xFFFFFFFFu; b[2][l] = b[3][l] = b[6][l] = b[7][l] = 0u;
                    CSH_UNROLL
                    for (uint32_t q = 0; q < GIF_PX; q++) {
                        if (cur[q][l] == shown[q][l]) continue;
                        const uint32_t x = px[q][l], y = py[q][l];
                        const uint32_t s = ((shown[q][l] >> 24) == 255u && (cur[q][l] >> 24) != 255u) ? 4u : 0u;   // an un-painted pixel counts in both boxes
                        for (uint32_t t = 0; t <= s; t += 4u) {
                            b[t][l] = x < b[t][l] ? x : b[t][l]; b[t + 1][l] = y < b[t + 1][l] ? y : b[t + 1][l];
                            b[t + 2][l] = x > b[t + 2][l] ? x : b[t + 2][l]; b[t + 3][l] = y > b[t + 3][l] ? y : b[t + 3][l];
                        }
                    }
                }
                uint32_t r[8];
                for (uint32_t t = 0; t < 8; t++) r[t] = (t & 2u) ? csh::lmax32(b[t]) : csh::lmin32(b[t]);
                uint32_t *st = stats + size_t(F.first + k) * GIF_STAT;
                LFOR(l) if (l == 0) {   // one set of vector atomics per wave that saw a change
                    atomicMin(&st[0], r[0]); atomicMin(&st[1], r[1]); atomicMax(&st[2], r[2]); atomicMax(&st[3], r[3]);
                    if (r[4] <= r[6]) { atomicMin(&st[4], r[4]); atomicMin(&st[5], r[5]); atomicMax(&st[6], r[6]); atomicMax(&st[7], r[7]); }
                }
            }
        }
        if (mode == GIF_WALK_PACK) {
            const GifFrame &pf = frames[F.first + (k ? k - 1u : 0u)];
            const bool clears = k > 0 && pf.odisposal == 2u;
            LFOR(l) {
                CSH_UNROLL
                for (uint32_t q = 0; q < GIF_PX; q++) {
                    const uint32_t x = px[q][l], y = py[q][l], c = cur[q][l];
                    if (clears && x - pf.ox < pf.ow && y - pf.oy < pf.oh) state[q][l] = 0u;
                    if (!(x - f.ox < f.ow && y - f.oy < f.oh)) continue;
                    uint32_t v;
                    if (state[q][l] == c && f.transparent != GIF_NO_INDEX) v = f.transparent;
                    else if ((c >> 24) != 255u) { v = 0u; flags[l] |= GIF_FLAG_HOLD; }   // nothing can make a pixel transparent but a disposal, and the rectangles saw to those
                    else {
                        // the colour's lowest index: the frame's own pixel knows it from the table's map; a colour another frame left is searched for
                        v = own[q][l] != GIF_NO_INDEX ? uint32_t(canon[size_t(f.pal) * 256u + own[q][l]]) : GIF_NO_INDEX;
                        if (v == GIF_NO_INDEX || v == f.transparent || v >= f.pal_n) v = gif_find_colour(table, f.pal_n, f.transparent, c);
                        if (v == GIF_NO_INDEX) { v = 0u; flags[l] |= state[q][l] == c ? GIF_FLAG_HOLD : GIF_FLAG_PALETTE; }
                        state[q][l] = c;
                    }
                    pool[f.out_off + size_t(y - f.oy) * f.ow + (x - f.ox)] = uint8_t(v);
                }
            }
        }
        LFOR(l) {
            CSH_UNROLL
            for (uint32_t q = 0; q < GIF_PX; q++) shown[q][l] = cur[q][l];
        }
    }
    if (mode == GIF_WALK_PACK) {
        const uint32_t raised = (lballot([&](int l) { return (flags[l] & GIF_FLAG_PALETTE) != 0u; }) ? uint32_t(GIF_FLAG_PALETTE) : 0u) |
                                (lballot([&](int l) { return (flags[l] & GIF_FLAG_HOLD) != 0u; }) ? uint32_t(GIF_FLAG_HOLD) : 0u);
        if (raised) LFOR(l) if (l == 0) atomicOr(&file_flags[blockIdx.y], raised);
    }
    if (mode == GIF_WALK_CANVAS)
        LFOR(l) {
            CSH_UNROLL
            for (uint32_t q = 0; q < GIF_PX; q++) {
                const uint32_t i = base + q * 64u + uint32_t(l);
                if (i < npx) reinterpret_cast<uint32_t *>(pool)[i] = shown[q][l];
            }
        }
}

void launch_gif_anim(hipStream_t st, int mode, const GifFile *files, uint32_t nfiles, uint64_t max_px, const GifFrame *frames, const uint8_t *indices, const uint32_t *tables, const uint8_t *canon,
                     uint32_t *stats, uint32_t *file_flags, uint8_t *pool, uint32_t target) {
    if (!nfiles || !max_px) return;
    CSH_LAUNCH(k_gif_anim, dim3(unsigned((max_px + GIF_TILE - 1) / GIF_TILE), unsigned(nfiles)), dim3(CSP_WAVE_THREADS), st, mode, files, frames, indices, tables, canon, stats, file_flags, pool, target);
}

}  // namespace csg
