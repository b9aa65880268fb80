// k_webp_anim.hip -- animated WebP inputs: the canvases of a file from its decoded frames, and what changed between them.  libcaesium hands such a file to
// libwebp's AnimDecoder and codes the canvases again; here every frame is a picture of the decode batch (k_webp_dec.hip), and this walk is the layer between
// the decoders and the encoders.  The arithmetic is AnimDecoder's (tests/test_webp_anim_emul.py pins it to libwebp through Pillow, canvas by canvas).
//
// One wave takes ANIM_TILE consecutive canvas pixels of one file, ANIM_PX per lane, and walks the file's frames in order with the canvas values in registers:
// pixels do not depend on one another, only the frame loop is serial.  A canvas is never stored (but for ANIM_WALK_CANVAS, the tests' tap): the first walk
// reduces, per frame, the bounding box of the pixels that differ from the canvas before; the host turns the boxes into rectangles; the second walk writes
// each frame's rectangle, packed, where the encoders take it.
#include "webp_kernels.h"
#include "vp8_dec.h"
#include "wave.h"

namespace csw {

using csh::LV;
using csh::lballot;
using csh::lmax32;
using csh::lmin32;

enum : uint32_t { ANIM_PX = 4, ANIM_TILE = 64 * ANIM_PX };

// a pixel is R | G << 8 | B << 16 | A << 24: the RGBA bytes of the pools as one little-endian word
// AnimDecoder's blend of a source pixel over the canvas, neither premultiplied
__host__ __device__ static inline uint32_t anim_blend(uint32_t s, uint32_t d) {
    const uint32_t sa = s >> 24;
    if (sa == 255u) return s;
    if (sa == 0u) return d;
    const uint32_t fa = ((d >> 24) * (256u - sa)) >> 8, a = sa + fa;   // a: sa .. 255
    const uint32_t scale = (1u << 24) / a;
    uint32_t r = a << 24;
    CSH_UNROLL
    for (int c = 0; c < 24; c += 8) r |= (((((s >> c) & 255u) * sa + ((d >> c) & 255u) * fa) * scale) >> 24) << c;   // the sum is at most 255 a: the product fits 32 bits
    return r;
}

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_webp_anim(int mode, const AnimFile *files, const AnimFrame *frames, const Vp8In *imgs, const uint8_t *rgb, uint32_t *stats, uint8_t *pool,
                                                                 uint32_t target) {
    const AnimFile F = files[blockIdx.y];
    const uint32_t npx = F.cw * F.ch, base = blockIdx.x * ANIM_TILE;   // (a canvas is at most 2^24 x 2^24 by its header; the host refuses what does not fit 2^31 pixels)
    if (base >= npx) return;
    LV<uint32_t> cur[ANIM_PX], px[ANIM_PX], py[ANIM_PX];
    LFOR(l) {
        CSH_UNROLL
        for (uint32_t q = 0; q < ANIM_PX; q++) {
            const uint32_t i = base + q * 64u + uint32_t(l);
            cur[q][l] = 0u;
            px[q][l] = i < npx ? i % F.cw : 0xFFFFFFFFu;   // a pixel past the canvas lies in no rectangle
            py[q][l] = i / F.cw;
        }
    }
    uint32_t pvx = 0, pvy = 0, pvw = 0, pvh = 0;   // the rectangle the frame before left to be cleared (none: empty)
    const uint32_t last = mode == ANIM_WALK_CANVAS ? (target < F.nframes ? target + 1u : F.nframes) : F.nframes;
    for (uint32_t k = 0; k < last; k++) {
        const AnimFrame f = frames[F.first + k];
        const Vp8In &im = imgs[f.image];
        const bool key = (f.flags & ANIM_KEY) != 0, copy = (f.flags & ANIM_NO_BLEND) != 0, translucent = im.has_alpha != 0;
        const uint8_t *src3 = rgb + im.rgb_off;
        const uint32_t *src4 = reinterpret_cast<const uint32_t *>(rgb + (translucent ? im.rgba_off : 0));
        LV<uint32_t> was[ANIM_PX];
        LFOR(l) {
            CSH_UNROLL
            for (uint32_t q = 0; q < ANIM_PX; q++) {
                uint32_t c = cur[q][l];
                was[q][l] = c;
                const uint32_t x = px[q][l], y = py[q][l];
                const bool cleared = key || (x - pvx < pvw && y - pvy < pvh);   // where the canvas was cleared in front of this frame, the frame is copied in
                if (cleared) c = 0u;
                if (x - f.x < f.w && y - f.y < f.h) {
                    const uint32_t i = (y - f.y) * f.w + (x - f.x);
                    const uint32_t s = translucent ? src4[i] : (uint32_t(src3[3 * size_t(i)]) | (uint32_t(src3[3 * size_t(i) + 1]) << 8) | (uint32_t(src3[3 * size_t(i) + 2]) << 16) | 0xFF000000u);
                    c = (cleared || copy) ? s : anim_blend(s, c);
                }
                cur[q][l] = c;
            }
        }
        if (f.flags & ANIM_DISPOSE) { pvx = f.x; pvy = f.y; pvw = f.w; pvh = f.h; } else pvw = pvh = 0;
        if (mode == ANIM_WALK_STATS) {
            if (k == 0) continue;   // frame 0 is written whole
            // most waves of most frames see no change: they leave here behind one ballot
            const uint64_t any = lballot([&](int l) { bool ch = false; for (uint32_t q = 0; q < ANIM_PX; q++) ch |= cur[q][l] != was[q][l]; return ch; });
            if (!any) continue;
            LV<uint32_t> x0, y0, x1, y1, nch, ntr;
            LFOR(l) {
                x0[l] = y0[l] = 0xFFFFFFFFu; x1[l] = y1[l] = 0u; nch[l] = ntr[l] = 0u;
                CSH_UNROLL
                for (uint32_t q = 0; q < ANIM_PX; q++)
                    if (cur[q][l] != was[q][l]) {
                        const uint32_t x = px[q][l], y = py[q][l];
                        x0[l] = x < x0[l] ? x : x0[l]; y0[l] = y < y0[l] ? y : y0[l]; x1[l] = x > x1[l] ? x : x1[l]; y1[l] = y > y1[l] ? y : y1[l];
                        nch[l]++; ntr[l] += (cur[q][l] >> 24) != 255u ? 1u : 0u;
                    }
            }
            const uint32_t mx0 = lmin32(x0), my0 = lmin32(y0), mx1 = lmax32(x1), my1 = lmax32(y1), sch = csh::lsum32(nch), str = csh::lsum32(ntr);
            uint32_t *st = stats + size_t(F.first + k) * ANIM_STAT;
            LFOR(l) if (l == 0) {   // one set of atomics per wave that saw a change
                atomicMin(&st[0], mx0); atomicMin(&st[1], my0); atomicMax(&st[2], mx1); atomicMax(&st[3], my1);
                atomicAdd(&st[4], sch);
                if (str) atomicAdd(&st[5], str);
            }
            continue;
        }
        if (mode == ANIM_WALK_PACK) {
            const bool holes = (f.flags & ANIM_HOLES) != 0;
            LV<uint32_t> alpha;
            LFOR(l) {
                alpha[l] = 0u;
                CSH_UNROLL
                for (uint32_t q = 0; q < ANIM_PX; q++) {
                    const uint32_t x = px[q][l], y = py[q][l];
                    if (!(x - f.ox < f.ow && y - f.oy < f.oh)) continue;
                    const uint32_t v = (holes && cur[q][l] == was[q][l]) ? 0u : cur[q][l];
                    const size_t i = size_t(y - f.oy) * f.ow + (x - f.ox);
                    if (f.split) {
                        uint8_t *o = pool + f.out_off + 3 * i;
                        o[0] = uint8_t(v); o[1] = uint8_t(v >> 8); o[2] = uint8_t(v >> 16);
                        pool[f.a_off + i] = uint8_t(v >> 24);
                    } else reinterpret_cast<uint32_t *>(pool + f.out_off)[i] = v;
                    alpha[l] |= (v >> 24) != 255u ? 1u : 0u;
                }
            }
            if (lballot([&](int l) { return alpha[l] != 0u; })) LFOR(l) if (l == 0) atomicOr(&stats[size_t(F.first + k) * ANIM_STAT + 6], 1u);
            continue;
        }
    }
    if (mode == ANIM_WALK_CANVAS)
        LFOR(l) {
            CSH_UNROLL
            for (uint32_t q = 0; q < ANIM_PX; q++) {
                const uint32_t i = base + q * 64u + uint32_t(l);
                if (i < npx) reinterpret_cast<uint32_t *>(pool)[i] = cur[q][l];
            }
        }
}

void launch_webp_anim(hipStream_t st, int mode, const AnimFile *files, int nfiles, uint64_t max_px, const AnimFrame *frames, const Vp8In *imgs, const uint8_t *rgb, uint32_t *stats, uint8_t *pool,
                      uint32_t frame) {
    if (nfiles <= 0 || !max_px) return;
    CSH_LAUNCH(k_webp_anim, dim3(unsigned((max_px + ANIM_TILE - 1) / ANIM_TILE), unsigned(nfiles)), dim3(CSP_WAVE_THREADS), st, mode, files, frames, imgs, rgb, stats, pool, frame);
}

}  // namespace csw
