// k_vp8l_enc.hip -- lossless WebP OUTPUT (webp.lossless: libcaesium's webp::compress encodes with libwebp's lossless coder,
// /root/reference/src/compressor.rs:427-429 sets it under --lossless; call sites compressor.rs:289-305).  A VP8L stream per picture, made
// of the format's tools that are data-parallel: subtract-green, the spatial predictor (best of the 14 modes per 16 x 16 block by the sum
// of absolute residuals -- every mode predicts from ORIGINAL neighbours, so all pixels are independent), and one group of optimal prefix
// codes limited to 15 bits (png_codes.h, shared with the DEFLATE coder).  No backward references, colour cache or meta prefix image here: this is the
// default coder, whose bytes the oracle states; CSH_VP8L=refs adds the first two (k_vp8l_refs.hip, on the residual image this front end leaves).
// What libwebp's coder adds on top is a few per cent on photographs and is a serial search; the bytes differ from libwebp's either way
// ("parity unpinned"), the invariant that is pinned is the format's: libwebp decodes the file to exactly the source pixels
// (tests/test_webp_lossless*.py), and so does this repo's own decoder (vp8l_dec.h).
//   k_vp8l_residuals  one workgroup per block: mode choice, residual ARGB
//   k_vp8l_hist       symbol counts of the four channels (an opaque source's alpha residuals are all one value: a code without bits)
//   k_vp8l_pack       one wave per picture: code lengths, canonical codes, the headers, then every pixel's three codes through the LDS
//                     bit window straight to their place, RIFF framing
#include "vp8l_pack.h"
#include "vp8l_dec.h"

namespace csw {

__device__ __forceinline__ static uint32_t sg_pixel(const Vp8lImg &im, uint32_t x, uint32_t y) {   // ARGB after subtract-green
    // channels: 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA; VP8L_ALPHA_OF + 2 / + 4: the ALPHA sample of such a picture taken as a grey picture (the ALPH
    // chunk of a lossy file is a VP8L stream whose green channel is the alpha plane)
    const uint32_t pick = im.channels >= VP8L_ALPHA_OF ? im.channels - VP8L_ALPHA_OF : 0u, nc = pick ? pick : im.channels;
    const uint8_t *p = im.rgb + (uint64_t(y) * im.width + x) * nc;
    if (pick) return 0xFF000000u | (uint32_t(p[nc - 1]) << 8);
    if (nc <= 2) return (nc == 2 ? uint32_t(p[1]) << 24 : 0xFF000000u) | (uint32_t(p[0]) << 8);   // grey: red - green = blue - green = 0
    const uint32_t r = p[0], g = p[1], b = p[2];
    return (nc == 4 ? uint32_t(p[3]) << 24 : 0xFF000000u) | (((r - g) & 255u) << 16) | (g << 8) | ((b - g) & 255u);
}
__device__ __forceinline__ static uint32_t res_cost(uint32_t r) {   // sum over the channels of the residual's distance from 0 (mod 256)
    uint32_t c = 0;
    for (int s = 0; s < 32; s += 8) { const uint32_t v = (r >> s) & 255u; c += v < 128u ? v : 256u - v; }
    return c;
}

// the predictor of pixel (x, y): libwebp's frame rules (first pixel: black; first row: left; first column: top), else the block's mode.
// The top-right neighbour of a row's last pixel is the first pixel of the row itself (the decoder reads one past the row above).
__device__ __forceinline__ static uint32_t predict_at(const Vp8lImg &im, uint32_t x, uint32_t y, int mode) {
    if (y == 0) return x == 0 ? 0xFF000000u : sg_pixel(im, x - 1, 0);
    if (x == 0) return sg_pixel(im, 0, y - 1);
    const uint32_t L = sg_pixel(im, x - 1, y), T = sg_pixel(im, x, y - 1), TL = sg_pixel(im, x - 1, y - 1);
    const uint32_t TR = x + 1 < im.width ? sg_pixel(im, x + 1, y - 1) : sg_pixel(im, 0, y);
    return lpredict_vals(mode, L, T, TR, TL);
}

__global__ void __launch_bounds__(256) k_vp8l_residuals(const Vp8lImg *imgs, uint32_t *work, uint8_t *modes) {
    CSH_SHARED uint32_t s_cost[16];
    CSH_SHARED uint32_t s_mode;
    const Vp8lImg &im = imgs[blockIdx.y];
    const uint32_t blk = blockIdx.x;
    const uint32_t by = im.bw ? blk / im.bw : 0u, bx = blk - by * im.bw;   // (bw = 0: a palette candidate's record, which has no block)
    const uint32_t tid = threadIdx.x, x = bx * 16u + (tid & 15u), y = by * 16u + (tid >> 4);
    const bool inside = blk < im.bw * im.bh && x < im.width && y < im.height;
    CSH_PHASE_LOOP(4) {
        if (blk >= im.bw * im.bh) continue;
        if (phase == 0) { if (tid < 16) s_cost[tid] = 0; continue; }
        if (phase == 1) {
            if (inside && x && y) {   // the frame's first row and column are predicted the same way whatever the mode
                const uint32_t me = sg_pixel(im, x, y);
                const uint32_t L = sg_pixel(im, x - 1, y), T = sg_pixel(im, x, y - 1), TL = sg_pixel(im, x - 1, y - 1);
                const uint32_t TR = x + 1 < im.width ? sg_pixel(im, x + 1, y - 1) : sg_pixel(im, 0, y);
                for (int m = 0; m < 14; m++) atomicAdd(&s_cost[m], res_cost(lsub(me, lpredict_vals(m, L, T, TR, TL))));
            }
            continue;
        }
        if (phase == 2) {
            if (tid == 0) {
                uint32_t best = 0;
                for (uint32_t m = 1; m < 14; m++) if (s_cost[m] < s_cost[best]) best = m;
                s_mode = best; modes[im.mode_off + blk] = uint8_t(best);
            }
            continue;
        }
        if (inside) work[im.res_off + uint64_t(y) * im.width + x] = lsub(sg_pixel(im, x, y), predict_at(im, x, y, int(s_mode)));
    }
}

__global__ void __launch_bounds__(256) k_vp8l_hist(const Vp8lImg *imgs, const uint32_t *work, uint32_t *hist) {
    CSH_SHARED uint32_t h[4 * 256];
    const Vp8lImg &im = imgs[blockIdx.y];
    const uint64_t npx = uint64_t(im.width) * im.height, i0 = uint64_t(blockIdx.x) * 4096u;
    CSH_PHASE_LOOP(3) {
        if (i0 >= npx) continue;
        if (phase == 0) { for (uint32_t i = threadIdx.x; i < 1024; i += 256) h[i] = 0; continue; }
        if (phase == 1) {
            for (uint32_t k = threadIdx.x; k < 4096; k += 256) {
                const uint64_t i = i0 + k;
                if (i >= npx) break;
                const uint32_t v = work[im.res_off + i];
                atomicAdd(&h[(v >> 8) & 255u], 1u); atomicAdd(&h[256 + ((v >> 16) & 255u)], 1u); atomicAdd(&h[512 + (v & 255u)], 1u); atomicAdd(&h[768 + (v >> 24)], 1u);
            }
            continue;
        }
        for (uint32_t i = threadIdx.x; i < 1024; i += 256) if (h[i]) atomicAdd(&hist[uint64_t(blockIdx.y) * 1024u + i], h[i]);
    }
}

// ---- one wave per picture
struct PackLds {
    uint8_t len[5][288];       // green (alphabet 280), red, blue, modes (alphabet 280), alpha
    uint16_t code[5][288];
    uint32_t mh[288];          // histogram of the modes, as a green alphabet
    uint32_t gh[288];          // the green histogram widened to its alphabet (256 literals + 24 length prefixes that are never used)
    uint32_t win[160];
    Vp8lCodeUse use[5];
};
struct PackPalLds { Vp8lPalCodes pal; Vp8lDescLds desc; };   // a palette candidate's head (CSH_VP8L=palette)

// pick: nullptr, or per record four words of which the first is 0 where this kernel writes the file (k_vp8l_refs.hip, k_vp8l_palette.hip).
// PAL: the records that are palette candidates, and only those -- no predictor: the head is the colour-indexing transform, the pixels are the bundled indices, the
// file is the parent's.  (Two kernels: the pictures' one is the default coder's and stays the code it was.)
template <bool PAL>
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_vp8l_pack(const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const uint32_t *hist, const uint32_t *pick, uint8_t *outp,
                                                                uint32_t *file_len, uint32_t *status) {
    CSH_SHARED PackLds S;
    const int image = blockIdx.x;
    if (image >= nimg) return;
    if (pick && pick[4 * image]) return;
    const Vp8lImg im = imgs[image];
    if (PAL != (im.pal != nullptr)) return;
    uint8_t *file = outp + im.out_off;
    const uint32_t *hh = hist + uint64_t(image) * 1024u;
    const uint32_t nblk = im.bw * im.bh;
    LFOR(l) for (int i = l; i < 288; i += 64) { S.mh[i] = 0; S.gh[i] = i < 256 ? hh[i] : 0u; }
    LFOR(l) for (int i = l; i < 160; i += 64) S.win[i] = 0;
    CSP_WAVE_SYNC();
    for (uint32_t b0 = 0; b0 < nblk; b0 += 64) LFOR(l) if (b0 + uint32_t(l) < nblk) atomicAdd(&S.mh[modes[im.mode_off + b0 + uint32_t(l)]], 1u);
    CSP_WAVE_SYNC();
    // five codes, one lane each (the arrays of code_lengths live in scratch)
    LFOR(l) if (l < 5) {
        const int n = (l == 0 || l == 3) ? 280 : 256;
        const uint32_t *f = l == 0 ? S.gh : l == 3 ? S.mh : l == 4 ? hh + 768u : hh + 256u * uint32_t(l);
        csp::code_lengths(f, n, 15, S.len[l]);
        const Vp8lCodeUse u = vp8l_code_use([&](int i) { return f[i]; }, n);
        if (u.nused <= 1) for (int i = 0; i < n; i++) S.len[l][i] = 0;   // a code with one symbol costs no bits (code_lengths always codes two)
        csp::canonical(S.len[l], n, S.code[l]);
        S.use[l] = u;
    }
    CSP_WAVE_SYNC();
    Vp8lPut P;
    P.begin(S.win, file + 20);
    if (PAL) {
        CSH_SHARED PackPalLds SP;
        vp8l_pal_codes(im.pal + 512, SP.pal);
        P.head_palette(im, SP.pal, SP.desc);
    } else P.head(im, modes, S.len[3], S.code[3], S.use[3]);
    P.put1(0, 1);                                   // the picture: no colour cache
    P.put1(0, 1);                                   // no meta prefix image
    P.code(S.len[0], S.use[0]); P.code(S.len[1], S.use[1]); P.code(S.len[2], S.use[2]); P.code(S.len[4], S.use[4]); P.single();   // green, red, blue, alpha (one symbol, no bits, in an opaque picture), distance
    const uint64_t npx = uint64_t(im.width) * im.height;
    for (uint64_t i0 = 0; i0 < npx; i0 += 64) {
        LV<uint64_t> val; LV<uint32_t> nb;
        LFOR(l) {
            const uint64_t i = i0 + uint32_t(l);
            const uint32_t v = i < npx ? work[im.res_off + i] : 0u;
            const uint32_t g = (v >> 8) & 255u, r = (v >> 16) & 255u, b = v & 255u, a = v >> 24;
            const uint32_t lg = S.len[0][g], lr = S.len[1][r], lb = S.len[2][b], la = S.len[4][a];
            nb[l] = i < npx ? lg + lr + lb + la : 0u;
            val[l] = uint64_t(S.code[0][g]) | (uint64_t(S.code[1][r]) << lg) | (uint64_t(S.code[2][b]) << (lg + lr)) | (uint64_t(S.code[4][a]) << (lg + lr + lb));
        }
        P.bo.put(val, nb);
    }
    P.finish(im, file, PAL ? int(im.parent) : image, file_len, status);
}

// (a palette candidate's record has bw = bh = 0: the residual kernel skips it, its index image is in work already; the counts are taken of every record)
void launch_vp8l_front(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist) {
    CSH_LAUNCH_PHASED(k_vp8l_residuals, 4, dim3(max_blocks, unsigned(nimg)), dim3(256), st, imgs, work, modes);
    CSH_LAUNCH_PHASED(k_vp8l_hist, 3, dim3(unsigned((max_pixels + 4095) / 4096), unsigned(nimg)), dim3(256), st, imgs, work, hist);
}
void launch_vp8l_pack_plain(hipStream_t st, const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const uint32_t *hist, const uint32_t *pick, uint8_t *out, uint32_t *file_len,
                            uint32_t *status) {
    CSH_LAUNCH(k_vp8l_pack<false>, dim3(unsigned(nimg)), dim3(CSP_WAVE_THREADS), st, imgs, nimg, work, modes, hist, pick, out, file_len, status);
}
void launch_vp8l_pack_candidates(hipStream_t st, const Vp8lImg *imgs, int first, int nimg, const uint32_t *work, const uint8_t *modes, const uint32_t *hist, const uint32_t *pick, uint8_t *out,
                                 uint32_t *file_len, uint32_t *status) {
    if (nimg <= first) return;
    CSH_LAUNCH(k_vp8l_pack<true>, dim3(unsigned(nimg - first)), dim3(CSP_WAVE_THREADS), st, imgs + first, nimg - first, work, modes, hist + uint64_t(first) * 1024u, pick + 4 * first, out, file_len, status);
}
void launch_vp8l_encode(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist, uint8_t *out, uint32_t *file_len,
                        uint32_t *status) {
    if (!nimg) return;
    launch_vp8l_front(st, imgs, nimg, max_blocks, max_pixels, work, modes, hist);
    launch_vp8l_pack_plain(st, imgs, nimg, work, modes, hist, nullptr, out, file_len, status);
}

}  // namespace csw
