// gif_kernels.h -- what the GIF kernels (k_gif_lzw.hip, k_gif_anim.hip) and their host side (gif_container.cpp, route_gif.cpp) share: the frame and file
// records of a batch, the walk's modes, the launchers.  One input frame is one output frame; DESIGN.md 8.3 holds the output rule.
#pragma once
#include "gpu_rt.h"

namespace csg {

enum : uint32_t { GIF_INTERLACED = 1u };
enum : uint32_t { GIF_NO_INDEX = 0xFFFFFFFFu };   // a frame without a transparent index
enum { GIF_WALK_STATS = 0, GIF_WALK_PACK = 1, GIF_WALK_CANVAS = 2 };
enum : uint32_t { GIF_STAT = 8 };                 // per frame: C_k as x0 y0 x1 y1, U_k as x0 y0 x1 y1 (a box is empty while x0 > x1)
enum : uint32_t { GIF_OK = 0, GIF_BAD_CODE = 1, GIF_SHORT = 2 };   // a frame's decode status
enum : uint32_t { GIF_FLAG_PALETTE = 1u, GIF_FLAG_HOLD = 2u };     // a file's fallback flags: a colour its frame's table lacks / a pixel that cannot be left alone

struct GifFrame {
    uint32_t x, y, w, h;          // the input rectangle
    uint32_t ox, oy, ow, oh;      // the output rectangle R_k (host, from the statistics)
    uint32_t flags, disposal;     // GIF_INTERLACED; the input's disposal method 0..3
    uint32_t odisposal;           // the output's: 1 or 2
    uint32_t transparent;         // the transparent index, or GIF_NO_INDEX
    uint32_t mcs, omcs;           // LZW minimum code size of the input data and of the output
    uint32_t pal, pal_n;          // colour table (256 words at pal * 256 of the table pool) and how many entries it has
    uint32_t data_len;            // bytes of the LZW stream
    uint32_t first_chunk, nchunks;
    uint32_t head_len;            // bytes in front of the coded data: graphic control extension, image descriptor, local table, code size (frame 0: the file's header too)
    uint64_t data_off, idx_off;   // the stream in the input pool; the decoded rectangle in the index pool
    uint64_t out_off, head_off;   // the output rectangle in the pack pool; the head bytes in the head pool
};
struct GifFile { uint32_t first, nframes, cw, ch; uint64_t out_off; };
struct GifChunk { uint32_t frame, index; uint64_t buf_off; };   // chunk `index` of an output frame's index stream; its bits in the chunk pool
// what k_gif_layout leaves per frame: where the frame starts in its file, and the bytes of its merged LZW stream
struct GifPlace { uint64_t pos; uint64_t data_bytes; };

// bytes a chunk of n pixels can code to at most: a code per pixel, a clear code per 2048 of them (a table lasts ~4000 codes), the closing codes; a multiple of 8
__host__ __device__ static inline uint64_t gif_chunk_cap(uint64_t n) { return ((((n + n / 2048 + 8) * 12 + 7) / 8 + 8 + 7) / 8) * 8; }

void launch_gif_lzw_decode(hipStream_t st, const GifFrame *frames, uint32_t nframes, const uint8_t *data, uint8_t *indices, uint32_t *status);
void launch_gif_anim(hipStream_t st, int mode, const GifFile *files, uint32_t nfiles, uint64_t max_px, const GifFrame *frames, const uint8_t *indices, const uint32_t *tables, const uint8_t *canon,
                     uint32_t *stats, uint32_t *file_flags, uint8_t *pool, uint32_t target);
void launch_gif_lzw_encode(hipStream_t st, const GifFrame *frames, const GifChunk *chunks, uint32_t nchunks, const uint8_t *pack, uint8_t *cbuf, uint32_t *cbits, uint32_t chunk_px);
// the lossy coder (CSH_GIF=lossy, D > 0).  A table's candidate rows: cand[(table * 256 + b) * 64 + l], l < count[table * 256 + b], is b itself (l = 0), then the
// canonical indices below the table's n whose colour lies within D of b's, by (distance squared, index), 63 at most
enum : uint32_t { GIF_NEAR_ROW = 64 };
void launch_gif_near(hipStream_t st, const uint32_t *tables, const uint8_t *canon, const uint32_t *table_n, uint32_t ntables, uint32_t dist, uint8_t *cand, uint8_t *count);
void launch_gif_lzw_encode_lossy(hipStream_t st, const GifFrame *frames, const GifChunk *chunks, uint32_t nchunks, const uint8_t *pack, const uint8_t *cand, const uint8_t *count, uint8_t *cbuf,
                                 uint32_t *cbits, uint32_t chunk_px);
void launch_gif_layout(hipStream_t st, const GifFile *files, uint32_t nfiles, const GifFrame *frames, const uint32_t *cbits, uint64_t *cstart, GifPlace *place, uint64_t *file_bytes);
void launch_gif_frame_head(hipStream_t st, const GifFile *files, const GifFrame *frames, const uint32_t *frame_file, uint32_t nframes, const uint8_t *heads, const GifPlace *place, uint8_t *out);
void launch_gif_merge(hipStream_t st, const GifFile *files, const GifFrame *frames, const uint32_t *frame_file, const GifChunk *chunks, uint32_t nchunks, const uint8_t *cbuf, const uint32_t *cbits,
                      const uint64_t *cstart, const GifPlace *place, uint8_t *out);

}  // namespace csg
