// webp_kernels.h -- the lossy WebP row on the device: descriptors and launchers (k_webp.hip: import and coder back end; k_vp8enc.hip:
// libwebp's encoder).  Statement: oracle/vp8enc_oracle.c (pinned to libwebp's WebPEncode byte for byte) and oracle/webp_oracle.c (the import).
#pragma once
#include <vector>

#include "gpu_rt.h"

namespace csh { template <class T> struct DevBuf; }

namespace csw {

enum { WEBP_MB_REC = 432 };   // int16 per macroblock in the level pool: 25 blocks x 16 levels + the info block (k_webp.hip)

struct WebpImg {
    uint32_t width, height, mbw, mbh, ncomp;   // ncomp: samples per input pixel: 3 = interleaved RGB, 1 = grey, 4 / 2 = the same with an alpha sample behind (skipped here)
    int32_t quality;                           // libwebp's quality 0..100
    uint32_t cls, qtab;                        // set by launch_webp_encode: the picture's size class (its plan of steps) and its quality table
    uint64_t rgb_off;                          // input pixels in the RGB pool
    uint64_t y_off, u_off, v_off;              // source planes, padded to whole macroblocks (work pool)
    uint64_t ry_off, ru_off, rv_off;           // the encoder's reconstruction (what a decoder will see)
    uint64_t lev_off;                          // quantised levels: WEBP_MB_REC int16 per macroblock (int16 index)
    uint64_t out_off;                          // output file region
    uint32_t out_cap;
    uint32_t image;                            // index of the image in the batch's status / size arrays
};

void launch_webp_yuv(hipStream_t st, const WebpImg *imgs, int nimg, uint32_t max_luma, const uint8_t *rgb, uint8_t *work);
// the encoder behind the import: analysis, segments, the macroblock loop step by step, statistics, then the two partitions and the file.  himgs: the host's
// pictures (cls / qtab are filled in here and the array copied over d_imgs, which the caller uploaded for launch_webp_yuv);
// scratch: a second region laid out like the output pool; part_size: nimg x 2.  `mid` (optional) is recorded between the macroblock loop and the coder.
// Returns with the stream idle; != 0 on an allocation / launch failure.
int launch_webp_encode(hipStream_t st, WebpImg *himgs, int nimg, WebpImg *d_imgs, uint8_t *work, int16_t *levels, uint8_t *scratch, uint32_t *part_size, uint8_t *out,
                       uint32_t *img_size, uint32_t *status, hipEvent_t mid);
struct Vp8FrameDev;
int launch_webp_backend(hipStream_t st, const WebpImg *imgs, const WebpImg *himgs, int nimg, const int16_t *levels, const Vp8FrameDev *frames, const std::vector<uint64_t> &base,
                        const uint64_t *d_base, csh::DevBuf<uint32_t> &d_cnt, const uint16_t *d_blk, uint8_t *scratch, uint32_t *part_size, uint8_t *out, uint32_t *img_size, uint32_t *status);

enum { VP8L_ALPHA_OF = 16 };   // Vp8lImg::channels = VP8L_ALPHA_OF + 2 / + 4: code the alpha sample of a grey + alpha / RGBA picture as a grey picture
// lossless WebP output (k_vp8l_enc.hip): one picture of 8-bit grey (channels 1), grey + alpha (2), RGB (3) or RGBA (4) pixels in device memory
struct Vp8lImg {
    const uint8_t *rgb;
    uint32_t width, height, channels, bw, bh;   // bw x bh blocks of 16 x 16 pixels
    uint64_t res_off;      // residual ARGB, one u32 per pixel (u32 index into the work pool)
    uint64_t mode_off;     // predictor mode of every block (byte index)
    uint64_t out_off;      // output file region
    uint32_t out_cap;
    // CSH_VP8L=refs only (k_vp8l_refs.hip); zero in plain mode
    uint32_t nchunk;       // chunks of VP8L_CHUNK positions of the scan order
    uint64_t tok_off;      // one u64 per pixel (u64 index into the token pool): the match candidate, then the parse's token
    uint64_t hit_off;      // one byte per pixel: bit k = the pixel hits the colour cache of option k (vp8l_cache_bits)
    uint64_t cst_off;      // colour-cache contents in front of every chunk, every option (u64 index): nchunk x VP8L_CACHE_STATE
    // CSH_VP8L=palette only (k_vp8l_palette.hip), and only in a CANDIDATE record: the bundled palette indices of picture `parent` as one more picture for the
    // refs stages.  width is then the packed width, bw = bh = 0 (no predictor: the front end's residual kernel has no block of it), out_off / out_cap the parent's
    const uint32_t *pal;   // this candidate's VP8L_PAL_BLOCK words (nullptr: a picture)
    uint32_t pal_n;        // colours, 1 .. 256
    uint32_t parent;       // the picture's record: its file region, its file_len / status entry
    uint32_t src_width;    // the picture's width
};
void launch_vp8l_encode(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist, uint8_t *out, uint32_t *file_len,
                        uint32_t *status);
// the same with backward references and a colour cache (CSH_VP8L=refs, k_vp8l_refs.hip); a picture whose stream would not be smaller is written by the plain coder
enum : uint32_t {
    VP8L_CHUNK = 4096,                    // positions per wave in the match, parse and cache stages
    VP8L_MAX_LEN = 4096,                  // the format's longest copy
    VP8L_WINDOW = (1u << 20) - 120,       // the farthest distance (libwebp's)
    VP8L_NOPT = 4,                        // colour-cache sizes tried per picture: vp8l_cache_bits(0 .. 3)
    VP8L_CACHE_STATE = 16 + 128 + 1024,   // slots of all the options with a cache
    VP8L_GREEN_MAX = 256 + 24 + 1024,     // the widest green alphabet
    VP8L_HIST = VP8L_GREEN_MAX + 3 * 256 + 40,   // counts of one option: green, red, blue, alpha, distance
    VP8L_LENS = 5 * VP8L_GREEN_MAX,       // code lengths of the chosen option, VP8L_GREEN_MAX bytes per code
};
__host__ __device__ static inline uint32_t vp8l_cache_bits(uint32_t opt) { return opt == 0 ? 0u : 1u + 3u * opt; }   // 0 (no cache), 4, 7, 10
struct Vp8lRefs {
    uint64_t *tok;         // tokens (Vp8lImg::tok_off)
    uint8_t *hit;          // cache hits (hit_off)
    uint64_t *cst;         // cache contents (cst_off)
    uint32_t *hist;        // per picture VP8L_NOPT x VP8L_HIST counts, zeroed by the caller
    uint8_t *lens;         // per picture VP8L_LENS
    uint32_t *pick;        // per record 4 words: who writes (0 the plain pack, 1 the refs pack, 2 neither: another record of the picture does, 3 the groups pack), the option, the two streams' bits behind the head
    // CSH_VP8L=groups only (k_vp8l_groups.hip); nullptr in the other modes
    const struct Vp8lGroupImg *gimg;   // per picture: its tiles
    uint8_t *label;        // per tile its group (Vp8lGroupImg::tile_off)
    uint32_t *feat;        // per tile VP8L_TILE_FEAT folded counts
    uint32_t *ghist;       // per picture VP8L_MAX_GROUPS x VP8L_HIST counts of the chosen option, zeroed by the caller
    uint8_t *glens;        // per picture VP8L_MAX_GROUPS x VP8L_LENS
    unsigned long long *ginfo;   // per picture VP8L_GROUP_INFO words: the number of groups (0: no grouped candidate), then every group's bits (descriptions and symbols)
};
void launch_vp8l_encode_refs(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &refs,
                             uint8_t *out, uint32_t *file_len, uint32_t *status);
// the two halves of launch_vp8l_encode_refs, for a caller that looks at pick in between (k_vp8l_palette.hip): everything up to the codes and pick; the two packs
void launch_vp8l_refs_stages(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &refs);
void launch_vp8l_refs_packs(hipStream_t st, const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const uint32_t *hist, const Vp8lRefs &refs, uint8_t *out, uint32_t *file_len,
                            uint32_t *status);
// the colour-indexing transform (CSH_VP8L=palette, k_vp8l_palette.hip).  A picture with at most VP8L_PAL_MAX distinct ARGB values gets a candidate record behind
// the pictures' records; the smallest of the picture's plain stream, its refs stream and the candidate's is written
enum : uint32_t {
    VP8L_PAL_MAX = 256,                   // the format's largest palette
    VP8L_PAL_SLOTS = 1024,                // hash slots of the colour count, per picture (u64 each: bit 32 = in use, the low word the ARGB)
    VP8L_PAL_STRIP = 16384,               // pixels per wave of the colour count
    VP8L_PAL_HIST = 288 + 3 * 256 + 40,   // counts of the palette's sub-image: green (as an alphabet of 280), red, blue, alpha, distance (none)
    VP8L_PAL_BLOCK = 2 * 256 + VP8L_PAL_HIST,   // per candidate: the palette ascending, its sub-image (entry minus predecessor), the counts
};
__host__ __device__ static inline uint32_t vp8l_pal_bits(uint32_t n) { return n <= 2 ? 3u : n <= 4 ? 2u : n <= 16 ? 1u : 0u; }   // 1 << bits indices per packed pixel
// count[i] of picture i < nimg: its distinct ARGB values if there are at most VP8L_PAL_MAX, something larger otherwise.  tabs: nimg x VP8L_PAL_SLOTS, zeroed like count
void launch_vp8l_pal_count(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, unsigned long long *tabs, uint32_t *count);
// imgs: nparent pictures, then ncand candidates (in the order of their parents).  Sorts the palettes, writes the candidates' index images into work, runs the refs
// stages over all the records, chooses per picture and packs
void launch_vp8l_encode_palette(hipStream_t st, const Vp8lImg *imgs, int nparent, int ncand, uint32_t max_blocks, uint64_t max_pixels, uint64_t max_packed, const unsigned long long *tabs,
                                uint32_t *pal, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &refs, uint8_t *out, uint32_t *file_len, uint32_t *status);
// the literals-only stream of the candidates first .. nimg - 1 whose pick[4 i] is 0 (k_vp8l_enc.hip: the plain pack with the palette's head; launch_vp8l_pack_plain
// itself passes candidates by)
void launch_vp8l_pack_candidates(hipStream_t st, const Vp8lImg *imgs, int first, int nimg, const uint32_t *work, const uint8_t *modes, const uint32_t *hist, const uint32_t *pick, uint8_t *out,
                                 uint32_t *file_len, uint32_t *status);
// the meta prefix (entropy) image (CSH_VP8L=groups, k_vp8l_groups.hip): everything CSH_VP8L=palette does, and for every picture one more candidate, its refs stream
// coded with up to VP8L_MAX_GROUPS sets of five prefix codes, one set per tile of (1 << bits)^2 pixels; written where it is strictly the smallest
enum : uint32_t {
    VP8L_MAX_GROUPS = 8,
    VP8L_MAX_TILES = 4096,                // per picture: the tile side is the smallest of 32 .. 512 that keeps to it
    VP8L_TILE_FEAT = 64,                  // folded counts per tile: 15 magnitude classes for each of green, red, blue, alpha; cache hits; copies; two unused
    VP8L_GROUP_INFO = 16,
};
struct Vp8lGroupImg {
    uint32_t bits;         // the tile side's log2, 5 .. 9; 0: the picture is one tile and has no grouped candidate
    uint32_t tw, th, ntile;
    uint64_t tile_off;     // the picture's first tile in the label pool (x VP8L_TILE_FEAT: in the feature pool)
};
__host__ __device__ static inline uint32_t vp8l_group_bits(uint32_t width, uint32_t height) {
    for (uint32_t b = 5; b < 9; b++) if (uint64_t((width + (1u << b) - 1) >> b) * ((height + (1u << b) - 1) >> b) <= VP8L_MAX_TILES) return b;
    return 9u;             // 16384 x 16384: 32 x 32 tiles
}
// behind launch_vp8l_refs_stages, for the pictures 0 .. nimg - 1: tile features, clustering, group histograms, group codes, the choice (pick[4 i] = 3 where the grouped
// stream is strictly smaller than the picture's two others); then the pack of those pictures
void launch_vp8l_group_stages(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_tiles, const uint32_t *work, const Vp8lRefs &refs);
void launch_vp8l_pack_groups(hipStream_t st, const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const Vp8lRefs &refs, uint8_t *out, uint32_t *file_len, uint32_t *status);
// launch_vp8l_encode_palette with the group stages between the refs stages and the palette's choice; max_tiles: the largest Vp8lGroupImg::ntile
void launch_vp8l_encode_groups(hipStream_t st, const Vp8lImg *imgs, int nparent, int ncand, uint32_t max_blocks, uint64_t max_pixels, uint64_t max_packed, uint32_t max_tiles,
                               const unsigned long long *tabs, uint32_t *pal, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &refs, uint8_t *out, uint32_t *file_len, uint32_t *status);
// a match finder over the whole window (CSH_VP8L=far, k_vp8l_far.hip): everything CSH_VP8L=groups does, and for every record a second token set from a hash chain
// over the whole record; the record keeps the set whose best stream is strictly smaller.  All of these pools exist in this mode only
enum : uint32_t {
    VP8L_FAR_LINKS = 8,                   // links walked per position
    VP8L_FAR_BLOCK = VP8L_CHUNK,          // entries per block of the sort
    VP8L_FAR_NONE = 0xFFFFFFFFu,          // prev: no link
    VP8L_FAR_TOT = 3 * 256 + 8,           // per record: the digit totals of the three passes, then the number of positions with a link
};
struct Vp8lFar {
    uint32_t *pos[2];      // the positions on their way through the sort, one u32 per pixel each (Vp8lImg::res_off)
    uint32_t *prev;        // per pixel (res_off): the nearest earlier position with the same hash, or VP8L_FAR_NONE
    uint32_t *cnt;         // per chunk of every record 256 digit counts: a record's are at 256 x (cst_off / VP8L_CACHE_STATE), digit-major
    uint32_t *dtot;        // per record VP8L_FAR_TOT words, zeroed by the caller
    uint32_t *won;         // per record: 1 where the second set replaced the first
    Vp8lRefs B;            // the second set's pools; hit, cst and gimg are the first set's (they do not depend on tokens), hist / ghist / ginfo zeroed by the caller
};
// the chain of the records 0 .. nimg - 1 into far.prev; the second set's candidates into far.B.tok (k_vp8l_match's fixed distances, then the chain)
void launch_vp8l_far_links(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, const uint32_t *work, const Vp8lFar &far);
void launch_vp8l_far_match(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, const uint32_t *work, const Vp8lFar &far);
// behind launch_vp8l_refs_stages and launch_vp8l_group_stages, in front of the palette's choice: the chain, the second set through the stages that depend on
// tokens, the choice per record, and the second set's pools over the first's where it won
void launch_vp8l_far_stages(hipStream_t st, const Vp8lImg *imgs, int nparent, int nimg, uint64_t max_pixels, uint32_t max_tiles, const uint32_t *work, const uint32_t *hist, const Vp8lRefs &refs,
                            const Vp8lFar &far);
// the stages of launch_vp8l_refs_stages that depend on tokens, over refs.tok as a match finder left it: the parse, the counts, the codes and pick (k_vp8l_refs.hip)
void launch_vp8l_token_stages(hipStream_t st, const Vp8lImg *imgs, int nimg, uint64_t max_pixels, const uint32_t *work, const uint32_t *hist, const Vp8lRefs &refs);
// launch_vp8l_encode_groups with launch_vp8l_far_stages in it
void launch_vp8l_encode_far(hipStream_t st, const Vp8lImg *imgs, int nparent, int ncand, uint32_t max_blocks, uint64_t max_pixels, uint64_t max_packed, uint32_t max_tiles,
                            const unsigned long long *tabs, uint32_t *pal, uint32_t *work, uint8_t *modes, uint32_t *hist, const Vp8lRefs &refs, const Vp8lFar &far, uint8_t *out, uint32_t *file_len,
                            uint32_t *status);
// pieces of launch_vp8l_encode (k_vp8l_enc.hip) the refs coder runs as they are: the front end, and the plain pack for the pictures whose pick[4 i] is 0 (pick = nullptr: all)
void launch_vp8l_front(hipStream_t st, const Vp8lImg *imgs, int nimg, uint32_t max_blocks, uint64_t max_pixels, uint32_t *work, uint8_t *modes, uint32_t *hist);
void launch_vp8l_pack_plain(hipStream_t st, const Vp8lImg *imgs, int nimg, const uint32_t *work, const uint8_t *modes, const uint32_t *hist, const uint32_t *pick, uint8_t *out, uint32_t *file_len,
                            uint32_t *status);

struct Vp8In;
// lossy WebP inputs (k_webp_dec.hip): every image's VP8 key frame -> RGB in the pixel pool; imgs[i].status = 0 or an error
void launch_vp8_decode(hipStream_t st, const uint8_t *pool, Vp8In *imgs, int n, uint8_t *work, uint8_t *rgb, int nsteps, int psteps_lossless, int psteps_alpha);
void launch_rgba_join(hipStream_t st, const uint8_t *rgb, const uint8_t *alpha, uint8_t *rgba, uint64_t npx);

// animated WebP inputs (k_webp_anim.hip): the canvases of a file rebuilt from its decoded frames (libwebp's AnimDecoder: blend and dispose), and what changed
// from one canvas to the next.  Every frame is a picture of the decode batch; a lane owns a canvas pixel and walks the file's frames in order
enum : uint32_t {
    ANIM_DISPOSE = 1,      // AnimFrame::flags: the frame's rectangle is cleared before the next frame (ANMF bit 0)
    ANIM_NO_BLEND = 2,     // the frame replaces what is under it (ANMF bit 1)
    ANIM_KEY = 4,          // set by the host: the canvas is cleared in front of this frame and the frame copied in (anim_key_frames)
    ANIM_HOLES = 8,        // output: the rectangle is written in blend form, an unchanged pixel as 0x00000000
};
enum : uint32_t { ANIM_STAT = 8 };   // words per frame of the statistics
struct AnimFrame {
    uint32_t image;        // the frame's picture: its Vp8In record
    uint32_t x, y, w, h;   // where it lies on the canvas
    uint32_t flags;
    // the frame as it is written again, set by the host between the two walks
    uint32_t ox, oy, ow, oh;
    uint32_t split;        // 1: RGB (3 bytes per pixel) at out_off and the alpha plane at a_off, for the lossy encoder; 0: RGBA at out_off
    uint64_t out_off, a_off;   // in the rectangle pool
};
struct AnimFile { uint32_t first, nframes, cw, ch; };   // a file's frames in the frame array, its canvas
// statistics of frame k against canvas k - 1, ANIM_STAT words: the bounding box of the changed pixels (min x, min y, max x, max y; the minima start at ~0),
// how many pixels changed, how many of those are not opaque; word 6 (the pack walk): 1 where the written rectangle holds an alpha below 255
enum { ANIM_WALK_STATS = 0, ANIM_WALK_PACK = 1, ANIM_WALK_CANVAS = 2 };
// mode ANIM_WALK_STATS: the statistics; ANIM_WALK_PACK: every frame's output rectangle into `pool`; ANIM_WALK_CANVAS: canvas `frame` of the one file given,
// as RGBA, into `pool`.  max_px: the largest canvas of the files, in pixels
void launch_webp_anim(hipStream_t st, int mode, const AnimFile *files, int nfiles, uint64_t max_px, const AnimFrame *frames, const Vp8In *imgs, const uint8_t *rgb, uint32_t *stats, uint8_t *pool,
                      uint32_t frame);

}  // namespace csw
