// tiff_kernels.h -- what the TIFF kernels (k_tiff.hip) and their host side (tiff_container.cpp, route_tiff.cpp) share: the segment, page and file records of a
// batch and the launchers.  A segment is one strip or one tile; DESIGN.md 8.4 holds the output rule and the layout of the output.
#pragma once
#include "gpu_rt.h"

namespace cst {

enum : uint32_t { TIFF_OK = 0, TIFF_BAD_CODE = 1, TIFF_SHORT = 2 };   // a segment's decode status
enum : uint32_t { TIFF_C_NONE = 1, TIFF_C_LZW = 5, TIFF_C_DEFLATE = 8, TIFF_C_ADOBE_DEFLATE = 32946, TIFF_C_PACKBITS = 32773 };   // tag 259
enum : uint32_t { TIFF_PRED_NONE = 0, TIFF_PRED_8 = 1, TIFF_PRED_16LE = 2, TIFF_PRED_16BE = 3 };   // how a row is differenced: bytes, or 16-bit words in the file's byte order
enum : uint32_t { TIFF_PRED_MAX_SPP = 64 };   // the un-predictor scans windows of whole pixels across the 64 lanes

// an input segment: its coded bytes in the input pool, its decoded bytes (rows x rowbytes) in the decoded pool -- the segments of a page stand back to back
// there, so a page of strips is one picture of height x rowbytes bytes, whichever way it was cut
struct TiffSeg {
    uint64_t data_off, dec_off;
    uint32_t data_len, dec_len;
    uint32_t comp;                 // TIFF_C_*
    uint32_t rowbytes, rows, row_base;   // row_base: the segment's first row among the batch's predicted rows (un-predictor: a wave a row)
    uint32_t pred, spp;            // TIFF_PRED_*; samples per pixel = the differencing stride in samples
};
// an output segment: bytes [src_off, src_off + len) of the decoded pool (and of the predicted pool), coded into the code pool at buf_off (variant 1, with Predictor
// 2, at buf_off + cap)
struct TiffOut {
    uint64_t src_off, buf_off;
    uint32_t len, cap;
    uint32_t rowbytes, rows, row_base;   // row_base: the segment's first row among the batch's output rows (PackBits: a wave a row)
    uint32_t pred, spp, page;
};
// the values block and the IFD of an output page as the host wrote them (variant 1: with tag 317), offsets in them relative to the blob
struct TiffHead {
    uint64_t off;                  // in the head pool
    uint32_t len;                  // values block, then the IFD; the last four bytes are the next-IFD pointer
    uint32_t ifd_pos;              // where the IFD begins
    uint32_t off_pos, cnt_pos;     // where the segments' offsets and byte counts go (LONGs): the arrays in the values block, or the entries' value fields (one segment)
    uint32_t reloc_first, nreloc;  // positions (head pool of relocs) of the LONG offsets the blob's place in the file is added to
};
struct TiffPage {
    uint32_t file, first_out, nout, both;   // both: coded with and without Predictor 2, the smaller sum wins
    TiffHead head[2];
};
struct TiffFile { uint32_t first_page, npages, big_endian, pad; uint64_t out_off; };
// what k_tiff_layout leaves per page
struct TiffPlace { uint64_t head_pos, next_ifd; uint32_t variant, pad; };

// bytes an LZW segment of n bytes can code to at most: a code per byte, a Clear per 3837 of them (entries 258 .. 4094) and the one in front, the code behind the
// last one, EOI; 12 bits each, written in words; a multiple of 16
__host__ __device__ static inline uint32_t tiff_lzw_cap(uint32_t n) { return uint32_t((((uint64_t(n) + n / 2048u + 8u) * 12u + 7u) / 8u + 8u + 15u) / 16u * 16u); }
// ... and a PackBits row of n bytes: a header per 128 literal bytes; a segment of rows: the rows' sum, to a multiple of 16
__host__ __device__ static inline uint32_t tiff_packbits_row_cap(uint32_t n) { return n + (n + 127u) / 128u; }
__host__ __device__ static inline uint32_t tiff_packbits_cap(uint32_t rowbytes, uint32_t rows) { return uint32_t((uint64_t(tiff_packbits_row_cap(rowbytes)) * rows + 15u) / 16u * 16u); }

void launch_tiff_lzw_decode(hipStream_t st, const TiffSeg *segs, const uint32_t *which, uint32_t n, const uint8_t *data, uint8_t *dec, uint32_t *status);
void launch_tiff_packbits_decode(hipStream_t st, const TiffSeg *segs, const uint32_t *which, uint32_t n, const uint8_t *data, uint8_t *dec, uint32_t *status);
// uncompressed segments: data -> dec (SHORT when the data is shorter than the segment); inflated segments: scratch (at scratch_off[i]) -> dec; max_len: the longest of them
void launch_tiff_place(hipStream_t st, const TiffSeg *segs, const uint32_t *which, uint32_t n, uint32_t max_len, const uint8_t *src, const uint64_t *scratch_off, uint8_t *dec, uint32_t *status);
void launch_tiff_unpredict(hipStream_t st, const TiffSeg *segs, const uint32_t *row_seg, uint32_t nrows, uint8_t *dec);
void launch_tiff_predict(hipStream_t st, const TiffOut *outs, const uint32_t *row_out, uint32_t nrows, const uint8_t *dec, uint8_t *pred);
void launch_tiff_lzw_encode(hipStream_t st, const TiffOut *outs, uint32_t nouts, const uint8_t *dec, const uint8_t *pred, uint8_t *cbuf, uint32_t *cbytes);
void launch_tiff_packbits_encode(hipStream_t st, const TiffOut *outs, const uint32_t *row_out, uint32_t nrows, uint32_t nouts, const uint8_t *dec, uint32_t *row_len, uint32_t *row_start, uint8_t *cbuf,
                                 uint32_t *cbytes);
void launch_tiff_layout(hipStream_t st, const TiffFile *files, uint32_t nfiles, const TiffPage *pages, const TiffOut *outs, uint32_t nouts, const uint32_t *cbytes, int raw, uint64_t *seg_pos, uint32_t *seg_bytes,
                        TiffPlace *place, uint64_t *file_bytes);
void launch_tiff_gather(hipStream_t st, const TiffFile *files, const TiffPage *pages, uint32_t npages, const TiffOut *outs, uint32_t nouts, const uint8_t *dec, const uint8_t *cbuf, int raw, const uint8_t *heads,
                        const uint64_t *seg_pos, const uint32_t *seg_bytes, const TiffPlace *place, uint8_t *out);
void launch_tiff_patch(hipStream_t st, const TiffFile *files, const TiffPage *pages, uint32_t npages, const uint32_t *relocs, const uint64_t *seg_pos, const uint32_t *seg_bytes, const TiffPlace *place, uint8_t *out);

}  // namespace cst
