// tiff_batch.hpp -- the TIFF input batch (route_tiff.cpp) and the container walk behind it (tiff_container.cpp): what a classic TIFF file's IFD chain says, page
// by page, and the values block and IFD of an output page
#pragma once
#include <string>
#include <vector>

#include "../../include/caesium_hip.h"
#include "devmem.hpp"
#include "tiff_kernels.h"

// one IFD entry as the file has it; at / bytes: where its value stands (the entry's own value field when it fits there) -- inside the file, the walk has seen to that
struct cst_entry { uint16_t tag = 0, type = 0; uint32_t count = 0; size_t at = 0, bytes = 0; };
struct cst_page_src {
    uint32_t width = 0, height = 0, spp = 1, bits = 1, comp = 1, rps = 0, tw = 0, tl = 0;
    bool tiled = false;
    uint32_t pred = cst::TIFF_PRED_NONE;   // how the input's rows are differenced
    uint32_t pred_ok = cst::TIFF_PRED_NONE;   // ... and how the output's may be (depth 8 or 16, at most TIFF_PRED_MAX_SPP samples a pixel)
    uint32_t rowbytes = 0, seg_rows = 0, nseg = 0;   // a segment's row, the rows of a whole segment (the last strip has what is left)
    uint64_t decoded = 0;                  // bytes of all segments
    std::vector<uint64_t> seg_off, seg_len;
    std::vector<cst_entry> entries, exif, gps;   // the IFD's entries in file order; with keep_metadata the entries of the private IFDs behind 34665 / 34853
    bool has_exif = false, has_gps = false;
};
struct cst_file {
    bool big_endian = false, pass = false;   // pass: a file this route does not code (DESIGN.md 8.4 lists them): it comes back as it is
    std::vector<cst_page_src> pages;
};
// 0 or CS_ERR_BAD_TIFF with msg
int cst_parse(const uint8_t *d, size_t n, bool keep_metadata, cst_file &f, std::string &msg);
// bytes all segments of all pages decode to (0 when the walk fails or the file is passed through), their rows and segments together, whether a page is Deflate-coded: with
// group_extent
uint64_t cst_declared_bytes(const uint8_t *d, size_t n, uint64_t *units = nullptr, bool *deflate = nullptr);
// the values block and the IFD of an output page, appended to heads (16-aligned) with the positions of its offsets in relocs: compression `comp` (tag 259's number), nout
// segments (strips: of rows_per_strip rows), tag 317 when with_pred
void cst_write_head(const uint8_t *d, const cst_file &f, const cst_page_src &s, bool keep_metadata, uint32_t comp, bool with_pred, uint32_t nout, uint32_t rows_per_strip, std::vector<uint8_t> &heads,
                    std::vector<uint32_t> &relocs, cst::TiffHead &H);

struct cst_batch {
    int device = 0;
    hipStream_t stream = 0;
    bool have_stream = false, keep_metadata = false, ran = false;
    int compression = CST_OUT_NONE;
    uint32_t strip_bytes = 65536;
    const CByteArray *inputs = nullptr;   // borrowed until the batch is destroyed
    struct Item { int code = 0; std::string msg; bool pass = false; int file = -1; uint64_t out_bytes = 0, host_off = 0; };   // host_off: the file in `out`
    std::vector<Item> items;
    std::vector<cst_file> parsed;         // per item (empty for one that failed)
    std::vector<cst::TiffFile> files;     // the device's files: items that parsed and are not passed through
    std::vector<size_t> file_item;
    std::vector<cst::TiffSeg> segs;       // the input's segments, page by page
    std::vector<uint32_t> page_first_seg; // per page of the batch (files[].first_page + page)
    std::vector<uint64_t> page_dec_off;
    std::vector<uint8_t> out;             // the coded files, read back, side by side
    csh::DevBuf<uint8_t> d_dec;
    cst_timing timing;
    ~cst_batch() { if (have_stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }
};
