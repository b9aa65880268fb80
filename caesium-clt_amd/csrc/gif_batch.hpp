// gif_batch.hpp -- the GIF input batch (route_gif.cpp) and the container walk behind it (gif_container.cpp): what a file's blocks say, frame by frame, with
// every frame's LZW data joined into one stream
#pragma once
#include <string>
#include <vector>

#include "../../include/caesium_hip.h"
#include "devmem.hpp"
#include "gif_kernels.h"

struct csg_range { size_t off = 0, len = 0; };   // bytes of the source file
struct csg_frame_src {
    uint32_t x = 0, y = 0, w = 0, h = 0, disposal = 0, delay = 0, mcs = 0;
    int transparent = -1;
    bool interlaced = false;
    csg_range lct;               // the local colour table's bytes; len 0: the frame uses the global table
    std::vector<uint8_t> data;   // the data sub-blocks, joined
};
struct csg_file {
    uint32_t cw = 0, ch = 0;
    uint8_t lsd[7] = {0};        // the logical screen descriptor as the file has it
    csg_range gct, loop;         // the global colour table; the whole NETSCAPE2.0 extension block
    std::vector<csg_range> meta; // comment extensions and the other application extensions, whole blocks in file order
    std::vector<csg_frame_src> frames;
    bool plain_text = false;     // a plain-text extension draws glyphs: the file is passed through
};
// 0 or CS_ERR_BAD_GIF with msg
int csg_parse(const uint8_t *d, size_t n, csg_file &f, std::string &msg);
// canvas x frames from a block walk that reads no data (0 when the header does not say)
uint64_t csg_declared_pixels(const uint8_t *d, size_t n);
// what stands in front of the first frame of the output: GIF89a, the screen descriptor, the global table, the loop extension, the kept extensions
void csg_write_file_head(const uint8_t *d, const csg_file &f, bool keep_metadata, std::vector<uint8_t> &out);
// what stands in front of frame k's data: graphic control extension, image descriptor (never interlaced), local table, minimum code size
void csg_write_frame_head(const uint8_t *d, const csg_frame_src &s, const csg::GifFrame &g, std::vector<uint8_t> &out);

struct csg_batch {
    int device = 0;
    hipStream_t stream = 0;
    bool have_stream = false, keep_metadata = false, ran = false;
    const CByteArray *inputs = nullptr;   // borrowed until the batch is destroyed
    struct Item { int code = 0; std::string msg; bool pass = false, palette = false, not_smaller = false; int file = -1; uint64_t out_bytes = 0; };
    std::vector<Item> items;
    std::vector<csg_file> parsed;         // per item (empty for one that failed)
    std::vector<csg::GifFile> files;      // the device's files: items that parsed and are not passed through
    std::vector<size_t> file_item;
    std::vector<csg::GifFrame> frames;
    std::vector<uint32_t> frame_file;
    std::vector<uint8_t> out;             // the device's output pool, read back
    csh::DevBuf<uint8_t> d_data, d_idx, d_canon, d_cand, d_cand_n;   // (the candidate rows and their lengths: a lossy batch with a distance alone)
    csh::DevBuf<uint32_t> d_tables, d_table_n;
    csh::DevBuf<csg::GifFrame> d_frames;
    csh::DevBuf<csg::GifFile> d_files;
    uint32_t chunk_pixels = 16384;
    uint32_t distance = 0;                // D of the lossy coder; 0: the exact coder
    uint32_t ntables = 0;                 // tables d_cand holds rows for (0 without a distance)
    csg_timing timing;
    ~csg_batch() { if (have_stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }
};
