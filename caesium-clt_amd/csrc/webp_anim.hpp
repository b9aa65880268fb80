// webp_anim.hpp -- the WebP input batch (webp_decode.cpp) as webp_anim.cpp sees it: a still file is one picture of the batch, an animated file a range of
// pictures (one per ANMF frame) and the header fields its output keeps
#pragma once
#include <string>
#include <vector>

#include "../../include/caesium_hip.h"
#include "devmem.hpp"
#include "webp_kernels.h"
#include "vp8_dec.h"

struct cswd_anim {
    uint32_t cw = 0, ch = 0, background = 0, loops = 0;
    std::vector<csw::AnimFrame> frames;   // image, x, y, w, h, flags (ANIM_KEY included) as the file states them
    std::vector<uint32_t> duration;       // per frame, 24 bits
};

struct cswd_batch {
    int device = 0;
    hipStream_t stream = 0;
    bool have_stream = false;
    struct Item { int code = 0; std::string msg; int image = -1, anim = -1; };   // a still file: image; an animated file: anim
    std::vector<Item> items;
    std::vector<cswd_anim> anims;
    std::vector<csw::Vp8In> imgs;
    std::vector<uint8_t> pool;
    csh::DevBuf<uint8_t> d_pool, d_work, d_rgb;
    csh::DevBuf<csw::Vp8In> d_imgs;
    uint64_t work_bytes = 0, rgb_bytes = 0;
    bool ran = false;
    ~cswd_batch() { if (have_stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }   // nothing queued may outlive the device blocks
};

// ANIM and every ANMF of an animated file (webp_anim.cpp).  Fills a (frames[k].image = k) and, per frame, where its bitstream and its ALPH chunk lie in the
// file; 0 or a CS_ERR_* code with msg
struct cswd_frame_src { size_t off = 0, len = 0, alph_off = 0, alph_len = 0; bool lossless = false; };
int cswd_parse_anim(const uint8_t *d, size_t n, cswd_anim &a, std::vector<cswd_frame_src> &src, std::string &msg);
