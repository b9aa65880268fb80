// png_batch.hpp -- the PNG batch object (csp_batch): its members grouped by the step that owns them.  png_container.cpp is the host-only
// container logic, png_plan.cpp fills the batch (png_create drives the steps), png_reduce.cpp is the reduction step between decode and
// filter, png_run.cpp pushes the batch through the kernels and fetches the files, png_convert.cpp holds the resize front half and the
// converters that go through pixels.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/caesium_hip.h"
#include "devmem.hpp"
#include "png_kernels.h"
#include "png_parse.h"
#include "webp_kernels.h"

namespace csp {

struct PngItem {
    int code = 0;
    std::string msg;
    int image = -1;
    size_t file_size = 0;
    uint32_t width = 0, height = 0, rowbytes = 0, bpp = 0, channels = 0, depth = 0, ctype = 0;
    bool no_reduce = false;   // a carried chunk is tied to the colour type (tRNS, bKGD, sBIT)
    bool pal_tied = false;    // a carried chunk counts on the palette as it is (bKGD, sBIT, hIST): an indexed image keeps its depth
    bool interlace = false;   // Adam7 input (the output never is)
    bool has_plte = false, has_trns = false;
    std::vector<uint8_t> plte, trns;                // PLTE / tRNS payloads (conversion to WebP and the resize read them)
    std::vector<std::pair<size_t, size_t>> idat;   // (offset, length) of every IDAT payload in the input
    size_t idat_len = 0;
    std::vector<uint8_t> prefix, suffix;            // output bytes in front of / behind the IDAT chunk
    bool transparent() const { return ctype == 4 || ctype == 6 || has_trns; }
};

enum PngMode { MODE_PNG = 0, MODE_WEBP = 1, MODE_DECODE = 2, MODE_DECODE_ANY = 3 };   // DECODE: the front half of a resize (no 16-bit); DECODE_ANY: of a conversion to JPEG
struct PreFail { int code; std::string msg; };

// kernel timing slots (csp_timing.kernel_ms): one row per slot, in slot order; names via csp_kernel_name().  A PNG batch closes INFLATE .. FINISH,
// a decode-only batch INFLATE and UNFILTER, a WebP batch INFLATE, UNFILTER and WEBP_ENCODE
enum PngSlot {
    KP_INFLATE, KP_UNFILTER, KP_REDUCE, KP_FILTER5, KP_SCORES, KP_BRUTE, KP_PICK, KP_HIST, KP_CODES, KP_CHOOSE, KP_DEEP, KP_EMIT, KP_FINISH, KP_SPARE0, KP_SPARE1, KP_SPARE2, KP_COUNT,
    // a WebP batch (csp_batch_create_webp) has no reduction step: the whole of run_to_webp (k_png_rgb, the VP8 encoder, its retries) is timed in the slot
    // that csp_kernel_name calls k_png_reduce
    KP_WEBP_ENCODE = KP_REDUCE
};
struct PngSlotRow { PngSlot slot; const char *name; };
constexpr PngSlotRow kPngSlots[] = {{KP_INFLATE, "k_png_inflate"}, {KP_UNFILTER, "k_png_unfilter"}, {KP_REDUCE, "k_png_reduce"}, {KP_FILTER5, "k_png_filter5"},
                                    {KP_SCORES, "k_png_scores"},   {KP_BRUTE, "k_png_brute"},       {KP_PICK, "k_png_pick"},     {KP_HIST, "k_png_hist"},
                                    {KP_CODES, "k_png_codes"},     {KP_CHOOSE, "k_png_choose"},     {KP_DEEP, "k_png_deep"},     {KP_EMIT, "k_png_emit"},
                                    {KP_FINISH, "k_png_finish"},   {KP_SPARE0, ""},                 {KP_SPARE1, ""},             {KP_SPARE2, ""}};
constexpr bool png_slots_in_order() {
    for (int i = 0; i < int(sizeof kPngSlots / sizeof kPngSlots[0]); i++) if (kPngSlots[i].slot != i) return false;
    return true;
}
static_assert(sizeof kPngSlots / sizeof kPngSlots[0] == CSP_NKERNELS && int(KP_COUNT) == int(CSP_NKERNELS), "one row per csp_timing.kernel_ms slot");
static_assert(png_slots_in_order(), "row i of kPngSlots describes slot i");

// The events of the batch, one after every kernel timing slot, on the batch's own stream: kernel_ms[i] = ev[i+1] - ev[i].  Created with the batch,
// released with it.  A mark names the slot it closes; slots are closed in order.
class PngMarks {
    hipEvent_t ev[CSP_NKERNELS + 1];
    int created = 0, next = 0;   // next: the slot the next mark closes

public:
    PngMarks() = default;
    PngMarks(const PngMarks &) = delete;
    PngMarks &operator=(const PngMarks &) = delete;
    ~PngMarks() { for (int i = 0; i < created; i++) (void)hipEventDestroy(ev[i]); }
    int create();                              // 0, or -1
    void start(hipStream_t st);                // a run begins: the event in front of the first slot
    int mark(PngSlot slot, hipStream_t st);    // 0, or -1 with the error set: `slot` is not the next one
    void read(csp_timing *t) const;            // kernel_ms of the slots closed by the last run, and total_ms
};

}  // namespace csp

struct csp_batch {
    // inputs and items; what kind of batch this is
    int device = 0;
    hipStream_t stream{};
    bool have_stream = false;
    std::vector<csp::PngItem> items;
    std::vector<const uint8_t *> inputs;
    bool from_pixels = false;       // csp_batch_create_pixels: no file to decode
    bool decode_only = false;       // the front half of a resize: stop at the pixels (decoded_image)
    bool to_webp = false;           // csp_batch_create_webp: the decoded pixels go to the VP8 encoder
    bool lossy = false;             // png.optimize not set: truecolour images with more than 256 colours are quantised (oracle: quantize)
    int png_quality = 80;

    // geometry and index arrays: the images, their reconstruction jobs, the carried bytes, who owns each row / chunk / group
    std::vector<csp::PngImg> imgs;
    std::vector<uint8_t> fixed;
    std::vector<csp::PngPass> passes;    // reconstruction jobs: one per image, seven per Adam7 image
    std::vector<csp::PngAdam7> adam7;
    uint64_t adam7_items = 0;
    uint32_t total_rows = 0, total_chunks = 0, total_groups = 0, max_pieces = 0;
    uint64_t raw_total = 0, pixels = 0;
    csh::DevBuf<csp::PngImg> d_imgs;
    csh::DevBuf<uint8_t> d_idat, d_work, d_fixed;   // d_work: inflated streams, then pixels (one buffer: a reduction swaps the two regions of an image)
    csh::DevBuf<csp::PngPass> d_passes;
    csh::DevBuf<csp::PngAdam7> d_adam7;
    csh::DevBuf<uint32_t> d_row_image, d_chunk_image, d_chunk_first, d_group_image, d_group_first, d_status, d_nmatch, d_file_len;

    // reduction (png_reduce.cpp)
    std::vector<uint32_t> flags0;   // reductions each image's format allows
    std::vector<uint32_t> cand0;    // channels of an image that may become indexed (8- or 16-bit truecolour, no PLTE, nothing tied to the colour type), else 0
    bool reduced = false;
    uint32_t n_reduced = 0;
    csh::DevBuf<csp::ReduceJob> d_jobs;
    csh::DevBuf<csp::PaletteJob> d_pjobs;
    csh::DevBuf<unsigned long long> d_keys;
    csh::DevBuf<uint16_t> d_slot_index;
    csh::DevBuf<uint32_t> d_flags, d_counts, d_cand, d_qbins, d_qn, d_qpal;
    csh::DevBuf<csp::QuantJob> d_qjobs;
    csh::DevBuf<csp::QBin> d_qlist;

    // filter / deflate / deep parse
    csp::PngPlan plan{};
    int slot_of_strategy[10];
    csh::DevBuf<uint8_t> d_streams, d_out, d_choice, d_trial_live;
    csh::DevBuf<uint32_t> d_adler, d_crc;
    csh::DevBuf<uint64_t> d_scores, d_trial_bytes;
    csh::DevBuf<int32_t> d_winner;
    csh::DevBuf<csp::PngChunk> d_chunks;
    csh::DevBuf<uint8_t> d_deep;         // the min-cost-path kernels' scratch areas (png_parse.h)
    uint32_t deep_slots = 0;
    csh::DevBuf<uint32_t> d_deep_queue, d_deep_list;
    int deep_iters = csp::CSP_DEEP_ITERS;   // png.force_zopfli: CSP_DEEP_ITERS_ZOPFLI

    // WebP conversion
    int webp_quality = 0;
    uint32_t webp_mb_bytes = 768, wmax_luma = 0, wmax_mbh = 0, rgb_max_h = 0;   // webp_mb_bytes: output bytes reserved per macroblock; grows on overflow, CSH_TEST_POOL_SHIFT divides this first value
    uint32_t last_run_pool_retries = 0;   // how often the last run repeated the encoder with a larger reservation (csp_timing.n_pool_retries)
    uint64_t wwork_bytes = 0, wlevels = 0, rgb_bytes = 0;
    std::vector<csw::WebpImg> wimgs;
    std::vector<csp::RgbJob> rgbjobs;
    std::vector<uint8_t> plte;
    std::vector<uint32_t> h_wstatus;
    std::vector<uint8_t> walpha;    // per image: 0, or the samples per pixel (2 / 4) of a picture whose last sample is alpha
    csh::DevBuf<csw::WebpImg> d_wimgs;
    csh::DevBuf<csp::RgbJob> d_rgbjobs;
    csh::DevBuf<uint8_t> d_plte, d_rgb, d_wwork, d_wscratch, d_wprobs, d_wupdate;
    csh::DevBuf<int16_t> d_wlevels;
    csh::DevBuf<uint32_t> d_wstats, d_wpart, d_wstatus;

    // events and state
    csp::PngMarks marks;
    bool ran = false;
    ~csp_batch() { if (have_stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }   // nothing queued may outlive the device blocks
};

namespace csp {

// png_container.cpp: the PNG container on the host
uint32_t be32(const uint8_t *p);
void append_chunk(std::vector<uint8_t> &dst, const char type[4], const uint8_t *data, uint32_t len);   // length, type, payload, CRC
void set_ihdr_format(std::vector<uint8_t> &prefix, uint32_t depth, uint32_t ctype);                    // patches the IHDR behind the signature, rewrites its CRC
uint32_t palette_depth(uint32_t n);                                   // the smallest index depth that holds n entries
uint32_t leading_transparent(const std::vector<uint32_t> &pal);       // ARGB entries: how many a tRNS chunk has to cover
void parse_png(const uint8_t *in, size_t n, bool keep_metadata, PngItem &it);
void pixels_item(const csp_pixels &src, uint32_t bits, PngItem &it);
int trial_set(int level, int *set);

// png_plan.cpp
int png_create(const CByteArray *inputs, const csp_pixels *px, size_t count, const CCSParameters *p, int device, int mode, csp_batch **out, const std::vector<PreFail> *pre = nullptr,
               const std::vector<uint8_t> *px_bits = nullptr);   // px_bits: 8 or 16 per pixel source (default 8)
int upload_chunk_index(csp_batch *b);
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// png_reduce.cpp
int reduce_step(csp_batch *b);

// png_run.cpp
int read_status_and_lengths(csp_batch *b, std::vector<uint32_t> &status, std::vector<uint32_t> *flen);
CCSResult png_result(int code, const char *msg);

// png_convert.cpp
int png_create_resized(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, int mode, csp_batch **out);
uint32_t rgb_channels(const PngItem &it, bool keep_alpha);   // samples per pixel k_png_rgb writes: grey or RGB, and alpha (or the tRNS chunk as one) if kept
RgbJob add_rgb_job(const PngItem &it, uint32_t out_nc, uint64_t src_off, uint64_t dst_off, std::vector<uint8_t> &tables);   // appends the item's PLTE, then tRNS to `tables`

}  // namespace csp
