// png_run.cpp -- one run of the PNG batch object: csp_batch_run pushes the whole group through
//   inflate -> unfilter / de-interlace -> reduction -> filter trials -> DEFLATE trials -> the winner's file
// on one stream, with one host round trip (the reduction step, png_reduce.cpp); a WebP batch leaves behind the pixels for the VP8 encoder,
// a decode-only batch stops there.  csp_batch_fetch brings the files back; the stage taps read what a run left on the device.
#include <cstring>

#include "png_batch.hpp"

namespace csp {

int PngMarks::create() {
    for (; created <= CSP_NKERNELS; created++) if (hipEventCreate(&ev[created]) != hipSuccess) return -1;
    return 0;
}
void PngMarks::start(hipStream_t st) { next = 0; (void)hipEventRecord(ev[0], st); }
int PngMarks::mark(PngSlot slot, hipStream_t st) {
    if (int(slot) != next || next >= CSP_NKERNELS) {
        csh_set_error("internal: timing mark '%s' out of order (slot %d is next)", slot < KP_COUNT ? kPngSlots[slot].name : "?", next);
        return -1;
    }
    (void)hipEventRecord(ev[++next], st);
    return 0;
}
void PngMarks::read(csp_timing *t) const {
    (void)hipEventElapsedTime(&t->total_ms, ev[0], ev[next]);
    for (int i = 0; i < next; i++) (void)hipEventElapsedTime(&t->kernel_ms[i], ev[i], ev[i + 1]);
}

CCSResult png_result(int code, const char *msg) {
    CCSResult r;
    r.success = code == 0; r.code = uint32_t(code); r.error_message = nullptr;
    if (code && msg) { size_t n = strlen(msg); char *m = (char *)malloc(n + 1); memcpy(m, msg, n + 1); r.error_message = m; }
    return r;
}

// the per-image status words of the batch and, if asked for, the lengths of its files
int read_status_and_lengths(csp_batch *b, std::vector<uint32_t> &status, std::vector<uint32_t> *flen) {
    const size_t nimg = b->imgs.size();
    status.assign(nimg + 1, 0);
    if (flen) flen->assign(nimg + 1, 0);
    if (!nimg) return 0;
    if (csh_copy_wait(status.data(), b->d_status.p, sizeof(uint32_t) * nimg, hipMemcpyDeviceToHost, b->stream) != hipSuccess) return -1;
    if (flen && csh_copy_wait(flen->data(), b->d_file_len.p, sizeof(uint32_t) * nimg, hipMemcpyDeviceToHost, b->stream) != hipSuccess) return -1;
    return 0;
}

namespace {

#define MARK(slot) do { if (b->marks.mark(slot, st)) return CS_ERR_NO_DEVICE; } while (0)

// the timing of the run that has just ended.  coded: the batch made PNG files -- their sizes and the failures are counted too
void fill_timing(csp_batch *b, csp_timing *t, bool coded) {
    if (!t) return;
    memset(t, 0, sizeof *t);
    if (b->decode_only) return;
    b->marks.read(t);
    if (coded) {
        std::vector<uint32_t> status, flen;
        (void)read_status_and_lengths(b, status, &flen);
        for (auto &it : b->items) {
            if (it.image < 0 || status[it.image]) { t->n_failed++; continue; }
            t->in_bytes += it.idat_len; t->out_bytes += flen[it.image];
        }
        t->n_trials = uint32_t(b->plan.ntrials);
    }
    t->pixels = b->pixels; t->raw_bytes = b->raw_total; t->n_images = uint32_t(b->imgs.size());
    t->n_pool_retries = b->last_run_pool_retries;
}

// conversion to WebP: pixels -> 8-bit RGB -> the VP8 encoder of webp_kernels.h (statement: oracle/webp_oracle.c).  The output pool is
// sized per macroblock and grows when a file overflows it, as in the JPEG -> WebP path (batch_run.cpp: Run::webp)
int run_to_webp(csp_batch *b) {
    hipStream_t st = b->stream;
    const int nimg = int(b->wimgs.size());
    if (!nimg) return 0;
    launch_png_rgb(st, b->d_rgbjobs.p, nimg, b->rgb_max_h, b->d_plte.p, b->d_work.p, b->d_rgb.p, b->d_status.p);
    const int q = b->webp_quality, quality = q < 0 ? 0 : q > 100 ? 100 : q;
    b->h_wstatus.assign(size_t(nimg), 0);
    for (int attempt = 0; attempt < 4; attempt++) {
        uint64_t out_bytes = 0;
        for (auto &wi : b->wimgs) {
            const uint64_t cap = 4096 + uint64_t(wi.mbw) * wi.mbh * (b->webp_mb_bytes + 2);
            wi.out_cap = uint32_t(std::min<uint64_t>(cap, 0xFFFFFF00u)); wi.out_off = out_bytes; wi.quality = quality;
            b->imgs[wi.image].out_off = out_bytes;
            out_bytes += (wi.out_cap + 63) & ~uint64_t(63);
        }
        if (b->d_out.alloc(out_bytes + 64) || b->d_wscratch.alloc(out_bytes + 64) || b->d_wimgs.upload(b->wimgs, st) || b->d_wstats.zero(st) || b->d_wstatus.zero(st) || b->d_file_len.zero(st)) return CS_ERR_NO_DEVICE;
        csw::launch_webp_yuv(st, b->d_wimgs.p, nimg, b->wmax_luma, b->d_rgb.p, b->d_wwork.p);
        if (csw::launch_webp_encode(st, b->wimgs.data(), nimg, b->d_wimgs.p, b->d_wwork.p, b->d_wlevels.p, b->d_wscratch.p, b->d_wpart.p, b->d_out.p, b->d_file_len.p, b->d_wstatus.p, nullptr)) return CS_ERR_NO_DEVICE;
        if (hipMemcpyAsync(b->h_wstatus.data(), b->d_wstatus.p, sizeof(uint32_t) * nimg, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
            hipGetLastError() != hipSuccess) { csh_set_error("WebP kernels failed"); return CS_ERR_NO_DEVICE; }
        bool pool = false;
        for (uint32_t s : b->h_wstatus) if (s == CS_ERR_POOL_OVERFLOW) pool = true;
        b->last_run_pool_retries = uint32_t(attempt);
        if (!pool || attempt == 3) break;   // every file has a region of its own: what still does not fit after three retries fails alone (its word in h_wstatus says so), the others are whole
        b->webp_mb_bytes *= 4;
    }
    csh_count_pool_retries(b->last_run_pool_retries);
    return 0;
}

FilterCtx filter_ctx(const csp_batch *b) {
    FilterCtx f{};
    f.imgs = b->d_imgs.p; f.nimg = int(b->imgs.size()); f.total_rows = b->total_rows; f.row_image = b->d_row_image.p; f.pix = b->d_work.p; f.streams = b->d_streams.p;
    f.scores = b->d_scores.p; f.choice = b->d_choice.p; f.plan = b->plan; f.status = b->d_status.p;
    for (const PngImg &im : b->imgs) f.max_rowbytes = std::max(f.max_rowbytes, im.rowbytes);
    return f;
}

// (behind the reduction step, which may have re-laid the chunk index and the carried bytes out)
DeflateCtx deflate_ctx(const csp_batch *b) {
    DeflateCtx d{};
    d.imgs = b->d_imgs.p; d.nimg = int(b->imgs.size()); d.total_chunks = b->total_chunks; d.chunk_image = b->d_chunk_image.p; d.chunk_first = b->d_chunk_first.p;
    d.total_groups = b->total_groups; d.group_image = b->d_group_image.p; d.group_first = b->d_group_first.p;
    d.streams = b->d_streams.p; d.chunks = b->d_chunks.p; d.plan = b->plan; d.trial_bytes = b->d_trial_bytes.p; d.winner = b->d_winner.p; d.trial_live = b->d_trial_live.p;
    d.adler_parts = b->d_adler.p; d.out = b->d_out.p; d.fixed = b->d_fixed.p; d.file_len = b->d_file_len.p; d.crc_parts = b->d_crc.p; d.status = b->d_status.p;
    return d;
}

// inflate, unfilter, de-interlace: the pixels of every image (nothing to do for a batch that was reduced already or started from pixels)
int run_decode(csp_batch *b) {
    hipStream_t st = b->stream;
    const bool decode = !b->reduced && !b->from_pixels;
    if (decode) launch_png_inflate(st, b->d_imgs.p, int(b->imgs.size()), b->d_idat.p, b->d_work.p, reinterpret_cast<uint64_t *>(b->d_streams.p), b->d_nmatch.p, b->d_status.p);
    MARK(KP_INFLATE);
    if (decode) {
        uint32_t mh = 0;
        for (const PngPass &pp : b->passes) mh = std::max(mh, pp.height);
        launch_png_unfilter(st, b->d_passes.p, int(b->passes.size()), mh, b->d_work.p, b->d_status.p);
        launch_png_deinterlace(st, b->d_imgs.p, b->d_adam7.p, int(b->adam7.size()), b->adam7_items, b->d_work.p, b->d_status.p);
    }
    MARK(KP_UNFILTER);
    return 0;
}

// the reduction step, the filter trials, the DEFLATE trials, the winner's file.  f: made in front of the reduction
int run_coder(csp_batch *b, const FilterCtx &f) {
    hipStream_t st = b->stream;
    if (!b->reduced && reduce_step(b)) return CS_ERR_NO_DEVICE;
    MARK(KP_REDUCE);
    DeflateCtx d = deflate_ctx(b);
    bool need_scores = false;
    for (int a = 0; a < b->plan.nadaptive; a++) if (b->plan.adaptive_strategy[a] != 9) need_scores = true;
    launch_png_filter5(st, f);
    MARK(KP_FILTER5);
    if (need_scores) launch_png_scores(st, f);
    MARK(KP_SCORES);
    if (b->plan.need_brute) launch_png_brute(st, f);
    MARK(KP_BRUTE);
    launch_png_pick(st, f);
    MARK(KP_PICK);
    {   // one scratch area per workgroup the device holds at the parse kernels' LDS footprint (three per CU), no more than there are items
        const uint64_t items = uint64_t(b->total_chunks) * uint32_t(b->plan.ntrials);
        b->deep_slots = uint32_t(std::min<uint64_t>(items, 768));
        if (b->deep_slots && (b->d_deep.alloc(size_t(b->deep_slots) * CSP_DEEP_SCRATCH) || b->d_deep_queue.alloc(4) || b->d_deep_list.alloc(size_t(items) + 1))) return CS_ERR_NO_DEVICE;
        d.deep_scratch = b->d_deep.p; d.deep_queue = b->d_deep_queue.p; d.deep_list = b->d_deep_list.p; d.deep_slots = b->deep_slots; d.deep_iters = b->deep_iters;
    }
    launch_png_hist(st, d);
    MARK(KP_HIST);
    launch_png_codes(st, d);
    MARK(KP_CODES);
    launch_png_choose(st, d);
    MARK(KP_CHOOSE);
    launch_png_deep(st, d);
    MARK(KP_DEEP);
    launch_png_emit(st, d);
    MARK(KP_EMIT);
    launch_png_finish(st, d, b->max_pieces);
    MARK(KP_FINISH);
    return 0;
}

const PngImg *tap_image(csp_batch *b, size_t image) {
    if (!b || !b->ran || image >= b->items.size() || b->items[image].image < 0) { csh_set_error("no such decoded PNG in the batch"); return nullptr; }
    return &b->imgs[b->items[image].image];
}

// pictures with transparency going to WebP: their alpha plane through the VP8L coder (the pixels are still in d_rgb), one call for all of them
struct AlphaPlanes {
    std::vector<CByteArray> out;
    std::vector<CCSResult> res;
    std::vector<int> at;            // per item: its place in px / out / res, or -1
    std::vector<csp_pixels> px;
    AlphaPlanes(csp_batch *b, const std::vector<uint32_t> &status) : at(b->items.size(), -1) {
        if (!b->to_webp) return;
        for (size_t i = 0; i < b->items.size(); i++) {
            const PngItem &it = b->items[i];
            if (it.code || it.image < 0 || status[it.image] || b->h_wstatus[it.image] || size_t(it.image) >= b->walpha.size() || !b->walpha[it.image]) continue;
            const csw::WebpImg *wi = nullptr;
            for (const csw::WebpImg &w : b->wimgs) if (int(w.image) == it.image) { wi = &w; break; }
            if (!wi) continue;
            at[i] = int(px.size());
            px.push_back(csp_pixels{b->d_rgb.p + wi->rgb_off, wi->width, wi->height, uint32_t(csw::VP8L_ALPHA_OF) + b->walpha[it.image]});
        }
        if (px.empty()) return;
        out.resize(px.size()); res.resize(px.size());
        csl_encode_pixels(px.data(), px.size(), b->device, out.data(), res.data());
    }
    ~AlphaPlanes() { for (size_t k = 0; k < out.size(); k++) { cs_free_bytes(&out[k]); cs_free_result(&res[k]); } }
};

}  // namespace
}  // namespace csp

using namespace csp;

extern "C" const char *csp_kernel_name(int i) { return (i >= 0 && i < CSP_NKERNELS) ? kPngSlots[i].name : ""; }
extern "C" void csp_batch_destroy(csp_batch *b) { delete b; }

extern "C" int csp_batch_run(csp_batch *b, csp_timing *t) {
    if (!b) return CS_ERR_NO_DEVICE;
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    hipStream_t st = b->stream;
    b->last_run_pool_retries = 0;
    if (!b->reduced && b->d_status.zero(st)) return CS_ERR_NO_DEVICE;
    const FilterCtx f = filter_ctx(b);
    b->marks.start(st);
    if (int rc = run_decode(b)) return rc;
    if (b->to_webp) {
        if (int rc = run_to_webp(b)) return rc;   // (synchronises)
        MARK(KP_WEBP_ENCODE);
    } else {
        if (!b->decode_only) if (int rc = run_coder(b, f)) return rc;
        if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { csh_set_error("PNG kernels failed"); return CS_ERR_NO_DEVICE; }
    }
    b->ran = true;
    fill_timing(b, t, !b->to_webp);
    return 0;
}

extern "C" int csp_batch_fetch(csp_batch *b, CByteArray *outputs, CCSResult *results) {
    if (!b || !b->ran || b->decode_only) { csh_set_error("csp_batch_fetch before csp_batch_run"); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) return -1;
    std::vector<uint32_t> status, flen;
    if (read_status_and_lengths(b, status, &flen)) { csh_set_error("download failed"); return -1; }
    int failed = 0;
    AlphaPlanes alpha(b, status);
    for (size_t i = 0; i < b->items.size(); i++) {
        PngItem &it = b->items[i];
        const int ai = alpha.at[i];
        outputs[i].data = nullptr; outputs[i].length = 0;
        int code = it.code;
        const char *msg = it.msg.c_str();
        if (!code && ai >= 0 && !alpha.out[size_t(ai)].data) { code = int(alpha.res[size_t(ai)].code ? alpha.res[size_t(ai)].code : CS_ERR_NO_DEVICE); msg = "alpha plane coder failed"; }
        if (!code && !status[it.image] && b->to_webp && b->h_wstatus[it.image]) { code = int(b->h_wstatus[it.image]); msg = code == int(CS_ERR_POOL_OVERFLOW) ? "device pools overflowed after 3 retries" : "WebP encoder failed"; }
        else if (!code && status[it.image]) { code = int(status[it.image]); msg = code == int(CSP_ERR_POOL) ? "internal device pool too small" : "malformed PNG data"; }
        if (code) { failed++; if (results) results[i] = png_result(code, msg); continue; }
        const size_t n = flen[it.image];
        if (!b->lossy && !b->to_webp && !b->from_pixels && n >= it.file_size) {   // oxipng: "file already optimized" -- the input comes back unchanged
            outputs[i].data = (uint8_t *)malloc(it.file_size ? it.file_size : 1);
            memcpy(outputs[i].data, b->inputs[i], it.file_size);
            outputs[i].length = it.file_size;
        } else {
            outputs[i].data = (uint8_t *)malloc(n ? n : 1);
            if (csh_copy_wait(outputs[i].data, b->d_out.p + b->imgs[it.image].out_off, n, hipMemcpyDeviceToHost, b->stream) != hipSuccess) { csh_set_error("download failed"); return -1; }
            outputs[i].length = n;
        }
        if (ai >= 0) {
            const csp_pixels &ap = alpha.px[size_t(ai)];
            if (csl_attach_alpha(&outputs[i], &alpha.out[size_t(ai)], ap.width, ap.height)) {
                cs_free_bytes(&outputs[i]); failed++;
                if (results) results[i] = png_result(CS_ERR_NO_DEVICE, "could not assemble the WebP file with its alpha plane");
                continue;
            }
        }
        if (results) results[i] = png_result(0, nullptr);
    }
    return failed;
}

// ---- stage taps
extern "C" int csp_batch_geometry(csp_batch *b, size_t image, uint32_t *width, uint32_t *height, uint32_t *rowbytes) {
    const PngImg *im = tap_image(b, image);
    if (!im) return -1;
    *width = im->width; *height = im->height; *rowbytes = im->rowbytes;
    return 0;
}
extern "C" int csp_batch_read_rows(csp_batch *b, size_t image, uint8_t *dst) {
    const PngImg *im = tap_image(b, image);
    if (!im) return -1;
    return csh_copy_wait(dst, b->d_work.p + im->pix_off, size_t(im->height) * im->rowbytes, hipMemcpyDeviceToHost, b->stream) == hipSuccess ? 0 : -1;
}
extern "C" int csp_batch_read_stream(csp_batch *b, size_t image, int strategy, uint8_t *dst) {
    const PngImg *im = tap_image(b, image);
    if (!im) return -1;
    if (strategy < 0 || strategy > 9 || b->slot_of_strategy[strategy] < 0) { csh_set_error("strategy %d is not part of this level's plan", strategy); return -1; }
    return csh_copy_wait(dst, b->d_streams.p + im->stream_off + uint64_t(b->slot_of_strategy[strategy]) * im->stream_stride, im->raw_len, hipMemcpyDeviceToHost, b->stream) == hipSuccess ? 0 : -1;
}
extern "C" int csp_batch_read_scores(csp_batch *b, size_t image, uint64_t *dst, int *have) {
    const PngImg *im = tap_image(b, image);
    if (!im) return -1;
    *have = 0;
    for (int a = 0; a < b->plan.nadaptive; a++) *have |= b->plan.adaptive_strategy[a] == 9 ? 16 : 15;
    return csh_copy_wait(dst, b->d_scores.p + size_t(im->row_base) * 25, sizeof(uint64_t) * 25 * im->height, hipMemcpyDeviceToHost, b->stream) == hipSuccess ? 0 : -1;
}
extern "C" int csp_batch_trials(csp_batch *b, size_t image, int *strategies, uint64_t *zlib_bytes, int *ntrials, int *winner) {
    const PngImg *im = tap_image(b, image);
    if (!im) return -1;
    const int idx = b->items[image].image;
    *ntrials = b->plan.ntrials;
    for (int t = 0; t < b->plan.ntrials; t++) strategies[t] = b->plan.trial_strategy[t];
    int32_t w = 0;
    if (csh_copy_wait(zlib_bytes, b->d_trial_bytes.p + size_t(idx) * CSP_MAX_STREAMS, sizeof(uint64_t) * b->plan.ntrials, hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
        csh_copy_wait(&w, b->d_winner.p + idx, sizeof w, hipMemcpyDeviceToHost, b->stream) != hipSuccess) return -1;
    *winner = w;
    return 0;
}
extern "C" int csp_batch_chunk_bits(csp_batch *b, size_t image, int trial, uint64_t *dst, size_t cap, size_t *nchunks) {
    const PngImg *im = tap_image(b, image);
    if (!im || trial < 0 || trial >= b->plan.ntrials) return -1;
    *nchunks = im->nchunks;
    std::vector<PngChunk> recs(im->nchunks);
    if (csh_copy_wait(recs.data(), b->d_chunks.p + size_t(im->chunk_base) + size_t(b->plan.trial_slot[trial]) * im->nchunks, sizeof(PngChunk) * im->nchunks, hipMemcpyDeviceToHost, b->stream) != hipSuccess) return -1;
    for (size_t i = 0; i < im->nchunks && i < cap; i++) dst[i] = recs[i].bits;
    return 0;
}
