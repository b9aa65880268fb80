// pipeline.cpp -- the device batch queue: what caesium-clt's rayon par_iter over files
// (/root/reference/src/compressor.rs:74-101) becomes on an MI355X.  One csh_batch = one group of input
// files resident in HBM (batch.hpp); this file is its C surface: create (batch_create drives the planner of batch_plan.cpp),
// run (the retry loop around batch_run.cpp's run_once), fetch and read-back, and the host pieces other batch objects share.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <memory>
#include <thread>

#include "batch.hpp"
#include "../../include/vp8_tables.h"
#include "resize_host.h"

static thread_local char g_err[512];
void csh_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
extern "C" const char *csh_last_error(void) { return g_err; }
// the extra runs with larger pools that the batch runs of this thread have made since it was last asked (read and reset): what a one-call entry, which hands
// out no csh_timing, leaves for a caller that wants to know whether its files went through a retry
static thread_local uint32_t g_pool_retries = 0;
void csh_count_pool_retries(uint32_t n) { g_pool_retries += n; }
extern "C" uint32_t csh_last_pool_retries(void) { const uint32_t n = g_pool_retries; g_pool_retries = 0; return n; }
int csh_test_pool_shift() { const char *e = getenv("CSH_TEST_POOL_SHIFT"); return e ? std::min(16, std::max(0, atoi(e))) : 0; }

#ifdef CSH_EMUL
thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
int csh_emul_reverse = 0;
thread_local int csh_emul_phase = 0;
extern "C" void csh_emul_set_reverse(int r) { csh_emul_reverse = r; }
namespace csh { extern int csh_emul_jacobi; }
extern "C" void csh_emul_set_jacobi(int j) { csh::csh_emul_jacobi = j; }
namespace csh { extern uint32_t csh_emul_ac_paths[8]; }
extern "C" void csh_emul_ac_paths(uint32_t *out) { for (int i = 0; i < 8; i++) { out[i] = csh::csh_emul_ac_paths[i]; csh::csh_emul_ac_paths[i] = 0u; } }   // (k_entropy.hip: read and reset)
#endif

using namespace csh;

// image-rs Lanczos3 taps of one axis (imageops::sample) -- host side, same libm calls as the oracle
static float sincf_(float t) { float a = t * 3.14159265358979323846f; return t == 0.0f ? 1.0f : sinf(a) / a; }
static float lanczos3f(float x) { return fabsf(x) < 3.0f ? sincf_(x) * sincf_(x / 3.0f) : 0.0f; }
void csh_lanczos_axis(int in_size, int out_size, bool identity, std::vector<ResizeTap> &taps, std::vector<float> &weights) {   // also used by png_convert.cpp (resize_host.h)
    for (int o = 0; o < out_size; o++) {
        ResizeTap t;
        t.woff = uint32_t(weights.size());
        if (identity) { t.left = o; t.n = 1; weights.push_back(1.0f); taps.push_back(t); continue; }
        float ratio = float(in_size) / float(out_size);
        float sratio = ratio < 1.0f ? 1.0f : ratio;
        float support = 3.0f * sratio;
        float center = (float(o) + 0.5f) * ratio;
        long left = long(floorf(center - support)); if (left < 0) left = 0; if (left > in_size - 1) left = in_size - 1;
        long right = long(ceilf(center + support)); if (right < left + 1) right = left + 1; if (right > in_size) right = in_size;
        center = center - 0.5f;
        float sum = 0.0f;
        for (long i = left; i < right; i++) { float w = lanczos3f((float(i) - center) / sratio); weights.push_back(w); sum += w; }
        for (size_t i = t.woff; i < weights.size(); i++) weights[i] /= sum;
        t.left = int(left); t.n = int(right - left);
        taps.push_back(t);
    }
}
// libcaesium resize.rs compute_dimensions [UPSTREAM-RECALL]: both given -> exact; one given -> keep aspect, f32, round half away
void csh_compute_dimensions(int ow, int oh, int dw, int dh, int &nw, int &nh) {
    if (dw > 0 && dh > 0) { nw = dw; nh = dh; }
    else {
        float ratio = float(ow) / float(oh);
        if (dw > 0) { nw = dw; nh = int(roundf(float(dw) / ratio)); }
        else { nh = dh; nw = int(roundf(float(dh) * ratio)); }
    }
    if (nw < 1) nw = 1;
    if (nh < 1) nh = 1;
}

// Device pools and pinned blocks of finished batches stay in per-device / process-wide caches (devmem.hpp: hipMalloc / hipFree cost more than
// the kernels); a caller that wants the memory back -- another process is about to use the device -- says so here.
extern "C" void csh_release_cached_memory(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    for (int d = 0; d < n && d < 64; d++) device_cache(d).trim(0);
    pinned_cache().trim(0);
}
// A process that knows it will use a device says so early, from a thread of its own: runtime start-up, the device's context and the library's code
// objects (the first launch loads them) take ~0.15 s that can pass while the caller is still reading its files (the CLI does: cli.cpp)
__global__ void k_warmup(uint32_t *p) { if (p && threadIdx.x == 1024) *p = 0; }
extern "C" void csh_warmup(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || hipSetDevice(device) != hipSuccess) return;
    hipStream_t st;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return;
    CSH_LAUNCH(k_warmup, dim3(1), dim3(1), st, static_cast<uint32_t *>(nullptr));
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
}
extern "C" int csh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int batch_create(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, bool webp, csh_batch **out, bool rgb_out = false, const csp_pixels *px = nullptr) {
    *out = nullptr;
    if (csh_device_count() <= device) { csh_set_error("no HIP device %d available (libcaesium_hip has no CPU path)", device); return CS_ERR_NO_DEVICE; }
    if (hipSetDevice(device) != hipSuccess) { csh_set_error("hipSetDevice(%d) failed", device); return CS_ERR_NO_DEVICE; }
    if (count > 6000) { csh_set_error("csh_batch_create: at most 6000 files per device batch (cs_batch_compress splits for you)"); return CS_ERR_POOL_OVERFLOW; }
    Laps laps;
    std::unique_ptr<csh_batch> b(new csh_batch);
    b->device = device;
    b->params = *p;
    b->lossless = p->jpeg_optimize && !webp && !rgb_out && !px;
    b->webp = webp; b->rgb_out = rgb_out;
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { csh_set_error("hipStreamCreate failed"); return CS_ERR_NO_DEVICE; }
    b->have_stream = true;
    BatchPlanner plan(b.get(), inputs, count, p, px);
    plan.begin();
    plan.parse();
    laps.lap("stream+parse");
    if (int rc = plan.reserve_pinned()) return rc;
    laps.lap("pinned");
    for (size_t n = 0; n < count; n++)
        if (int rc = plan.plan_image(n)) return rc;
    if (int rc = plan.plan_search_stages()) return rc;
    if (int rc = plan.plan_trellis()) return rc;
    plan.finish_descriptors();
    laps.lap("descriptors");
    if (int rc = plan.upload(laps)) return rc;
    if (laps.trace) fprintf(stderr, "[csh] create %zu files:%s\n", count, laps.text.c_str());
    *out = b.release();
    return 0;
}
extern "C" int csh_batch_create(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, csh_batch **out) { return batch_create(inputs, count, p, device, false, out); }
// JPEG in, pixels out (the front half of convert_in_memory to PNG): decode and resize only; the RGB stays in device memory (csh_batch_pixels)
extern "C" int csh_batch_create_pixels(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, csh_batch **out) { return batch_create(inputs, count, p, device, false, out, true); }
// JPEG in, WebP out (caesium::convert_in_memory to SupportedFileTypes::WebP, compressor.rs:289,300): same decode and resize, then the VP8 encoder
extern "C" int csh_batch_create_webp(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, csh_batch **out) { return batch_create(inputs, count, p, device, true, out); }

// Pixels in, JPEG out (the back half of convert_in_memory to JPEG): the batch object derives every descriptor from a parsed JPEG, so a
// pixel source presents itself as one -- a baseline 4:4:4 (or grey) file of its size whose every block is empty (two bits per block:
// DC difference 0, end of block) -- and its RGB is copied over what those planes would have given, in front of the resize branch.
// The decode of the stand-in costs a few bits per block and one IDCT over zeros; everything behind the RGB is the resize path as is.
static std::vector<uint8_t> standin_jpeg(uint32_t w, uint32_t h, uint32_t nc) {
    std::vector<uint8_t> f = {0xFF, 0xD8, 0xFF, 0xDB, 0x00, 0x43, 0x00};
    f.insert(f.end(), 64, 1);                                                                    // DQT 0: all ones
    const uint8_t sof[] = {0xFF, 0xC0, 0x00, uint8_t(8 + 3 * nc), 8, uint8_t(h >> 8), uint8_t(h), uint8_t(w >> 8), uint8_t(w), uint8_t(nc)};
    f.insert(f.end(), sof, sof + sizeof sof);
    for (uint32_t c = 0; c < nc; c++) { f.push_back(uint8_t(c + 1)); f.push_back(0x11); f.push_back(0); }
    for (int cls = 0; cls < 2; cls++) {                                                          // DHT: one 1-bit code, symbol 0 (DC category 0 / AC end of block)
        const uint8_t dht[] = {0xFF, 0xC4, 0x00, 0x14, uint8_t(cls << 4), 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x00};
        f.insert(f.end(), dht, dht + sizeof dht);
    }
    const uint8_t sos[] = {0xFF, 0xDA, 0x00, uint8_t(6 + 2 * nc), uint8_t(nc)};
    f.insert(f.end(), sos, sos + sizeof sos);
    for (uint32_t c = 0; c < nc; c++) { f.push_back(uint8_t(c + 1)); f.push_back(0x00); }
    f.push_back(0); f.push_back(63); f.push_back(0);
    const uint64_t bits = uint64_t((w + 7) / 8) * ((h + 7) / 8) * nc * 2;
    f.insert(f.end(), size_t(bits / 8), 0x00);
    if (bits % 8) f.push_back(uint8_t(0xFF >> (bits % 8)));                                      // the last byte is padded with one-bits
    f.push_back(0xFF); f.push_back(0xD9);
    return f;
}
// (answered per file: a source that cannot be one is handed on as a file of unknown type)
static int create_from_pixels(const csp_pixels *sources, size_t count, const CCSParameters *p, int device, csh_batch **out, bool webp, bool rgb_out) {
    *out = nullptr;
    const uint32_t max_side = webp ? 16383 : 65535;
    std::vector<std::vector<uint8_t>> files(count);
    std::vector<CByteArray> in(count);
    for (size_t i = 0; i < count; i++) {
        const csp_pixels &s = sources[i];
        if (!s.device_pixels || !s.width || !s.height || s.width > max_side || s.height > max_side || (s.channels != 1 && s.channels != 3)) files[i] = {'?'};
        else files[i] = standin_jpeg(s.width, s.height, s.channels);
        in[i].data = files[i].data(); in[i].length = files[i].size();
    }
    return batch_create(in.data(), count, p, device, webp, out, rgb_out, sources);
}
extern "C" int csh_batch_create_from_pixels(const csp_pixels *sources, size_t count, const CCSParameters *p, int device, csh_batch **out) { return create_from_pixels(sources, count, p, device, out, false, false); }
// pixels in, (resized) pixels out: the resize branch alone, for WebP -> PNG with a size
extern "C" int csh_batch_create_from_pixels_rgb(const csp_pixels *sources, size_t count, const CCSParameters *p, int device, csh_batch **out) { return create_from_pixels(sources, count, p, device, out, false, true); }
extern "C" int csh_batch_create_webp_from_pixels(const csp_pixels *sources, size_t count, const CCSParameters *p, int device, csh_batch **out) { return create_from_pixels(sources, count, p, device, out, true, false); }

extern "C" void csh_batch_destroy(csh_batch *b) { delete b; }

// names of the kernel timing slots (batch.hpp kKernelSlots); a WebP batch has its own for the three behind the resize slot
extern "C" const char *csh_kernel_name(int i) { return (i >= 0 && i < CSH_NKERNELS) ? kKernelSlots[i].name : ""; }
extern "C" const char *csh_kernel_name_webp(int i) {
    return i == KS_WEBP_YUV ? "k_webp_yuv" : i == KS_WEBP_ENCODE ? "k_vp8_analyse+segments+loop" : i == KS_WEBP_ASSEMBLE ? "k_webp_hdr+decisions+bool+assemble" : csh_kernel_name(i);
}

static int batch_run(csh_batch *b, csh_timing *t, bool requant_only);
extern "C" int csh_batch_run(csh_batch *b, csh_timing *t) { return batch_run(b, t, false); }

// size targeting (caesium::compress_to_size_in_memory, compressor.rs:295,298): keep the unquantised DCT of the first run ...
extern "C" int csh_batch_retain_dct(csh_batch *b, int on) {
    if (b->lossless) { csh_set_error("retain_dct: a coefficient transcode has no quality to re-target"); return -1; }
    b->retain_dct = on != 0;
    if (b->retain_dct && b->nimg && b->pix.d_dct_raw.n == 0 && b->pix.d_dct_raw.alloc(size_t(b->ntiles_out) * CSH_TILE_I16)) return -1;
    return 0;
}
// ... give some images another quality (quality[i] == 0: unchanged; indexed like the inputs) ...
extern "C" int csh_batch_set_quality(csh_batch *b, const uint32_t *quality) {
    if (b->lossless) { csh_set_error("set_quality on a lossless batch"); return -1; }
    b->enc.hdr_pool.clear(); b->enc.hdr_off.clear();
    for (size_t n = 0; n < b->items.size(); n++) {
        Item &it = b->items[n];
        if (it.image < 0) continue;
        ImgDesc &im = b->imgs[it.image];
        if (quality[n]) {
            int q = int(quality[n]) < 1 ? 1 : (quality[n] > 100 ? 100 : int(quality[n]));
            for (int c = 0; c < im.ncomp; c++) im.qt_out[c] = b->q_base + q;
        }
        JpegInfo hdr = it.out;
        int qidx = im.qt_out[0];
        uint16_t nat[64];
        for (int k = 0; k < 64; k++) nat[kZigZag[k]] = b->quants[qidx].q[k];
        memcpy(hdr.qt[0], nat, 128); memcpy(hdr.qt[1], nat, 128);
        std::vector<uint8_t> fh = build_frame_header(hdr, b->progressive, it.meta_out.empty() ? nullptr : &it.meta_out);
        b->enc.hdr_off.push_back(uint32_t(b->enc.hdr_pool.size()));
        b->enc.hdr_pool.insert(b->enc.hdr_pool.end(), fh.begin(), fh.end());
    }
    b->enc.hdr_off.push_back(uint32_t(b->enc.hdr_pool.size()));
    if (!b->nimg) return 0;
    if (hipSetDevice(b->device) != hipSuccess) return -1;
    if (b->d_imgs.upload(b->imgs, b->stream) || b->enc.d_hdr.upload(b->enc.hdr_pool, b->stream) || b->enc.d_hdr_off.upload(b->enc.hdr_off, b->stream)) return -1;
    CSH_CHECK(hipStreamSynchronize(b->stream));
    return 0;
}
// ... and re-run only re-quantisation + entropy coding + assembly.
extern "C" int csh_batch_rerun_encode(csh_batch *b, csh_timing *t) {
    if (!b->have_dct) { csh_set_error("rerun_encode needs a completed csh_batch_run after csh_batch_retain_dct(1)"); return -1; }
    return batch_run(b, t, true);
}

static int batch_run(csh_batch *b, csh_timing *t, bool requant_only) {
    if (t) memset(t, 0, sizeof *t);
    if (!b->nimg) { b->out.ran = true; return 0; }
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    uint32_t retries = 0;
    for (int attempt = 0; attempt < 4; attempt++) {
        if (run_once(b, t, requant_only)) return CS_ERR_NO_DEVICE;
        uint32_t ovf[4] = {0, 0, 0, 0};
        if (csh_copy_wait(ovf, b->out.d_overflow.p, sizeof ovf, hipMemcpyDeviceToHost, b->stream) != hipSuccess) { csh_set_error("D2H failed"); return CS_ERR_NO_DEVICE; }
        b->out.h_status.resize(b->nimg);
        if (csh_copy_wait(b->out.h_status.data(), b->out.d_status.p, b->nimg * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream) != hipSuccess) return CS_ERR_NO_DEVICE;
        bool pool = ovf[0] != 0;
        if (ovf[1]) {   // token pool (k_tokens)
            pool = true; b->enc.tok_scale *= 4;
            layout_token_pool(b);
            if (b->enc.d_regions.upload(b->enc.regions, b->stream) || b->enc.d_nzlists.upload(b->enc.nzlists, b->stream) || hipStreamSynchronize(b->stream) != hipSuccess) return CS_ERR_NO_DEVICE;
        }
        for (uint32_t s : b->out.h_status) if (s == CS_ERR_POOL_OVERFLOW) pool = true;
        retries = uint32_t(attempt);
        if (pool && getenv("CSH_TRACE")) {
            size_t nfull = 0;
            for (uint32_t s : b->out.h_status) nfull += s == CS_ERR_POOL_OVERFLOW;
            fprintf(stderr, "[csh] attempt %d overflowed: raw / output pool %u, token / list pools %u, files without room %zu\n", attempt, ovf[0], ovf[1], nfull);
        }
        if (!pool) break;
        // A WebP file has a region of its own: the files that fit are whole after any attempt, so the ones that still do not fit fail alone (their status word says
        // CS_ERR_POOL_OVERFLOW).  The JPEG coder's pools are shared by the batch: there the call fails and the route tries smaller groups
        if (attempt == 3 && b->webp && !ovf[0] && !ovf[1]) break;
        if (attempt == 3) { csh_count_pool_retries(retries); if (t) t->n_pool_retries = retries; csh_set_error("device pools overflowed after 3 retries"); return CS_ERR_POOL_OVERFLOW; }
        b->out.raw_bytes_cap *= 4; b->out.out_cap = b->out.raw_bytes_cap;  // rare: output larger than 2x the input
        b->wp.webp_mb_bytes *= 4;
    }
    b->out.h_img_size.resize(b->nimg);
    b->out.h_img_off.resize(b->nimg + 1);
    if (csh_copy_wait(b->out.h_img_size.data(), b->out.d_img_size.p, b->nimg * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
        csh_copy_wait(b->out.h_img_off.data(), b->out.d_img_off.p, (b->nimg + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream) != hipSuccess) {
        csh_set_error("D2H of sizes failed"); return CS_ERR_NO_DEVICE;
    }
    if (t) {
        std::vector<uint32_t> ns(size_t(b->nimg) + CSH_DEC_NSTATS);   // the images' words and the decoder's counters behind them
        if (csh_copy_wait(ns.data(), b->dec.d_need_seq.p, ns.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream) != hipSuccess) return CS_ERR_NO_DEVICE;
        if (getenv("CSH_TRACE") && b->dec.d_relax_cnt.n) {   // sub-sequences re-listed after each relaxation round
            std::vector<uint32_t> rc(b->dec.d_relax_cnt.n);
            if (csh_copy_wait(rc.data(), b->dec.d_relax_cnt.p, rc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream) == hipSuccess) {
                fprintf(stderr, "[csh] relax list sizes (of %u sub-sequences):", b->dec.total_sub);
                for (size_t i = 0; i < rc.size() && (i < 16 || rc[i]); i++) fprintf(stderr, " %u", rc[i]);
                fprintf(stderr, "\n");
            }
        }
        t->n_dec_walked = ns[size_t(b->nimg) + CSH_DEC_STAT_WALKED]; t->n_dec_chain_scans = ns[size_t(b->nimg) + CSH_DEC_STAT_CHAIN_SCANS]; t->n_dec_chain_failed = ns[size_t(b->nimg) + CSH_DEC_STAT_CHAIN_FAILED];
        ns.resize(b->nimg);
        for (const ProgChain &pc : b->dec.chains) if (pc.refine && ns[size_t(pc.image)] == 4) t->n_refine_chains++;
        for (uint32_t v : ns) { if (v == 4) { t->n_prog_decoded++; continue; } if (v) t->n_seq_decoded++; if (v == 2 || v == 3) t->n_par_fallback++; if (v == 3) t->n_par_short++; }
        t->n_images = uint32_t(b->nimg);
        t->n_search_extra = b->enc.search ? b->enc.n_gated_runs : 0u;
        t->n_fused_lists = b->enc.last_run_fused;
        t->n_list_refine = b->enc.last_run_refine;
        t->n_ac_in_lists = b->enc.last_run_ac_lists;
        t->n_list_runs = b->enc.last_run_list_runs;
        t->n_ref_packed = b->enc.last_run_ref_packed;
        t->n_dec_group = b->dec.group; t->n_dec_seeds = b->dec.last_run_seeds; t->n_dec_relaxed = b->dec.last_run_relaxed; t->n_dec_rounds = b->dec.last_run_rounds;
        for (const Item &it : b->items) if (it.image < 0) t->n_failed++;
        for (int i = 0; i < b->nimg; i++) { t->out_bytes += b->out.h_img_size[i]; t->pixels += uint64_t(b->imgs[i].width) * b->imgs[i].height; }
        t->in_bytes = b->dec.bits_pool.size();
        uint64_t in_tiles = 0;
        for (const ImgDesc &im : b->imgs) for (int c = 0; c < im.ncomp_in; c++) in_tiles += im.in[c].ntiles;
        t->coef_bytes = in_tiles * CSH_TILE_I16 * 2;
        t->n_pool_retries = retries;
    }
    csh_count_pool_retries(retries);
    b->out.ran = true;
    if (!requant_only) b->have_dct = (b->retain_dct || b->tr.trellis) && !b->lossless;
    return 0;
}

static void set_result(CCSResult *r, int code, const std::string &msg) {
    r->success = code == 0;
    r->code = uint32_t(code);
    r->error_message = nullptr;
    if (code) { char *m = (char *)malloc(msg.size() + 1); memcpy(m, msg.c_str(), msg.size() + 1); r->error_message = m; }
}

// the decoded (and resized) image of a csh_batch_create_pixels batch, still in device memory: interleaved 8-bit samples, 1 or 3 per pixel.
// Returns the file's CCSResult code (0: the pointers are set; they live as long as the batch)
extern "C" int csh_batch_pixels(csh_batch *b, size_t image, const uint8_t **device_pixels, uint32_t *width, uint32_t *height, uint32_t *channels, const char **message) {
    *device_pixels = nullptr; *width = *height = *channels = 0;
    if (message) *message = "";
    if (!b || !b->out.ran || !b->rgb_out || image >= b->items.size()) { csh_set_error("csh_batch_pixels: not a pixel batch that has run"); if (message) *message = "not a pixel batch that has run"; return CS_ERR_NO_DEVICE; }
    const Item &it = b->items[image];
    if (it.code) { if (message) *message = it.msg.c_str(); return it.code; }
    if (b->out.h_status[it.image]) { if (message) *message = "device reported a malformed stream"; return int(b->out.h_status[it.image]); }
    if (size_t(it.image) < b->pix.rwork.size() && b->pix.rwork[size_t(it.image)].image == it.image) {   // every image of a pixel batch has its resize work item, in image order
        const ResizeWork &rw = b->pix.rwork[size_t(it.image)];
        *device_pixels = b->pix.d_rgb.p + rw.rgb_dst_off; *width = uint32_t(rw.nw); *height = uint32_t(rw.nh); *channels = uint32_t(b->imgs[it.image].ncomp);
        return 0;
    }
    if (message) *message = "image has no pixel output";
    return CS_ERR_NO_DEVICE;
}

extern "C" int csh_batch_fetch(csh_batch *b, CByteArray *outputs, CCSResult *results) {
    if (!b->out.ran) { csh_set_error("csh_batch_fetch before csh_batch_run"); return -1; }
    if (b->rgb_out) { csh_set_error("csh_batch_fetch: a pixel batch has no files (csh_batch_pixels)"); return -1; }
    struct PinnedOut { uint8_t *p = nullptr; size_t cap = 0; ~PinnedOut() { if (p) pinned_cache().put(p, cap); } uint8_t *data() const { return p; } } host;
    if (b->nimg && b->out.h_img_off[b->nimg]) {
        host.p = static_cast<uint8_t *>(pinned_cache().get(b->out.h_img_off[b->nimg], host.cap));
        if (!host.p) { csh_set_error("out of pinned host memory"); return -1; }
        if (csh_copy_wait(host.p, b->out.d_out.p, b->out.h_img_off[b->nimg], hipMemcpyDeviceToHost, b->stream) != hipSuccess) { csh_set_error("D2H of output failed"); return -1; }
    }
    std::atomic<int> failed{0};
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (size_t n; (n = next++) < b->items.size();) {
            Item &it = b->items[n];
            outputs[n].data = nullptr; outputs[n].length = 0;
            int code = it.code;
            std::string msg = it.msg;
            if (!code && it.image >= 0 && b->out.h_status[it.image]) { code = int(b->out.h_status[it.image]); msg = code == CS_ERR_POOL_OVERFLOW ? "device pools overflowed after 3 retries" : "device reported a malformed stream"; }
            if (!code) {
                size_t len = b->out.h_img_size[it.image];
                outputs[n].data = (uint8_t *)malloc(len ? len : 1);
                memcpy(outputs[n].data, host.data() + b->out.h_img_off[it.image], len);
                outputs[n].length = len;
            } else failed++;
            if (results) set_result(&results[n], code, msg);
        }
    };
    size_t nthreads = std::min<size_t>(std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency())), b->items.size() / 64 + 1);
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; t++) pool.emplace_back(worker);
    worker();
    for (auto &t : pool) t.join();
    return failed.load();
}

extern "C" int csh_batch_geometry(csh_batch *b, size_t image, int comp, int which, int *bw, int *bh, int *real_bw, int *real_bh) {
    if (image >= b->items.size() || b->items[image].image < 0) { csh_set_error("image not on the device"); return -1; }
    const ImgDesc &im = b->imgs[b->items[image].image];
    if (comp < 0 || comp >= (which ? im.ncomp : im.ncomp_in)) { csh_set_error("bad component"); return -1; }
    const CompGeom &g = which ? im.out[comp] : im.in[comp];
    *bw = g.bw; *bh = g.bh; *real_bw = g.real_bw; *real_bh = g.real_bh;
    return 0;
}

extern "C" int csh_batch_read_coefs(csh_batch *b, size_t image, int comp, int which, int16_t *dst) {
    int bw, bh, rbw, rbh;
    if (csh_batch_geometry(b, image, comp, which, &bw, &bh, &rbw, &rbh)) return -1;
    const ImgDesc &im = b->imgs[b->items[image].image];
    const CompGeom &g = which ? im.out[comp] : im.in[comp];
    {   // a component whose AC levels the last run kept in its level-0 list alone: they are written into its tiles here, on the batch's stream, before the copy
        const size_t at = size_t(b->items[image].image) * CSH_MAX_COMPS + size_t(comp);
        const int si = (which && b->enc.last_run_ac_lists && at < b->enc.nzset_of.size()) ? b->enc.nzset_of[at] : -1;
        if (si >= 0 && size_t(si) < b->enc.nzset_ac_lists.size() && b->enc.nzset_ac_lists[size_t(si)]) {
            if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return -1; }
            launch_nz_to_tiles(b->stream, b->enc.d_nzsets.p, b->enc.d_nzlists.p, b->enc.d_nz_pool.p, b->enc.d_nz_chunk_off.p, b->enc.d_nz_chunk_cnt.p, uint32_t(si),
                               (b->enc.nzsets[size_t(si)].nunits + 255u) / 256u, b->d_coef.p);
        }
    }
    std::vector<int16_t> tiles(size_t(g.ntiles) * CSH_TILE_I16);
    if (csh_copy_wait(tiles.data(), b->d_coef.p + size_t(g.tile_base) * CSH_TILE_I16, tiles.size() * 2, hipMemcpyDeviceToHost, b->stream) != hipSuccess) { csh_set_error("D2H failed"); return -1; }
    for (int blk = 0; blk < bw * bh; blk++)
        for (int k = 0; k < 64; k++) dst[size_t(blk) * 64 + k] = tiles[size_t(blk >> 6) * CSH_TILE_I16 + (blk & 63) * CSH_BLK_STRIDE + coef_off(k)];
    return 0;
}
