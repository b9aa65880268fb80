// png_plan.cpp -- the planner of the PNG batch object: png_create drives its steps.  The order in which the steps append to the batch's vectors
// and take their device blocks is what every offset in the descriptors is derived from.
#include <cstring>

#include "png_batch.hpp"

namespace csp {
namespace {

// what the per-image steps add up while the batch is laid out
struct Layout {
    int nslots = 0;                  // filtered streams per image: none for a conversion or a decode-only batch
    csh::PinnedBytes idat_pool;
    size_t work_bytes = 0, stream_bytes = 256, out_bytes = 0;   // the tokenizer reads up to 8 bytes in front of a stream
    uint64_t nchunk_recs = 0;
};

// step 1: the device, the batch object with its switches, its stream and its events
int open_device(int device, const CCSParameters *p, int mode, bool from_pixels, std::unique_ptr<csp_batch> &b) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { csh_set_error("no HIP device: libcaesium_hip has no CPU path"); return CS_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { csh_set_error("device %d out of range (%d visible)", device, ndev); return CS_ERR_NO_DEVICE; }
    if (hipSetDevice(device) != hipSuccess) { csh_set_error("hipSetDevice(%d) failed", device); return CS_ERR_NO_DEVICE; }
    b.reset(new csp_batch);
    b->device = device;
    b->lossy = !p->png_optimize; b->png_quality = int(p->png_quality);
    b->deep_iters = (p->png_optimize && p->png_force_zopfli) ? int(CSP_DEEP_ITERS_ZOPFLI) : int(CSP_DEEP_ITERS);
    b->from_pixels = from_pixels;
    b->decode_only = mode == MODE_DECODE || mode == MODE_DECODE_ANY;
    b->to_webp = mode == MODE_WEBP; b->webp_quality = int(p->webp_quality);
    b->webp_mb_bytes >>= csh_test_pool_shift();   // (tests: CSH_TEST_POOL_SHIFT, read once per batch object as in batch_plan.cpp layout_token_pool)
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { csh_set_error("hipStreamCreate failed"); return CS_ERR_NO_DEVICE; }
    b->have_stream = true;
    if (b->marks.create()) { csh_set_error("hipEventCreate failed"); return CS_ERR_NO_DEVICE; }
    return 0;
}

// step 2: the trial plan: the five fixed streams always exist (the adaptive ones are gathered out of them)
void make_trial_plan(csp_batch *b, int level) {
    int set[10];
    PngPlan &plan = b->plan;
    plan.ntrials = trial_set(level, set);
    for (int s = 0; s < 10; s++) b->slot_of_strategy[s] = s < 5 ? s : -1;
    for (int t = 0; t < plan.ntrials; t++) {
        const int s = set[t];
        if (s >= 5 && b->slot_of_strategy[s] < 0) { b->slot_of_strategy[s] = 5 + plan.nadaptive; plan.adaptive_strategy[plan.nadaptive++] = s; if (s == 9) plan.need_brute = 1; }
        plan.trial_slot[t] = b->slot_of_strategy[s]; plan.trial_strategy[t] = s;
    }
}

// step 3a: two regions of the work buffer per image.  Plain image: A takes the inflated stream, B the pixels.  Adam7: A takes the
// seven passes' streams, B their reconstructed rows, and the gather puts the image back into A
void layout_work_regions(csp_batch *b, const PngItem &it, PngImg &im, Layout &L) {
    static const uint32_t XS[7] = {0, 4, 0, 2, 0, 1, 0}, YS[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
    const uint64_t bits = uint64_t(it.channels) * it.depth, image_bytes = uint64_t(it.height) * it.rowbytes;
    uint64_t pass_stream = 0, pass_pixels = 0;
    uint32_t pw[7], ph[7], prb[7];
    for (int p = 0; p < 7; p++) {
        pw[p] = (it.width + DX[p] - 1 - XS[p]) / DX[p]; ph[p] = (it.height + DY[p] - 1 - YS[p]) / DY[p];
        prb[p] = (pw[p] && ph[p]) ? uint32_t((uint64_t(pw[p]) * bits + 7) / 8) : 0u;
        if (prb[p]) { pass_stream += uint64_t(ph[p]) * (1 + prb[p]); pass_pixels += uint64_t(ph[p]) * prb[p]; }
    }
    im.inflate_len = it.interlace ? pass_stream : im.raw_len;
    const uint64_t A = L.work_bytes; L.work_bytes += align_up(std::max(im.inflate_len, image_bytes) + CSP_RAW_SLACK, 256);
    const uint64_t B = L.work_bytes; L.work_bytes += align_up(std::max(image_bytes, it.interlace ? pass_pixels : 0) + 64, 256);
    im.inflate_off = A;
    const uint32_t image_index = uint32_t(b->imgs.size());
    if (!it.interlace) {
        im.raw_off = A; im.pix_off = B;
        b->passes.push_back(PngPass{image_index, it.rowbytes, it.height, it.bpp, A, B});
        return;
    }
    im.pix_off = A; im.raw_off = B;
    PngAdam7 a{};
    a.image = image_index; a.bits = uint32_t(bits);
    uint64_t so = A, po = B;
    for (int p = 0; p < 7; p++) {
        a.base[p] = po; a.prb[p] = prb[p];
        if (!prb[p]) continue;
        b->passes.push_back(PngPass{image_index, prb[p], ph[p], it.bpp, so, po});
        so += uint64_t(ph[p]) * (1 + prb[p]); po += uint64_t(ph[p]) * prb[p];
    }
    b->adam7.push_back(a);
    b->adam7_items = std::max<uint64_t>(b->adam7_items, bits >= 8 ? uint64_t(it.width) * it.height : image_bytes);
}

// step 4: the WebP descriptors of one image: its expansion to 8-bit samples and its place in the VP8 encoder's buffers
void add_webp_image(csp_batch *b, const PngItem &it, const PngImg &im) {
    // 8-bit grey / RGB for the VP8 encoder; an alpha channel or a tRNS chunk rides along as a fourth (second) sample: the encoder skips it, the
    // VP8L coder makes the file's ALPH chunk of it when the results are fetched
    const uint32_t nc = rgb_channels(it, true);
    const RgbJob j = add_rgb_job(it, nc, im.pix_off, b->rgb_bytes, b->plte);
    b->walpha.resize(b->imgs.size() + 1, 0);
    b->walpha[b->imgs.size()] = it.transparent() ? uint8_t(nc) : uint8_t(0);
    b->rgb_bytes += align_up(uint64_t(it.width) * it.height * nc + 64, 256);
    b->rgb_max_h = std::max(b->rgb_max_h, it.height);
    b->rgbjobs.push_back(j);
    csw::WebpImg wi{};
    wi.width = it.width; wi.height = it.height; wi.mbw = (it.width + 15) / 16; wi.mbh = (it.height + 15) / 16; wi.ncomp = nc;
    wi.rgb_off = j.dst_off; wi.image = uint32_t(it.image);
    const uint64_t ly = uint64_t(wi.mbw) * wi.mbh * 256, lc = uint64_t(wi.mbw) * wi.mbh * 64;
    auto take = [&](uint64_t n) { uint64_t at = b->wwork_bytes; b->wwork_bytes += (n + 63) & ~uint64_t(63); return at; };
    wi.y_off = take(ly); wi.u_off = take(lc); wi.v_off = take(lc); wi.ry_off = take(ly); wi.ru_off = take(lc); wi.rv_off = take(lc);
    wi.lev_off = b->wlevels; b->wlevels += uint64_t(wi.mbw) * wi.mbh * csw::WEBP_MB_REC;
    b->wmax_luma = std::max<uint32_t>(b->wmax_luma, uint32_t(ly));
    b->wmax_mbh = std::max(b->wmax_mbh, wi.mbh);
    b->wimgs.push_back(wi);
}

// step 3: one image: its IDAT bytes into the pinned pool, its regions, streams, chunks, reduction flags, carried bytes and output space.  Returns an
// error of the whole batch; a file that cannot be taken gets its code in `it` and no image
int layout_image(csp_batch *b, PngItem &it, const uint8_t *file, bool from_pixels, Layout &L) {
    auto refuse = [&](int code, const char *msg) { it.code = code; it.msg = msg; return 0; };
    if (b->to_webp && uint64_t((it.width + 15) / 16) * ((it.height + 15) / 16) * 256 > 0x7FFFFFFFu) return refuse(CS_ERR_UNSUPPORTED, "PNG too large for one device batch");
    if (b->decode_only && it.has_trns && it.trns.size() != (it.ctype == 3 ? it.trns.size() : it.ctype == 0 ? 2u : it.ctype == 2 ? 6u : ~size_t(0))) return refuse(CS_ERR_BAD_PNG, "bad tRNS");
    PngImg im{};
    im.width = it.width; im.height = it.height; im.rowbytes = it.rowbytes; im.bpp = it.bpp;
    im.raw_len = uint64_t(it.height) * (uint64_t(it.rowbytes) + 1);
    if (im.raw_len > (uint64_t(1) << 36) || uint64_t(b->total_rows) + it.height > 0x7FFFFFFFu) return refuse(CS_ERR_UNSUPPORTED, "PNG too large for one device batch");
    im.idat_off = L.idat_pool.size(); im.idat_len = uint32_t(it.idat_len);
    if (!from_pixels) {   // the IDAT payloads back to back (a stream may be cut anywhere, even inside the zlib header)
        size_t at = L.idat_pool.size(), end = align_up(at + it.idat_len + 8, 256);
        if (!L.idat_pool.reserve(end)) { csh_set_error("out of pinned host memory"); return CS_ERR_NO_DEVICE; }
        for (auto &r : it.idat) { L.idat_pool.pending.push_back({at, file + r.first, r.second, 0}); at += r.second; }
        L.idat_pool.pending.push_back({at, file, 0, end - at});
        L.idat_pool.n = end;
    }
    layout_work_regions(b, it, im, L);
    im.stream_stride = align_up(im.raw_len + 64, 256);
    im.stream_off = L.stream_bytes; im.match_off = L.stream_bytes / 8;   // a match is at least three bytes long
    L.stream_bytes += std::max<uint64_t>(im.stream_stride * uint64_t(L.nslots), align_up((im.inflate_len / 3 + 128) * 8, 256));
    im.row_base = b->total_rows; b->total_rows += it.height;
    im.nchunks = uint32_t((im.raw_len + CSP_CHUNK - 1) / CSP_CHUNK);
    im.chunk_base = uint32_t(L.nchunk_recs); L.nchunk_recs += uint64_t(im.nchunks) * L.nslots;
    im.chunk_stride = im.nchunks;
    im.channels = it.channels; im.bps = (it.ctype != 3 && it.depth >= 8) ? it.depth / 8 : 0;
    b->cand0.push_back((!it.no_reduce && !it.has_plte && im.bps && (im.channels == 3 || im.channels == 4)) ? im.channels : 0u);
    // bits 1 / 2 / 4 / 8-32: 16 -> 8 bits, alpha away, colour -> grey, grey depth 4 / 2 / 1; bit 64: an 8-bit indexed image (k_png_used finds the palette entries it uses)
    b->flags0.push_back((it.ctype == 3 && it.depth == 8 && !it.pal_tied && !from_pixels) ? 64u
                        : (it.no_reduce || !im.bps) ? 0u : ((im.bps == 2 ? 1u : 0u) | ((im.channels == 2 || im.channels == 4) ? 2u : 0u) | (im.channels >= 3 ? 4u : 0u) | 56u));
    if (L.nchunk_recs > 0x7FFFFFFFu) { csh_set_error("PNG batch too large"); return CS_ERR_POOL_OVERFLOW; }
    im.prefix_len = uint32_t(it.prefix.size()); im.suffix_len = uint32_t(it.suffix.size());
    im.fix_off = b->fixed.size();
    b->fixed.insert(b->fixed.end(), it.prefix.begin(), it.prefix.end());
    b->fixed.insert(b->fixed.end(), it.suffix.begin(), it.suffix.end());
    im.out_cap = uint64_t(im.prefix_len) + 1100 /* a PLTE and a tRNS chunk a reduction may add */ + 12 + im.suffix_len + 6 + uint64_t(im.nchunks) * (CSP_CHUNK + CSP_CHUNK / 8 + 1024);
    if (im.out_cap > 0xFFFFFFF0u) return refuse(CS_ERR_UNSUPPORTED, "PNG too large for one device batch");
    im.out_off = L.out_bytes;
    if (!b->to_webp && !b->decode_only) L.out_bytes += align_up(im.out_cap + 16, 256);
    const uint32_t pieces = uint32_t((im.out_cap + 1023) / 1024);
    if (pieces > b->max_pieces) b->max_pieces = pieces;
    it.image = int(b->imgs.size());
    if (b->to_webp) add_webp_image(b, it, im);
    b->imgs.push_back(im);
    b->raw_total += im.raw_len; b->pixels += uint64_t(it.width) * it.height;
    return 0;
}

// step 5: which image every row belongs to
std::vector<uint32_t> build_row_index(const csp_batch *b) {
    std::vector<uint32_t> row_image(b->total_rows);
    uint32_t r = 0;
    for (size_t i = 0; i < b->imgs.size(); i++) for (uint32_t y = 0; y < b->imgs[i].height; y++) row_image[r++] = uint32_t(i);
    return row_image;
}

// step 6: every device block of the batch; the descriptors go up as their blocks are taken
int allocate(csp_batch *b, const Layout &L, const std::vector<uint32_t> &row_image) {
    hipStream_t st = b->stream;
    const size_t nimg = b->imgs.size();
    if (upload_chunk_index(b)) return CS_ERR_NO_DEVICE;
    if (b->d_imgs.upload(b->imgs, st) || b->d_row_image.upload(row_image, st) || b->d_fixed.upload(b->fixed, st) || b->d_flags.alloc(nimg + 1) || b->d_jobs.alloc(nimg + 1))
        return CS_ERR_NO_DEVICE;
    if (b->d_idat.alloc(L.idat_pool.size() + 256) || b->d_work.alloc(L.work_bytes + 256) || b->d_passes.upload(b->passes, st) || b->d_adam7.upload(b->adam7, st) || b->d_streams.alloc(L.stream_bytes + 256) ||
        b->d_out.alloc(L.out_bytes + 256) || b->d_choice.alloc(size_t(5) * b->total_rows + 1) || b->d_status.alloc(nimg + 1) || b->d_file_len.alloc(nimg + 1) ||
        b->d_adler.alloc(2 * size_t(b->total_chunks) + 2) || b->d_crc.alloc(nimg * b->max_pieces + 1) || b->d_scores.alloc(size_t(b->total_rows) * 25 + 1) ||
        b->d_trial_bytes.alloc(nimg * CSP_MAX_STREAMS + 1) || b->d_nmatch.alloc(nimg + 1) || b->d_winner.alloc(nimg + 1) || b->d_trial_live.alloc(nimg * CSP_MAX_STREAMS + 1) || b->d_chunks.alloc(size_t(L.nchunk_recs) + 1))
        return CS_ERR_NO_DEVICE;
    if (b->to_webp && (b->d_rgbjobs.upload(b->rgbjobs, st) || b->d_plte.upload(b->plte, st) || b->d_rgb.alloc(b->rgb_bytes + 256) || b->d_wwork.alloc(b->wwork_bytes + 64) ||
                       b->d_wlevels.alloc(b->wlevels + 64) || b->d_wstats.alloc(nimg * 2112 + 8) || b->d_wprobs.alloc(nimg * 1056 + 8) || b->d_wupdate.alloc(nimg * 1056 + 8) ||
                       b->d_wpart.alloc(nimg * 9 + 9) || b->d_wstatus.alloc(nimg + 1)))
        return CS_ERR_NO_DEVICE;
    return 0;
}

// step 7: the sources: the IDAT pool, or the pixels of a batch that starts from pixels (device to device)
int upload_sources(csp_batch *b, const Layout &L, const csp_pixels *px, size_t count) {
    hipStream_t st = b->stream;
    if (L.idat_pool.size()) {
        if (hipMemcpyAsync(b->d_idat.p, L.idat_pool.p, L.idat_pool.size(), hipMemcpyHostToDevice, st) != hipSuccess) { csh_set_error("upload failed"); return CS_ERR_NO_DEVICE; }
    }
    for (size_t i = 0; px && i < count; i++) {
        const PngItem &it = b->items[i];
        if (it.image < 0) continue;
        if (hipMemcpyAsync(b->d_work.p + b->imgs[it.image].pix_off, px[i].device_pixels, size_t(it.height) * it.rowbytes, hipMemcpyDeviceToDevice, st) != hipSuccess) { csh_set_error("pixel copy failed"); return CS_ERR_NO_DEVICE; }
    }
    if (hipStreamSynchronize(st) != hipSuccess) { csh_set_error("upload failed"); return CS_ERR_NO_DEVICE; }   // the pinned pool goes back to the cache
    return 0;
}

}  // namespace

// (re)build the per-chunk / per-group index arrays from the current geometry of the images
int upload_chunk_index(csp_batch *b) {
    const int nimg = int(b->imgs.size());
    std::vector<uint32_t> chunk_image, chunk_first(size_t(nimg) + 1), group_image, group_first(size_t(nimg) + 1);
    for (int i = 0; i < nimg; i++) {
        chunk_first[i] = uint32_t(chunk_image.size()); group_first[i] = uint32_t(group_image.size());
        for (uint32_t k = 0; k < b->imgs[i].nchunks; k++) chunk_image.push_back(uint32_t(i));
        for (uint32_t g = 0; g < (b->imgs[i].nchunks + CSP_GROUP - 1) / CSP_GROUP; g++) group_image.push_back(uint32_t(i));
    }
    chunk_first[nimg] = uint32_t(chunk_image.size()); group_first[nimg] = uint32_t(group_image.size());
    b->total_chunks = uint32_t(chunk_image.size()); b->total_groups = uint32_t(group_image.size());
    chunk_image.push_back(0); group_image.push_back(0);
    if (b->d_chunk_image.upload(chunk_image, b->stream) || b->d_chunk_first.upload(chunk_first, b->stream) || b->d_group_image.upload(group_image, b->stream) ||
        b->d_group_first.upload(group_first, b->stream))
        return -1;
    return hipStreamSynchronize(b->stream) == hipSuccess ? 0 : -1;   // the host vectors go out of scope
}

int png_create(const CByteArray *inputs, const csp_pixels *px, size_t count, const CCSParameters *p, int device, int mode, csp_batch **out, const std::vector<PreFail> *pre,
               const std::vector<uint8_t> *px_bits) {
    *out = nullptr;
    std::unique_ptr<csp_batch> b;
    if (int rc = open_device(device, p, mode, px != nullptr, b)) return rc;
    make_trial_plan(b.get(), int(p->png_optimization_level));
    Layout L;
    L.nslots = (b->to_webp || b->decode_only) ? 0 : 5 + b->plan.nadaptive;   // a conversion has no filtered streams
    b->items.resize(count);
    b->inputs.resize(count);
    for (size_t i = 0; i < count; i++) {
        PngItem &it = b->items[i];
        b->inputs[i] = px ? nullptr : inputs[i].data;
        if (pre && (*pre)[i].code) { it.code = (*pre)[i].code; it.msg = (*pre)[i].msg; }
        else if (px) pixels_item(px[i], px_bits ? (*px_bits)[i] : 8, it);
        else parse_png(inputs[i].data, inputs[i].length, p->keep_metadata, it);
        if (it.code) continue;
        if (int rc = layout_image(b.get(), it, b->inputs[i], px != nullptr, L)) return rc;
    }
    L.idat_pool.flush_copies();
    const std::vector<uint32_t> row_image = build_row_index(b.get());
    if (int rc = allocate(b.get(), L, row_image)) return rc;
    if (int rc = upload_sources(b.get(), L, px, count)) return rc;
    *out = b.release();
    return 0;
}

}  // namespace csp
