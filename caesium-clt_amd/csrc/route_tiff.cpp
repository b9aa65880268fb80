// route_tiff.cpp -- TIFF inputs with CSH_TIFF set: the cst_batch (container walk on the host; the segments' decode, the predictor both ways, the
// coders and the assembly of the files on the device) and the route that feeds it in groups.  The output holds the input's samples, page for page, with the
// compression asked for; whatever this route does not code comes back as it is.
#include <algorithm>
#include <cstring>

#include "png_kernels.h"
#include "routes.hpp"
#include "tiff_batch.hpp"

using namespace csh;
using namespace cst;

namespace {
enum { K_LZW_DEC, K_PB_DEC, K_PLACE, K_INFLATE, K_UNPREDICT, K_PREDICT, K_LZW_ENC, K_PB_ENC, K_LAYOUT, K_GATHER, K_PATCH };
const char *const KERNEL_NAMES[CST_NKERNELS] = {"tiff_lzw_decode", "tiff_packbits_decode", "tiff_place", "tiff_inflate", "tiff_unpredict", "tiff_predict", "tiff_lzw_encode", "tiff_packbits_encode",
                                                "tiff_layout", "tiff_gather", "tiff_patch"};

uint32_t strip_bytes_from_env() {
    const char *e = getenv("CSH_TIFF_STRIP");
    if (!e || !*e) return 65536;
    char *end = nullptr;
    const unsigned long v = strtoul(e, &end, 10);
    return (*end || v < 256 || v > 1048576) ? 65536u : uint32_t(v);   // anything else is not a strip size: the default stands
}
template <class T> T align_to(T v, T a) { return (v + a - 1) / a * a; }
}  // namespace

extern "C" const char *cst_kernel_name(int slot) { return slot >= 0 && slot < CST_NKERNELS ? KERNEL_NAMES[slot] : ""; }

extern "C" int cst_batch_create(const CByteArray *inputs, size_t count, const CCSParameters *p, int compression, int device, cst_batch **out) {
    *out = nullptr;
    if (compression != CST_OUT_NONE && compression != CST_OUT_LZW && compression != CST_OUT_PACKBITS) { csh_set_error("cst_batch_create: the compression is none of CST_OUT_NONE / LZW / PACKBITS"); return CS_ERR_UNSUPPORTED; }
    if (hipSetDevice(device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    cst_batch *b = new cst_batch;
    b->device = device; b->inputs = inputs; b->keep_metadata = p->keep_metadata; b->compression = compression; b->strip_bytes = strip_bytes_from_env();
    memset(&b->timing, 0, sizeof b->timing);
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) { delete b; csh_set_error("hipStreamCreate failed"); return CS_ERR_NO_DEVICE; }
    b->have_stream = true;
    b->items.resize(count); b->parsed.resize(count);
    uint32_t npages = 0;
    for (size_t i = 0; i < count; i++) {
        cst_batch::Item &it = b->items[i];
        cst_file &f = b->parsed[i];
        it.code = cst_parse(inputs[i].data, inputs[i].length, b->keep_metadata, f, it.msg);
        if (it.code) { f = cst_file(); continue; }
        if (f.pass) { it.pass = true; continue; }
        it.file = int(b->files.size());
        b->files.push_back(TiffFile{npages, uint32_t(f.pages.size()), f.big_endian ? 1u : 0u, 0u, 0});
        b->file_item.push_back(i);
        npages += uint32_t(f.pages.size());
    }
    *out = b;
    return 0;
}

extern "C" void cst_batch_destroy(cst_batch *b) { delete b; }

extern "C" int cst_batch_run(cst_batch *b, cst_timing *t) {
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    const hipStream_t st = b->stream;
    cst_timing &T = b->timing;
    memset(&T, 0, sizeof T);
    T.strip_bytes = b->strip_bytes; T.n_files = uint32_t(b->items.size());
    for (const cst_batch::Item &it : b->items) { if (it.code) T.n_failed++; if (it.pass) T.n_passed++; }
    hipEvent_t ev[2 * CST_NKERNELS + 2] = {};
    bool launched[CST_NKERNELS] = {false};
    auto timed = [&](int slot, auto fn) { (void)hipEventRecord(ev[2 * slot], st); fn(); (void)hipEventRecord(ev[2 * slot + 1], st); launched[slot] = true; };
    auto done = [&](int rc) { for (hipEvent_t &e : ev) if (e) (void)hipEventDestroy(e); if (t) *t = T; return rc; };
    for (hipEvent_t &e : ev) if (hipEventCreate(&e) != hipSuccess) { e = nullptr; csh_set_error("hipEventCreate failed"); return done(CS_ERR_NO_DEVICE); }
    (void)hipEventRecord(ev[2 * CST_NKERNELS], st);
    const uint32_t nfiles = uint32_t(b->files.size());
    b->out.clear();
    if (!nfiles) { b->ran = true; return done(0); }

    // ---- the input's segments: the files in one pool (Deflate segments once more, word-aligned for the inflate kernel), the decoded pages in another
    std::vector<uint8_t> data;
    std::vector<TiffSeg> &segs = b->segs;
    segs.clear(); b->page_first_seg.clear(); b->page_dec_off.clear();
    std::vector<uint32_t> which[4], unp_rows;   // segments by codec: LZW, PackBits, uncompressed, Deflate; the rows to un-predict, each with its segment
    std::vector<const cst_page_src *> page_src;
    uint64_t dec_bytes = 0;
    for (uint32_t fi = 0; fi < nfiles; fi++) {
        const size_t item = b->file_item[fi];
        const uint64_t base = data.size();
        data.insert(data.end(), b->inputs[item].data, b->inputs[item].data + b->inputs[item].length);
        data.resize(align_to<size_t>(data.size(), 64), 0);
        for (const cst_page_src &s : b->parsed[item].pages) {
            dec_bytes = align_to<uint64_t>(dec_bytes, 16);
            b->page_dec_off.push_back(dec_bytes); b->page_first_seg.push_back(uint32_t(segs.size())); page_src.push_back(&s);
            for (uint32_t k = 0; k < s.nseg; k++) {
                TiffSeg g;
                memset(&g, 0, sizeof g);
                g.data_off = base + s.seg_off[k]; g.data_len = uint32_t(s.seg_len[k]); g.comp = s.comp;
                g.rowbytes = s.rowbytes; g.rows = s.tiled ? s.tl : std::min(s.rps, s.height - k * s.rps);
                g.dec_off = dec_bytes; g.dec_len = g.rows * g.rowbytes; g.pred = s.pred; g.spp = s.spp;
                dec_bytes += g.dec_len;
                if (g.pred != TIFF_PRED_NONE) { g.row_base = uint32_t(unp_rows.size()); unp_rows.insert(unp_rows.end(), g.rows, uint32_t(segs.size())); }
                which[s.comp == TIFF_C_LZW ? 0 : s.comp == TIFF_C_PACKBITS ? 1 : s.comp == TIFF_C_NONE ? 2 : 3].push_back(uint32_t(segs.size()));
                segs.push_back(g);
            }
        }
    }
    std::vector<csp::PngImg> imgs;
    std::vector<uint64_t> scratch_off;
    uint64_t scratch_bytes = 0, match_words = 0;
    for (uint32_t si : which[3]) {
        TiffSeg &g = segs[si];
        const uint64_t from = g.data_off;
        g.data_off = data.size();
        data.resize(size_t(g.data_off) + g.data_len);
        memcpy(&data[size_t(g.data_off)], &data[size_t(from)], g.data_len);
        data.resize(align_to<size_t>(data.size(), 64), 0);
        csp::PngImg im;
        memset(&im, 0, sizeof im);
        im.idat_off = g.data_off; im.idat_len = g.data_len; im.inflate_off = scratch_bytes; im.inflate_len = g.dec_len; im.match_off = match_words;
        scratch_off.push_back(scratch_bytes);
        scratch_bytes += align_to<uint64_t>(uint64_t(g.dec_len) + csp::CSP_RAW_SLACK, 256);
        match_words += align_to<uint64_t>(uint64_t(g.dec_len) / 3 + 128, 32);   // a match is at least three bytes long
        imgs.push_back(im);
    }
    data.resize(data.size() + 64, 0);
    const uint32_t nseg = uint32_t(segs.size()), npages = uint32_t(page_src.size());
    T.n_pages = npages;

    std::vector<uint32_t> status(nseg, 0u), zstatus(imgs.size() + 1, 0u);
    DevBuf<uint8_t> d_data, d_scratch;
    DevBuf<TiffSeg> d_segs;
    DevBuf<uint32_t> d_which[4], d_unp_rows, d_status, d_zstatus, d_nmatch;
    DevBuf<uint64_t> d_scratch_off, d_matches;
    DevBuf<csp::PngImg> d_imgs;
    if (d_data.upload(data, st) || d_segs.upload(segs, st) || d_status.upload(status, st) || b->d_dec.alloc(size_t(dec_bytes) + 64) || d_unp_rows.upload(unp_rows, st)) return done(CS_ERR_NO_DEVICE);
    for (int c = 0; c < 4; c++) if (d_which[c].upload(which[c], st)) return done(CS_ERR_NO_DEVICE);
    timed(K_LZW_DEC, [&] { launch_tiff_lzw_decode(st, d_segs.p, d_which[0].p, uint32_t(which[0].size()), d_data.p, b->d_dec.p, d_status.p); });
    timed(K_PB_DEC, [&] { launch_tiff_packbits_decode(st, d_segs.p, d_which[1].p, uint32_t(which[1].size()), d_data.p, b->d_dec.p, d_status.p); });
    uint32_t longest[4] = {0, 0, 0, 0};
    for (int c = 0; c < 4; c++) for (uint32_t si : which[c]) longest[c] = std::max(longest[c], segs[si].dec_len);
    timed(K_PLACE, [&] { launch_tiff_place(st, d_segs.p, d_which[2].p, uint32_t(which[2].size()), longest[2], d_data.p, nullptr, b->d_dec.p, d_status.p); });
    if (!imgs.empty()) {
        if (d_imgs.upload(imgs, st) || d_scratch_off.upload(scratch_off, st) || d_zstatus.upload(zstatus, st) || d_nmatch.alloc(imgs.size() + 1) || d_scratch.alloc(size_t(scratch_bytes) + 256) ||
            d_matches.alloc(size_t(match_words) + 32)) return done(CS_ERR_NO_DEVICE);
        timed(K_INFLATE, [&] {
            csp::launch_png_inflate(st, d_imgs.p, int(imgs.size()), d_data.p, d_scratch.p, d_matches.p, d_nmatch.p, d_zstatus.p);
            launch_tiff_place(st, d_segs.p, d_which[3].p, uint32_t(which[3].size()), longest[3], d_scratch.p, d_scratch_off.p, b->d_dec.p, d_status.p);
        });
    }
    timed(K_UNPREDICT, [&] { launch_tiff_unpredict(st, d_segs.p, d_unp_rows.p, uint32_t(unp_rows.size()), b->d_dec.p); });
    if (csh_copy_wait(status.data(), d_status.p, status.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (!imgs.empty() && csh_copy_wait(zstatus.data(), d_zstatus.p, imgs.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess) || hipGetLastError() != hipSuccess) {
        csh_set_error("TIFF: the decoders failed on the device"); return done(CS_ERR_NO_DEVICE);
    }
    for (size_t k = 0; k < which[3].size(); k++) if (zstatus[k]) status[which[3][k]] = TIFF_BAD_CODE;
    b->ran = true;   // the tap reads the decoded pages from here on
    for (uint32_t fi = 0, pg = 0; fi < nfiles; fi++) {
        cst_batch::Item &it = b->items[b->file_item[fi]];
        for (uint32_t k = 0; k < b->files[fi].npages; k++, pg++) {
            const uint32_t s0 = b->page_first_seg[pg], s1 = s0 + page_src[pg]->nseg;
            for (uint32_t s = s0; s < s1 && !it.code; s++) if (status[s] != TIFF_OK) {
                it.code = CS_ERR_BAD_TIFF; T.n_failed++;
                it.msg = status[s] == TIFF_SHORT ? "TIFF: a strip's / tile's data ends before the segment is full" :
                         segs[s].comp == TIFF_C_LZW ? "TIFF: an LZW code beyond the next free table entry" :
                         segs[s].comp == TIFF_C_PACKBITS ? "TIFF: a PackBits packet that overruns its strip / tile" : "TIFF: a Deflate strip / tile that does not inflate to the segment";
            }
        }
    }

    // ---- the output rule: strips re-cut to CSH_TIFF_STRIP bytes, tiles as they are; LZW pages at depth 8 / 16 coded with and without Predictor 2
    const int mode = b->compression;
    const bool raw = mode == CST_OUT_NONE;
    const uint32_t comp_tag = mode == CST_OUT_LZW ? uint32_t(TIFF_C_LZW) : mode == CST_OUT_PACKBITS ? uint32_t(TIFF_C_PACKBITS) : uint32_t(TIFF_C_NONE);
    std::vector<TiffOut> outs;
    std::vector<TiffPage> pages(npages);
    std::vector<uint32_t> rows, relocs;   // LZW: the rows to predict; PackBits: every row; each with its output segment
    std::vector<uint8_t> heads;
    uint64_t cbuf_bytes = 0, out_bytes = 0;
    for (uint32_t fi = 0, pg = 0; fi < nfiles; fi++) {
        const cst_file &f = b->parsed[b->file_item[fi]];
        const uint8_t *d = b->inputs[b->file_item[fi]].data;
        uint64_t cap = 8;
        for (uint32_t k = 0; k < b->files[fi].npages; k++, pg++) {
            const cst_page_src &s = *page_src[pg];
            TiffPage &P = pages[pg];
            memset(&P, 0, sizeof P);
            const uint32_t R = s.tiled ? s.tl : std::max(1u, std::min(s.height, b->strip_bytes / s.rowbytes));
            const uint32_t pred = mode == CST_OUT_LZW ? s.pred_ok : uint32_t(TIFF_PRED_NONE);
            P.file = fi; P.first_out = uint32_t(outs.size()); P.nout = s.tiled ? s.nseg : (s.height + R - 1) / R; P.both = pred != TIFF_PRED_NONE;
            for (uint32_t j = 0; j < P.nout; j++) {
                TiffOut o;
                memset(&o, 0, sizeof o);
                o.rowbytes = s.rowbytes; o.rows = s.tiled ? R : std::min(R, s.height - j * R);
                o.src_off = b->page_dec_off[pg] + uint64_t(j) * R * s.rowbytes; o.len = o.rows * o.rowbytes;
                o.pred = pred; o.spp = s.spp; o.page = pg;
                o.cap = mode == CST_OUT_LZW ? tiff_lzw_cap(o.len) : mode == CST_OUT_PACKBITS ? tiff_packbits_cap(o.rowbytes, o.rows) : 0u;
                o.buf_off = cbuf_bytes; cbuf_bytes += uint64_t(o.cap) * (P.both ? 2 : 1);
                if (mode == CST_OUT_PACKBITS || pred != TIFF_PRED_NONE) { o.row_base = uint32_t(rows.size()); rows.insert(rows.end(), o.rows, uint32_t(outs.size())); }
                cap += uint64_t(raw ? o.len : o.cap) + 1;
                outs.push_back(o);
            }
            cst_write_head(d, f, s, b->keep_metadata, comp_tag, false, P.nout, R, heads, relocs, P.head[0]);
            if (P.both) cst_write_head(d, f, s, b->keep_metadata, comp_tag, true, P.nout, R, heads, relocs, P.head[1]);
            cap += std::max(P.head[0].len, P.head[1].len) + 2;
        }
        b->files[fi].out_off = out_bytes; out_bytes += align_to<uint64_t>(cap, 64);
        if (cap > 0xFFFFFFF0u && !b->items[b->file_item[fi]].code) {   // a classic TIFF's offsets are 32 bits wide
            b->items[b->file_item[fi]].pass = true; T.n_passed++;
        }
    }
    heads.resize(heads.size() + 64, 0); relocs.push_back(0);
    const uint32_t nouts = uint32_t(outs.size()), nrows = uint32_t(rows.size());
    T.n_segments = nouts;
    std::vector<uint32_t> cbytes(size_t(nouts) * 2, 0u);
    DevBuf<TiffOut> d_outs;
    DevBuf<TiffPage> d_pages;
    DevBuf<TiffFile> d_files;
    DevBuf<TiffPlace> d_place;
    DevBuf<uint32_t> d_rows, d_relocs, d_cbytes, d_row_len, d_row_start, d_seg_bytes;
    DevBuf<uint64_t> d_seg_pos, d_file_bytes;
    DevBuf<uint8_t> d_pred, d_cbuf, d_heads, d_out;
    if (d_outs.upload(outs, st) || d_pages.upload(pages, st) || d_files.upload(b->files, st) || d_rows.upload(rows, st) || d_relocs.upload(relocs, st) || d_cbytes.upload(cbytes, st) || d_heads.upload(heads, st) ||
        d_place.alloc(npages) || d_seg_bytes.alloc(nouts) || d_seg_pos.alloc(nouts) || d_file_bytes.alloc(nfiles) || d_cbuf.alloc(size_t(cbuf_bytes) + 64) || d_out.alloc(size_t(out_bytes) + 64) || d_out.zero(st))
        return done(CS_ERR_NO_DEVICE);
    if (mode == CST_OUT_LZW) {
        if (nrows && d_pred.alloc(size_t(dec_bytes) + 64)) return done(CS_ERR_NO_DEVICE);
        timed(K_PREDICT, [&] { launch_tiff_predict(st, d_outs.p, d_rows.p, nrows, b->d_dec.p, d_pred.p); });
        timed(K_LZW_ENC, [&] { launch_tiff_lzw_encode(st, d_outs.p, nouts, b->d_dec.p, d_pred.p, d_cbuf.p, d_cbytes.p); });
    } else if (mode == CST_OUT_PACKBITS) {
        if (d_row_len.alloc(nrows + 1) || d_row_start.alloc(nrows + 1)) return done(CS_ERR_NO_DEVICE);
        timed(K_PB_ENC, [&] { launch_tiff_packbits_encode(st, d_outs.p, d_rows.p, nrows, nouts, b->d_dec.p, d_row_len.p, d_row_start.p, d_cbuf.p, d_cbytes.p); });
    }
    timed(K_LAYOUT, [&] { launch_tiff_layout(st, d_files.p, nfiles, d_pages.p, d_outs.p, nouts, d_cbytes.p, raw ? 1 : 0, d_seg_pos.p, d_seg_bytes.p, d_place.p, d_file_bytes.p); });
    timed(K_GATHER, [&] { launch_tiff_gather(st, d_files.p, d_pages.p, npages, d_outs.p, nouts, b->d_dec.p, d_cbuf.p, raw ? 1 : 0, d_heads.p, d_seg_pos.p, d_seg_bytes.p, d_place.p, d_out.p); });
    timed(K_PATCH, [&] { launch_tiff_patch(st, d_files.p, d_pages.p, npages, d_relocs.p, d_seg_pos.p, d_seg_bytes.p, d_place.p, d_out.p); });
    (void)hipEventRecord(ev[2 * CST_NKERNELS + 1], st);

    // ---- sizes, verdicts, bytes
    std::vector<uint64_t> file_bytes(nfiles, 0);
    std::vector<TiffPlace> place(npages);
    if (csh_copy_wait(file_bytes.data(), d_file_bytes.p, size_t(nfiles) * 8, hipMemcpyDeviceToHost, st) != hipSuccess || csh_copy_wait(place.data(), d_place.p, size_t(npages) * sizeof(TiffPlace), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipGetLastError() != hipSuccess) { csh_set_error("TIFF: the coders failed on the device"); return done(CS_ERR_NO_DEVICE); }
    uint64_t host_bytes = 0;   // the files side by side on the host: what they came to, not what they were given room for
    for (uint32_t fi = 0; fi < nfiles; fi++) {
        cst_batch::Item &it = b->items[b->file_item[fi]];
        if (it.code || it.pass) continue;
        it.out_bytes = file_bytes[fi]; it.host_off = host_bytes; host_bytes += it.out_bytes;
        T.in_bytes += b->inputs[b->file_item[fi]].length; T.out_bytes += it.out_bytes;
        for (uint32_t k = 0; k < b->files[fi].npages; k++) if (pages[b->files[fi].first_page + k].both) (place[b->files[fi].first_page + k].variant ? T.n_pred_won : T.n_pred_lost)++;
    }
    b->out.resize(size_t(host_bytes));
    for (uint32_t fi = 0; fi < nfiles; fi++) {
        const cst_batch::Item &it = b->items[b->file_item[fi]];
        if (it.code || it.pass) continue;
        if (hipMemcpyAsync(b->out.data() + it.host_off, d_out.p + b->files[fi].out_off, size_t(it.out_bytes), hipMemcpyDeviceToHost, st) != hipSuccess) { csh_set_error("TIFF: reading the files back failed"); return done(CS_ERR_NO_DEVICE); }
    }
    if (hipStreamSynchronize(st) != hipSuccess) { csh_set_error("TIFF: reading the files back failed"); return done(CS_ERR_NO_DEVICE); }
    for (int s = 0; s < CST_NKERNELS; s++) if (launched[s]) (void)hipEventElapsedTime(&T.kernel_ms[s], ev[2 * s], ev[2 * s + 1]);
    (void)hipEventElapsedTime(&T.total_ms, ev[2 * CST_NKERNELS], ev[2 * CST_NKERNELS + 1]);
    return done(0);
}

extern "C" int cst_batch_fetch(cst_batch *b, CByteArray *outputs, CCSResult *results) {
    if (!b->ran && !b->files.empty()) { csh_set_error("cst_batch_fetch: batch not run"); return -1; }
    int failed = 0;
    for (size_t i = 0; i < b->items.size(); i++) {
        const cst_batch::Item &it = b->items[i];
        outputs[i].data = nullptr; outputs[i].length = 0;
        if (it.code) { results[i] = make_result(it.code, it.msg.c_str()); failed++; continue; }
        const uint8_t *src = it.pass ? b->inputs[i].data : b->out.data() + it.host_off;   // a file that is passed through: the input's bytes
        const size_t len = it.pass ? b->inputs[i].length : size_t(it.out_bytes);
        outputs[i].data = static_cast<uint8_t *>(malloc(len ? len : 1));
        if (!outputs[i].data) { results[i] = make_result(CS_ERR_NO_DEVICE, "out of memory"); failed++; continue; }
        memcpy(outputs[i].data, src, len); outputs[i].length = len;
        results[i] = make_result(0, nullptr);
    }
    return failed;
}

// ---- the tests' taps
static const cst_page_src *tap_page(cst_batch *b, size_t file, uint32_t page, const char *who, int *rc) {
    if (file >= b->items.size()) { csh_set_error("%s: index out of range", who); *rc = -1; return nullptr; }
    const cst_batch::Item &it = b->items[file];
    if (it.code) { *rc = it.code; return nullptr; }
    if (it.file < 0) { csh_set_error("%s: the file is passed through", who); *rc = -2; return nullptr; }
    if (page >= b->parsed[file].pages.size()) { csh_set_error("%s: no such page", who); *rc = -1; return nullptr; }
    *rc = 0;
    return &b->parsed[file].pages[page];
}
extern "C" int cst_batch_pages(cst_batch *b, size_t file, uint32_t *npages) {
    *npages = 0;
    int rc;
    if (!tap_page(b, file, 0, "cst_batch_pages", &rc)) return rc;
    *npages = uint32_t(b->parsed[file].pages.size());
    return 0;
}
extern "C" int cst_batch_page_info(cst_batch *b, size_t file, uint32_t page, uint32_t *width, uint32_t *height, uint32_t *rowbytes, uint32_t *nsegments, uint32_t *tiled, uint64_t *decoded_bytes) {
    int rc;
    const cst_page_src *s = tap_page(b, file, page, "cst_batch_page_info", &rc);
    if (!s) return rc;
    *width = s->width; *height = s->height; *rowbytes = s->rowbytes; *nsegments = s->nseg; *tiled = s->tiled ? 1u : 0u; *decoded_bytes = s->decoded;
    return 0;
}
extern "C" int cst_batch_read_decoded(cst_batch *b, size_t file, uint32_t page, uint8_t *dst) {
    int rc;
    const cst_page_src *s = tap_page(b, file, page, "cst_batch_read_decoded", &rc);
    if (!s) return rc;
    if (!b->ran) { csh_set_error("cst_batch_read_decoded: batch not run"); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) { csh_set_error("hipSetDevice failed"); return CS_ERR_NO_DEVICE; }
    const uint64_t at = b->page_dec_off[b->files[size_t(b->items[file].file)].first_page + page];
    if (csh_copy_wait(dst, b->d_dec.p + at, size_t(s->decoded), hipMemcpyDeviceToHost, b->stream) != hipSuccess) { csh_set_error("cst_batch_read_decoded: copy failed"); return CS_ERR_NO_DEVICE; }
    return 0;
}

namespace route {

// TIFF -> TIFF: groups of at most 1024 files, sized by what cst_batch_run holds on the device -- the file twice, and per decoded byte 8 bytes: the byte itself, its
// predicted twin, 1.5 each for the two LZW variants' code buffers (tiff_lzw_cap) and for the output pool, which is given room by the same caps; 4 more when a page is
// Deflate-coded (the inflate scratch and a match record of 8 bytes per 3).  That is twice the 4 bytes the route was specified with: 4 undercounts what is allocated.
// A row or a segment counts as the 2^-25th of the pool cap besides: a group then holds at most 2^25 of them (a file holds no more: cst_parse), the grids' limit.
int tiff_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, int compression) {
    int failed_total = 0;
    const uint64_t pool_cap = uint64_t(96) << 30;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        n = group_extent(inputs + g0, count - g0, 1024, uint64_t(2) << 30, pool_cap, [&](const CByteArray &f) {
            uint64_t units = 0;
            bool deflate = false;
            const uint64_t decoded = cst_declared_bytes(f.data, f.length, &units, &deflate);
            return uint64_t(1 << 20) + 2 * uint64_t(f.length) + decoded * (deflate ? 12 : 8) + units * (pool_cap >> 25);
        });
        cst_batch *b = nullptr;
        int rc = cst_batch_create(inputs + g0, n, p, compression, device, &b);
        if (rc == 0) rc = cst_batch_run(b, nullptr);
        if (rc != 0) {
            for (size_t i = 0; i < n; i++) { outputs[g0 + i].data = nullptr; outputs[g0 + i].length = 0; results[g0 + i] = make_result(rc, csh_last_error()); }
            failed_total += int(n);
        } else {
            const int failed = cst_batch_fetch(b, outputs + g0, results + g0);
            failed_total += failed < 0 ? int(n) : failed;
        }
        cst_batch_destroy(b);
    }
    return failed_total;
}

}  // namespace route
