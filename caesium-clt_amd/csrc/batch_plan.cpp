// batch_plan.cpp -- the planner of the JPEG batch object: parsed files -> the host descriptors of every phase, their pool layout,
// the device allocations and the upload.  Host work is limited to container logic: marker parsing, table/script setup, descriptor
// building.  batch_create (pipeline.cpp) calls the steps of BatchPlanner in order; the order in which they append to the batch's
// vectors is what the descriptors' offsets are derived from.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>

#include "batch.hpp"
#include "resize_host.h"
#include "result.h"

namespace csh {

// ------------------------------------------------------------------------------------------------
static void build_dev_huff(const HuffSpec &h, DevHuff &d) {
    memset(&d, 0, sizeof d);
    for (int l = 0; l < 18; l++) d.maxcode[l] = -1;
    if (!h.present) return;
    int code = 0, p = 0;
    for (int l = 1; l <= 16; l++) {
        if (h.bits[l]) {
            d.valptr[l] = p - code;
            for (int i = 0; i < h.bits[l]; i++, p++, code++)
                if (l <= 9) {
                    int base = code << (9 - l);
                    for (int k = 0; k < (1 << (9 - l)); k++) d.look[(base + k) & 511] = uint16_t((l << 8) | h.vals[p]);
                }
            d.maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    d.maxcode[17] = 0x7FFFFFFF;
    memcpy(d.vals, h.vals, 256);
}
// two-level table of the parallel decoder; returns false when the shared sub-table pool is exhausted
static bool build_par_huff(const HuffSpec &h, uint16_t root[512], uint16_t *sub, int &sub_used) {
    memset(root, 0, 512 * sizeof(uint16_t));
    if (!h.present) return true;
    // canonical codes, left-aligned to 16 bits
    struct Code { uint16_t first; uint8_t len, sym; };
    std::vector<Code> longc;
    int code = 0, p = 0;
    for (int l = 1; l <= 16; l++) {
        for (int i = 0; i < h.bits[l]; i++, p++, code++) {
            if (l <= 9) {
                int base = code << (9 - l);
                for (int k = 0; k < (1 << (9 - l)); k++) root[(base + k) & 511] = uint16_t((l << 8) | h.vals[p]);
            } else longc.push_back({uint16_t(code << (16 - l)), uint8_t(l), h.vals[p]});
        }
        code <<= 1;
    }
    for (size_t i = 0; i < longc.size();) {
        const int prefix = longc[i].first >> 7;
        size_t j = i;
        int maxlen = 0;
        while (j < longc.size() && (longc[j].first >> 7) == prefix) { maxlen = std::max<int>(maxlen, longc[j].len); j++; }
        const int nbits = maxlen - 9, n = 1 << nbits;
        if (sub_used + n > CSH_PAR_SUB) return false;
        uint16_t *t = sub + sub_used;
        memset(t, 0, n * sizeof(uint16_t));
        for (size_t c = i; c < j; c++) {
            int lo = (longc[c].first & 127) >> (7 - nbits), span = 1 << (maxlen - longc[c].len);
            for (int k = 0; k < span; k++) t[lo + k] = uint16_t((longc[c].len << 8) | longc[c].sym);
        }
        root[prefix & 511] = uint16_t(0x8000 | (nbits << 12) | sub_used);
        sub_used += n;
        i = j;
    }
    return true;
}

static void make_quant(const uint16_t nat[64], DevQuant &q) {
    for (int k = 0; k < 64; k++) {
        q.q[k] = nat[kZigZag[k]];
        q.div[k] = int32_t(q.q[k]) * 8;
        q.rcp[k] = float((1.0 / double(q.div[k])) * (1.0 + 1.0 / 524288.0));   // the pixel kernels' quantiser: one fma (k_pixel.hip quant_one); exact for every 16-bit q
        q.lt[k] = float(1.0 / double(int(q.q[k]) * int(q.q[k])));   // mozjpeg quantize_trellis, mode 1: lambda_table[i] = 1.0 / (q * q)
        q.mul[k] = 0; q.sh[k] = 0;
        if (q.div[k] > 0 && q.div[k] < (1 << 14)) {
            int lg = 0;
            while ((2 << lg) <= q.div[k]) lg++;   // floor(log2 div)
            const int P = std::max(25, lg + 18);
            q.mul[k] = uint32_t((1ull << P) / uint64_t(q.div[k])) + 1u;
            q.sh[k] = uint32_t(32 - P);
        }
    }
}

static void fill_geom(const JComp &c, CompGeom &g, uint32_t &ntiles) {
    g.h = c.h; g.v = c.v; g.comp_w = c.comp_w; g.comp_h = c.comp_h;
    g.real_bw = c.real_bw; g.real_bh = c.real_bh; g.bw = c.bw; g.bh = c.bh;
    g.ntiles = (c.bw * c.bh + 63) / 64;
    g.tile_base = ntiles;
    ntiles += g.ntiles;
}

// output script -> EncScan entries (progressive: libjpeg jpeg_simple_progression; sequential: one interleaved scan).
// A component's Huffman table ids are its libjpeg table number in the frame's colour space (table_class): Y 0 and chroma 1; R, G, B and
// C, M, Y, K all 0; of YCCK, Y and K 0, Cb and Cr 1.
static void add_script(std::vector<EncScan> &v, int ncomp, bool progressive, int space) {
    for (const OutScan &o : output_script(ncomp, progressive, space == CSH_CS_YCC)) {
        EncScan e;
        memset(&e, 0, sizeof e);
        e.ncomp = o.ncomp; e.Ss = o.Ss; e.Se = o.Se; e.Ah = o.Ah; e.Al = o.Al;
        for (int k = 0; k < o.ncomp; k++) e.comp[k] = o.comp[k];
        if (!progressive) {
            e.sequential = 1;
            for (int k = 0; k < o.ncomp; k++) {   // DHT order: per component DC then AC, each table once (libjpeg write_scan_header)
                int id = table_class(space, o.comp[k]);
                int di = -1, ai = -1;
                for (int t = 0; t < e.ntables; t++) { if (e.dht_id[t] == id) di = t; if (e.dht_id[t] == (0x10 | id)) ai = t; }
                if (di < 0) { di = e.ntables; e.dht_id[e.ntables++] = id; }
                if (ai < 0) { ai = e.ntables; e.dht_id[e.ntables++] = 0x10 | id; }
                e.dc_tbl[k] = di; e.ac_tbl[k] = ai;
                e.sos_tdta[k] = (id << 4) | id;
            }
        } else if (o.Ss == 0) {
            if (o.Ah == 0) {
                e.ntables = 0;
                for (int k = 0; k < o.ncomp; k++) {
                    int id = table_class(space, o.comp[k]);
                    int idx = -1;
                    for (int t = 0; t < e.ntables; t++) if (e.dht_id[t] == id) idx = t;
                    if (idx < 0) { idx = e.ntables; e.dht_id[e.ntables++] = id; }
                    e.dc_tbl[k] = idx;
                    e.sos_tdta[k] = id << 4;
                }
            }
        } else {
            int id = table_class(space, o.comp[0]);
            e.ntables = 1; e.dht_id[0] = 0x10 | id; e.sos_tdta[0] = id;
        }
        v.push_back(e);
    }
}

// decoded plane -> full resolution: libjpeg-turbo's choice of upsampling method (jdsample.c jinit_upsampler), cw the downsampled width
static UpDesc up_desc(int hx, int vx, int cw) {
    UpDesc u; u.hx = uint8_t(hx); u.vx = uint8_t(vx); u.pad = 0;
    if (hx == 1 && vx == 1) u.cls = CSH_UP_COPY;
    else if (hx == 2 && vx == 1 && cw > 2) u.cls = CSH_UP_H2V1;
    else if (hx == 1 && vx == 2) u.cls = CSH_UP_H1V2;
    else if (hx == 2 && vx == 2 && cw > 2) u.cls = CSH_UP_H2V2;
    else u.cls = CSH_UP_REP;
    return u;
}
// full resolution -> encoder plane (jcsample.c): the output layouts are 4:4:4, 4:2:2, 4:2:0 and 4:1:1 (plan_item)
static int dn_kind(int hx, int vx) { return hx == 1 ? CSH_DN_FULL : (hx == 4 ? CSH_DN_H4V1 : (vx == 2 ? CSH_DN_H2V2 : CSH_DN_H2V1)); }

// decide the output frame for one parsed JPEG; returns 0 or an error code.  to_rgb: the run goes through the image's RGB (a resize, WebP or
// pixel output): an RGB / CMYK / YCCK source is converted there (k_planes_to_rgb_space) and what follows is an ordinary three-component image
static int plan_item(Item &it, const CCSParameters &p, bool lossless, bool to_rgb) {
    const JpegInfo &in = it.in;
    if (in.ncomp != 1 && in.ncomp != 3 && in.ncomp != 4) { it.msg = "unsupported component count"; return CS_ERR_JPEG_FEATURE; }
    // one image's planes, tiles and unit arrays are indexed with 32 bits and take ~25 bytes per pixel of HBM: a header that declares
    // more than 2^28 pixels (16384 x 16384) fails here, by itself, instead of sizing the whole batch's pools
    if (uint64_t(in.width) * uint64_t(in.height) > (1ull << 28)) { it.msg = "image dimensions too large for the device path"; return CS_ERR_JPEG_FEATURE; }
    const bool other_space = in.space != CSH_CS_GREY && in.space != CSH_CS_YCC;   // RGB, CMYK, YCCK: coded in their own space (mozjpeg with out_color_space = jpeg_color_space)
    const bool converted = other_space && to_rgb;
    it.out = JpegInfo();
    JpegInfo &o = it.out;
    o.width = in.width; o.height = in.height; o.ncomp = converted ? 3 : in.ncomp;
    o.space = converted ? CSH_CS_YCC : in.space;
    if (other_space && !converted) { o.write_jfif = false; o.write_adobe = in.adobe_transform; }   // the Adobe segment exactly when the source has one, with its transform
    if (p.width || p.height) {
        if (lossless) { it.msg = "resize + lossless transcode not on the device path"; return CS_ERR_UNSUPPORTED; }
        csh_compute_dimensions(in.width, in.height, int(p.width), int(p.height), o.width, o.height);
        if (o.width > 65500 || o.height > 65500 || uint64_t(o.width) * uint64_t(o.height) > (1ull << 28)) { it.msg = "resize target too large for JPEG"; return CS_ERR_JPEG_FEATURE; }
    }
    if (in.ncomp >= 3 && (!lossless || in.ncomp == 4)) {
        // any layout libjpeg decodes: every component's up factors hmax / h and vmax / v integers in 1..4 (jdsample.c int_upsample), at most
        // 10 blocks per MCU (D_MAX_BLOCKS_IN_MCU)
        int blocks = 0;
        for (int c = 0; c < in.ncomp; c++) {
            const JComp &k = in.comp[c];
            blocks += k.h * k.v;
            if (in.hmax % k.h || in.vmax % k.v) { it.msg = "fractional chroma sampling ratio (component factors do not divide the largest ones)"; return CS_ERR_JPEG_FEATURE; }
            if (in.hmax / k.h > 4 || in.vmax / k.v > 4) { it.msg = "chroma sampling ratio above 4"; return CS_ERR_JPEG_FEATURE; }
        }
        if (blocks > 10) { it.msg = "more than 10 blocks per MCU"; return CS_ERR_JPEG_FEATURE; }
    }
    if (lossless) {
        // the output carries the slots as the file leaves them (frame_header): a component decoded with other contents cannot be
        // transcoded (libjpeg jpeg_copy_critical_parameters: JERR_MISMATCHED_QUANT_TABLE)
        for (int c = 0; c < in.ncomp; c++)
            if (memcmp(in.comp[c].qt, in.qt[in.comp[c].tq], sizeof in.comp[c].qt)) { it.msg = "a component was decoded with a quantisation table that its slot no longer holds"; return CS_ERR_JPEG_FEATURE; }
        for (int c = 0; c < in.ncomp; c++) o.comp[c] = in.comp[c];
        jpeg_geometry(o);
        return 0;
    }
    int ss = int(p.jpeg_chroma_subsampling);
    if (ss == 0) ss = 420;
    // libjpeg jpeg_set_colorspace: ids 1.. (R G B / C M Y K by letter), every component 1x1, the table number of its class
    static const char kRgbIds[] = "RGB", kCmykIds[] = "CMYK";
    for (int c = 0; c < o.ncomp; c++) {
        o.comp[c].id = o.space == CSH_CS_RGB ? kRgbIds[c] : (o.space == CSH_CS_CMYK ? kCmykIds[c] : c + 1);
        o.comp[c].h = o.comp[c].v = 1; o.comp[c].tq = table_class(o.space, c);
    }
    // the subsampling setting shapes YCbCr and YCCK frames (K follows Y); R, G, B and C, M, Y, K stay at full resolution
    if (o.space == CSH_CS_YCC || o.space == CSH_CS_YCCK) {
        int h = 1, v = 1;
        if (ss == 420) { h = 2; v = 2; }
        else if (ss == 422) { h = 2; v = 1; }
        else if (ss == 411) { h = 4; v = 1; }
        else if (ss != 444) { it.msg = "unknown output chroma subsampling"; return CS_ERR_JPEG_FEATURE; }
        o.comp[0].h = h; o.comp[0].v = v;
        if (o.space == CSH_CS_YCCK) { o.comp[3].h = h; o.comp[3].v = v; }
    }
    jpeg_geometry(o);
    return 0;
}

// token pool (k_entropy.hip): every region gets its estimate x tok_scale (the scale grows on overflow, like the other pools)
void layout_token_pool(csh_batch *b) {
    b->enc.regions.resize(b->enc.region_est.size());
    // CSH_TEST_POOL_SHIFT=n (tests): every estimate divided by 2^n, so that the first runs overflow and the batch goes through its retries with larger pools
    // (read once per batch object, at its first layout: the retries of a run keep what the run started with -- ADVICE r05; an unsupported test hook)
    // The same read divides the WebP tail's first reservation per macroblock (batch.hpp WebpTail): 768 -> 48 with shift 4, -> 0 with shift 16, which no retry makes larger
    if (b->test_pool_shift < 0) { b->test_pool_shift = csh_test_pool_shift(); b->wp.webp_mb_bytes >>= b->test_pool_shift; }
    const int shift = b->test_pool_shift;
    uint64_t at = 0;
    for (size_t i = 0; i < b->enc.regions.size(); i++) {
        const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>((uint64_t(b->enc.region_est[i]) * b->enc.tok_scale) >> shift, 64), 0xFFFFFFF0ull);
        b->enc.regions[i].base = at; b->enc.regions[i].cap = uint32_t(cap); b->enc.regions[i].pad = 0;
        at += (cap + 3) & ~uint64_t(3);
    }
    b->enc.tok_cap = at + 64;
    // the list pool (k_aclist.hip): the same rule, capped by what a list can hold at most; regions start on 16-byte boundaries
    at = 0;
    for (size_t i = 0; i < b->enc.nzlists.size(); i++) {
        const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>((uint64_t(b->enc.nz_est[i]) * b->enc.tok_scale) >> shift, 64), b->enc.nz_worst[i]);
        b->enc.nzlists[i].base = at; b->enc.nzlists[i].cap = uint32_t(cap);
        at += (cap + 3) & ~uint64_t(3);
    }
    b->enc.nz_cap = at + 64;
}

PlanSwitches PlanSwitches::read() {
    auto is = [](const char *name, const char *v) { const char *e = getenv(name); return e && !strcmp(e, v); };
    PlanSwitches s;
    const char *penv = getenv("CSH_PROFILE");
    s.profile = penv && *penv ? penv : "mozjpeg";
    s.nz_once = !is("CSH_NZ_ONCE", "0");
    s.tr_sort = !is("CSH_TR_SORT", "0");
    s.nz_fused = !is("CSH_NZ_FUSED", "0");
    s.ac_tiles = is("CSH_AC_TILES", "1");
    s.ref_list = is("CSH_REF_LIST", "1") || (s.ref_list && !is("CSH_REF_LIST", "0"));   // "1" / "0" name the path, anything else leaves the default
    s.ref_pack = s.ref_list && (is("CSH_REF_PACK", "1") || (s.ref_pack && !is("CSH_REF_PACK", "0")));   // the same; CSH_REF_LIST=0 switches it off by itself
    const char *pp = getenv("CSH_PROG_PAR");
    s.prog_par = pp && !strcmp(pp, "0") ? 0 : (pp && !strcmp(pp, "1") ? 1 : -1);
    s.fused_420 = !getenv("CSH_NO_FUSED_420");
    if (const char *lr = getenv("CSH_LIST_RUN")) { if (*lr) s.list_run = uint32_t(std::min(32, std::max(1, atoi(lr)))); }
    s.ac_runs_slot = is("CSH_AC_RUNS", "slot");
    for (uint32_t g : {1u, 2u, 4u, 8u}) if (is("CSH_DEC_GROUP", std::to_string(g).c_str())) s.dec_group = g;
    s.dec_clear_front = is("CSH_DEC_CLEAR", "front");
    if (const char *tr = getenv("CSH_TEST_DEC_ROUNDS")) { if (*tr) s.test_dec_rounds = std::max(0, atoi(tr)); }   // (an unsupported test hook, like CSH_TEST_POOL_SHIFT)
    s.dec_lanes = is("CSH_DEC_LANES", "192") ? 192u : is("CSH_DEC_LANES", "256") ? 256u : 0u;
    return s;
}

Laps::Laps() : trace(getenv("CSH_TRACE") != nullptr) {}
void Laps::lap(const char *what) {
    if (!trace) return;
    const auto now = std::chrono::steady_clock::now();
    char buf[64];
    snprintf(buf, sizeof buf, " %s %.1f", what, std::chrono::duration<double, std::milli>(now - at).count());
    text += buf; at = now;
}

BatchPlanner::BatchPlanner(csh_batch *b_, const CByteArray *inputs_, size_t count_, const CCSParameters *p_, const csp_pixels *px_)
    : b(b_), inputs(inputs_), count(count_), p(p_), px(px_), sw(PlanSwitches::read()), progressive(p_->jpeg_progressive) {}

// modes from the profile, the output quantisation tables, the stock scripts
void BatchPlanner::begin() {
    b->items.resize(count);
    quality_table(int(p->jpeg_quality), qout_nat);
    DevQuant qo; make_quant(qout_nat, qo);
    b->quants.push_back(qo);  // index 0: output table (luma == chroma in mozjpeg's profile 3)
    b->q_base = int(b->quants.size()) - 1;   // then one table per quality 1..100 (size targeting re-targets per image)
    for (int q = 1; q <= 100; q++) { uint16_t tq[64]; quality_table(q, tq); DevQuant dq; make_quant(tq, dq); b->quants.push_back(dq); }
    b->progressive = progressive;
    b->enc.list_run = sw.list_run;
    b->enc.ac_runs_slot = sw.ac_runs_slot;
    b->enc.ref_pack = sw.ref_pack;

    add_script(b->enc.script, 3, true, CSH_CS_YCC);    // entries 0..9
    add_script(b->enc.script, 1, true, CSH_CS_GREY);   // entries 10..15
    add_script(b->enc.script, 3, false, CSH_CS_YCC);   // entry 16
    add_script(b->enc.script, 1, false, CSH_CS_GREY);  // entry 17
    script_base3 = progressive ? 0 : 16; script_base1 = progressive ? 10 : 17;   // (the scripts of RGB, CMYK and YCCK frames: space_script, on first use)
    // CSH_PROFILE names what stands in for libcaesium's JPEG engine.  Unset or "mozjpeg": the whole JCP_MAX_COMPRESSION profile libcaesium's
    // -q runs (compressor.rs:415,427): scan search + trellis quantisation + overshoot deringing.  "scalar": the scan search over the scalar
    // quantiser (the pieces pinned by samples/j0.JPG and libjpeg-turbo); "plain": the stock jpeg_simple_progression script over the
    // scalar quantiser (whole files equal libjpeg-turbo's); "mozjpeg-trellis" / "mozjpeg-dering": one half of the quantiser each (scan search kept)
    const bool webp = b->webp, rgb_out = b->rgb_out;
    const std::string &profile = sw.profile;
    b->enc.search = progressive && !webp && !rgb_out && profile != "plain";
    const bool lossy_jpeg = !b->lossless && !webp && !rgb_out;
    b->tr.trellis = lossy_jpeg && (profile == "mozjpeg" || profile == "mozjpeg-trellis");
    b->tr.dering = lossy_jpeg && (profile == "mozjpeg" || profile == "mozjpeg-dering");
    // (CSH_NZ_ONCE=0: the coding stages build their level-0 lists from the coefficient tiles again, as before round 5; CSH_TR_SORT=0 implies it -- the per-block list offsets come with the sort's counts)
    b->tr.nz_once = b->tr.trellis && progressive && sw.nz_once && sw.tr_sort;
}

// EncScan entries made on first use, by key: (component, Ss, Se, Ah, Al) for the search's candidates and the other one-off scans
template <class Fill>
int BatchPlanner::enc_scan(const std::array<int, 5> &key, Fill fill) {
    auto f = b->enc.cand_script.find(key);
    if (f != b->enc.cand_script.end()) return f->second;
    EncScan e;
    memset(&e, 0, sizeof e);
    fill(e);
    b->enc.script.push_back(e);
    return b->enc.cand_script[key] = int(b->enc.script.size()) - 1;
}
// the stock script of a frame in `space`: its first EncScan and the number of them
int BatchPlanner::space_script(int ncomp, int space, int &ns) {
    ns = progressive ? (space == CSH_CS_YCC ? 10 : 2 + 4 * ncomp) : 1;
    if (space == CSH_CS_YCC) return script_base3;
    if (space == CSH_CS_GREY) return script_base1;
    auto f = other_scripts.find(space);
    if (f == other_scripts.end()) {
        f = other_scripts.emplace(space, int(b->enc.script.size())).first;
        add_script(b->enc.script, ncomp, progressive, space);
    }
    return f->second;
}
// cls: the component's table number (table_class); a key of its own where it is not the YCbCr one, so that component 1 of an RGB frame and Cb do not share an entry
int BatchPlanner::cand_index(int comp, int Ss, int Se, int Ah, int Al, int cls) {
    const int ycc = comp ? 1 : 0;
    if (cls < 0) cls = ycc;
    return enc_scan({cls == ycc ? comp : comp + 16 * (1 + cls), Ss, Se, Ah, Al}, [&](EncScan &e) {
        const int id = cls;
        e.ncomp = 1; e.comp[0] = comp; e.Ss = Ss; e.Se = Se; e.Ah = Ah; e.Al = Al;
        e.ntables = 1; e.dht_id[0] = 0x10 | id; e.sos_tdta[0] = id;
    });
}
int BatchPlanner::dc_scan_index(int ncomp) {   // first DC scan of all components at Al = 0 (dc_scan_opt_mode 0)
    return enc_scan({-ncomp, 0, 0, 0, 0}, [&](EncScan &e) {
        e.ncomp = ncomp;
        for (int k = 0; k < ncomp; k++) {
            e.comp[k] = k;
            const int id = k ? 1 : 0;
            int idx = -1;
            for (int t = 0; t < e.ntables; t++) if (e.dht_id[t] == id) idx = t;
            if (idx < 0) { idx = e.ntables; e.dht_id[e.ntables++] = id; }
            e.dc_tbl[k] = idx; e.sos_tdta[k] = id << 4;
        }
    });
}
int BatchPlanner::seq1_index(int comp, int cls) {   // a one-component sequential scan (the trellis stage's statistics scan of a sequential output)
    const int ycc = comp ? 1 : 0;
    if (cls < 0) cls = ycc;
    return enc_scan({cls == ycc ? comp : comp + 16 * (1 + cls), 0, 63, -1, -1}, [&](EncScan &e) {
        const int id = cls;
        e.ncomp = 1; e.comp[0] = comp; e.Ss = 0; e.Se = 63; e.sequential = 1;
        e.ntables = 2; e.dht_id[0] = id; e.dht_id[1] = 0x10 | id; e.dc_tbl[0] = 0; e.ac_tbl[0] = 1; e.sos_tdta[0] = (id << 4) | id;
    });
}

// blocks of the encoded image, all components (what a file's bytes are shared out over)
static uint64_t blocks_of(const ImgDesc &im) {
    uint64_t n = 0;
    for (int k = 0; k < im.ncomp; k++) n += uint64_t(im.out[k].real_bw) * im.out[k].real_bh;
    return n;
}

// the NzList of (image, component, Al), made on first use (k_aclist.hip): the list itself, level 0 (what the others are filtered from), the set
uint32_t BatchPlanner::nz_list(int img_index, int comp, int Al, const ImgDesc &im, size_t in_len) {
    if (b->enc.nzset_of.size() < size_t(img_index + 1) * CSH_MAX_COMPS) b->enc.nzset_of.resize(size_t(img_index + 1) * CSH_MAX_COMPS, -1);
    int &si = b->enc.nzset_of[size_t(img_index) * CSH_MAX_COMPS + size_t(comp)];
    const uint32_t nu = uint32_t(im.out[comp].real_bw * im.out[comp].real_bh);
    if (si < 0) {
        NzSet S;
        memset(&S, 0, sizeof S);
        for (int L = 0; L < CSH_NZ_LEVELS; L++) S.list[L] = 0xFFFFFFFFu;
        S.cnt_base = 0xFFFFFFFFu;
        S.nunits = nu; S.real_bw = im.out[comp].real_bw; S.bw = im.out[comp].bw; S.tile_base = im.out[comp].tile_base;   // rebased with the plans below
        si = int(b->enc.nzsets.size());
        b->enc.nzsets.push_back(S); b->enc.nzset_built.push_back(0u); b->enc.nzset_comp.push_back(comp); b->enc.nzset_image.push_back(img_index);
    }
    const uint64_t blocks_all = blocks_of(im);
    // a non-zero coefficient costs a source file 3 bits at the very least and ~5 at ordinary qualities; one of magnitude >= 2^Al more
    static const uint32_t kShare[CSH_NZ_LEVELS] = {20, 16, 12, 9};   // eighths of the file's bytes, per level
    for (int L : {0, Al}) {
        if (b->enc.nzsets[size_t(si)].list[L] != 0xFFFFFFFFu) continue;
        const uint32_t nch = (nu + 255) / 256;
        NzList R;
        memset(&R, 0, sizeof R);
        R.chunk0 = b->enc.nz_nrec; b->enc.nz_nrec += nch;
        b->enc.nzsets[size_t(si)].list[L] = uint32_t(b->enc.nzlists.size());
        b->enc.nzlists.push_back(R);
        const uint64_t est = uint64_t(in_len) * kShare[L] / 8 * nu / std::max<uint64_t>(1, blocks_all) + nu + 4ull * nch + 256;
        const uint64_t worst = uint64_t(nu) * 64 + 4ull * nch;
        b->enc.nz_est.push_back(uint32_t(std::min<uint64_t>(est, worst)));
        b->enc.nz_worst.push_back(uint32_t(std::min<uint64_t>(worst, 0xFFFFFFF0ull)));
    }
    return b->enc.nzsets[size_t(si)].list[Al];
}

// work items, slots, token chunks and plans of one image for a list of scans (EncScan indices), in list order
void BatchPlanner::add_works(Item &it, ImgDesc &im, int img_index, const std::vector<int> &list, size_t in_len, const JpegInfo &o, bool stats_only) {
    const int w_first = int(b->enc.swork.size());
    uint32_t nz_need[CSH_MAX_COMPS] = {0, 0, 0}, nz_gate[CSH_MAX_COMPS] = {0, 0, 0};
    for (int sidx : list) {
        const EncScan &e = b->enc.script[sidx];
        ScanWork w;
        memset(&w, 0, sizeof w);
        w.image = img_index; w.scan = sidx;
        w.out_off = 0xFFFFFFFFu;   // not part of a file until k_layout says so (a conditional stage of the scan search may never run)
        // progressive AC scans are coded from the component's compacted list at their Al: first-pass scans entirely (k_list_stats, k_list_pack), refinement
        // scans by k_list_refine and k_list_refine_pack (CSH_REF_PACK=0: through tokens k_list_refine makes from it; CSH_REF_LIST=0: through k_tokens' kind-0 chunks,
        // from the tiles); everything else from tokens
        const bool from_list = e.Ss > 0 && !e.sequential && e.Ah == 0;
        const bool ref_list = sw.ref_list && e.Ss > 0 && !e.sequential && e.Ah != 0;
        w.list = 0xFFFFFFFFu; w.rs_base = 0xFFFFFFFFu; w.lr_base = 0xFFFFFFFFu; w.rr_base = 0xFFFFFFFFu;
        if (from_list || ref_list) {
            if (e.Al >= CSH_NZ_LEVELS) { it.code = CS_ERR_JPEG_FEATURE; it.msg = "internal: output scan script outside what the list coder carries"; }
            else {
                w.list = nz_list(img_index, e.comp[0], e.Al, im, in_len);
                if (!nz_need[e.comp[0]]) nz_gate[e.comp[0]] = uint32_t(b->enc.swork.size());
                nz_need[e.comp[0]] |= 1u << e.Al;
            }
        }
        if (e.Ss == 0 && e.ncomp > 1) w.nunits = uint32_t(im.omcus_x * im.omcus_y);
        else w.nunits = uint32_t(im.out[e.comp[0]].real_bw * im.out[e.comp[0]].real_bh);
        w.unit_base = uint32_t(b->enc.total_units);
        b->enc.total_units += w.nunits;
        w.corr_base = 0xFFFFFFFFu;
        if (e.Ss > 0 && !e.sequential && e.Ah) { w.corr_base = uint32_t(b->enc.total_corr); b->enc.total_corr += w.nunits; }
        w.word_base = uint32_t(b->enc.total_words);
        if (e.Ss) b->enc.total_words += (w.nunits + 63) / 64;
        w.table_base = uint32_t(b->enc.ntables);
        b->enc.ntables += e.ntables;
        b->enc.max_units = std::max(b->enc.max_units, w.nunits);
        {   // its slots, one per 256 units: counted here, written by k_make_slots (k_aclist.hip) from this record
            const uint32_t nch = (w.nunits + 255) / 256;
            w.first_chunk = b->enc.nslots; b->enc.nslots += nch;
            w.hist_row0 = b->enc.hist_rows; b->enc.hist_rows += nch * uint32_t(e.ntables);
            // a refinement scan packed from its list (CSH_REF_PACK) is in neither slot list: k_list_refine_pack takes it by its runs
            if (ref_list && sw.ref_pack && w.list != 0xFFFFFFFFu) w.ls_base = 0xFFFFFFFFu;
            else {
                uint32_t &cursor = (from_list && w.list != 0xFFFFFFFFu) ? b->enc.nlist_slots : b->enc.ntok_slots;
                w.ls_base = cursor; cursor += nch;
            }
            if (ref_list && w.list != 0xFFFFFFFFu) { w.rs_base = b->enc.nref_slots; b->enc.nref_slots += nch; }
            // ... and its runs of up to list_run chunks, one wave of the list kernels each
            const uint32_t nruns = (nch + b->enc.list_run - 1) / b->enc.list_run;
            if (from_list && w.list != 0xFFFFFFFFu) { w.lr_base = b->enc.nlist_runs; b->enc.nlist_runs += nruns; }
            if (ref_list && w.list != 0xFFFFFFFFu) { w.rr_base = b->enc.nref_runs; b->enc.nref_runs += nruns; }
        }
        if (e.Ss == 0 || e.sequential) {   // DC scans and sequential-mode scans: one token workgroup per (scan, 256 units)
            // tokens of a DC scan are known exactly (one per block, or one per fifteen blocks' bits); a sequential-mode block has at most 64 + 3
            uint32_t blocks = 0;
            for (int k = 0; k < e.ncomp; k++) blocks += e.ncomp > 1 ? uint32_t(o.comp[e.comp[k]].h * o.comp[e.comp[k]].v) : 1u;
            const uint32_t per_unit = e.sequential ? blocks * 20u : (e.Ah ? (blocks + 14u) / 15u : blocks);
            for (uint32_t j = 0; j < (w.nunits + 255) / 256; j++) b->enc.echunks.push_back(EChunk{uint32_t(b->enc.swork.size()), 0, 1, j, 0, uint32_t(b->enc.region_est.size())});
            b->enc.region_est.push_back(stats_only ? 64u : w.nunits * per_unit + 64);
        }
        b->enc.swork.push_back(w);
    }
    // the lists this call's scans need and no earlier stage makes: one builder wave per 256 blocks (the trellis stage's statistics
    // scans are coded from the scalar-quantised coefficients, the other stages from the trellis's: that stage makes its level 0 anew)
    for (int c = 0; c < im.ncomp; c++) {
        if (!nz_need[c]) continue;
        const int si = b->enc.nzset_of[size_t(img_index) * CSH_MAX_COMPS + size_t(c)];
        uint32_t levels = stats_only ? (nz_need[c] | 1u) : ((nz_need[c] | 1u) & ~b->enc.nzset_built[size_t(si)]);
        b->enc.nzset_built[size_t(si)] |= levels;
        // the trellis stage's statistics list takes the trellis's levels (k_trellis_ac): a coding stage does not build level 0 from the tiles, it drops the list's zero entries
        if (!stats_only && b->tr.nz_once && (levels & 1u)) levels = (levels & ~1u) | CSH_NZ_COMPACT0;
        const uint32_t nu = b->enc.nzsets[size_t(si)].nunits;
        for (uint32_t j = 0; levels && j < (nu + 255) / 256; j++) b->enc.nzchunks.push_back(NzChunk{uint32_t(si), j, levels, nz_gate[c]});
    }
    // the progressive AC refinement scans of a component share one region of the token pool and (CSH_REF_LIST=0) one pass of k_tokens over its blocks
    for (int c = 0; c < im.ncomp; c++) {
        int nac = 0;
        for (int sidx : list) { const EncScan &e = b->enc.script[sidx]; if (e.Ss > 0 && !e.sequential && e.Ah && e.comp[0] == c) { nac++; if (e.Al > 3 && !sw.ref_list) nac = 99; } }
        // (what a TokPlan carries limits k_tokens' kind-0 chunks only; on the list path a scan outside the list levels has failed its file above and has no slot in ref_slots)
        const bool too_many = !sw.ref_list && nac > CSH_TK_MAXSLOT;
        if (too_many) { it.code = CS_ERR_JPEG_FEATURE; it.msg = "internal: output scan script outside what the token kernel carries"; }
        const uint32_t nu = uint32_t(im.out[c].real_bw * im.out[c].real_bh);
        if (!nac || too_many) continue;
        // every non-zero coefficient becomes a token in exactly one scan of a script (~5 bits of a source file each), plus an EOB per
        // block and scan; the search's lists hold several scripts' worth
        const uint64_t blocks_all = blocks_of(im);
        const uint64_t scripts = b->enc.search ? uint64_t(nac + 1) / 2 : 1;
        const uint64_t est = uint64_t(in_len) * 3 * scripts * nu / std::max<uint64_t>(1, blocks_all) + uint64_t(nu) * nac + 1024;
        if (sw.ref_list && sw.ref_pack) continue;   // coded and packed from the lists: no plan, no token chunk, no region
        if (sw.ref_list) {   // coded from the lists: no plan, no token chunk -- the scans' slots name the component's region themselves
            for (size_t k = 0; k < list.size(); k++) {
                const EncScan &e = b->enc.script[list[k]];
                if (e.Ss > 0 && !e.sequential && e.Ah && e.comp[0] == c && b->enc.swork[size_t(w_first) + k].rs_base != 0xFFFFFFFFu) b->enc.swork[size_t(w_first) + k].region = uint32_t(b->enc.region_est.size());
            }
            b->enc.region_est.push_back(stats_only ? 64u : uint32_t(std::min<uint64_t>(est, 0x3FFFFFFFu)));
            continue;
        }
        TokPlan P;
        memset(&P, 0, sizeof P);
        P.nunits = nu; P.real_bw = im.out[c].real_bw; P.bw = im.out[c].bw; P.tile_base = im.out[c].tile_base;   // tile_base of re-quantised tiles is rebased below
        P.work0 = 0xFFFFFFFFu;
        for (size_t k = 0; k < list.size(); k++) {
            const EncScan &e = b->enc.script[list[k]];
            if (!(e.Ss > 0 && !e.sequential && e.Ah && e.comp[0] == c)) continue;
            const ScanWork &w = b->enc.swork[size_t(w_first) + k];
            if (P.work0 == 0xFFFFFFFFu) P.work0 = uint32_t(w_first) + uint32_t(k);   // the plan's scans are coded or skipped together: the first stands for all
            AcSlot &a = P.s[P.nslot++];
            a.unit_base = w.unit_base; a.word_base = w.word_base; a.first_chunk = w.first_chunk; a.table_base = w.table_base; a.nunits_work = w.nunits; a.corr_base = w.corr_base;
            a.Ss = uint8_t(e.Ss); a.Se = uint8_t(e.Se); a.Ah = uint8_t(e.Ah); a.Al = uint8_t(e.Al);
        }
        for (uint32_t j = 0; j < (nu + 255) / 256; j++) b->enc.echunks.push_back(EChunk{uint32_t(img_index), uint16_t(c), 0, j, uint32_t(b->enc.plans.size()), uint32_t(b->enc.region_est.size())});
        b->enc.region_est.push_back(stats_only ? 64u : uint32_t(std::min<uint64_t>(est, 0x3FFFFFFFu)));
        b->enc.plan_comp.push_back(c); b->enc.plan_image.push_back(img_index);
        b->enc.plans.push_back(P);
    }
}

// marker parsing is per file and touches every byte of it once (the hunt for the end of each scan): all cores
void BatchPlanner::parse() {
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (size_t n; (n = next++) < count;) {
            Item &it = b->items[n];
            it.file_size = inputs[n].length;
            int type = sniff(inputs[n].data, inputs[n].length);
            if (type == CS_TYPE_UNKN) { it.code = CS_ERR_UNKNOWN_TYPE; it.msg = "unknown file type"; }
            else if (type != CS_TYPE_JPEG) { it.code = CS_ERR_UNSUPPORTED; it.msg = "this input format has no device path in this build (built: JPEG, PNG)"; }
            else it.code = parse_jpeg(inputs[n].data, inputs[n].length, it.in, it.msg);
        }
    };
    size_t nthreads = std::min<size_t>(std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())), (count + 15) / 16);
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; t++) pool.emplace_back(worker);
    worker();
    for (auto &t : pool) t.join();
}

int BatchPlanner::reserve_pinned() {
    size_t total = 0;
    for (size_t n = 0; n < count; n++) total += inputs[n].length;
    // DecScan / ParScan address the pool with 32 bits (types.h): a group whose entropy data (plus the per-restart-interval copies)
    // could pass 4 GiB is refused as a whole -- cs_batch_extent() sizes groups well below this, so only a direct caller sees it
    if (total + total / 16 + (64u << 10) >= 0xF0000000ull) { csh_set_error("csh_batch_create: more than 3.75 GiB of input in one device batch (cs_batch_extent sizes groups)"); return CS_ERR_POOL_OVERFLOW; }
    if (!b->dec.bits_pool.reserve(total + total / 16 + (64u << 10))) { csh_set_error("out of pinned host memory"); return CS_ERR_NO_DEVICE; }
    return 0;
}

// geometry of the decoded and the encoded image, the source's quantisation tables (de-duplicated by content)
void BatchPlanner::image_geometry(Item &it, ImgDesc &im) {
    const JpegInfo &in = it.in, &o = it.out;
    im.width = in.width; im.height = in.height; im.ncomp = o.ncomp; im.ncomp_in = in.ncomp;
    im.mcus_x = in.mcus_x; im.mcus_y = in.mcus_y;
    im.progressive_in = in.progressive;
    for (int c = 0; c < in.ncomp; c++) {
        fill_geom(in.comp[c], im.in[c], b->ntiles_in);
        std::vector<uint16_t> key(in.comp[c].qt, in.comp[c].qt + 64);
        auto f = quant_index.find(key);
        if (f == quant_index.end()) {
            DevQuant q; make_quant(key.data(), q);
            f = quant_index.emplace(key, int(b->quants.size())).first;
            b->quants.push_back(q);
        }
        im.qt_in[c] = f->second;
        b->max_tiles = std::max<uint32_t>(b->max_tiles, im.in[c].ntiles);
    }
    for (int c = 0; c < o.ncomp; c++) {
        if (b->lossless) im.out[c] = im.in[c];
        else fill_geom(o.comp[c], im.out[c], b->ntiles_out);  // rebased behind all decoded tiles below
        im.comp_id[c] = o.comp[c].id;
        im.qt_out[c] = 0;
        b->max_tiles = std::max<uint32_t>(b->max_tiles, im.out[c].ntiles);
        uint32_t nd = uint32_t(im.out[c].bw * im.out[c].bh - im.out[c].real_bw * im.out[c].real_bh);
        b->max_dummy = std::max(b->max_dummy, nd);
    }
    im.omcus_x = o.mcus_x; im.omcus_y = o.mcus_y;
    im.enc_w = o.width; im.enc_h = o.height;
    for (int c = 0; c < in.ncomp; c++) im.src[c] = im.in[c];
}

// Huffman set of a scan, de-duplicated by content: the sequential decoder's form and the parallel decoder's two LDS forms
int BatchPlanner::huff_set(const JScan &js) {
    std::vector<uint8_t> key;
    for (int t = 0; t < 4; t++)
        for (const HuffSpec *h : {&js.dc[t], &js.ac[t]}) {
            key.push_back(h->present);
            if (h->present) { key.insert(key.end(), h->bits, h->bits + 17); key.insert(key.end(), h->vals, h->vals + h->nvals); }
        }
    int found = -1;
    for (auto &kv : hset_keys) if (kv.first == key) { found = kv.second; break; }
    if (found >= 0) return found;
    found = int(b->dec.hsets.size());
    DevHuffSet hs;
    for (int t = 0; t < 4; t++) { build_dev_huff(js.dc[t], hs.dc[t]); build_dev_huff(js.ac[t], hs.ac[t]); }
    b->dec.hsets.push_back(hs);
    ParHuffSet phs;
    memset(&phs, 0, sizeof phs);
    int sub_used = 0;
    bool fits = true;
    for (int t = 0; t < 4; t++) fits = fits && build_par_huff(js.dc[t], phs.root[t], phs.sub, sub_used) && build_par_huff(js.ac[t], phs.root[4 + t], phs.sub, sub_used);
    b->dec.phsets.push_back(phs);
    b->dec.phset_fits.push_back(fits ? 1 : 0);
    ParHuffSet4 ph4;
    memset(&ph4, 0, sizeof ph4);
    std::array<int8_t, 8> slots;
    slots.fill(-1);
    int nslot = 0, sub4 = 0;
    bool fits4 = true;
    for (int t = 0; t < 8 && fits4; t++) {
        const HuffSpec &h = t < 4 ? js.dc[t] : js.ac[t - 4];
        if (!h.present) continue;
        if (nslot == 4) { fits4 = false; break; }
        uint16_t tmp_sub[CSH_PAR_SUB];
        int used = 0;
        if (!build_par_huff(h, ph4.root[nslot], tmp_sub, used) || sub4 + used > CSH_PAR_SUB4) { fits4 = false; break; }
        for (int e = 0; e < 512; e++) if (ph4.root[nslot][e] & 0x8000u) ph4.root[nslot][e] = uint16_t(ph4.root[nslot][e] + sub4);   // rebase the sub-table offsets
        memcpy(ph4.sub + sub4, tmp_sub, used * sizeof(uint16_t));
        sub4 += used;
        slots[t] = int8_t(nslot++);
    }
    if (!fits4) b->dec.use4 = false;
    b->dec.phsets4.push_back(ph4);
    b->dec.slot4.push_back(slots);
    hset_keys.emplace_back(key, found);
    return found;
}

// entropy-coded scans of one file -> DecScan; returns non-zero when the batch cannot be built (it.code: this file only)
int BatchPlanner::decode_scans(Item &it, ImgDesc &im, const uint8_t *d) {
    const JpegInfo &in = it.in;
    im.first_scan = int(b->dec.dscans.size());
    im.nscans_in = int(in.scans.size());
    for (const JScan &js : in.scans) {
        DecScan ds;
        memset(&ds, 0, sizeof ds);
        ds.bits_off = uint32_t(b->dec.bits_pool.size());
        ds.bits_len = uint32_t(js.data_len);
        if (!b->dec.bits_pool.append_aligned(d + js.data_off, js.data_len)) { csh_set_error("out of pinned host memory"); return CS_ERR_NO_DEVICE; }
        ds.ncomp = js.ncomp;
        if (js.ncomp > CSH_MAX_COMPS) { it.code = CS_ERR_JPEG_FEATURE; it.msg = "scan with more than 3 components"; break; }
        for (int k = 0; k < js.ncomp; k++) { ds.comp[k] = js.comp_idx[k]; ds.td[k] = js.td[k]; ds.ta[k] = js.ta[k]; }
        ds.Ss = js.Ss; ds.Se = js.Se; ds.Ah = js.Ah; ds.Al = js.Al;
        ds.restart_interval = js.restart_interval;
        ds.par_index = -1;
        ds.huff_set = huff_set(js);
        // tables the scan needs must exist
        for (int k = 0; k < js.ncomp; k++) {
            bool need_dc = in.progressive ? (js.Ss == 0 && js.Ah == 0) : true;
            bool need_ac = in.progressive ? (js.Ss != 0) : true;
            if ((need_dc && !js.dc[js.td[k]].present) || (need_ac && !js.ac[js.ta[k]].present)) { it.code = CS_ERR_BAD_JPEG; it.msg = "scan refers to a missing Huffman table"; }
        }
        b->dec.dscans.push_back(ds);
    }
    return 0;
}

// units of a scan: MCUs, or the blocks of its one component
static uint32_t scan_units(const JpegInfo &in, const JScan &js) {
    return js.ncomp > 1 ? uint32_t(in.mcus_x * in.mcus_y) : uint32_t(in.comp[js.comp_idx[0]].real_bw * in.comp[js.comp_idx[0]].real_bh);
}

// where the blocks of `units` units of a scan lie, per block of the MCU; dc_rows: the scan's DC differences get rows of the DC pool;
// subseqs: the scan is cut into sub-sequences
void BatchPlanner::place_blocks(ParScan &ps, const JpegInfo &in, const JScan &js, uint32_t units, bool dc_rows, bool subseqs) {
    int m = 0;
    for (int k = 0; k < js.ncomp; k++) {
        const JComp &jc = in.comp[js.comp_idx[k]];
        const int nh = js.ncomp > 1 ? jc.h : 1, nv = js.ncomp > 1 ? jc.v : 1;
        const uint32_t nblocks = units * uint32_t(nh * nv);
        for (int y = 0; y < nv; y++)
            for (int x = 0; x < nh; x++, m++) {
                if (m >= 10) break;
                ps.comp_of[m] = js.comp_idx[k]; ps.by_of[m] = y; ps.bx_of[m] = x; ps.dct[m] = js.td[k]; ps.act[m] = js.ta[k];
                ps.dc_base[m] = b->dec.dc_total; ps.dc_per_mcu[m] = uint32_t(nh * nv); ps.dc_idx[m] = uint32_t(y * nh + x);
            }
        if (dc_rows) b->dec.dc_total += nblocks;
        ps.total_blocks += nblocks;
    }
    ps.nb_mcu = m;
    b->dec.max_par_blocks = std::max(b->dec.max_par_blocks, ps.total_blocks);
    if (subseqs) {
        const uint32_t nsub = (ps.bits_len + CSH_SUBSEQ_BYTES - 1) / CSH_SUBSEQ_BYTES;
        b->dec.total_sub += nsub;
        b->dec.max_sub = std::max(b->dec.max_sub, nsub);
    }
}

// sequential-mode scans go to the parallel self-synchronising decoder: a scan without restart markers as one
// ParScan, a scan with them as one ParScan per restart interval (each interval is an independent stream whose DC
// prediction starts at zero -- exactly what a ParScan is); the intervals are copied into the pool once more, each
// 64-byte aligned, because the unstuffing pass works on aligned segments
// par_ok: false when the file goes to another decoder.  Returns non-zero when the batch cannot be built.
int BatchPlanner::sequential_split(const Item &it, const ImgDesc &im, const uint8_t *d, int img_index, bool &par_ok) {
    const JpegInfo &in = it.in;
    par_ok = !in.progressive;
    for (size_t s = 0; s < in.scans.size(); s++) if (!b->dec.phset_fits[b->dec.dscans[im.first_scan + s].huff_set]) par_ok = false;
    for (const JScan &js : in.scans) if (js.data_len >= (1u << 28)) par_ok = false;
    if (uint64_t(in.mcus_x) * uint64_t(in.mcus_y) * 10 >= (1u << 24)) par_ok = false;   // k_decode_par.hip uses 24-bit multiplies on block counts
    {   // a component coded by two scans (malformed, but libjpeg decodes it: the later scan wins) must not be written by two
        // segments at once: leave the order to the sequential kernel
        int seen[4] = {0, 0, 0, 0};
        for (const JScan &js : in.scans) for (int k = 0; k < js.ncomp; k++) if (seen[js.comp_idx[k] & 3]++) par_ok = false;
    }
    struct Piece { size_t off, len; uint32_t first_mcu, nmcus; };   // a scan, or one restart interval of it
    std::vector<std::vector<Piece>> pieces(in.scans.size());
    for (size_t s = 0; s < in.scans.size() && par_ok; s++) {
        const JScan &js = in.scans[s];
        const uint32_t units = scan_units(in, js);
        if (js.restart_interval == 0) {
            if (js.has_marker) par_ok = false;   // marker bytes inside the data: leave it to the sequential kernel's libjpeg-like handling
            else pieces[s].push_back({js.data_off, js.data_len, 0u, units});
            continue;
        }
        // restart intervals: RSTm markers must come in order, one after every `restart_interval` MCUs, none missing
        const uint32_t ri = uint32_t(js.restart_interval), want = (units + ri - 1) / ri;
        size_t pos = js.data_off, end = js.data_off + js.data_len, start = pos;
        uint32_t idx = 0;
        bool ok = true;
        while (pos + 1 < end) {
            const void *f = memchr(d + pos, 0xFF, end - 1 - pos);
            if (!f) break;
            pos = size_t(static_cast<const uint8_t *>(f) - d);
            if (d[pos + 1] != 0x00) {
                if (d[pos + 1] != 0xD0 + (idx & 7)) { ok = false; break; }
                pieces[s].push_back({start, pos - start, idx * ri, std::min(ri, units - idx * ri)});
                idx++;
                if (idx >= want) { ok = false; break; }
                pos += 2; start = pos;
            } else pos++;
        }
        if (ok && end > start && d[end - 1] == 0xFF) ok = false;
        if (ok) pieces[s].push_back({start, end - start, idx * ri, std::min(ri, units - idx * ri)});
        if (!ok || pieces[s].size() != want) par_ok = false;
    }
    // the unstuffing pass finds a byte's ParScan by bisection: the list stays sorted by bits_off.  A file with a restart interval in any scan
    // therefore gets every piece copied behind what the pool holds, a scan without restarts among them
    bool any_restart = false;
    for (const JScan &js : in.scans) any_restart = any_restart || js.restart_interval != 0;
    for (size_t s = 0; s < in.scans.size() && par_ok; s++) {   // one ParScan per piece
        const JScan &js = in.scans[s];
        const DecScan &ds = b->dec.dscans[im.first_scan + s];
        for (const Piece &pc : pieces[s]) {
            ParScan ps;
            memset(&ps, 0, sizeof ps);
            if (!any_restart) { ps.bits_off = ds.bits_off; ps.bits_len = ds.bits_len; }
            else {
                ps.bits_off = uint32_t(b->dec.bits_pool.size()); ps.bits_len = uint32_t(pc.len);
                if (!b->dec.bits_pool.append_aligned(d + pc.off, pc.len)) { csh_set_error("out of pinned host memory"); return CS_ERR_NO_DEVICE; }
            }
            ps.huff_set = ds.huff_set; ps.image = img_index; ps.ncomp = js.ncomp; ps.first_mcu = pc.first_mcu;
            ps.sub_base = b->dec.total_sub; ps.par_index = uint32_t(b->dec.pscans.size());
            place_blocks(ps, in, js, pc.nmcus, true, true);
            b->dec.pscans.push_back(ps);
        }
    }
    return 0;
}

// The parallel kinds run side by side and in front of the refinement chains: sound only for a REGULAR progression -- every coefficient of every
// component gets its first scan (Ah = 0) once and before any refinement, and each refinement takes over where the scan before it left the
// coefficient (Ah = that scan's Al, Al = Ah - 1).  A damaged header can say otherwise (two first scans over one band: the later one wins in file
// order, and two waves writing the same coefficient do not know which of them is later); libjpeg warns and decodes in file order: so do the chains.
static bool regular_progression(const JpegInfo &in) {
    bool regular = true;
    int state[CSH_MAX_COMPS][64];
    for (auto &row : state) for (int &v : row) v = -1;
    for (const JScan &js : in.scans)
        for (int k = 0; k < js.ncomp && regular; k++) {
            const int c = js.comp_idx[k];
            if (c < 0 || c >= CSH_MAX_COMPS || js.Ss < 0 || js.Se > 63 || js.Ss > js.Se) { regular = false; break; }
            for (int z = js.Ss; z <= js.Se; z++) {
                if (js.Ah == 0 ? state[c][z] != -1 : (state[c][z] != js.Ah || js.Al != js.Ah - 1)) { regular = false; break; }
                state[c][z] = js.Al;
            }
        }
    return regular;
}

// progressive scans without restart markers: one wave per chain (k_decode_prog.hip); the scans are listed as ParScans
// of kind 1 so that the unstuffing pre-pass covers them
bool BatchPlanner::progressive_plan(const Item &it, const ImgDesc &im, int img_index) {
    const JpegInfo &in = it.in;
    bool prog_ok = in.progressive;
    for (size_t s = 0; s < in.scans.size(); s++) {
        const JScan &js = in.scans[s];
        if (js.restart_interval != 0 || js.has_marker || js.data_len >= (1u << 28) || !b->dec.phset_fits[b->dec.dscans[im.first_scan + s].huff_set]) prog_ok = false;
    }
    if (!prog_ok) return false;
    // The scans of a progressive file, by what they are to the decoder (k_decode_par.hip, k_decode_prog.hip):
    //   DC first / AC first scans  self-synchronising like sequential scans -- cut into sub-sequences, speculated, relaxed, written
    //                              (CSH_PS_DC_FIRST / CSH_PS_AC_FIRST).  They carry most of a file's bits;
    //   DC refinement              one bit per block: unstuffed, then scattered (CSH_PS_DC_REFINE);
    //   AC refinement              a chain per component, one wave each (the bits between two symbols depend on the block's history:
    //                              a decoder that does not know its block cannot find the next symbol) -- CSH_PS_UNSTUFF + ProgChain.
    // CSH_PROG_PAR=0 (or a file beyond the parallel decoder's 24-bit block counts) leaves every scan to the chains, as before round 4.
    const bool par_first = regular_progression(in) && sw.prog_par != 0 && uint64_t(in.mcus_x) * uint64_t(in.mcus_y) * 10 < (1u << 24);
    for (size_t s = 0; s < in.scans.size(); s++) {
        const JScan &js = in.scans[s];
        DecScan &ds = b->dec.dscans[im.first_scan + s];
        ParScan ps;
        memset(&ps, 0, sizeof ps);
        ps.bits_off = ds.bits_off; ps.bits_len = ds.bits_len; ps.huff_set = ds.huff_set; ps.image = img_index; ps.ncomp = ds.ncomp; ps.nb_mcu = 1;
        ps.Ss = js.Ss; ps.Se = js.Se; ps.Al = js.Al;
        ps.kind = !par_first ? CSH_PS_UNSTUFF : js.Ss == 0 ? (js.Ah == 0 ? CSH_PS_DC_FIRST : CSH_PS_DC_REFINE) : (js.Ah == 0 ? CSH_PS_AC_FIRST : CSH_PS_UNSTUFF);
        ps.sub_base = b->dec.total_sub; ps.par_index = uint32_t(b->dec.pscans.size());
        // where the blocks of the scan lie (as for a sequential-mode scan)
        if (ps.kind != CSH_PS_UNSTUFF) place_blocks(ps, in, js, scan_units(in, js), ps.kind == CSH_PS_DC_FIRST, ps.kind != CSH_PS_DC_REFINE);
        ds.par_index = int(b->dec.pscans.size());
        b->dec.pscans.push_back(ps);
    }
    // CSH_PROG_PAR=1: the first scans in parallel, refinement chains in one wave each (k_decode_prog.hip) as before k_decode_refine.hip
    const bool refine_split = par_first && sw.prog_par != 1;
    for (int chain = 0; chain <= in.ncomp; chain++) {   // 0: DC scans; c + 1: AC scans of component c -- those the parallel decoder does not take
        ProgChain pc;
        memset(&pc, 0, sizeof pc);
        pc.image = img_index; pc.first = int(b->dec.chain_scans.size());
        bool all_refine = chain != 0;
        for (size_t s = 0; s < in.scans.size(); s++) {
            const JScan &js = in.scans[s];
            const bool mine = chain == 0 ? js.Ss == 0 : (js.Ss != 0 && js.comp_idx[0] == chain - 1);
            if (mine && b->dec.pscans[size_t(b->dec.dscans[im.first_scan + s].par_index)].kind == CSH_PS_UNSTUFF) {
                b->dec.chain_scans.push_back(im.first_scan + int(s)); pc.count++;
                if (js.Ah == 0 || js.data_len >= (1u << 27)) all_refine = false;
            }
        }
        if (pc.count && refine_split && all_refine) {   // parse + apply: room for a mask per block and a position per block and scan
            const JComp &jc = in.comp[chain - 1];
            const uint64_t nblocks = uint64_t(jc.real_bw) * uint64_t(jc.real_bh);
            if (nblocks && uint64_t(b->dec.refine_pos) + nblocks * uint64_t(pc.count) < (1ull << 32)) {
                pc.refine = 1; pc.comp = chain - 1; pc.nblocks = uint32_t(nblocks);
                pc.hist_off = b->dec.refine_hist; pc.pos_off = b->dec.refine_pos;
                b->dec.refine_hist += pc.nblocks; b->dec.refine_pos += pc.nblocks * uint32_t(pc.count);
                b->dec.refine_max_blocks = std::max(b->dec.refine_max_blocks, pc.nblocks);
            }
        }
        if (pc.count) b->dec.chains.push_back(pc);
    }
    return true;
}

// pixel work + planes
void BatchPlanner::plane_work(ImgDesc &im, const JpegInfo &in, const JpegInfo &o, int img_index, bool resized) {
    for (int c = 0; c < in.ncomp; c++) {
        PlaneWork w; w.image = img_index; w.comp = c; w.nzset = 0xFFFFFFFFu; w.ac_lists = 0u;   // (finish_descriptors names the set: the lists are planned behind the pixel work)
        if (c >= o.ncomp) {   // K of a CMYK / YCCK source that is converted: its plane feeds k_planes_to_rgb_space, the output frame has three components
            w.up = up_desc(1, 1, 0); w.dn = CSH_DN_FULL; w.mode = CSH_MODE_DECODE;
            im.plane_off[c] = plane_off;
            plane_off += uint64_t(im.in[c].real_bw * 8) * uint64_t(im.in[c].real_bh * 8);
            plane_off = (plane_off + 63u) & ~uint64_t(63);
            b->pix.pwork.push_back(w);
            continue;
        }
        w.up = resized ? up_desc(1, 1, 0) : up_desc(in.hmax / in.comp[c].h, in.vmax / in.comp[c].v, in.comp[c].comp_w);
        w.dn = dn_kind(o.hmax / o.comp[c].h, o.vmax / o.comp[c].v);
        // the layouts k_resample_plane takes keep its mode numbers (in: 0 full, 1 h2v2, 2 h2v1 by the up factors); every other one is CSH_MODE_ANY
        const int in_kind = (w.up.hx == 1 && w.up.vx == 1) ? 0 : (w.up.hx == 2 && w.up.vx == 2) ? 1 : (w.up.hx == 2 && w.up.vx == 1) ? 2 : -1;
        if (in_kind < 0 || w.dn == CSH_DN_H4V1) w.mode = CSH_MODE_ANY;
        else if (resized) w.mode = 1 + w.dn;   // encoder side is fed full-resolution planes of the resized image (k_resize.hip)
        else w.mode = (in_kind == 0 && w.dn == CSH_DN_FULL) ? 0 : 1 + 3 * in_kind + w.dn;
        if (w.mode == CSH_MODE_ANY) b->pix.any_layout = true;
        // the camera case (4:2:0 kept, no resize) goes through k_resample_fdct_420 and has no encoder-side plane
        const bool fused = w.mode == 5 && !resized && im.in[c].comp_w > 2 && im.in[c].real_bw == im.out[c].real_bw && im.in[c].real_bh == im.out[c].real_bh &&
                           im.in[c].comp_w == im.out[c].comp_w && im.in[c].comp_h == im.out[c].comp_h && sw.fused_420;
        if (fused) w.mode = 10;
        if (w.mode) {
            im.plane_off[c] = plane_off;
            plane_off += uint64_t(im.in[c].real_bw * 8) * uint64_t(im.in[c].real_bh * 8);
            plane_off = (plane_off + 63u) & ~uint64_t(63);
            im.splane_off[c] = im.plane_off[c];
            if (resized) {   // full-resolution plane of the resized image, pitch = luma's padded width
                JComp full; full.h = full.v = 1;
                JpegInfo tmpj; tmpj.width = o.width; tmpj.height = o.height; tmpj.ncomp = 1; tmpj.comp[0] = full; jpeg_geometry(tmpj);
                uint32_t dummy = 0; fill_geom(tmpj.comp[0], im.src[c], dummy);
                im.splane_off[c] = plane_off;
                plane_off += uint64_t(im.src[c].real_bw * 8) * uint64_t(im.src[c].real_bh * 8);
                plane_off = (plane_off + 63u) & ~uint64_t(63);
            }
            im.oplane_off[c] = oplane_off;
            const uint64_t osz = fused ? 0 : uint64_t(im.out[c].real_bw) * 8 * uint64_t(im.out[c].real_bh) * 8;   // <= 2^28 + edge blocks (plan_item)
            oplane_off = (oplane_off + osz + 63u) & ~uint64_t(63);
            b->pix.max_quads = std::max(b->pix.max_quads, uint32_t(osz / 4));
        }
        b->pix.pwork.push_back(w);
    }
}

void BatchPlanner::resize_work(const JpegInfo &in, const JpegInfo &o, int img_index) {
    ResizeWork rw;
    memset(&rw, 0, sizeof rw);
    rw.image = img_index; rw.nw = o.width; rw.nh = o.height;
    rw.in_kind = in.ncomp == 1 ? 0 : ((in.comp[1].h == in.hmax && in.comp[1].v == in.vmax) ? 0 : (in.comp[1].v == in.vmax ? 2 : 1));
    for (int c = 0; c < in.ncomp; c++) rw.up[c] = up_desc(in.hmax / in.comp[c].h, in.vmax / in.comp[c].v, in.comp[c].comp_w);
    const int nc = o.ncomp;   // samples per pixel of the image's RGB
    if (in.space != CSH_CS_GREY && in.space != CSH_CS_YCC) {   // planes in another colour space: k_planes_to_rgb_space
        rw.in_kind = CSH_RZ_SPACE; rw.space = in.space;
        b->pix.any_space_rgb = true;
    } else if (in.ncomp == 3) {   // k_planes_to_rgb takes full luma and Cb, Cr both 1x1 (full), 2x2 or 2x1 below it
        auto same = [&](int c, int hx, int vx) { return rw.up[c].hx == hx && rw.up[c].vx == vx; };
        const bool legacy = same(0, 1, 1) && rw.up[1].hx == rw.up[2].hx && rw.up[1].vx == rw.up[2].vx &&
                            (same(1, 1, 1) || same(1, 2, 2) || same(1, 2, 1));
        if (!legacy) { rw.in_kind = CSH_RZ_ANY; b->pix.any_layout_rgb = true; }
    }
    if (px) rw.in_kind = -1;   // the RGB of this image is not made from decoded planes: it is copied in below (csh_batch_create_from_pixels)
    const uint64_t src_bytes = uint64_t(in.width) * in.height * nc, dst_bytes = uint64_t(o.width) * o.height * nc;
    rw.rgb_src_off = b->pix.rgb_bytes; b->pix.rgb_bytes += (src_bytes + 63) & ~uint64_t(63);
    rw.rgb_dst_off = b->pix.rgb_bytes; b->pix.rgb_bytes += (dst_bytes + 63) & ~uint64_t(63);
    const uint64_t tmpn = uint64_t(o.height) * in.width * nc;
    rw.tmp_off = b->pix.tmp_floats; b->pix.tmp_floats += tmpn;
    const bool same = o.width == in.width && o.height == in.height;   // image-rs copies instead of resampling
    rw.vtap_base = uint32_t(b->pix.rtaps.size()); csh_lanczos_axis(in.height, o.height, same, b->pix.rtaps, b->pix.rweights);
    rw.htap_base = uint32_t(b->pix.rtaps.size()); csh_lanczos_axis(in.width, o.width, same, b->pix.rtaps, b->pix.rweights);
    b->pix.max_src_px = std::max<uint32_t>(b->pix.max_src_px, uint32_t(in.width) * in.height);
    b->pix.max_tmp = std::max(b->pix.max_tmp, tmpn);
    b->pix.max_row_in = std::max(b->pix.max_row_in, uint32_t(in.width) * uint32_t(nc)); b->pix.max_out_w = std::max(b->pix.max_out_w, uint32_t(o.width));
    b->pix.max_nh = std::max(b->pix.max_nh, uint32_t(o.height));
    b->pix.max_dst = std::max(b->pix.max_dst, dst_bytes);
    b->pix.rwork.push_back(rw);
    if (b->webp) {
        csw::WebpImg wi;
        memset(&wi, 0, sizeof wi);
        wi.width = uint32_t(o.width); wi.height = uint32_t(o.height); wi.mbw = (wi.width + 15) / 16; wi.mbh = (wi.height + 15) / 16; wi.ncomp = uint32_t(nc);
        wi.rgb_off = rw.rgb_dst_off; wi.image = uint32_t(img_index);
        const uint64_t ly = uint64_t(wi.mbw) * wi.mbh * 256, lc = uint64_t(wi.mbw) * wi.mbh * 64;
        auto take = [&](uint64_t n) { uint64_t at = b->wp.wwork_bytes; b->wp.wwork_bytes += (n + 63) & ~uint64_t(63); return at; };
        wi.y_off = take(ly); wi.u_off = take(lc); wi.v_off = take(lc); wi.ry_off = take(ly); wi.ru_off = take(lc); wi.rv_off = take(lc);
        wi.lev_off = b->wp.wlevels; b->wp.wlevels += uint64_t(wi.mbw) * wi.mbh * csw::WEBP_MB_REC;
        b->wp.wmax_luma = std::max<uint32_t>(b->wp.wmax_luma, uint32_t(ly));
        b->wp.wmax_mbh = std::max(b->wp.wmax_mbh, wi.mbh);
        b->wp.wimgs.push_back(wi);
    }
}

// output scans: the plain script, or stage 1 of the search
void BatchPlanner::output_scans(Item &it, ImgDesc &im, int img_index, size_t in_len) {
    const JpegInfo &o = it.out;
    im.first_work = int(b->enc.swork.size());
    const bool fixed = o.space != CSH_CS_GREY && o.space != CSH_CS_YCC;   // RGB, CMYK, YCCK: the stock script, whatever the profile
    if (!b->enc.search || fixed) {
        int ns = 0;
        const int sb = space_script(o.ncomp, o.space, ns);
        std::vector<int> list;
        for (int s = 0; s < ns; s++) list.push_back(sb + s);
        add_works(it, im, img_index, list, in_len, o);
        for (int s = 0; s < ns; s++) b->enc.img_list.push_back(uint32_t(im.first_work + s));
        b->enc.img_list.resize(size_t(img_index + 1) * CSH_LIST_MAX, 0u);
        b->enc.img_nlist.push_back(uint32_t(ns));
        if (b->enc.search) {   // among searched images: nothing to decide, no later stage
            SearchImg si;
            for (int &cw : si.cand_work) cw = -1;
            si.ncand = 0; si.fixed = true;
            b->enc.simg.push_back(si);
        }
    } else {
        // stage 1 of the search: the DC scan and every candidate whose Al is fixed (oracle/jpeg_oracle.c cso_search_progression)
        SearchImg si;
        for (int &cw : si.cand_work) cw = -1;
        std::vector<int> list, cands;
        auto add = [&](int cand, int idx) { cands.push_back(cand); list.push_back(idx); };
        add(0, dc_scan_index(o.ncomp));
        add(1, cand_index(0, 1, 8, 0, 0)); add(2, cand_index(0, 9, 63, 0, 0));
        // luma at Al 1 and 2 (mozjpeg tries Al 3 only when Al 2 beat Al 1: candidates 9-11 are stage ST_1B)
        for (int Al = 0; Al < 2; Al++) { add(3 + 3 * Al, cand_index(0, 1, 63, Al + 1, Al)); add(4 + 3 * Al, cand_index(0, 1, 8, 0, Al + 1)); add(5 + 3 * Al, cand_index(0, 9, 63, 0, Al + 1)); }
        if (o.ncomp == 3) {
            add(26, cand_index(1, 1, 8, 0, 0)); add(27, cand_index(1, 9, 63, 0, 0)); add(28, cand_index(2, 1, 8, 0, 0)); add(29, cand_index(2, 9, 63, 0, 0));
            for (int Al = 0; Al < 2; Al++) {
                add(30 + 6 * Al, cand_index(1, 1, 63, Al + 1, Al)); add(31 + 6 * Al, cand_index(2, 1, 63, Al + 1, Al));
                add(32 + 6 * Al, cand_index(1, 1, 8, 0, Al + 1)); add(33 + 6 * Al, cand_index(1, 9, 63, 0, Al + 1));
                add(34 + 6 * Al, cand_index(2, 1, 8, 0, Al + 1)); add(35 + 6 * Al, cand_index(2, 9, 63, 0, Al + 1));
            }
        }
        add_works(it, im, img_index, list, in_len, o);
        for (size_t k = 0; k < cands.size(); k++) si.cand_work[cands[k]] = im.first_work + int(k);
        si.ncand = o.ncomp == 3 ? 64 : 23;
        b->enc.simg.push_back(si);
        b->enc.img_list.resize(size_t(img_index + 1) * CSH_LIST_MAX, 0u);
        b->enc.img_nlist.push_back(0u);
    }
    if (b->enc.total_units > 0xFFFFFFF0ull) { it.code = CS_ERR_POOL_OVERFLOW; it.msg = "batch too large"; }
}

// frame header (host-built): SOI, JFIF, [metadata], DQT, SOF
void BatchPlanner::frame_header(Item &it) {
    const JpegInfo &in = it.in, &o = it.out;
    JpegInfo hdr = o;
    if (b->lossless) memcpy(hdr.qt, in.qt, sizeof hdr.qt);           // coefficient transcode keeps the source tables
    else { memcpy(hdr.qt[0], qout_nat, 128); memcpy(hdr.qt[1], qout_nat, 128); }
    // metadata carry-over (host logic): APPn/COM when keep_metadata (compressor.rs:431); ICC profile segments follow
    // jpeg_preserve_icc = !--strip-icc (compressor.rs:425) independently of it
    std::vector<uint8_t> meta;
    for (size_t mo = 0; mo + 4 <= in.meta.size();) {
        size_t L = (size_t(in.meta[mo + 2]) << 8) | in.meta[mo + 3];
        bool is_icc = in.meta[mo + 1] == 0xE2 && L >= 14 && !memcmp(&in.meta[mo + 4], "ICC_PROFILE\0", 12);
        const bool is_adobe = in.meta[mo + 1] == 0xEE && L >= 14 && !memcmp(&in.meta[mo + 4], "Adobe", 5);
        // an RGB / CMYK / YCCK source: a frame in the source's space writes the segment itself (build_frame_header), a converted one is YCbCr and must not carry it
        if (is_adobe && in.space != CSH_CS_GREY && in.space != CSH_CS_YCC) { mo += 2 + L; continue; }
        if (is_icc ? p->jpeg_preserve_icc : p->keep_metadata) meta.insert(meta.end(), in.meta.begin() + mo, in.meta.begin() + mo + 2 + L);
        mo += 2 + L;
    }
    it.meta_out = meta;
    std::vector<uint8_t> fh = build_frame_header(hdr, progressive, meta.empty() ? nullptr : &meta);
    b->enc.hdr_off.push_back(uint32_t(b->enc.hdr_pool.size()));
    b->enc.hdr_pool.insert(b->enc.hdr_pool.end(), fh.begin(), fh.end());
}

// everything of one file, step by step; returns non-zero when the batch cannot be built (a file that cannot be: it.code)
int BatchPlanner::plan_image(size_t n) {
    Item &it = b->items[n];
    const uint8_t *d = inputs[n].data;
    if (it.code) return 0;
    const bool to_rgb = ((p->width || p->height) && !b->lossless) || b->webp || b->rgb_out || px;
    it.code = plan_item(it, *p, b->lossless, to_rgb);
    if (it.code) return 0;

    ImgDesc im;
    memset(&im, 0, sizeof im);
    const JpegInfo &in = it.in, &o = it.out;
    const int img_index = int(b->imgs.size());
    image_geometry(it, im);
    const bool resized = to_rgb;   // the WebP encoder takes the RGB the resize branch produces (a plain copy at equal size)
    if (int rc = decode_scans(it, im, d)) return rc;
    if (it.code) { b->dec.dscans.resize(im.first_scan); return 0; }
    bool par_ok = false;
    if (int rc = sequential_split(it, im, d, img_index, par_ok)) return rc;
    const bool prog_ok = progressive_plan(it, im, img_index);
    b->dec.need_seq_init.push_back(par_ok ? 0u : (prog_ok ? 4u : 1u));

    if (!b->lossless) plane_work(im, in, o, img_index, resized);
    if (resized) resize_work(in, o, img_index);
    output_scans(it, im, img_index, inputs[n].length);
    frame_header(it);

    it.image = img_index;
    b->imgs.push_back(im);
    b->out.raw_bytes_cap += (b->enc.search ? 8 : 2) * inputs[n].length + (b->enc.search ? 256 : 64) * 1024;   // the search's candidates are ten scripts' worth of scans (of the OUTPUT's size)
    return 0;
}

// the later stages of the search, each contiguous: make(image, add) lists the stage's candidates of one image
template <class Make>
void BatchPlanner::add_stage(int sid, Make make) {
    // one unused slot between the stages: each stage's exclusive scan of chunk sizes writes one entry past its slots
    b->enc.nslots++;
    Stage &sg = b->enc.stage[sid];
    b->enc.stage_begin(sg);
    for (size_t n = 0; n < count; n++) {
        Item &it = b->items[n];
        if (it.image < 0) continue;
        ImgDesc &im = b->imgs[size_t(it.image)];
        SearchImg &si = b->enc.simg[size_t(it.image)];
        if (si.fixed) continue;
        std::vector<int> list, cands;
        auto add = [&](int cand, int idx) { cands.push_back(cand); list.push_back(idx); };
        make(im, add);
        const int first = int(b->enc.swork.size());
        add_works(it, im, it.image, list, inputs[n].length, it.out);
        for (size_t k = 0; k < cands.size(); k++) si.cand_work[cands[k]] = first + int(k);
    }
    b->enc.stage_end(sg);
}
static const int kSplit[5] = {2, 8, 5, 12, 18};
// ST_2: the frequency-split candidates every search looks at: the whole band, the splits at 2 and at 5 (the split at 8 IS stage 1's
// pair of band scans at the chosen Al: nothing is coded for it).  Their Al is the one stage 1 chooses: entered as 0, patched before the stage runs
template <class Add>
void BatchPlanner::splits(const ImgDesc &im, Add &add, int i0, int i1, bool whole) {
    if (whole) add(12, cand_index(0, 1, 63, 0, 0));
    for (int i = i0; i <= i1; i++) if (i != 1) { add(13 + 2 * i, cand_index(0, 1, kSplit[i], 0, 0)); add(14 + 2 * i, cand_index(0, kSplit[i] + 1, 63, 0, 0)); }
    if (im.ncomp == 3) {
        if (whole) { add(42, cand_index(1, 1, 63, 0, 0)); add(43, cand_index(2, 1, 63, 0, 0)); }
        for (int i = i0; i <= i1; i++) if (i != 1) {
            add(44 + 4 * i, cand_index(1, 1, kSplit[i], 0, 0)); add(45 + 4 * i, cand_index(1, kSplit[i] + 1, 63, 0, 0));
            add(46 + 4 * i, cand_index(2, 1, kSplit[i], 0, 0)); add(47 + 4 * i, cand_index(2, kSplit[i] + 1, 63, 0, 0));
        }
    }
}
int BatchPlanner::plan_search_stages() {
    b->enc.hdr_off.push_back(uint32_t(b->enc.hdr_pool.size()));
    b->nimg = int(b->imgs.size());
    // stage boundary: everything made so far is stage 1 (without the search: all there is)
    b->enc.stage_end(b->enc.stage[0]);
    if (!b->enc.search) return 0;
    // ST_1B: luma at Al 3 -- the refinement that brings it back to 2 and the two band scans
    add_stage(EncodePlan::ST_1B, [&](const ImgDesc &, auto &add) { add(9, cand_index(0, 1, 63, 3, 2)); add(10, cand_index(0, 1, 8, 0, 3)); add(11, cand_index(0, 9, 63, 0, 3)); });
    add_stage(EncodePlan::ST_2, [&](const ImgDesc &im, auto &add) { splits(im, add, 0, 2, true); });
    add_stage(EncodePlan::ST_2B, [&](const ImgDesc &im, auto &add) { splits(im, add, 3, 3, false); });   // the split at 12: only if the split at 8 leads after the third
    add_stage(EncodePlan::ST_2C, [&](const ImgDesc &im, auto &add) { splits(im, add, 4, 4, false); });   // the split at 18: only if the split at 12 leads after the fourth
    for (int c = 0; c < 3; c++) for (int i = -1; i < 5; i++) for (int Al = 1; Al <= (c ? 2 : 3); Al++) {   // the variants the Al patch may pick
        if (i < 0) cand_index(c, 1, 63, 0, Al); else { cand_index(c, 1, kSplit[i], 0, Al); cand_index(c, kSplit[i] + 1, 63, 0, Al); }
    }
    b->enc.work_active.assign(b->enc.swork.size(), 0);
    if (b->enc.total_units > 0xFFFFFFF0ull) { csh_set_error("csh_batch_create: batch too large for the scan search's candidate lists (fewer files per batch)"); return CS_ERR_POOL_OVERFLOW; }
    return 0;
}

int BatchPlanner::plan_trellis() {
    if (!b->tr.trellis) return 0;
    // the trellis stage: per component one statistics scan in the output mode's entropy coder -- progressive: the component alone,
    // 1-63 at Al 0 (EOBRUN symbols included); sequential: a one-component sequential scan (DC and AC tables) -- coded for its
    // histograms only (mozjpeg jcmaster.c: the huff_opt pass in front of every trellis pass; oracle: cso_trellis_tables)
    b->enc.nslots++;
    Stage &tg = b->tr.tstage;
    b->enc.stage_begin(tg);
    for (size_t n = 0; n < count; n++) {
        Item &it = b->items[n];
        if (it.image < 0) continue;
        ImgDesc &im = b->imgs[size_t(it.image)];
        std::vector<int> list;
        const int space = it.out.space;
        for (int c = 0; c < im.ncomp; c++) list.push_back(progressive ? cand_index(c, 1, 63, 0, 0, table_class(space, c)) : seq1_index(c, table_class(space, c)));
        const size_t first = b->enc.swork.size();
        add_works(it, im, it.image, list, inputs[n].length, it.out, true);
        for (int c = 0; c < im.ncomp; c++) {
            const ScanWork &w = b->enc.swork[first + size_t(c)];
            TrellisWork tw;
            memset(&tw, 0, sizeof tw);
            tw.image = it.image; tw.comp = c; tw.dc_cls = uint32_t(table_class(space, c));
            tw.table_ac = w.table_base + (progressive ? 0u : 1u);
            tw.table_dc = progressive ? -1 : int32_t(w.table_base);
            tw.nunits = w.nunits; tw.unit_base = b->tr.t_units;
            b->tr.t_units += w.nunits;
            b->tr.t_max_rows = std::max<uint32_t>(b->tr.t_max_rows, uint32_t((im.out[c].real_bh + im.out[c].v - 1) / im.out[c].v));
            tw.nzset = 0xFFFFFFFFu;
            if (progressive) {
                const int si = b->enc.nzset_of[size_t(it.image) * CSH_MAX_COMPS + size_t(c)];
                b->enc.nzsets[size_t(si)].cnt_base = tw.unit_base;   // the statistics list's builder counts every block's entries
                if (b->tr.nz_once) tw.nzset = uint32_t(si);
            }
            b->tr.twork.push_back(tw);
        }
    }
    b->enc.stage_end(tg);
    {   // the AC kernel's runs, j-major: the chunks at the front of a work item hold its longest lists (k_trellis_sort), so the queue
        // hands out the heavy chunks of every component first and ends on light ones
        std::vector<uint32_t> nch(b->tr.twork.size());
        uint32_t most = 0;
        for (size_t wi = 0; wi < b->tr.twork.size(); wi++) { nch[wi] = (b->tr.twork[wi].nunits + CSH_TR_WG - 1) / CSH_TR_WG; most = std::max(most, nch[wi]); }
        for (uint32_t j = 0; j < most; j += CSH_TR_RUN)
            for (size_t wi = 0; wi < b->tr.twork.size(); wi++)
                if (j < nch[wi]) b->tr.truns.push_back(TrellisRun{uint32_t(wi), j, std::min<uint32_t>(CSH_TR_RUN, nch[wi] - j)});
    }
    {   // the DC walks, longest first (a wave's 64 lanes then walk rows of a length)
        b->tr.t_sort = progressive && sw.tr_sort;
        std::vector<std::pair<uint32_t, uint32_t>> rows;
        for (size_t wi = 0; wi < b->tr.twork.size(); wi++) {
            const CompGeom &g = b->imgs[size_t(b->tr.twork[wi].image)].out[b->tr.twork[wi].comp];
            for (int r = 0; r < (g.real_bh + g.v - 1) / g.v; r++) rows.push_back({uint32_t(g.real_bw * g.v), uint32_t(wi << 16) | uint32_t(r)});
        }
        std::stable_sort(rows.begin(), rows.end(), [](const auto &a, const auto &b2) { return a.first > b2.first; });
        for (const auto &r : rows) b->tr.trows.push_back(r.second);
    }
    if (b->enc.total_units > 0xFFFFFFF0ull) { csh_set_error("csh_batch_create: batch too large (fewer files per batch)"); return CS_ERR_POOL_OVERFLOW; }
    return 0;
}

void BatchPlanner::finish_descriptors() {
    // pool layout: [all decoded tiles][all re-quantised tiles]; only the first part must start at zero for the decoder
    if (!b->lossless)
        for (ImgDesc &im : b->imgs) for (int c = 0; c < im.ncomp; c++) im.out[c].tile_base += b->ntiles_in;
    for (size_t i = 0; i < b->enc.plans.size(); i++) b->enc.plans[i].tile_base = b->imgs[size_t(b->enc.plan_image[i])].out[b->enc.plan_comp[i]].tile_base;
    for (size_t i = 0; i < b->enc.nzsets.size(); i++) b->enc.nzsets[i].tile_base = b->imgs[size_t(b->enc.nzset_image[i])].out[b->enc.nzset_comp[i]].tile_base;
    {   // Which components' level-0 lists do the forward-DCT kernels build (k_pixel.hip nzf_*)?  Those whose real block grid is as wide as the padded one: a
        // workgroup's 256 padded blocks are then the 256 real blocks of a list chunk.  Their chunks lose bit 0 in the grid such a run takes.  Not under the
        // trellis quantiser without CSH_NZ_ONCE (or CSH_TR_SORT): the coding stages then build level 0 a second time, from the tiles the trellis rewrote.
        b->enc.nzchunks_fused = b->enc.nzchunks;
        const bool allowed = sw.nz_fused && !b->lossless && !b->webp && !b->rgb_out && !(b->tr.trellis && progressive && !b->tr.nz_once);
        std::vector<uint8_t> fused(b->enc.nzsets.size(), 0);
        // ... and of which of those does nothing read the quantised AC levels from the tiles any more (PlaneWork::ac_lists)?  Progressive output whose refinement scans
        // are coded from the lists too (no kind-0 chunk of k_tokens: no TokPlan of the component) and, under the trellis quantiser, whose trellis writes its levels
        // into the list (t_sort and nz_once).  Each of the fallback switches keeps the tiles whole by itself, in every profile; so does CSH_AC_TILES=1
        const bool lists_only = progressive && !sw.ac_tiles && sw.ref_list && sw.nz_once && sw.tr_sort && (!b->tr.trellis || (b->tr.t_sort && b->tr.nz_once));
        std::vector<uint8_t> planned(b->enc.nzsets.size(), 0);   // some TokPlan reads the component's tiles
        for (size_t i = 0; i < b->enc.plans.size(); i++) {
            const size_t at = size_t(b->enc.plan_image[i]) * CSH_MAX_COMPS + size_t(b->enc.plan_comp[i]);
            if (at < b->enc.nzset_of.size() && b->enc.nzset_of[at] >= 0) planned[size_t(b->enc.nzset_of[at])] = 1;
        }
        b->enc.nzset_ac_lists.assign(b->enc.nzsets.size(), 0);
        for (PlaneWork &w : b->pix.pwork) {
            w.ac_lists = 0u;
            const size_t at = size_t(w.image) * CSH_MAX_COMPS + size_t(w.comp);
            const int si = allowed && at < b->enc.nzset_of.size() ? b->enc.nzset_of[at] : -1;
            if (si < 0) continue;
            const NzSet &S = b->enc.nzsets[size_t(si)];
            if (S.real_bw != S.bw || S.list[0] == 0xFFFFFFFFu) continue;
            w.nzset = uint32_t(si); fused[size_t(si)] = 1; b->enc.n_fused++;
            if (lists_only && !planned[size_t(si)]) { w.ac_lists = 1u; b->enc.nzset_ac_lists[size_t(si)] = 1; b->enc.n_ac_lists++; }
        }
        for (TrellisWork &tw : b->tr.twork) tw.ac_lists = (tw.nzset != 0xFFFFFFFFu && b->enc.nzset_ac_lists[tw.nzset]) ? 1u : 0u;
        for (NzChunk &ch : b->enc.nzchunks_fused) if (fused[ch.set]) ch.levels &= ~1u;
        auto flags = [&](Stage &sg) {
            for (int f = 0; f < 2; f++) {
                const std::vector<NzChunk> &v = f ? b->enc.nzchunks_fused : b->enc.nzchunks;
                sg.nz_build[f] = sg.nz_filter[f] = false;
                for (uint32_t i = sg.nzc0; i < sg.nzc0 + sg.nnzc; i++) { sg.nz_build[f] |= (v[i].levels & 1u) != 0u; sg.nz_filter[f] |= (v[i].levels & ~1u) != 0u; }
            }
        };
        for (Stage &sg : b->enc.stage) flags(sg);
        flags(b->tr.tstage);
    }
    for (ParScan &ps : b->dec.pscans)   // table selectors: slot numbers of the table-set form the batch uses
        for (int m = 0; m < ps.nb_mcu && m < 10; m++) {
            int dcs = ps.dct[m] & 3, acs = 4 + (ps.act[m] & 3);
            if (b->dec.use4) { dcs = std::max<int>(0, b->dec.slot4[ps.huff_set][dcs]); acs = std::max<int>(0, b->dec.slot4[ps.huff_set][acs]); }
            ps.sel |= uint64_t(dcs | (acs << 3)) << (6 * m);
        }
    {   // the scans of the refinement chains as units of k_refine_parse, scan-major: a unit's predecessor has a smaller number
        std::vector<int> last(b->dec.chains.size(), -1);
        for (int s = 0;; s++) {
            bool any = false;
            for (size_t c = 0; c < b->dec.chains.size(); c++)
                if (b->dec.chains[c].refine && b->dec.chains[c].count > s) {
                    RefineUnit u; u.chain = int(c); u.s = s; u.prev = last[c];
                    last[c] = int(b->dec.refine_units.size());
                    b->dec.refine_units.push_back(u);
                    any = true;
                }
            if (!any) break;
        }
    }
    b->ntiles = b->ntiles_in + b->ntiles_out;
    b->pix.plane_bytes = plane_off;
    b->pix.oplane_bytes = oplane_off;
    b->out.out_cap = b->out.raw_bytes_cap;
    layout_token_pool(b);
}

// allocation and the upload of what never changes between runs
int BatchPlanner::upload(Laps &laps) {
    hipStream_t st = b->stream;
    if (!b->nimg) return 0;
    b->dec.bits_pool.flush_copies();
    laps.lap("copy_in");
    b->dec.need_seq_init.resize(size_t(b->nimg) + CSH_DEC_NSTATS, 0u);   // behind the images' words: the decoder's counters (kernels.h), zero in front of every run by the copy that resets need_seq
    if (b->dec.d_bits.alloc(b->dec.bits_pool.size()) || (b->dec.bits_pool.size() && hipMemcpyAsync(b->dec.d_bits.p, b->dec.bits_pool.p, b->dec.bits_pool.size(), hipMemcpyHostToDevice, st) != hipSuccess) ||
        b->d_imgs.upload(b->imgs, st) || b->dec.d_dscans.upload(b->dec.dscans, st) || b->dec.d_chains.upload(b->dec.chains, st) || b->dec.d_chain_scans.upload(b->dec.chain_scans, st) ||
        b->dec.d_hsets.upload(b->dec.hsets, st) || b->dec.d_phsets.upload(b->dec.phsets, st) || (b->dec.use4 && b->dec.d_phsets4.upload(b->dec.phsets4, st)) || b->d_quants.upload(b->quants, st) || b->pix.d_pwork.upload(b->pix.pwork, st) ||
        b->enc.d_script.upload(b->enc.script, st) || b->enc.d_swork.upload(b->enc.swork, st) || b->enc.d_slot_work.alloc(size_t(b->enc.nslots) + 1) || b->enc.d_slots.alloc(size_t(b->enc.nslots) + 1) || b->enc.d_plans.upload(b->enc.plans, st) || b->enc.d_echunks.upload(b->enc.echunks, st) || b->enc.d_hdr.upload(b->enc.hdr_pool, st) ||
        b->enc.d_hdr_off.upload(b->enc.hdr_off, st) || b->dec.d_pscans.upload(b->dec.pscans, st) || b->pix.d_rwork.upload(b->pix.rwork, st) || b->pix.d_rtaps.upload(b->pix.rtaps, st) ||
        b->pix.d_rweights.upload(b->pix.rweights, st) || b->pix.d_rgb.alloc(b->pix.rgb_bytes + 64) || b->pix.d_rtmp.alloc((resize_is_fused(b->pix.max_row_in) ? 0 : b->pix.tmp_floats) + 16) || b->dec.d_need_seq_init.upload(b->dec.need_seq_init, st))
        return CS_ERR_NO_DEVICE;
    size_t nchunks = b->dec.bits_pool.size() / 64 + 1, nst = size_t(b->dec.total_sub) + b->dec.pscans.size() + 1;
    b->dec.group = sw.dec_group ? sw.dec_group : dec_group_for(b->dec.total_sub);
    b->dec.spec_lanes = sw.dec_lanes ? sw.dec_lanes : kDecSpecLanes;
    b->dec.clear_front = sw.dec_clear_front;
    b->dec.test_rounds = sw.test_dec_rounds;
    if (b->dec.d_seed_cnt.alloc(b->dec.pscans.size() + 1) || b->dec.d_seed_off.alloc(b->dec.pscans.size() + 2)) return CS_ERR_NO_DEVICE;
    if (b->dec.d_clean.alloc(b->dec.bits_pool.size() + 64) || b->dec.d_unstuff_cnt.alloc(nchunks + 1) || b->dec.d_unstuff_off.alloc(nchunks + 2) ||
        b->dec.d_pstate.alloc(nst) || b->dec.d_relax_list[0].alloc(nst) || b->dec.d_relax_list[1].alloc(nst) || b->dec.d_relax_cnt.alloc(512) || b->dec.d_scan_pending.alloc(b->dec.pscans.size() + 1) || b->dec.d_cut_block.alloc(b->dec.pscans.size() + 1) || b->dec.d_claim.alloc(size_t(b->dec.total_sub) + 1) || b->dec.d_hyp.alloc((size_t(b->dec.total_sub) + 1) * 10) ||
        b->dec.d_nblk.alloc(size_t(b->dec.total_sub) + 1) || b->dec.d_blk_off.alloc(size_t(b->dec.total_sub) + 2) || b->dec.d_need_seq.alloc(size_t(b->nimg) + CSH_DEC_NSTATS + 1) ||
        b->dec.d_dcdiff.alloc(size_t(b->dec.dc_total) + 1) || b->dec.d_dc_off.alloc(size_t(b->dec.dc_total) + 2) ||
        b->dec.d_refine_hist.alloc(size_t(b->dec.refine_hist) + 1) || b->dec.d_refine_pos.alloc(size_t(b->dec.refine_pos) + 1) || b->dec.d_refine_units.upload(b->dec.refine_units, st) ||
        b->dec.d_refine_prog.alloc(b->dec.refine_units.size() + 1))
        return CS_ERR_NO_DEVICE;
    if (b->d_coef.alloc(size_t(b->ntiles) * CSH_TILE_I16) || b->pix.d_planes.alloc(b->pix.plane_bytes + 64) || b->pix.d_oplanes.alloc(b->pix.oplane_bytes + 64) ||
        b->enc.d_symbits.alloc(b->enc.total_words + 1) || b->enc.d_eobbits.alloc(b->enc.total_words + 1) ||
        b->enc.d_long_runs.alloc(2 * (b->enc.total_units / 512 + b->enc.swork.size() + 16)) || b->enc.d_long_cnt.alloc(4) || b->enc.d_tail.alloc(b->enc.total_units + 1) || b->enc.d_eobrun.alloc(b->enc.total_units + 1) || b->enc.d_corr.alloc(b->enc.total_corr + 1) || b->enc.d_lastn.alloc((b->enc.ref_pack ? b->enc.total_corr : 0) + 1) ||
        b->enc.d_tok_off.alloc(4 * size_t(b->enc.nslots) + 4) || b->enc.d_chunk_ntok.alloc(4 * size_t(b->enc.nslots) + 4) || b->enc.d_slot_hist.alloc(size_t(b->enc.hist_rows) * 256 + 256) ||
        b->enc.d_slot_raw.alloc(size_t(b->enc.nslots) + 1) || b->enc.d_img_list.upload(b->enc.img_list, st) || b->enc.d_img_nlist.upload(b->enc.img_nlist, st) || b->enc.d_scan_cost.alloc(b->enc.swork.size() + 1) || b->enc.d_slot_eobh.alloc(16 * size_t(b->enc.nslots) + 16) || b->enc.d_chunk_bits.alloc(size_t(b->enc.nslots) + 1) || b->enc.d_chunk_off.alloc(size_t(b->enc.nslots) + 2) || b->enc.d_tok_cursor.alloc(b->enc.region_est.size() + 1) || b->enc.d_regions.upload(b->enc.regions, st) ||
        b->enc.d_tables.alloc(b->enc.ntables) || b->enc.d_scan_pad.alloc(b->enc.swork.size() + 1) ||
        b->enc.d_nzlists.upload(b->enc.nzlists, st) || b->enc.d_nzsets.upload(b->enc.nzsets, st) || b->enc.d_nzchunks.upload(b->enc.nzchunks, st) || (b->enc.n_fused && b->enc.d_nzchunks_fused.upload(b->enc.nzchunks_fused, st)) || b->enc.d_list_slots.alloc(size_t(b->enc.nlist_slots) + 1) || b->enc.d_tok_slots.alloc(size_t(b->enc.ntok_slots) + 1) || b->enc.d_ref_slots.alloc(size_t(b->enc.nref_slots) + 1) || b->enc.d_list_runs.alloc(size_t(b->enc.nlist_runs) + 1) || b->enc.d_ref_runs.alloc(size_t(b->enc.nref_runs) + 1) ||
        b->enc.d_nz_cursor.alloc(b->enc.nzlists.size() + 1) || b->enc.d_nz_chunk_off.alloc(size_t(b->enc.nz_nrec) + 1) || b->enc.d_nz_chunk_cnt.alloc(size_t(b->enc.nz_nrec) + 1) ||
        b->enc.d_scan_raw_off.alloc(b->enc.swork.size() + 2) || b->out.d_img_size.alloc(b->nimg + 1) || b->out.d_img_size_pad.alloc(b->nimg + 1) ||
        b->out.d_img_off.alloc(b->nimg + 2) || b->out.d_status.alloc(b->nimg) || b->out.d_overflow.alloc(4))
        return CS_ERR_NO_DEVICE;
    // the slots of every work item, written where they are used (the host counted them: add_works)
    if (hipMemsetAsync(b->enc.d_slots.p, 0, (size_t(b->enc.nslots) + 1) * sizeof(SlotRec), st) != hipSuccess ||
        hipMemsetAsync(b->enc.d_slot_work.p, 0, (size_t(b->enc.nslots) + 1) * sizeof(uint32_t), st) != hipSuccess) { csh_set_error("hipMemsetAsync failed"); return CS_ERR_NO_DEVICE; }
    launch_make_slots(st, b->enc.d_swork.p, uint32_t(b->enc.swork.size()), b->enc.d_script.p, b->enc.d_nzlists.p, b->enc.d_slots.p, b->enc.d_slot_work.p, b->enc.d_list_slots.p, b->enc.d_tok_slots.p, b->enc.d_ref_slots.p, b->enc.d_list_runs.p, b->enc.d_ref_runs.p, b->enc.list_run);
    if (b->tr.trellis && (b->tr.d_trows.upload(b->tr.trows, st) || (b->tr.t_sort && (b->tr.d_tperm.alloc(size_t(b->tr.t_units) + 1) || b->tr.d_tblk_cnt.alloc(size_t(b->tr.t_units) + 1) || (b->tr.nz_once && b->tr.d_tblk_off.alloc(size_t(b->tr.t_units) + 1)))))) return CS_ERR_NO_DEVICE;
    if (b->tr.trellis && (b->tr.d_twork.upload(b->tr.twork, st) || b->tr.d_truns.upload(b->tr.truns, st) || b->tr.d_tqueue.alloc(1) || b->tr.d_tlambda.alloc(size_t(b->tr.t_units) + 1) || b->tr.d_tdcbt.alloc(size_t(b->tr.t_units) + 1) ||
                       b->tr.d_tspill.alloc(trellis_spill_words(trellis_ac_slots())) || b->pix.d_dct_raw.alloc(size_t(b->ntiles_out) * CSH_TILE_I16)))
        return CS_ERR_NO_DEVICE;
    for (size_t n = 0; px && n < count; n++) {
        const Item &it = b->items[n];
        if (it.image < 0) continue;
        const ResizeWork &rw = b->pix.rwork[size_t(it.image)];   // every image of such a batch has its resize work item, in image order
        if (rw.image != it.image) { csh_set_error("internal: resize work out of order"); return CS_ERR_NO_DEVICE; }
        if (hipMemcpyAsync(b->pix.d_rgb.p + rw.rgb_src_off, px[n].device_pixels, size_t(px[n].width) * px[n].height * px[n].channels, hipMemcpyDeviceToDevice, st) != hipSuccess) { csh_set_error("pixel copy failed"); return CS_ERR_NO_DEVICE; }
    }
    laps.lap("alloc+enqueue");
    if (hipStreamSynchronize(st) != hipSuccess) { csh_set_error("upload failed"); return CS_ERR_NO_DEVICE; }
    laps.lap("upload_wait");
    return 0;
}

}  // namespace csh
