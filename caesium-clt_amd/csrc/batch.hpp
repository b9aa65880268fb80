// batch.hpp -- the JPEG batch object (csh_batch): its members grouped by the phase that owns them, each group holding its host
// descriptors, its counters and its device buffers together.  batch_plan.cpp fills it (batch_create in pipeline.cpp drives the steps),
// batch_run.cpp pushes it through the kernels, scan_search.cpp is the host half of the scan search, pipeline.cpp is the C surface.
#pragma once
#include <array>
#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "../../include/caesium_hip.h"
#include "devmem.hpp"
#include "jpeg_host.hpp"
#include "kernels.h"
#include "webp_kernels.h"

namespace csh {

struct Item {
    int code = 0;
    std::string msg;
    JpegInfo in;
    JpegInfo out;     // output geometry (comp ids / sampling / tq)
    int image = -1;   // index among the images that reached the device, or -1
    size_t file_size = 0;
    std::vector<uint8_t> meta_out;  // APPn/COM segments that survive the metadata/ICC policy (frame header rebuilds)
};

// phase 0: entropy decode (k_decode*.hip)
// grouped speculation (k_decode_par.hip k_dec_spec_group): the workgroup's lanes, and the group length by the batch's size in sub-sequences (a 1080p
// file of the bench has 5012).  DESIGN 4.2 has the sweeps: 8 wins from 256 files up (by 0.9 ms per step at 2048), 4 at 128 files -- the CLI's device batch --,
// 2 at 16 and 32; nothing smaller was measured, and such a batch keeps one lane per sub-sequence
constexpr uint32_t kDecSpecLanes = 256;
static inline uint32_t dec_group_for(uint32_t total_sub) { return total_sub >= (1u << 20) ? 8u : total_sub >= (1u << 19) ? 4u : total_sub >= (1u << 16) ? 2u : 1u; }

struct DecodePlan {
    PinnedBytes bits_pool;
    std::vector<DecScan> dscans;
    std::vector<DevHuffSet> hsets;
    std::vector<ParHuffSet> phsets;   // the same sets in the parallel decoder's LDS form
    std::vector<char> phset_fits;     // 0: sub-table pool overflow -> sequential decoder
    std::vector<ParHuffSet4> phsets4; // compact form (types.h); slot4[set][0..3 DC, 4..7 AC] = slot or -1
    std::vector<std::array<int8_t, 8>> slot4;
    bool use4 = true;                 // every table set of the batch fits the compact form
    std::vector<ParScan> pscans;
    std::vector<uint32_t> need_seq_init;
    std::vector<ProgChain> chains;        // progressive inputs (k_decode_prog.hip)
    std::vector<int> chain_scans;
    std::vector<RefineUnit> refine_units;
    uint32_t refine_hist = 0, refine_pos = 0, refine_max_blocks = 0;   // AC refinement chains (k_decode_refine.hip): history masks, block positions, largest chain
    uint32_t total_sub = 0, max_sub = 0, max_par_blocks = 0, dc_total = 0;
    // sub-sequences a lane of the speculation pass carries its state through (PlanSwitches::dec_group, or the planner's choice by total_sub).  1: k_dec_dense<0>,
    // k_dec_dense<1>, list rounds; 2, 4, 8: k_dec_spec_group of spec_lanes lanes, k_dec_seed, the seam round, list rounds
    uint32_t group = 1, spec_lanes = 256;
    bool clear_front = false;                               // PlanSwitches::dec_clear_front: a memset in front of the phase clears the tiles, no decoding pass does (measurements)
    std::vector<uint32_t> h_relax_cnt;                      // the host's copy of d_relax_cnt (the read-backs between the list rounds)
    uint32_t last_run_seeds = 0, last_run_relaxed = 0;      // csh_timing.n_dec_seeds / n_dec_relaxed of the last run
    int test_rounds = -1;                                   // PlanSwitches::test_dec_rounds: the list rounds stop there (-1: at the length of d_relax_cnt)
    uint32_t last_run_rounds = 0;                           // csh_timing.n_dec_rounds of the last run
    DevBuf<uint32_t> d_seed_cnt;
    DevBuf<uint64_t> d_seed_off;

    DevBuf<uint8_t> d_bits, d_clean;
    DevBuf<ParScan> d_pscans;
    DevBuf<uint64_t> d_pstate, d_relax_list[2], d_unstuff_off, d_blk_off, d_dc_off;
    DevBuf<uint32_t> d_unstuff_cnt, d_nblk, d_need_seq, d_need_seq_init, d_relax_cnt, d_scan_pending, d_cut_block, d_claim;
    DevBuf<uint16_t> d_hyp;
    DevBuf<int32_t> d_dcdiff;
    DevBuf<DecScan> d_dscans;
    DevBuf<ProgChain> d_chains;
    DevBuf<int> d_chain_scans;
    DevBuf<uint64_t> d_refine_hist;
    DevBuf<uint32_t> d_refine_pos, d_refine_prog;
    DevBuf<RefineUnit> d_refine_units;
    DevBuf<DevHuffSet> d_hsets;
    DevBuf<ParHuffSet> d_phsets;
    DevBuf<ParHuffSet4> d_phsets4;
};

// phase 1: planes, the resize branch, the forward DCT (k_pixel.hip, k_resize.hip)
struct PixelPlan {
    std::vector<PlaneWork> pwork;
    std::vector<ResizeWork> rwork;
    std::vector<ResizeTap> rtaps;
    std::vector<float> rweights;
    uint64_t rgb_bytes = 0, tmp_floats = 0, max_tmp = 0, max_dst = 0;
    uint32_t max_row_in = 0, max_out_w = 0, max_nh = 0;   // resize launches: samples per source row, pixels per resized row, resized rows
    uint32_t max_src_px = 0;
    uint64_t plane_bytes = 0, oplane_bytes = 0;
    uint32_t max_quads = 0;
    bool any_layout = false, any_layout_rgb = false;   // some work item is CSH_MODE_ANY / some resize item CSH_RZ_ANY: the batch launches k_resample_any / k_planes_to_rgb_any
    bool any_space_rgb = false;                        // some resize item is CSH_RZ_SPACE: the batch launches k_planes_to_rgb_space

    DevBuf<uint8_t> d_planes, d_oplanes, d_rgb;
    DevBuf<PlaneWork> d_pwork;
    DevBuf<ResizeWork> d_rwork;
    DevBuf<ResizeTap> d_rtaps;
    DevBuf<float> d_rweights, d_rtmp;
    DevBuf<int16_t> d_dct_raw;   // the unquantised DCT: size targeting and the trellis quantiser work from it
};

// a contiguous range of everything the coding kernels index: work items, slots, token chunks, tables, plans, list builder chunks, slot lists
struct Stage {
    uint32_t work0 = 0, nwork = 0, slot0 = 0, nslots = 0, ech0 = 0, nech = 0, table0 = 0, ntables = 0, plan0 = 0, nplans = 0, nzc0 = 0, nnzc = 0, ls0 = 0, nls = 0, ts0 = 0, nts = 0, rs0 = 0, nrs = 0, lr0 = 0, nlr = 0, rr0 = 0, nrr = 0;
    // does some NzChunk of the stage ask for level 0 from the tiles (k_nzlist) / for a filtered level (k_nzfilter)?  [0]: as planned (EncodePlan::nzchunks), [1]: in a run whose forward-DCT kernels built lists (nzchunks_fused)
    bool nz_build[2] = {true, true}, nz_filter[2] = {true, true};
};
struct SearchImg {
    int cand_work[64]; int ncand;       // candidate number -> work item (-1: not coded by itself -- see search_work)
    int Al_luma = 0, Al_chroma = 0;
    uint64_t best_luma = 0, best_chroma = 0;   // running minimum of the decision in progress
    int split_luma = 0, split_chroma = 0;
    bool luma_on = false, chroma_on = false;    // the decision in progress needs the next stage's candidates
    bool fixed = false;                         // an RGB / CMYK / YCCK frame: no search (mozjpeg's jpeg_search_progression declines), its list of scans stands from the start
};

// phases 2..6: tokens, lists, tables, sizes, packing, assembly (k_entropy.hip, k_aclist.hip, k_assemble.hip) and the scan search's stages
struct EncodePlan {
    std::vector<EncScan> script;
    std::vector<ScanWork> swork;
    // per (work item, 256-unit chunk) slot: its work item, its SlotRec, its place in the list-coded / token-coded slot lists -- ~3.9 k slots per 1080p image
    // under the scan search (64 MB of records per 256 files): the host only counts them, k_make_slots writes them on the device from the work items
    uint32_t nslots = 0, nlist_slots = 0, ntok_slots = 0;
    uint32_t nref_slots = 0;              // those of the token-coded slots whose tokens k_list_refine makes (refinement scans coded from their list)
    uint32_t last_run_refine = 0;         // refinement work items the last run coded from lists (csh_timing.n_list_refine)
    uint32_t last_run_ref_packed = 0;     // ... and those of them it packed from the lists, without tokens (csh_timing.n_ref_packed)
    bool ref_pack = true;                 // PlanSwitches::ref_pack
    // k_list_stats, k_list_pack and k_list_refine take one wave per run of up to list_run consecutive chunks of a work item: the runs are counted beside the slots
    uint32_t list_run = CSH_LIST_RUN;     // PlanSwitches::list_run
    uint32_t nlist_runs = 0, nref_runs = 0;
    bool ac_runs_slot = false;            // PlanSwitches::ac_runs_slot
    uint32_t last_run_list_runs = 0;      // list and refinement runs of the work items the last run coded, all stages (csh_timing.n_list_runs)
    uint64_t total_corr = 0;              // correction words: one per unit of a refinement scan
    uint64_t total_units = 0, total_words = 0;
    uint32_t max_units = 0;
    int ntables = 0;
    std::vector<TokPlan> plans;
    std::vector<int> plan_comp, plan_image;
    std::vector<EChunk> echunks;          // the token kernel's workgroups
    uint64_t tok_cap = 0;                 // token pool capacity: the sum of the regions
    uint32_t tok_scale = 1;               // grows on overflow
    std::vector<TokRegion> regions;       // one per TokPlan, then one per DC / sequential work item
    std::vector<uint32_t> region_est;     // estimated tokens of each (x tok_scale = its capacity)
    uint32_t hist_rows = 0;               // rows of 256 symbol counts over all slots
    // the compacted coefficient lists the progressive AC first-pass scans are coded from (k_aclist.hip; types.h NzList)
    std::vector<NzList> nzlists;          // one per (image, component, Al) some scan of the batch needs
    std::vector<NzSet> nzsets;            // one per (image, component)
    std::vector<int> nzset_of;            // [image * CSH_MAX_COMPS + component] -> NzSet, -1
    std::vector<uint32_t> nzset_built;    // per set: levels some stage's builder makes
    std::vector<int> nzset_comp, nzset_image;
    std::vector<NzChunk> nzchunks;        // the builder's grid, stage after stage
    // the same grid for a run in which the forward-DCT kernels build the level-0 lists of the components that allow it (k_pixel.hip nzf_*; PlaneWork::nzset): those
    // components' chunks without bit 0.  A run that does not come through the transform (the re-quantisation of size targeting) takes `nzchunks`
    std::vector<NzChunk> nzchunks_fused;
    uint32_t n_fused = 0;                 // components whose list the transform builds (csh_timing.n_fused_lists of a run that does)
    uint32_t last_run_fused = 0;          // ... of the last run
    // of those, the components whose quantised AC levels no coding kernel reads from the tiles (PlaneWork::ac_lists): a run whose transform builds the lists does not
    // store them there (csh_timing.n_ac_in_lists), and csh_batch_read_coefs writes them back from the lists on demand
    uint32_t n_ac_lists = 0;
    uint32_t last_run_ac_lists = 0;       // ... of the last run
    std::vector<uint8_t> nzset_ac_lists;  // per set: such a component
    std::vector<uint32_t> nz_est, nz_worst; // per list: estimated / largest possible number of entries
    uint32_t nz_nrec = 0;                 // per-(list, chunk) records
    uint64_t nz_cap = 0;                  // pool capacity: the sum of the regions
    // mozjpeg's scan search (the default profile; CSH_PROFILE=plain keeps the stock script): the candidate scans are coded in stages
    // -- work items, slots, token chunks and tables of one stage behind those of the stage before -- and the host replays
    // jcmaster.c select_scans on their sizes in between.  mozjpeg codes its candidates one after the other and skips ahead as soon as
    // a decision is made; the stages follow that order: what every image needs (ST_1, ST_2), and what only an image whose search runs
    // on needs (ST_1B: luma at Al 3; ST_2B / ST_2C: the fourth and fifth frequency split) -- those stages run only when some image
    // asks for them, and then only over the work items of those images (EncCtx::work_active).
    bool search = false;
    enum { ST_1 = 0, ST_1B = 1, ST_2 = 2, ST_2B = 3, ST_2C = 4, ST_N = 5 };
    Stage stage[ST_N];
    void stage_begin(Stage &sg) {
        sg.work0 = uint32_t(swork.size()); sg.slot0 = nslots; sg.ech0 = uint32_t(echunks.size()); sg.table0 = uint32_t(ntables); sg.plan0 = uint32_t(plans.size());
        sg.nzc0 = uint32_t(nzchunks.size()); sg.ls0 = nlist_slots; sg.ts0 = ntok_slots; sg.rs0 = nref_slots; sg.lr0 = nlist_runs; sg.rr0 = nref_runs;
    }
    void stage_end(Stage &sg) {
        sg.nwork = uint32_t(swork.size()) - sg.work0; sg.nslots = nslots - sg.slot0; sg.nech = uint32_t(echunks.size()) - sg.ech0;
        sg.ntables = uint32_t(ntables) - sg.table0; sg.nplans = uint32_t(plans.size()) - sg.plan0;
        sg.nnzc = uint32_t(nzchunks.size()) - sg.nzc0; sg.nls = nlist_slots - sg.ls0; sg.nts = ntok_slots - sg.ts0; sg.nrs = nref_slots - sg.rs0; sg.nlr = nlist_runs - sg.lr0; sg.nrr = nref_runs - sg.rr0;
    }
    std::vector<SearchImg> simg;
    std::vector<uint8_t> work_active;               // per work item: coded in the (gated) stage about to run
    uint32_t n_gated_runs = 0;                      // how many of the conditional stages the last run needed (csh_timing.n_search_extra)
    std::vector<uint32_t> img_list, img_nlist, h_cost;
    std::map<std::array<int, 5>, int> cand_script;   // (component, Ss, Se, Ah, Al) -> EncScan index
    std::vector<uint8_t> hdr_pool;
    std::vector<uint32_t> hdr_off;

    DevBuf<uint8_t> d_hdr, d_tail, d_scan_tmp, d_work_active;
    DevBuf<EncScan> d_script;
    DevBuf<ScanWork> d_swork;
    DevBuf<uint32_t> d_slot_work;
    DevBuf<EChunk> d_echunks;
    DevBuf<SlotRec> d_slots;
    DevBuf<TokPlan> d_plans;
    DevBuf<uint64_t> d_corr, d_symbits, d_eobbits, d_tok_off, d_chunk_off, d_scan_raw_off;
    DevBuf<uint32_t> d_tok_cursor;
    DevBuf<TokRegion> d_regions;
    DevBuf<uint16_t> d_eobrun, d_slot_hist, d_lastn;
    DevBuf<uint32_t> d_img_list, d_img_nlist, d_scan_cost, d_slot_raw, d_slot_eobh, d_long_runs, d_long_cnt, d_tokens, d_chunk_ntok, d_chunk_bits, d_raw, d_scan_pad, d_chunk_ff, d_hdr_off;
    DevBuf<DevEncTable> d_tables;
    DevBuf<NzList> d_nzlists;
    DevBuf<NzSet> d_nzsets;
    DevBuf<NzChunk> d_nzchunks, d_nzchunks_fused;
    DevBuf<uint32_t> d_nz_pool, d_nz_cursor, d_nz_chunk_off, d_nz_chunk_cnt, d_list_slots, d_tok_slots, d_ref_slots, d_list_runs, d_ref_runs;
};

// mozjpeg's quantiser half (CSH_PROFILE=mozjpeg): overshoot deringing in front of every forward DCT; trellis quantisation behind it --
// a third stage of work items (one statistics scan per component, coded for its histogram only) and the two k_trellis kernels
struct TrellisPlan {
    bool trellis = false, dering = false;
    Stage tstage;
    std::vector<TrellisWork> twork;
    std::vector<TrellisRun> truns;        // k_trellis_ac's queue: runs of up to CSH_TR_RUN chunks, every work item's first run, then every second one, ..
    uint32_t t_units = 0, t_max_rows = 0;
    std::vector<uint32_t> trows;          // k_trellis_dc: (work item << 16 | iMCU row), longest rows first
    bool t_sort = false;                  // k_trellis_ac takes its blocks in order of list length (progressive output: the statistics lists count them)
    bool nz_once = false;                 // progressive output under the trellis quantiser: its levels go into the statistics scan's level-0 lists and the coding stages filter those (no second k_nzlist over the tiles)

    DevBuf<TrellisWork> d_twork;
    DevBuf<TrellisRun> d_truns;
    DevBuf<uint32_t> d_tqueue, d_trows, d_tperm, d_tspill;
    DevBuf<uint8_t> d_tblk_cnt;
    DevBuf<uint16_t> d_tblk_off;
    DevBuf<uint64_t> d_tlambda, d_tdcbt;
};

// the VP8 encoder behind the resize branch (k_webp.hip, k_vp8enc.hip)
struct WebpTail {
    uint32_t webp_mb_bytes = 768;  // output bytes reserved per macroblock (grows on overflow; CSH_TEST_POOL_SHIFT divides this first value: layout_token_pool)
    std::vector<csw::WebpImg> wimgs;
    uint64_t wwork_bytes = 0, wlevels = 0;
    uint32_t wmax_luma = 0, wmax_mbh = 0;

    DevBuf<csw::WebpImg> d_wimgs;
    DevBuf<uint8_t> d_wwork, d_wscratch, d_wprobs, d_wupdate;
    DevBuf<uint32_t> d_wpart, d_wstats;
    DevBuf<int16_t> d_wlevels;
};

// what a run leaves: the files, their sizes and places, per-image status
struct Outputs {
    uint64_t raw_bytes_cap = 0, out_cap = 0;
    DevBuf<uint8_t> d_out;
    DevBuf<uint64_t> d_img_off;
    DevBuf<uint32_t> d_img_size, d_img_size_pad, d_status, d_overflow;
    std::vector<uint32_t> h_img_size;
    std::vector<uint64_t> h_img_off;
    std::vector<uint32_t> h_status;
    bool ran = false;
};

}  // namespace csh

struct csh_batch {
    int device = 0;
    hipStream_t stream = 0;
    bool have_stream = false;
    CCSParameters params;
    std::vector<csh::Item> items;
    int nimg = 0;
    bool lossless = false;
    bool rgb_out = false;          // csh_batch_create_pixels: stop after the resize branch's RGB
    bool webp = false;             // target container: the decoded (and resized) RGB goes to the VP8 encoder instead of the JPEG one
    int test_pool_shift = -1;      // CSH_TEST_POOL_SHIFT as read at the first pool layout of this batch (-1: not read yet)
    bool progressive = true;
    bool retain_dct = false;       // size targeting: keep the unquantised DCT so that another quality only re-quantises
    bool have_dct = false;
    int q_base = 0;               // quants[q_base + q] = output table for quality q (1..100)

    // what every phase reads: the images, the quantisation tables, the coefficient tiles ([all decoded tiles][all re-quantised tiles])
    std::vector<csh::ImgDesc> imgs;
    std::vector<csh::DevQuant> quants;
    uint32_t ntiles = 0, ntiles_in = 0, ntiles_out = 0, max_tiles = 0, max_dummy = 0;
    csh::DevBuf<csh::ImgDesc> d_imgs;
    csh::DevBuf<csh::DevQuant> d_quants;
    csh::DevBuf<int16_t> d_coef;

    csh::DecodePlan dec;
    csh::PixelPlan pix;
    csh::EncodePlan enc;
    csh::TrellisPlan tr;
    csh::WebpTail wp;
    csh::Outputs out;

    // (wait for whatever is still queued -- a run that failed half-way leaves launches behind -- before the members hand their device blocks back to the cache)
    ~csh_batch() { if (have_stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }
};

namespace csh {

// kernel timing slots (csh_timing.kernel_ms): one row per slot, in slot order; names via csh_kernel_name()
enum KernelSlot {
    KS_MEMSET_COEF, KS_UNSTUFF, KS_DEC_SPEC, KS_DEC_RELAX0, KS_DEC_RELAX, KS_DEC_WRITE, KS_DC_SCATTER, KS_REFINE_CHAINS, KS_DECODE_PROG_SEQ,
    KS_IDCT_PLANE, KS_RESIZE, KS_XFORM_DIRECT, KS_RESAMPLE_FDCT, KS_FIX_DUMMY, KS_MEMSET_ENC, KS_TRELLIS_STATS, KS_TRELLIS_AC, KS_TRELLIS_DC,
    KS_NZLIST, KS_TOKENS, KS_LIST_STATS, KS_AC_RUNS, KS_GEN_TABLES, KS_CHUNK_SIZES, KS_SCAN_CHUNK_BITS, KS_SCAN_LAYOUT, KS_PACK, KS_LIST_PACK,
    KS_FF_COUNT, KS_SCAN_SEARCH, KS_LAYOUT, KS_SCAN_IMAGES, KS_EMIT, KS_SPARE0, KS_SPARE1, KS_SPARE2, KS_COUNT,
    // a WebP batch (csh_batch_create_webp) leaves the JPEG path behind the resize slot: its next three slots are these
    KS_WEBP_YUV = KS_XFORM_DIRECT, KS_WEBP_ENCODE = KS_RESAMPLE_FDCT, KS_WEBP_ASSEMBLE = KS_FIX_DUMMY
};
// the trellis slots (statistics scan = k_tokens without tokens + k_ac_runs + k_gen_tables; the two k_trellis kernels + k_fix_dummy) count
// as phase 1: they are the quantiser; zero unless CSH_PROFILE=mozjpeg
struct KernelSlotRow { KernelSlot slot; const char *name; int phase; };
constexpr KernelSlotRow kKernelSlots[] = {
    {KS_MEMSET_COEF, "memset_coef", 0},        {KS_UNSTUFF, "unstuff", 0},                 {KS_DEC_SPEC, "k_dec_spec", 0},
    {KS_DEC_RELAX0, "k_dec_relax0", 0},        {KS_DEC_RELAX, "k_dec_relax1_4", 0},        {KS_DEC_WRITE, "k_dec_write", 0},
    {KS_DC_SCATTER, "k_dc_scatter", 0},        {KS_REFINE_CHAINS, "k_refine_chains", 0},   {KS_DECODE_PROG_SEQ, "k_decode_prog+seq", 0},
    {KS_IDCT_PLANE, "k_idct_plane", 1},        {KS_RESIZE, "resize", 1},                   {KS_XFORM_DIRECT, "k_xform_direct", 1},
    {KS_RESAMPLE_FDCT, "k_resample+k_plane_fdct", 1}, {KS_FIX_DUMMY, "k_fix_dummy", 1},    {KS_MEMSET_ENC, "memset_enc", 2},
    {KS_TRELLIS_STATS, "trellis_stats", 1},    {KS_TRELLIS_AC, "k_trellis_ac", 1},         {KS_TRELLIS_DC, "k_trellis_dc", 1},
    {KS_NZLIST, "k_nzlist", 2},                {KS_TOKENS, "k_tokens", 2},                 {KS_LIST_STATS, "k_list_stats", 2},
    {KS_AC_RUNS, "k_ac_runs", 2},              {KS_GEN_TABLES, "k_gen_tables", 3},         {KS_CHUNK_SIZES, "k_chunk_sizes", 4},
    {KS_SCAN_CHUNK_BITS, "scan_chunk_bits", 4}, {KS_SCAN_LAYOUT, "scan_layout", 4},        {KS_PACK, "k_pack", 5},
    {KS_LIST_PACK, "k_list_pack", 5},          {KS_FF_COUNT, "k_ff_count", 6},             {KS_SCAN_SEARCH, "scan_search_stage2", 7},
    {KS_LAYOUT, "k_layout", 6},                {KS_SCAN_IMAGES, "scan_images", 6},         {KS_EMIT, "k_emit", 6},
    {KS_SPARE0, "", 7},                        {KS_SPARE1, "", 7},                         {KS_SPARE2, "", 7}};
constexpr bool kernel_slots_in_order() {
    for (int i = 0; i < int(sizeof kKernelSlots / sizeof kKernelSlots[0]); i++) if (kKernelSlots[i].slot != i) return false;
    return true;
}
static_assert(sizeof kKernelSlots / sizeof kKernelSlots[0] == CSH_NKERNELS && int(KS_COUNT) == int(CSH_NKERNELS), "one row per csh_timing.kernel_ms slot");
static_assert(kernel_slots_in_order(), "row i of kKernelSlots describes slot i");

// switches of the environment that shape the plan, read once where the batch is created
struct PlanSwitches {
    std::string profile;        // CSH_PROFILE, "mozjpeg" when unset or empty
    bool nz_once = true;        // CSH_NZ_ONCE != "0"
    bool tr_sort = true;        // CSH_TR_SORT != "0"
    int prog_par = -1;          // CSH_PROG_PAR: 0, 1, or -1 for anything else
    bool fused_420 = true;      // CSH_NO_FUSED_420 unset
    bool nz_fused = true;       // CSH_NZ_FUSED != "0": the forward-DCT kernels build the level-0 coefficient lists
    bool ref_list = true;       // CSH_REF_LIST != "0": the AC refinement scans are coded from the coefficient lists (k_list_refine), not from the tiles (k_tokens' kind-0 chunks)
    bool ref_pack = true;       // CSH_REF_PACK != "0" (and ref_list): those scans are packed from the lists too (k_list_refine_pack): no token, no token region, not in tok_slots
    uint32_t list_run = CSH_LIST_RUN;   // CSH_LIST_RUN, clamped to 1..32: chunks per wave of k_list_stats, k_list_pack and k_list_refine (1: one wave per chunk)
    bool ac_runs_slot = false;  // CSH_AC_RUNS == "slot": k_ac_runs takes one wave per slot, as before it took one per 16 slots (k_ac_runs_words)
    bool ac_tiles = false;      // CSH_AC_TILES == "1": every component's AC levels are stored to its tiles, as before they lived in the lists
    uint32_t dec_group = 0;     // CSH_DEC_GROUP: 1, 2, 4 or 8 (DecodePlan::group); 0 for anything else: the planner chooses by the batch's size
    bool dec_clear_front = false;   // CSH_DEC_CLEAR == "front": the tiles and the EOBRUN array are cleared by memsets, not behind the speculation pass's work (what the clearing costs there: DESIGN 10)
    int test_dec_rounds = -1;   // CSH_TEST_DEC_ROUNDS=n (tests): at most n list rounds, so that small inputs reach k_dec_chain and the sequential kernel's hand-over; -1 when unset
    uint32_t dec_lanes = 0;     // CSH_DEC_LANES: 192 or 256 lanes a workgroup of k_dec_spec_group; 0 for anything else: the default
    static PlanSwitches read();
};

// CSH_TRACE: host-side laps of batch_create on stderr (what the boundary pays in front of the first kernel)
struct Laps {
    const bool trace;
    std::chrono::steady_clock::time_point at = std::chrono::steady_clock::now();
    std::string text;
    Laps();
    void lap(const char *what);
};

// The planner (batch_plan.cpp): batch_create calls its steps in this order.  The order in which the steps append to the batch's vectors
// is what every offset in the descriptors is derived from.
struct BatchPlanner {
    csh_batch *const b;
    const CByteArray *const inputs;
    const size_t count;
    const CCSParameters *const p;
    const csp_pixels *const px;       // csh_batch_create_from_pixels: the RGB of every image is copied in, not decoded
    const PlanSwitches sw;
    const bool progressive;
    uint16_t qout_nat[64];
    int script_base3 = 0, script_base1 = 0;
    std::map<int, int> other_scripts;   // CSH_CS_RGB / CMYK / YCCK -> first EncScan of the frame's stock script
    std::vector<std::pair<std::vector<uint8_t>, int>> hset_keys;
    std::map<std::vector<uint16_t>, int> quant_index;
    uint64_t plane_off = 64, oplane_off = 0;  // 64-bit: a resize batch of 1024 1080p files has 7 GB of planes; 64 bytes in front of the first plane: k_resample_fdct_420 reads a row's window from four bytes before it

    BatchPlanner(csh_batch *b, const CByteArray *inputs, size_t count, const CCSParameters *p, const csp_pixels *px);
    void begin();                     // modes from the profile, output tables, the stock scripts
    void parse();                     // the thread pool over the files
    int reserve_pinned();
    int plan_image(size_t n);         // everything of one file
    int plan_search_stages();         // closes stage 1; the search's later stages
    int plan_trellis();
    void finish_descriptors();        // tile rebasing, table selectors, refine units, pool layout
    int upload(Laps &laps);           // allocation + upload, k_make_slots, the pixel copy-in

private:
    void image_geometry(Item &it, ImgDesc &im);
    int decode_scans(Item &it, ImgDesc &im, const uint8_t *d);
    int huff_set(const JScan &js);
    void place_blocks(ParScan &ps, const JpegInfo &in, const JScan &js, uint32_t units, bool dc_rows, bool subseqs);
    int sequential_split(const Item &it, const ImgDesc &im, const uint8_t *d, int img_index, bool &par_ok);
    bool progressive_plan(const Item &it, const ImgDesc &im, int img_index);
    void plane_work(ImgDesc &im, const JpegInfo &in, const JpegInfo &o, int img_index, bool resized);
    void resize_work(const JpegInfo &in, const JpegInfo &o, int img_index);
    void output_scans(Item &it, ImgDesc &im, int img_index, size_t in_len);
    void frame_header(Item &it);
    template <class Fill> int enc_scan(const std::array<int, 5> &key, Fill fill);
    int space_script(int ncomp, int space, int &ns);
    int cand_index(int comp, int Ss, int Se, int Ah, int Al, int cls = -1);
    int dc_scan_index(int ncomp);
    int seq1_index(int comp, int cls = -1);
    uint32_t nz_list(int img_index, int comp, int Al, const ImgDesc &im, size_t in_len);
    void add_works(Item &it, ImgDesc &im, int img_index, const std::vector<int> &list, size_t in_len, const JpegInfo &o, bool stats_only = false);
    template <class Make> void add_stage(int sid, Make make);
    template <class Add> void splits(const ImgDesc &im, Add &add, int i0, int i1, bool whole);
};

// token pool (k_entropy.hip) and list pool (k_aclist.hip): every region gets its estimate x tok_scale
void layout_token_pool(csh_batch *b);

// batch_run.cpp: one pass of the batch through its kernels (the caller retries with larger pools on overflow)
int run_once(csh_batch *b, csh_timing *t, bool requant_only);

// scan_search.cpp: the host replay of mozjpeg's select_scans between the coding stages
int search_costs(csh_batch *b, AsmCtx &a, int stage);
uint32_t search_gate(csh_batch *b, int stage, int (*want)(const SearchImg &));
int search_decide(csh_batch *b, int stage);
int search_lists(csh_batch *b);

}  // namespace csh
