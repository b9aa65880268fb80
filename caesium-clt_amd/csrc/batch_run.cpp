// batch_run.cpp -- one run of the JPEG batch object: csh_batch_run pushes the whole group through
//   entropy decode -> pixel-domain transcode -> masks/flags/runs -> stats/tables -> sizes/scan -> pack
//   -> stuffing/assembly
// on one stream with no host round trip (every size and offset is produced by device scans) -- but for the decoder's look at its
// relaxation list and the scan search's decisions between its stages.
#include <algorithm>

#include "batch.hpp"

namespace csh {
namespace {

// The events of one run, one after every kernel timing slot, on the batch's own stream: kernel_ms[i] = ev[i+1] - ev[i].  A run owns
// its set: whatever was created is destroyed on every way out of the run.  A mark names the slot it closes; slots are closed in order.
class KernelMarks {
    hipEvent_t ev[CSH_NKERNELS + 1];
    int created = 0, next = 0;   // next: the slot the next mark closes
    const hipStream_t st;

public:
    explicit KernelMarks(hipStream_t s) : st(s) {}
    KernelMarks(const KernelMarks &) = delete;
    KernelMarks &operator=(const KernelMarks &) = delete;
    ~KernelMarks() { for (int i = 0; i < created; i++) (void)hipEventDestroy(ev[i]); }
    int start() {
        for (; created <= CSH_NKERNELS; created++) CSH_CHECK(hipEventCreate(&ev[created]));
        CSH_CHECK(hipEventRecord(ev[0], st));
        return 0;
    }
    // the event that closes `slot`, for a launcher that records it itself
    int claim(KernelSlot slot, hipEvent_t *e) {
        if (int(slot) != next || next >= CSH_NKERNELS) {
            csh_set_error("internal: timing mark '%s' out of order (slot %d is next)", slot < KS_COUNT ? kKernelSlots[slot].name : "?", next);
            return -1;
        }
        *e = ev[++next];
        return 0;
    }
    int mark(KernelSlot slot) {
        hipEvent_t e;
        if (claim(slot, &e)) return -1;
        CSH_CHECK(hipEventRecord(e, st));
        return 0;
    }
    // closes every slot in front of `slot` here: they stay empty, or the first of them carries what was launched before
    int skip_to(KernelSlot slot) {
        while (next < int(slot)) if (mark(KernelSlot(next))) return -1;
        return int(slot) == next ? 0 : mark(slot);   // (behind `slot` already: mark() reports it)
    }
    // kernel_ms of the slots closed so far and total_ms; phases: the sums per phase too, everything else zero (the JPEG path)
    int read(csh_timing *t, bool phases) const {
        if (phases) {
            for (int i = 0; i < CSH_NPHASES; i++) t->phase_ms[i] = 0;
            for (int i = 0; i < CSH_NKERNELS; i++) t->kernel_ms[i] = 0;
        }
        for (int i = 0; i < next; i++) {
            CSH_CHECK(hipEventElapsedTime(&t->kernel_ms[i], ev[i], ev[i + 1]));
            if (phases) t->phase_ms[kKernelSlots[i].phase] += t->kernel_ms[i];
        }
        CSH_CHECK(hipEventElapsedTime(&t->total_ms, ev[0], ev[next]));
        return 0;
    }
};
#define MARK(slot) do { if (marks.mark(slot)) return -1; } while (0)

struct Run {
    csh_batch *const b;
    csh_timing *const t;
    const hipStream_t st;
    const int nimg;
    KernelMarks marks;
    uint64_t raw_chunks = 0;
    bool eobrun_cleared = false;   // the decode phase's store-less passes have cleared the encoder's EOBRUN array on the side (k_dec_dense clear_share)
    bool fused = false;            // the forward-DCT kernels of this run built level-0 lists: the stages take the builder's grid without them (EncodePlan::nzchunks_fused)
    EncCtx c;
    AsmCtx a;

    Run(csh_batch *b_, csh_timing *t_) : b(b_), t(t_), st(b_->stream), nimg(b_->nimg), marks(b_->stream) {}

    // the pools whose size a retry changes
    int pools() {
        raw_chunks = (b->out.raw_bytes_cap + 63) / 64;
        if (b->enc.d_raw.n != raw_chunks * 16) {
            if (b->enc.d_raw.alloc(raw_chunks * 16) || b->enc.d_chunk_ff.alloc(raw_chunks + 1) || b->out.d_out.alloc(b->out.out_cap + 64))
                return -1;
            const uint64_t longest = std::max({uint64_t(size_t(b->enc.nslots)), uint64_t(b->enc.swork.size()), uint64_t(b->dec.dc_total), uint64_t(b->dec.total_sub), uint64_t(b->dec.pscans.size()), uint64_t(b->dec.bits_pool.size() / 64), uint64_t(nimg)});
            size_t tmp = exclusive_scan_tmp_bytes(longest + 1);   // the longest input any exclusive scan of a run gets
            if (b->enc.d_scan_tmp.alloc(tmp)) return -1;
        }
        if (b->enc.d_tokens.n < b->enc.tok_cap && b->enc.d_tokens.alloc(b->enc.tok_cap)) return -1;
        if (b->enc.d_nz_pool.n < b->enc.nz_cap && b->enc.d_nz_pool.alloc(b->enc.nz_cap)) return -1;
        return 0;
    }

    // a re-run at another quality from the retained DCT: only the first of the decode + pixel phases' slots carries time (k_requant + k_fix_dummy)
    int requant() {
        if (b->out.d_status.zero(st) || b->out.d_overflow.zero(st)) return -1;
        launch_requant(st, b->d_imgs.p, b->pix.d_pwork.p, int(b->pix.pwork.size()), b->max_tiles, b->d_quants.p, b->pix.d_dct_raw.p, b->ntiles_in, b->d_coef.p);
        launch_fix_dummy(st, b->d_imgs.p, nimg, b->max_dummy, b->d_coef.p);
        return marks.skip_to(KS_MEMSET_ENC);
    }
    // a re-run from the decoded coefficients that are still in the pool: the decode phase's slots stay empty
    int skip_decode() {
        if (b->out.d_status.zero(st) || b->out.d_overflow.zero(st)) return -1;
        return marks.skip_to(KS_IDCT_PLANE);
    }

    // ---- phase 0: entropy decode (tiles must start at zero: the decoder only writes non-zero coefficients).  Where the speculation pass runs, its workgroups
    // clear the tiles on the side (k_dec_dense<0>); a memset in front of the phase otherwise (only progressive / irregular scans listed)
    int decode() {
        const bool spec = !b->dec.pscans.empty() && b->dec.max_sub != 0, zero_in_spec = spec && !b->dec.clear_front;
        if (!zero_in_spec) CSH_CHECK(hipMemsetAsync(b->d_coef.p, 0, size_t(b->ntiles_in) * CSH_TILE_I16 * sizeof(int16_t), st));
        if (b->out.d_status.zero(st) || b->out.d_overflow.zero(st)) return -1;
        CSH_CHECK(hipMemcpyAsync(b->dec.d_need_seq.p, b->dec.d_need_seq_init.p, (size_t(nimg) + CSH_DEC_NSTATS) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));   // (and the counters behind them: zero)
        MARK(KS_MEMSET_COEF);
        {   // parallel self-synchronising decode of sequential-mode scans
            int nps = int(b->dec.pscans.size());
            uint32_t nchunks = uint32_t(b->dec.bits_pool.size() / 64);
            if (nps) {
                launch_unstuff_count(st, b->dec.d_bits.p, b->dec.d_pscans.p, nps, nchunks, b->dec.d_unstuff_cnt.p);
                launch_exclusive_scan(st, b->dec.d_unstuff_cnt.p, b->dec.d_unstuff_off.p, nchunks, b->enc.d_scan_tmp.p, b->enc.d_scan_tmp.n);
                launch_unstuff_copy(st, b->dec.d_bits.p, b->dec.d_clean.p, b->dec.d_pscans.p, nps, nchunks, b->dec.d_unstuff_off.p);
            }
            MARK(KS_UNSTUFF);
            DenseArgs da;
            memset(&da, 0, sizeof da);
            da.clean = b->dec.d_clean.p; da.pss = b->dec.d_pscans.p; da.huffs = b->dec.use4 ? static_cast<const void *>(b->dec.d_phsets4.p) : static_cast<const void *>(b->dec.d_phsets.p); da.compact = b->dec.use4 ? 1 : 0; da.state = b->dec.d_pstate.p; da.nblk = b->dec.d_nblk.p;
            da.list_out = b->dec.d_relax_list[0].p; da.cnt_out = b->dec.d_relax_cnt.p; da.blk_off = b->dec.d_blk_off.p; da.imgs = b->d_imgs.p;
            da.coef = b->d_coef.p; da.dcdiff = b->dec.d_dcdiff.p; da.need_seq = b->dec.d_need_seq.p; da.cut_block = b->dec.d_cut_block.p;
            CSH_CHECK(hipMemsetAsync(b->dec.d_cut_block.p, 0xFF, b->dec.d_cut_block.n * sizeof(uint32_t), st));
            const uint64_t zero_all = uint64_t(b->ntiles_in) * CSH_TILE_I16 * sizeof(int16_t), zero_half = (zero_all / 2) & ~uint64_t(15);
            const uint64_t eob_all = (uint64_t(b->enc.d_eobrun.n) * sizeof(uint16_t)) & ~uint64_t(15), eob_half = (eob_all / 2) & ~uint64_t(15);   // (the last < 16 bytes: a memset below)
            da.live_cnt = b->dec.d_relax_cnt.p + b->dec.d_relax_cnt.n - 1; da.seed_cnt = b->dec.d_seed_cnt.p;   // (the last count: no round's)
            const uint32_t G = spec ? b->dec.group : 1u;   // (nothing to speculate on: every launch below does nothing)
            uint32_t *const dec_stats = b->dec.d_need_seq.p + nimg;   // (kernels.h CSH_DEC_STAT_*)
            const int seam = G > 1 ? 1 : 0;                        // the seam round takes list 0 / count 0: list round R then reads list (R + seam) & 1 and count R + seam
            const uint64_t eob_tail = uint64_t(b->enc.d_eobrun.n) * sizeof(uint16_t) - eob_all;
            if (G > 1) {
                // a lane carries its state through G sub-sequences; only the first of every group is then known to start from a guess.  Both arrays are cleared behind this pass
                if (zero_in_spec) {
                    da.zero_ptr = reinterpret_cast<uint8_t *>(b->d_coef.p); da.zero_bytes = zero_all; da.zero2_ptr = reinterpret_cast<uint8_t *>(b->enc.d_eobrun.p); da.zero2_bytes = eob_all;
                    if (eob_tail) CSH_CHECK(hipMemsetAsync(reinterpret_cast<uint8_t *>(b->enc.d_eobrun.p) + eob_all, 0, eob_tail, st));
                    eobrun_cleared = b->enc.d_eobrun.n != 0;
                }
                launch_dec_spec_group(st, nps, b->dec.max_sub, G, b->dec.spec_lanes, da);
                da.zero_bytes = 0; da.zero2_bytes = 0;
                MARK(KS_DEC_SPEC);
                CSH_CHECK(hipMemsetAsync(b->dec.d_relax_cnt.p, 0, b->dec.d_relax_cnt.n * sizeof(uint32_t), st));
                if (b->dec.d_claim.zero(st)) return -1;
                // the seams in scan order, evaluated by a list round of their own: it lists what they change and does not walk
                launch_exclusive_scan(st, b->dec.d_seed_cnt.p, b->dec.d_seed_off.p, uint64_t(nps), b->enc.d_scan_tmp.p, b->enc.d_scan_tmp.n);
                launch_dec_seed(st, b->dec.d_seed_off.p, nps, b->dec.max_sub, G, b->dec.d_relax_list[0].p, b->dec.d_relax_cnt.p);
                launch_dec_relax_list(st, b->dec.d_clean.p, b->dec.d_pscans.p, b->dec.total_sub, da.huffs, da.compact, b->dec.d_pstate.p, b->dec.d_nblk.p, b->dec.d_relax_list[0].p,
                                      b->dec.d_relax_cnt.p, b->dec.d_relax_list[1].p, b->dec.d_relax_cnt.p + 1, b->dec.d_pstate.n, b->dec.d_claim.p, 0x80000000u, dec_stats, false);
                MARK(KS_DEC_RELAX0);
            } else {
                if (zero_in_spec) { da.zero_ptr = reinterpret_cast<uint8_t *>(b->d_coef.p); da.zero_bytes = zero_half; da.zero2_ptr = reinterpret_cast<uint8_t *>(b->enc.d_eobrun.p); da.zero2_bytes = eob_half; }
                launch_dec_dense(st, 0, nps, b->dec.max_sub, da);
                da.zero_bytes = 0; da.zero2_bytes = 0;
                MARK(KS_DEC_SPEC);
                if (nps) CSH_CHECK(hipMemsetAsync(b->dec.d_relax_cnt.p, 0, b->dec.d_relax_cnt.n * sizeof(uint32_t), st));
                if (nps && b->dec.d_claim.zero(st)) return -1;
                if (zero_in_spec) {   // (the other halves: k_dec_dense<1>)
                    da.zero_ptr = reinterpret_cast<uint8_t *>(b->d_coef.p) + zero_half; da.zero_bytes = zero_all - zero_half;
                    da.zero2_ptr = reinterpret_cast<uint8_t *>(b->enc.d_eobrun.p) + eob_half; da.zero2_bytes = eob_all - eob_half;
                    if (eob_tail) CSH_CHECK(hipMemsetAsync(reinterpret_cast<uint8_t *>(b->enc.d_eobrun.p) + eob_all, 0, eob_tail, st));
                    eobrun_cleared = b->enc.d_eobrun.n != 0;
                }
                launch_dec_dense(st, 1, nps, b->dec.max_sub, da);
                da.zero_bytes = 0; da.zero2_bytes = 0;
                MARK(KS_DEC_RELAX0);
            }
            // list rounds until the list is empty.  How many that takes depends on the data: stock tables at ordinary quality settle
            // in ~8 (the list shrinks by 60 % a round), 50 bytes per block in ~30, 85 bytes per block in more than a hundred (a
            // wrong state then survives most of the cuts it crosses) -- so the host looks at the list length after 12 rounds and
            // then after every 8 (a read-back of the counts; an empty round is a ~6 us launch), up to kMaxRounds.  What is still listed
            // after that goes through the label chain below or to the sequential kernel.
            // (CSH_TEST_DEC_ROUNDS, for the tests: fewer rounds, so that small files are still listed behind them)
            const int kAllRounds = int(b->dec.d_relax_cnt.n) - 2 - seam;   // (the last count is DenseArgs::live_cnt)
            const int kMaxRounds = b->dec.test_rounds >= 0 ? std::min(b->dec.test_rounds, kAllRounds) : kAllRounds;
            std::vector<uint32_t> &cnt = b->dec.h_relax_cnt;
            cnt.assign(b->dec.d_relax_cnt.n, 0u);
            int R = 0;
            for (int group = 12; nps && R < kMaxRounds; group = 8) {
                for (int g = 0; g < group && R < kMaxRounds; g++, R++)
                    launch_dec_relax_list(st, b->dec.d_clean.p, b->dec.d_pscans.p, b->dec.total_sub, da.huffs, da.compact, b->dec.d_pstate.p, b->dec.d_nblk.p, b->dec.d_relax_list[(R + seam) & 1].p,
                                          b->dec.d_relax_cnt.p + R + seam, b->dec.d_relax_list[((R + seam) & 1) ^ 1].p, b->dec.d_relax_cnt.p + R + seam + 1, b->dec.d_pstate.n, b->dec.d_claim.p, uint32_t(R + 1), dec_stats);
                // (the whole array, 2 KB: the counts in front of the last one are csh_timing's n_dec_seeds and n_dec_relaxed)
                CSH_CHECK(hipMemcpyAsync(cnt.data(), b->dec.d_relax_cnt.p, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                CSH_CHECK(hipStreamSynchronize(st));
                if (!cnt[size_t(R + seam)]) break;
            }
            if (nps && !R) {   // (no round at all: the counts of the passes in front of them)
                CSH_CHECK(hipMemcpyAsync(cnt.data(), b->dec.d_relax_cnt.p, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                CSH_CHECK(hipStreamSynchronize(st));
            }
            b->dec.last_run_rounds = uint32_t(R);
            b->dec.last_run_seeds = cnt[0];
            b->dec.last_run_relaxed = cnt.back();   // (G = 1: what the dense relaxation pass evaluated)
            for (int r = 0; r < R + seam; r++) b->dec.last_run_relaxed += cnt[size_t(r)];
            if (nps) {   // scans that are still listed: settle their block-in-MCU labels exactly (k_dec_chain), or hand the image to k_decode_seq
                if (b->dec.d_scan_pending.zero(st)) return -1;
                launch_dec_mark_pending(st, b->dec.d_pscans.p, b->dec.total_sub, b->dec.d_relax_list[(R + seam) & 1].p, b->dec.d_relax_cnt.p + R + seam, b->dec.d_scan_pending.p);
                da.hyp = b->dec.d_hyp.p; da.scan_pending = b->dec.d_scan_pending.p;
                launch_dec_dense(st, 3, nps, b->dec.max_sub, da);
                launch_dec_chain(st, b->dec.d_pscans.p, nps, b->dec.d_pstate.p, b->dec.d_nblk.p, b->dec.d_hyp.p, b->dec.d_scan_pending.p, b->dec.d_need_seq.p, dec_stats);
            }
            MARK(KS_DEC_RELAX);
            if (nps) launch_exclusive_scan(st, b->dec.d_nblk.p, b->dec.d_blk_off.p, b->dec.total_sub, b->enc.d_scan_tmp.p, b->enc.d_scan_tmp.n);
            launch_dec_dense(st, 2, nps, b->dec.max_sub, da);
            MARK(KS_DEC_WRITE);
            if (nps) launch_exclusive_scan(st, reinterpret_cast<uint32_t *>(b->dec.d_dcdiff.p), b->dec.d_dc_off.p, b->dec.dc_total, b->enc.d_scan_tmp.p, b->enc.d_scan_tmp.n);
            launch_dc_scatter(st, b->dec.d_pscans.p, nps, b->dec.max_par_blocks, b->d_imgs.p, b->dec.d_dc_off.p, b->d_coef.p, b->dec.d_need_seq.p, b->dec.d_cut_block.p);
            launch_dc_refine(st, b->dec.d_clean.p, b->dec.d_pscans.p, nps, b->dec.max_par_blocks, b->d_imgs.p, b->d_coef.p, b->dec.d_need_seq.p);
            MARK(KS_DC_SCATTER);
        }
        launch_refine_chains(st, b->dec.d_clean.p, b->dec.d_pscans.p, b->dec.d_phsets.p, b->dec.d_dscans.p, b->dec.d_chains.p, b->dec.d_chain_scans.p, int(b->dec.chains.size()), b->dec.d_refine_units.p,
                             int(b->dec.refine_units.size()), b->dec.refine_max_blocks, b->d_imgs.p, b->d_coef.p, b->dec.d_need_seq.p, b->dec.d_refine_hist.p, b->dec.d_refine_pos.p, b->dec.d_refine_prog.p);
        MARK(KS_REFINE_CHAINS);
        launch_decode_prog(st, b->dec.d_clean.p, b->dec.d_pscans.p, b->dec.d_phsets.p, b->dec.d_dscans.p, b->dec.d_chains.p, b->dec.d_chain_scans.p, int(b->dec.chains.size()), b->d_imgs.p,
                           b->d_coef.p, b->dec.d_need_seq.p);
        launch_decode_seq(st, b->dec.d_bits.p, b->d_imgs.p, b->dec.d_dscans.p, b->dec.d_hsets.p, b->d_coef.p, nimg, b->dec.d_need_seq.p);
        MARK(KS_DECODE_PROG_SEQ);
        return 0;
    }

    // ---- phase 1: pixel-domain transcode.  Decoded planes and the resize branch ...
    int planes() {
        int nw = b->lossless ? 0 : int(b->pix.pwork.size());
        launch_idct_plane(st, b->d_imgs.p, b->pix.d_pwork.p, nw, b->max_tiles, b->d_quants.p, b->d_coef.p, b->pix.d_planes.p);
        MARK(KS_IDCT_PLANE);
        launch_resize(st, b->d_imgs.p, b->pix.d_rwork.p, int(b->pix.rwork.size()), b->pix.d_rtaps.p, b->pix.d_rweights.p, b->pix.d_planes.p, b->pix.d_rgb.p, b->pix.d_rtmp.p,
                      b->pix.max_src_px, b->pix.max_tmp, b->pix.max_dst, b->pix.max_row_in, b->pix.max_out_w, b->pix.max_nh, !(b->webp || b->rgb_out), b->pix.any_layout_rgb, b->pix.any_space_rgb);
        MARK(KS_RESIZE);
        return 0;
    }
    // ... and the forward DCT of what the encoder takes
    int pixels() {
        const int nw = b->lossless ? 0 : int(b->pix.pwork.size());
        int16_t *rawp = ((b->retain_dct || b->tr.trellis) && !b->lossless) ? b->pix.d_dct_raw.p : nullptr;   // the trellis quantiser works from the unquantised DCT
        // the level-0 coefficient lists of the components that allow it are built here (PlaneWork::nzset): what the kernels add to must be zero in front of them
        NzFuse nzf;
        memset(&nzf, 0, sizeof nzf);
        fused = nw && b->enc.n_fused;
        if (fused) {
            if (b->enc.d_nz_cursor.zero(st) || b->enc.d_nz_chunk_cnt.zero(st)) return -1;
            nzf.nzsets = b->enc.d_nzsets.p; nzf.nzlists = b->enc.d_nzlists.p; nzf.nz_pool = b->enc.d_nz_pool.p; nzf.nz_cursor = b->enc.d_nz_cursor.p;
            nzf.nz_chunk_off = b->enc.d_nz_chunk_off.p; nzf.nz_chunk_cnt = b->enc.d_nz_chunk_cnt.p; nzf.overflow = b->out.d_overflow.p;
            nzf.blk_cnt = (b->tr.trellis && b->tr.t_sort) ? b->tr.d_tblk_cnt.p : nullptr;
            nzf.blk_off = (nzf.blk_cnt && b->tr.nz_once) ? b->tr.d_tblk_off.p : nullptr;
        }
        // (CSH_DEBUG bit 32768, for the tests: the output tiles start the run as garbage.  A component whose AC levels live in the lists -- PlaneWork::ac_lists -- carries
        // it in octets 1..7 through the whole run: a kernel that still read them there would change the files)
        if (nw && getenv("CSH_DEBUG") && (uint32_t(atoi(getenv("CSH_DEBUG"))) & 32768u))
            CSH_CHECK(hipMemsetAsync(b->d_coef.p + size_t(b->ntiles_in) * CSH_TILE_I16, 0x5A, size_t(b->ntiles - b->ntiles_in) * CSH_TILE_I16 * sizeof(int16_t), st));
        launch_xform_direct(st, b->d_imgs.p, b->pix.d_pwork.p, nw, b->max_tiles, b->d_quants.p, b->d_coef.p, b->d_coef.p, rawp, b->ntiles_in, b->tr.dering, nzf);
        MARK(KS_XFORM_DIRECT);
        launch_resample_plane(st, b->d_imgs.p, b->pix.d_pwork.p, nw, b->pix.max_quads, b->pix.d_planes.p, b->pix.d_oplanes.p);
        if (b->pix.any_layout) launch_resample_any(st, b->d_imgs.p, b->pix.d_pwork.p, nw, b->pix.max_quads, b->pix.d_planes.p, b->pix.d_oplanes.p);
        launch_plane_fdct(st, b->d_imgs.p, b->pix.d_pwork.p, nw, b->max_tiles, b->d_quants.p, b->pix.d_oplanes.p, b->d_coef.p, rawp, b->ntiles_in, b->tr.dering, nzf);
        launch_resample_fdct_420(st, b->d_imgs.p, b->pix.d_pwork.p, nw, b->max_tiles, b->d_quants.p, b->pix.d_planes.p, b->d_coef.p, rawp, b->ntiles_in, b->tr.dering, nzf);
        MARK(KS_RESAMPLE_FDCT);
        if (!b->lossless) launch_fix_dummy(st, b->d_imgs.p, nimg, b->max_dummy, b->d_coef.p);
        MARK(KS_FIX_DUMMY);
        return 0;
    }

    void fill_enc_ctx() {
        memset(&c, 0, sizeof c);
        c.imgs = b->d_imgs.p; c.script = b->enc.d_script.p; c.work = b->enc.d_swork.p; c.nwork = int(b->enc.swork.size());
        c.echunks = b->enc.d_echunks.p; c.plans = b->enc.d_plans.p; c.nechunks = uint32_t(b->enc.echunks.size()); c.slot_work = b->enc.d_slot_work.p; c.slots = b->enc.d_slots.p; c.nslots = b->enc.nslots;
        c.coef = b->d_coef.p; c.sym_bits = b->enc.d_symbits.p; c.eob_bits = b->enc.d_eobbits.p; c.tail = b->enc.d_tail.p;
        c.eobrun = b->enc.d_eobrun.p; c.long_runs = b->enc.d_long_runs.p; c.long_cnt = b->enc.d_long_cnt.p; c.corr = b->enc.d_corr.p; c.lastn = b->enc.d_lastn.p; c.ref_pack = b->enc.ref_pack ? 1u : 0u;
        c.tokens = b->enc.d_tokens.p; c.regions = b->enc.d_regions.p; c.tok_cursor = b->enc.d_tok_cursor.p; c.tok_off = b->enc.d_tok_off.p; c.chunk_ntok = b->enc.d_chunk_ntok.p; c.slot_hist = b->enc.d_slot_hist.p; c.slot_raw = b->enc.d_slot_raw.p; c.slot_eobh = b->enc.d_slot_eobh.p;
        c.chunk_bits = b->enc.d_chunk_bits.p; c.chunk_off = b->enc.d_chunk_off.p; c.tables = b->enc.d_tables.p;
        c.raw = b->enc.d_raw.p; c.raw_words = raw_chunks * 16; c.status = b->out.d_status.p; c.overflow = b->out.d_overflow.p;
        c.nzlists = b->enc.d_nzlists.p; c.nzsets = b->enc.d_nzsets.p; c.nz_pool = b->enc.d_nz_pool.p; c.nz_cursor = b->enc.d_nz_cursor.p; c.nz_chunk_off = b->enc.d_nz_chunk_off.p; c.nz_chunk_cnt = b->enc.d_nz_chunk_cnt.p;
        c.debug = getenv("CSH_DEBUG") ? uint32_t(atoi(getenv("CSH_DEBUG"))) : 0u;
    }
    void fill_asm_ctx() {
        memset(&a, 0, sizeof a);
        a.imgs = b->d_imgs.p; a.script = b->enc.d_script.p; a.work = b->enc.d_swork.p; a.nimg = nimg;
        a.nwork = b->tr.trellis ? int(b->tr.tstage.work0) : c.nwork;   // the trellis stage's statistics scans (the last work items) put nothing into a file
        a.tables = b->enc.d_tables.p; a.chunk_off = b->enc.d_chunk_off.p; a.scan_pad_bytes = b->enc.d_scan_pad.p; a.scan_raw_off = b->enc.d_scan_raw_off.p;
        a.raw = b->enc.d_raw.p; a.raw_chunks = raw_chunks; a.chunk_ff = b->enc.d_chunk_ff.p;
        a.hdr_pool = b->enc.d_hdr.p; a.hdr_off = b->enc.d_hdr_off.p; a.img_size = b->out.d_img_size.p; a.img_size_pad = b->out.d_img_size_pad.p;
        a.img_off = b->out.d_img_off.p; a.out = b->out.d_out.p; a.out_cap = b->out.out_cap; a.status = b->out.d_status.p; a.overflow = b->out.d_overflow.p;
        a.img_list = b->enc.d_img_list.p; a.img_nlist = b->enc.d_img_nlist.p; a.scan_cost = b->enc.d_scan_cost.p;
    }
    void fill_trellis_ctx(TrellisCtx &tc) {
        memset(&tc, 0, sizeof tc);
        tc.imgs = b->d_imgs.p; tc.quant = b->d_quants.p; tc.work = b->tr.d_twork.p; tc.nwork = int(b->tr.twork.size()); tc.runs = b->tr.d_truns.p; tc.nruns = uint32_t(b->tr.truns.size());
        tc.tables = b->enc.d_tables.p; tc.raw = b->pix.d_dct_raw.p; tc.raw_tile0 = b->ntiles_in; tc.coef = b->d_coef.p; tc.dcrec = b->tr.d_tlambda.p; tc.dcbt = b->tr.d_tdcbt.p;
        tc.spill = b->tr.d_tspill.p; tc.nslots = uint32_t(b->tr.d_tspill.n / trellis_spill_words(1)); tc.max_rows = b->tr.t_max_rows;
        tc.queue = b->tr.d_tqueue.p;
        tc.rows = b->tr.d_trows.p; tc.nrows = uint32_t(b->tr.trows.size());
        if (b->tr.t_sort) { tc.blk_cnt = b->tr.d_tblk_cnt.p; tc.perm = b->tr.d_tperm.p; }
        if (b->tr.t_sort && b->tr.nz_once) {
            tc.nz_pool = b->enc.d_nz_pool.p; tc.nzlists = b->enc.d_nzlists.p; tc.nzsets = b->enc.d_nzsets.p; tc.nz_chunk_off = b->enc.d_nz_chunk_off.p; tc.nz_chunk_cnt = b->enc.d_nz_chunk_cnt.p;
            tc.blk_off = b->tr.d_tblk_off.p;
        }
        tc.ac_lists = fused ? 1u : 0u;   // (only a run whose transform built the lists left the flagged components' AC levels out of the tiles)
        tc.debug = getenv("CSH_TR_DEBUG") ? uint32_t(atoi(getenv("CSH_TR_DEBUG"))) : 0u;
    }

    // ---- phase 2: tokens (+ flags + statistics), EOB runs
    int encode_begin() {
        fill_enc_ctx();
        launch_reset_works(st, b->enc.d_swork.p, c.nwork);
        if (!fused && (b->enc.d_nz_cursor.zero(st) || b->enc.d_nz_chunk_cnt.zero(st))) return -1;   // (a fused run: zeroed in front of the transform, which has added to them)
        if (b->enc.d_symbits.zero(st) || b->enc.d_eobbits.zero(st) || (!eobrun_cleared && b->enc.d_eobrun.zero(st)) || b->enc.d_tables.zero(st) || b->enc.d_tok_cursor.zero(st) || b->enc.d_slot_eobh.zero(st) || b->enc.d_scan_pad.zero(st)) return -1;
#ifdef CSH_EMUL
        if (b->enc.d_raw.zero(st)) return -1;   // the emulation's packer ORs every word into the pool (no LDS window there)
#else
        if ((c.debug & 8192u) && b->enc.d_raw.zero(st)) return -1;
#endif
        MARK(KS_MEMSET_ENC);
        return 0;
    }

    // csh_timing.n_list_runs: the list and refinement runs of the stage's work items that are coded (a gated stage launches the runs of the others too: they do nothing)
    void count_list_runs(const Stage &sg, bool gate) {
        for (uint32_t wi = sg.work0; (sg.nlr || sg.nrr) && wi < sg.work0 + sg.nwork; wi++) {
            const ScanWork &w = b->enc.swork[wi];
            if ((w.lr_base != 0xFFFFFFFFu || w.rr_base != 0xFFFFFFFFu) && (!gate || b->enc.work_active[wi])) b->enc.last_run_list_runs += ((w.nunits + 255u) / 256u + b->enc.list_run - 1u) / b->enc.list_run;
        }
    }

    void set_stage(const Stage &sg) {
        c.echunks = b->enc.d_echunks.p + sg.ech0; c.nechunks = sg.nech; c.slot0 = sg.slot0; c.nslots = sg.nslots;
        c.nzchunks = (fused ? b->enc.d_nzchunks_fused.p : b->enc.d_nzchunks.p) + sg.nzc0; c.nnzchunks = sg.nnzc;
        c.nz_build = sg.nz_build[fused ? 1 : 0]; c.nz_filter = sg.nz_filter[fused ? 1 : 0];
        c.list_slots = b->enc.d_list_slots.p + sg.ls0; c.nlist_slots = sg.nls; c.tok_slots = b->enc.d_tok_slots.p + sg.ts0; c.ntok_slots = sg.nts;
        c.ref_slots = b->enc.d_ref_slots.p + sg.rs0; c.nref_slots = sg.nrs;
        c.list_runs = b->enc.d_list_runs.p + sg.lr0; c.nlist_runs = sg.nlr; c.ref_runs = b->enc.d_ref_runs.p + sg.rr0; c.nref_runs = sg.nrr; c.list_run = b->enc.list_run;
        c.ac_runs_slot = b->enc.ac_runs_slot ? 1u : 0u;
    }

    // ---- mozjpeg's trellis quantiser (CSH_PROFILE=mozjpeg): per component a statistics scan over the scalar-quantised coefficients
    // (tokens without tokens: histograms, flags, EOB runs -> optimal tables), then every block re-quantised from the retained DCT
    int trellis() {
        const Stage &tg = b->tr.tstage;
        set_stage(tg);
        c.stats_only = 1;
        if (b->enc.d_long_cnt.zero(st)) return -1;
        c.nz_blk_cnt = b->tr.t_sort ? b->tr.d_tblk_cnt.p : nullptr;
        c.nz_blk_off = (b->tr.t_sort && b->tr.nz_once) ? b->tr.d_tblk_off.p : nullptr;
        launch_nzlist(st, c);       // level 0 of the scalar-quantised coefficients (progressive output: the statistics scans are list slots)
        c.nz_blk_cnt = nullptr; c.nz_blk_off = nullptr;
        if (b->tr.t_sort) {   // the blocks of every component in order of list length (timed with the statistics)
            TrellisCtx ts;
            memset(&ts, 0, sizeof ts);
            ts.work = b->tr.d_twork.p; ts.nwork = int(b->tr.twork.size()); ts.blk_cnt = b->tr.d_tblk_cnt.p; ts.perm = b->tr.d_tperm.p;
            launch_trellis_sort(st, ts);
        }
        launch_tokens(st, c);       // (sequential output: one-component sequential scans, histograms only)
        launch_list_stats(st, c);
        count_list_runs(tg, false);
        launch_ac_runs(st, c);
        launch_gen_tables(st, b->enc.d_tables.p + tg.table0, int(tg.ntables));
        c.stats_only = 0;
        if (b->enc.d_nz_cursor.zero(st)) return -1;   // the lists are made again from what the trellis leaves
        MARK(KS_TRELLIS_STATS);
        TrellisCtx tc;
        fill_trellis_ctx(tc);
        if (b->tr.d_tqueue.zero(st)) return -1;   // every run of the batch (size targeting, repeated runs) starts the queue at its head
        launch_trellis_ac(st, tc);
        MARK(KS_TRELLIS_AC);
        launch_trellis_dc(st, tc);
        launch_fix_dummy(st, b->d_imgs.p, nimg, b->max_dummy, b->d_coef.p);   // the dummy blocks copy DC values the trellis has just changed
        MARK(KS_TRELLIS_DC);
        return 0;
    }

    // one stage = tokens -> runs -> tables -> chunk sizes -> offsets -> pack -> stuffing counts, over a contiguous range of work items
    // (without the scan search: one stage, everything).  mark: timing slots are recorded for stage 1 only, stage 2 gets one slot.
    int stage(const Stage &sg, bool mark, bool gate) {
#define SMARK(slot) do { if (mark) MARK(slot); } while (0)
        set_stage(sg);
        c.work_active = gate ? b->enc.d_work_active.p : nullptr;
        a.work0 = int(sg.work0); a.nwork_run = int(sg.nwork);
        if (b->enc.d_long_cnt.zero(st)) return -1;
        launch_nzlist(st, c);       // the lists this stage's first-pass scans are coded from and no earlier stage made
        SMARK(KS_NZLIST);
        launch_list_refine(st, c);  // AC refinement scans, from the lists (timed with k_tokens, whose kind-0 chunks they were)
        for (uint32_t wi = sg.work0; sg.nrs && wi < sg.work0 + sg.nwork; wi++)
            if (b->enc.swork[wi].rs_base != 0xFFFFFFFFu && (!gate || b->enc.work_active[wi])) { b->enc.last_run_refine++; if (b->enc.ref_pack) b->enc.last_run_ref_packed++; }
        count_list_runs(sg, gate);
        launch_tokens(st, c);       // DC and sequential-mode scans (CSH_REF_LIST=0: the refinement scans too, from the tiles)
        SMARK(KS_TOKENS);
        launch_list_stats(st, c);   // AC first-pass scans
        SMARK(KS_LIST_STATS);
        launch_ac_runs(st, c);
        SMARK(KS_AC_RUNS);
        launch_gen_tables(st, b->enc.d_tables.p + sg.table0, int(sg.ntables));
        SMARK(KS_GEN_TABLES);
        launch_chunk_sizes(st, c);
        SMARK(KS_CHUNK_SIZES);
        launch_exclusive_scan(st, b->enc.d_chunk_bits.p + sg.slot0, b->enc.d_chunk_off.p + sg.slot0, sg.nslots, b->enc.d_scan_tmp.p, b->enc.d_scan_tmp.n);
        SMARK(KS_SCAN_CHUNK_BITS);
        launch_scan_sizes(st, a);
        launch_exclusive_scan(st, b->enc.d_scan_pad.p, b->enc.d_scan_raw_off.p, uint64_t(a.nwork), b->enc.d_scan_tmp.p, b->enc.d_scan_tmp.n);   // all work items: those of a later stage still count zero
        launch_scan_place(st, a);
        launch_zero_edges(st, c);
        SMARK(KS_SCAN_LAYOUT);
        launch_pack(st, c);
        launch_list_refine_pack(st, c);   // AC refinement scans, from the lists (CSH_REF_PACK; timed with k_pack, which packed their tokens)
        SMARK(KS_PACK);
        launch_list_pack(st, c);
        SMARK(KS_LIST_PACK);
        launch_ff_count(st, a);
        SMARK(KS_FF_COUNT);
#undef SMARK
        return 0;
    }

    // a conditional stage: coded only if some image's search asks for it, and then only for those images (work_active)
    int gated_stage(int sid, int (*want)(const SearchImg &)) {
        if (!search_gate(b, sid, want)) return 0;
        b->enc.n_gated_runs++;
        if (b->enc.d_work_active.upload(b->enc.work_active, st)) return -1;
        if (stage(b->enc.stage[sid], false, true) || search_costs(b, a, sid)) return -1;
        return search_decide(b, sid);
    }
    int search() {
        b->enc.n_gated_runs = 0;
        if (search_costs(b, a, EncodePlan::ST_1) || search_decide(b, EncodePlan::ST_1)) return -1;      // Al of luma (unless Al 3 is still to be tried) and of chroma
        if (gated_stage(EncodePlan::ST_1B, [](const SearchImg &si) { return si.luma_on ? 1 : 0; })) return -1;
        if (stage(b->enc.stage[EncodePlan::ST_2], false, false)) return -1;
        if (search_costs(b, a, EncodePlan::ST_2) || search_decide(b, EncodePlan::ST_2)) return -1;      // the splits up to the third
        for (int sid : {int(EncodePlan::ST_2B), int(EncodePlan::ST_2C)})
            if (gated_stage(sid, [](const SearchImg &si) { return (si.luma_on ? 1 : 0) | (si.chroma_on ? 2 : 0); })) return -1;
        if (search_lists(b)) return -1;
        return 0;
    }

    int emit() {
        MARK(KS_SCAN_SEARCH);
        launch_layout(st, a);
        MARK(KS_LAYOUT);
        launch_exclusive_scan(st, b->out.d_img_size_pad.p, b->out.d_img_off.p, uint64_t(nimg), b->enc.d_scan_tmp.p, b->enc.d_scan_tmp.n);
        MARK(KS_SCAN_IMAGES);
        launch_emit(st, a);
        MARK(KS_EMIT);
        return 0;
    }

    int finish(bool phases) {
        CSH_CHECK(hipStreamSynchronize(st));
        CSH_CHECK(hipGetLastError());
        if (t && marks.read(t, phases)) return -1;
        if (t && !phases) t->n_images = uint32_t(nimg);
        return 0;
    }

    // the WebP tail of a run: RGB (resize branch) -> YUV 4:2:0 -> macroblocks -> tokens; files land in the batch's output pool at
    // fixed offsets (capacity per macroblock grows on overflow, like the JPEG pools)
    int webp() {
        const int nwimg = int(b->wp.wimgs.size());
        uint64_t out_bytes = 0;
        std::vector<uint64_t> off(size_t(b->nimg) + 1, 0);
        for (auto &wi : b->wp.wimgs) {
            const uint64_t cap = 4096 + uint64_t(wi.mbw) * wi.mbh * (b->wp.webp_mb_bytes + 2);
            wi.out_cap = uint32_t(std::min<uint64_t>(cap, 0xFFFFFF00u)); wi.out_off = out_bytes;
            off[wi.image] = out_bytes;
            out_bytes += (wi.out_cap + 63) & ~uint64_t(63);
            const int q = int(b->params.webp_quality);
            wi.quality = q < 0 ? 0 : q > 100 ? 100 : q;
        }
        off[b->nimg] = out_bytes;
        if (b->out.d_out.n < out_bytes + 64 && b->out.d_out.alloc(out_bytes + 64)) return -1;
        if ((b->wp.d_wscratch.n < out_bytes + 64 && b->wp.d_wscratch.alloc(out_bytes + 64)) || (b->wp.d_wpart.n < size_t(b->nimg) * 9 + 9 && b->wp.d_wpart.alloc(size_t(b->nimg) * 9 + 9)) ||
            (b->wp.d_wstats.n < size_t(b->nimg) * 2112 + 8 && (b->wp.d_wstats.alloc(size_t(b->nimg) * 2112 + 8) || b->wp.d_wprobs.alloc(size_t(b->nimg) * 1056 + 8) || b->wp.d_wupdate.alloc(size_t(b->nimg) * 1056 + 8))))
            return -1;
        if (b->wp.d_wstats.zero(st)) return -1;
        if (b->wp.d_wimgs.upload(b->wp.wimgs, st) || (b->wp.d_wwork.n < b->wp.wwork_bytes + 64 && b->wp.d_wwork.alloc(b->wp.wwork_bytes + 64)) ||
            (b->wp.d_wlevels.n < b->wp.wlevels + 64 && b->wp.d_wlevels.alloc(b->wp.wlevels + 64)))
            return -1;
        CSH_CHECK(hipMemcpyAsync(b->out.d_img_off.p, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (b->out.d_img_size.zero(st)) return -1;
        csw::launch_webp_yuv(st, b->wp.d_wimgs.p, nwimg, b->wp.wmax_luma, b->pix.d_rgb.p, b->wp.d_wwork.p);
        MARK(KS_WEBP_YUV);
        hipEvent_t mid;
        if (marks.claim(KS_WEBP_ENCODE, &mid)) return -1;
        if (csw::launch_webp_encode(st, b->wp.wimgs.data(), nwimg, b->wp.d_wimgs.p, b->wp.d_wwork.p, b->wp.d_wlevels.p, b->wp.d_wscratch.p, b->wp.d_wpart.p, b->out.d_out.p, b->out.d_img_size.p, b->out.d_status.p, mid)) return -1;
        MARK(KS_WEBP_ASSEMBLE);
        return finish(false);
    }
};

}  // namespace

int run_once(csh_batch *b, csh_timing *t, bool requant_only) {
    Run r(b, t);
    b->enc.last_run_list_runs = 0;
    b->dec.last_run_seeds = 0; b->dec.last_run_relaxed = 0; b->dec.last_run_rounds = 0;   // (a run that does not decode reports none)
    b->enc.last_run_fused = 0; b->enc.last_run_refine = 0; b->enc.last_run_ref_packed = 0; b->enc.last_run_ac_lists = 0;
    if (r.pools() || r.marks.start()) return -1;
    // a re-run at another quality (size targeting): from the retained DCT -- unless the batch derings: the overshoot mozjpeg's deringing allows
    // depends on the DC quantiser (jcdctmgr.c preprocess_deringing), so the forward DCT's input changes with the table and the re-run starts
    // at the pixel phase, from the decoded coefficients that are still in the pool
    const bool from_pixels = requant_only && b->tr.dering;
    if (requant_only && !from_pixels) {
        if (r.requant()) return -1;
    } else {
        if (from_pixels ? r.skip_decode() : r.decode()) return -1;
        if (r.planes()) return -1;
        if (b->webp) return r.webp();
        if (b->rgb_out) return (r.marks.mark(KS_XFORM_DIRECT) || r.finish(false)) ? -1 : 0;   // csh_batch_create_pixels: nothing behind the resize branch (one empty slot ends the run)
        if (r.pixels()) return -1;
    }
    if (r.encode_begin()) return -1;
    b->enc.last_run_fused = r.fused ? b->enc.n_fused : 0u;
    b->enc.last_run_ac_lists = r.fused ? b->enc.n_ac_lists : 0u;
    if (b->tr.trellis ? r.trellis() : r.marks.skip_to(KS_NZLIST)) return -1;
    r.fill_asm_ctx();
    if (r.stage(b->enc.stage[0], true, false)) return -1;
    if (b->enc.search && r.search()) return -1;
    return (r.emit() || r.finish(true)) ? -1 : 0;
}

}  // namespace csh
