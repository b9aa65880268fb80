// du_entropy.cpp -- device units over caesium-clt_amd/csrc/k_entropy.hip: its DPP scans (wave_scan_dpp with + and |, wave_incl_scan), wave_or64, wave_last
// and pk_abs16, and the whole of k_gen_tables through its launcher.  In the scan units a thread is a lane in both builds.  wave_scan_dpp and wave_last exist in the product build only (the emulation, whose lanes run one
// after the other, has nothing to put there): their entries answer CSDU_DEVICE_ONLY from the emulation build.  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_entropy.hip"
#include "du_common.h"
using namespace csh;
#define CSDU_DEVICE_ONLY (-100)

// op: 0 wave_scan_dpp +   1 wave_scan_dpp |   2 wave_incl_scan(the wave's 64 words, lane)   3 wave_last(v)   4 wave_last(wave_incl_sum(v)): the total over the
// active lanes.  Thread i of the grid takes in[i]; n: the number of threads launched (3 and 4: any workgroup size, so that a last wave is partly filled).
__global__ void __launch_bounds__(256) k_du_escan(int op, const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t r = 0;
    if (op == 2) r = wave_incl_scan(in + (i & ~63u), lane_id());
#ifndef CSH_EMUL
    else if (op == 0) r = wave_scan_dpp(in[i], [](uint32_t a, uint32_t b) { return a + b; });
    else if (op == 1) r = wave_scan_dpp(in[i], [](uint32_t a, uint32_t b) { return a | b; });
    else if (op == 3) r = wave_last(in[i]);
    else if (op == 4) r = wave_last(wave_incl_sum(in[i]));
#endif
    out[i] = r;
}
__global__ void __launch_bounds__(256) k_du_or64(const uint64_t *__restrict__ in, uint64_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = wave_or64(in[i]);
}
__global__ void __launch_bounds__(256) k_du_abs16(int n, const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) out[i] = pk_abs16(in[i]);
}

extern "C" {
// in / out: [nblocks * nthreads].  ops 0..2 want whole waves (nthreads 64 or 256); 3 and 4 take any nthreads <= 256
int csdu_escan(int op, int nblocks, int nthreads, const uint32_t *in, uint32_t *out) {
    if (op < 0 || op > 4 || nblocks <= 0 || nthreads <= 0 || nthreads > 256 || (op <= 2 && nthreads != 64 && nthreads != 256)) return -1;
#ifdef CSH_EMUL
    if (op != 2) return CSDU_DEVICE_ONLY;
#endif
    DuBufs B;
    uint32_t *d_in, *d_o;
    const size_t n = size_t(nblocks) * nthreads, nb = n * 4;
    DU_TRY(B.upload(&d_in, in, nb));
    DU_TRY(B.zeroed(&d_o, nb, 0x55));
    CSH_LAUNCH(k_du_escan, dim3(unsigned(nblocks)), dim3(unsigned(nthreads)), 0, op, d_in, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, nb);
}
int csdu_or64(int nblocks, int nthreads, const uint64_t *in, uint64_t *out) {
    if (nblocks <= 0 || (nthreads != 64 && nthreads != 256)) return -1;
    DuBufs B;
    uint64_t *d_in, *d_o;
    const size_t nb = size_t(nblocks) * nthreads * 8;
    DU_TRY(B.upload(&d_in, in, nb));
    DU_TRY(B.zeroed(&d_o, nb, 0x55));
    CSH_LAUNCH(k_du_or64, dim3(unsigned(nblocks)), dim3(unsigned(nthreads)), 0, d_in, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, nb);
}
int csdu_abs16(int n, const uint32_t *in, uint32_t *out) {
    if (n <= 0) return -1;
    DuBufs B;
    uint32_t *d_in, *d_o;
    DU_TRY(B.upload(&d_in, in, size_t(n) * 4));
    DU_TRY(B.zeroed(&d_o, size_t(n) * 4, 0x55));
    CSH_LAUNCH(k_du_abs16, dim3(unsigned((n + 255) / 256)), dim3(256), 0, n, d_in, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, size_t(n) * 4);
}
// k_gen_tables as the pipeline launches it: a wave per table, four to a workgroup (the last one partly filled unless ntables % 4 == 0).  tables: in, freq[0..255]
// (the kernel sets freq[256] itself); out, everything behind it.  The struct is the library's own: the caller checks its layout against csdu_sizeof_enctable().
size_t csdu_sizeof_enctable() { return sizeof(DevEncTable); }
int csdu_gen_tables(int ntables, DevEncTable *tables) {
    if (ntables <= 0) return -1;
    DuBufs B;
    DevEncTable *d_t;
    const size_t nb = size_t(ntables) * sizeof(DevEncTable);
    DU_TRY(B.upload(&d_t, tables, nb));
    launch_gen_tables(0, d_t, ntables);
    DU_TRY(du_finish());
    return du_download(tables, d_t, nb);
}
}
