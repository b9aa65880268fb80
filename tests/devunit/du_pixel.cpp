// du_pixel.cpp -- device units over caesium-clt_amd/csrc/k_pixel.hip: the block arithmetic (forward transform + quantiser in the six forms the file has,
// deringing, inverse transform), one block per lane as the kernels run it, and the packed 16-bit primitives they are written in.  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_pixel.hip"
#include "du_common.h"
using namespace csh;

// V: 0 fdct_quant_store<false, true>   1 fdct_quant_store<false, false>   2 + 2 * DERING + CENTRED: fdct_quant_store_pk<DERING, CENTRED>
// samples: level-shifted, natural order, [nblocks][64]; an uncentred form is given them + 128, as its callers do
template <int V>
__global__ void __launch_bounds__(256) k_du_fdct(const int16_t *__restrict__ samples, const DevQuant *__restrict__ quant, int16_t *__restrict__ coef, int16_t *__restrict__ raw, int nblocks) {
    CSH_SHARED int16_t s_dr[64][256];
    constexpr bool CENTRED = V < 2 ? V == 0 : ((V - 2) & 1) != 0;
    constexpr bool DERING = V >= 4;
    const int b = int(blockIdx.x * blockDim.x + threadIdx.x);
    bool has_raw = false;
    do {
        if (b >= nblocks) break;
        int x[64];
        CSH_UNROLL
        for (int i = 0; i < 64; i++) x[i] = int(samples[size_t(b) * 64 + i]) + (CENTRED ? 0 : 128);
        uint4 lv[8];
        const BlkOut o{coef, 0u, b, raw, 0u};
        if (V < 2) {
            fdct_quant_store<false, CENTRED>(x, quant[0], o, lv, s_dr);
        } else {
            uint32_t pr[8][4];
            pack_rows(x, pr);
            fdct_quant_store_pk<DERING, CENTRED>(pr, quant[0], o, lv, s_dr);
        }
        has_raw = true;
    } while (0);
    raw_copy_out(raw + raw_index(0u, b & ~63), has_raw, s_dr, int(threadIdx.x));   // every lane of the wave, as in the kernels
}

template <bool CENTRED>
__global__ void __launch_bounds__(256) k_du_idct(const int16_t *__restrict__ coef, const DevQuant *__restrict__ quant, int16_t *__restrict__ out, int nblocks) {
    const int b = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= nblocks) return;
    int x[64];
    load_idct<CENTRED>(coef + coef_index(0u, b, 0), quant[0], x);
    CSH_UNROLL
    for (int i = 0; i < 64; i++) out[size_t(b) * 64 + i] = int16_t(x[i]);
}

// op: 0 pk_add  1 pk_sub  2 pk_max  3 dot2 (acc)  4 pack_halves  5 pack_hi_halves  6..9 bytes_to_halves<0,1> <2,3> <3,2> <1,0> (of a)  10 nzf_ones (of a)
__global__ void __launch_bounds__(256) k_du_pk(int op, int n, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, const int32_t *__restrict__ acc, uint32_t *__restrict__ out) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const uint32_t x = a[i], y = b[i];
    uint32_t r = 0;
    switch (op) {
        case 0: r = pk_add(x, y); break;
        case 1: r = pk_sub(x, y); break;
        case 2: r = pk_max(x, y); break;
        case 3: r = uint32_t(dot2(x, y, acc[i])); break;
        case 4: r = pack_halves(x, y); break;
        case 5: r = pack_hi_halves(x, y); break;
        case 6: r = bytes_to_halves<0, 1>(x); break;
        case 7: r = bytes_to_halves<2, 3>(x); break;
        case 8: r = bytes_to_halves<3, 2>(x); break;
        case 9: r = bytes_to_halves<1, 0>(x); break;
        case 10: r = nzf_ones(x, 0x00010001u); break;
    }
    out[i] = r;
}

template <int V>
static void du_launch_fdct(int nthreads, int nblocks, const int16_t *s, const DevQuant *q, int16_t *coef, int16_t *raw) {
    CSH_LAUNCH(k_du_fdct<V>, dim3(unsigned((nblocks + nthreads - 1) / nthreads)), dim3(unsigned(nthreads)), 0, s, q, coef, raw, nblocks);
}

extern "C" {
// raw_out / lev_out: [nblocks][64], zig-zag order -- the retained DCT and the quantised levels as the function stored them.  nthreads: 64 or 256
int csdu_fdct(int variant, int nthreads, int nblocks, const int16_t *samples, const DevQuant *q, int16_t *raw_out, int16_t *lev_out) {
    if (variant < 0 || variant > 5 || (nthreads != 64 && nthreads != 256) || nblocks <= 0) return -1;
    const size_t ntiles = size_t(nblocks + 63) / 64, nround = ntiles * 64;
    DuBufs B;
    int16_t *d_s, *d_coef, *d_raw;
    DevQuant *d_q;
    DU_TRY(B.upload(&d_s, samples, size_t(nblocks) * 64 * 2));
    DU_TRY(B.upload(&d_q, q, sizeof(DevQuant)));
    DU_TRY(B.zeroed(&d_coef, ntiles * CSH_TILE_I16 * 2, 0x55));
    DU_TRY(B.zeroed(&d_raw, nround * 64 * 2, 0x55));
    switch (variant) {
        case 0: du_launch_fdct<0>(nthreads, nblocks, d_s, d_q, d_coef, d_raw); break;
        case 1: du_launch_fdct<1>(nthreads, nblocks, d_s, d_q, d_coef, d_raw); break;
        case 2: du_launch_fdct<2>(nthreads, nblocks, d_s, d_q, d_coef, d_raw); break;
        case 3: du_launch_fdct<3>(nthreads, nblocks, d_s, d_q, d_coef, d_raw); break;
        case 4: du_launch_fdct<4>(nthreads, nblocks, d_s, d_q, d_coef, d_raw); break;
        default: du_launch_fdct<5>(nthreads, nblocks, d_s, d_q, d_coef, d_raw); break;
    }
    DU_TRY(du_finish());
    int16_t *tiles = static_cast<int16_t *>(malloc(ntiles * CSH_TILE_I16 * 2));
    if (!tiles) return -2;
    int e = du_download(tiles, d_coef, ntiles * CSH_TILE_I16 * 2);
    if (e == 0) e = du_download(raw_out, d_raw, size_t(nblocks) * 64 * 2);
    if (e == 0)
        for (int b = 0; b < nblocks; b++) for (int k = 0; k < 64; k++) lev_out[size_t(b) * 64 + k] = tiles[coef_index(0u, b, k)];
    free(tiles);
    return e;
}
// coef_zz: [nblocks][64] zig-zag; out: [nblocks][64] natural order, the samples as load_idct<CENTRED> leaves them
int csdu_idct(int centred, int nthreads, int nblocks, const int16_t *coef_zz, const DevQuant *q, int16_t *out) {
    if ((nthreads != 64 && nthreads != 256) || nblocks <= 0) return -1;
    const size_t ntiles = size_t(nblocks + 63) / 64;
    int16_t *tiles = static_cast<int16_t *>(calloc(ntiles * CSH_TILE_I16, 2));
    if (!tiles) return -2;
    for (int b = 0; b < nblocks; b++) for (int k = 0; k < 64; k++) tiles[coef_index(0u, b, k)] = coef_zz[size_t(b) * 64 + k];
    DuBufs B;
    int16_t *d_coef = nullptr, *d_out = nullptr;
    DevQuant *d_q = nullptr;
    int e = B.upload(&d_coef, tiles, ntiles * CSH_TILE_I16 * 2);
    free(tiles);
    if (e) return e;
    DU_TRY(B.upload(&d_q, q, sizeof(DevQuant)));
    DU_TRY(B.zeroed(&d_out, size_t(nblocks) * 64 * 2, 0x55));
    const dim3 grid(unsigned((nblocks + nthreads - 1) / nthreads)), block{unsigned(nthreads)};
    if (centred) CSH_LAUNCH(k_du_idct<true>, grid, block, 0, d_coef, d_q, d_out, nblocks);
    else CSH_LAUNCH(k_du_idct<false>, grid, block, 0, d_coef, d_q, d_out, nblocks);
    DU_TRY(du_finish());
    return du_download(out, d_out, size_t(nblocks) * 64 * 2);
}
int csdu_pk(int op, int n, const uint32_t *a, const uint32_t *b, const int32_t *acc, uint32_t *out) {
    if (op < 0 || op > 10 || n <= 0) return -1;
    DuBufs B;
    uint32_t *d_a, *d_b, *d_o;
    int32_t *d_c;
    DU_TRY(B.upload(&d_a, a, size_t(n) * 4));
    DU_TRY(B.upload(&d_b, b, size_t(n) * 4));
    DU_TRY(B.upload(&d_c, acc, size_t(n) * 4));
    DU_TRY(B.zeroed(&d_o, size_t(n) * 4, 0x55));
    CSH_LAUNCH(k_du_pk, dim3(unsigned((n + 255) / 256)), dim3(256), 0, op, n, d_a, d_b, d_c, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, size_t(n) * 4);
}
// the table as the kernels take it, from natural-order values (the fields the block functions read: q, div, rcp -- types.h DevQuant)
size_t csdu_sizeof_devquant() { return sizeof(DevQuant); }
void csdu_make_quant(const uint16_t nat[64], DevQuant *q) {
    memset(q, 0, sizeof *q);
    for (int k = 0; k < 64; k++) { q->q[k] = nat[kZ2N[k]]; q->div[k] = int32_t(q->q[k]) * 8; q->rcp[k] = float((1.0 / double(q->div[k])) * (1.0 + 1.0 / 524288.0)); }
}
}
