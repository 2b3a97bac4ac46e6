// gw.hip -- the diagonal of the screened interaction between orbital pairs on a grid of imaginary frequencies, fused: the intermediate
// Y = Wc B never leaves the registers.
//
//     W[k, n, m] = sum_{P, R} Bn[n, P, m] Wc[k][P, R] Bn[n, R, m]      ( = (n m| Wc(i w_k) |m n), the G0W0 self-energy needs no more )
//
// Bn[n, P, m]: one (naux, ldm) slab per target orbital n, ldm the orbital count padded to a multiple of 16 (what mp2.transform_ov makes);
// Wc[k]: (naux, naux), symmetric, of which ONLY the elements P >= R are ever read:
//
//     W[k, n, m] = sum_P Bn[n, P, m] Y[P, m],      Y[P, m] = sum_{R <= P} c_PR Wc[k][P, R] Bn[n, R, m],   c_PR = 2 (R < P), 1 (R = P)
//
// One block (eight waves) owns one frequency k and one tile of 128 columns (n, m0 ... m0 + 127), eight MFMA tiles of 16 columns.  It
// sweeps the row panels Pp of 128 rows; wave w owns tile row P = 8 Pp + w and the eight accumulators Y[16 rows][8 x 16 columns] of
// v_mfma_f64_16x16x4_f64 (64 VGPRs).  The sum over R runs in chunks of GW_KC = 32 from 0 to the end of the diagonal panel: the block
// stages the 128 x 32 block of Wc [row][k] and the 32 x 128 block of Bn [k][column] in LDS (each element read from memory once per
// block; the next chunk is asked for before the MFMAs of this one and stored after them into a second pair of buffers: 64 KB in flight
// per block under 4096 cycles of MFMAs per wave, one barrier per chunk).  The weight c_PR is applied when the Wc block is staged -- a multiplication by two is exact, so this is the sum
// with doubled off-diagonal accumulators bit for bit, with one loop for both kinds of panel -- and the elements R > P are staged as
// 0.0 without being loaded.  In the diagonal panel a wave skips the chunks, and in its own chunk the k-steps, that lie wholly above its
// rows; the chunk that holds its own rows P is the last one it needs, and IS the staged Bn[P, m] of the row dot: the lane reads its
// values [row q + 4 r][column 16 t + l15] from the same LDS block, adds Bn[P, m] Y[P, m] to its eight per-column partial sums and
// clears the accumulators.
// LDS: Wc rows at stride 34 doubles (== 2 mod 32), the fragment read [row = lane & 15][k = lane >> 4] of a 32-lane half touches 32
// different 8-byte banks (the argument in the header of rpa.hip); Bn rows at stride 144 doubles (== 16 mod 32), the other operand
// orientation [k = lane >> 4][column = lane & 15]: the two k rows of a half sit 16 banks apart (mp2_pair_kernel) -- both conflict-free
// with ds_read_b64.  Wc[k] has no alignment to offer (naux is any number): its rows are read as single doubles, 32 consecutive per 32
// lanes (a wave instruction: two rows of 256 contiguous bytes).
// Epilogue: the partial sums of the four row groups of a wave and of the eight waves meet in LDS (the Wc block's memory) and one
// thread per column adds the 32 of them in a fixed order.  Every element of W is written once, by one lane: no atomics,
// bit-reproducible.
// Blocks are ordered frequency-major: the column tiles of one frequency are adjacent, so the blocks in flight share one Wc[k] (10.7 MB
// at naux 1156: more than an XCD's L2, resident in the Infinity Cache).
// Padding: columns m >= nm are staged as 0.0 (selected, not multiplied) and never stored, rows P, R >= naux are staged as 0.0 without
// being loaded.  Whatever the padding holds, it contributes exactly zero.
//
// Tile: 128 rows x 128 columns x 32 -- 16 flop per byte staged.  The first version (64 x 64 x 16, four waves, 8 flop per byte, one
// chunk of 1024 MFMA cycles to hide a load under) waited on memory: 13 % of the fp64 MFMA rate, a third of the speed of the library
// route.  This one still does -- 31 to 35 % of the MFMA rate: 1.24 x the library route on ten target orbitals, 0.86 x on all 208 of
// the 20-atom molecule (docs/LOG_r24.md has the measurements and what is left to try).
#include "common.hpp"
#include "mfma_tile.hpp"

namespace dqc {

constexpr int GW_KC = 32;    // R per LDS chunk
constexpr int GW_PW = 128;   // row panel (eight tiles, one per wave)
constexpr int GW_CW = 128;   // column tile (eight tiles)
constexpr int GW_NT = 512;   // threads
constexpr int GW_WS = 34;    // LDS stride of the Wc rows in doubles
constexpr int GW_BS = 144;   // LDS stride of the Bn rows in doubles
constexpr int GW_CT = GW_CW / 16, GW_CPP = GW_PW / GW_KC;   // column tiles per wave, chunks per panel

struct GwArgs {
    const double *wc, *bn;
    double *w;
    int ntarget, nm, ldm, naux, nfreq;
    int nct;   // column tiles per target orbital: ceil(nm / 128)
    int np;    // row panels: ceil(naux / 128)
    int nrc;   // chunks of 32 rows: ceil(naux / 32)
};

// the MFMAs of one chunk for a wave: NL live column tiles, the whole chunk (unrolled) or its first klim rows.  swr: the lane's Wc row
// [row l15][q], sbc: the lane's Bn column [q][l15].  No branch inside a k-step: with one (a tile past nm, a k-step past the diagonal)
// the compiler waits for every LDS read right in front of its MFMA (1 % here, where the kernel waits on memory: docs/LOG_r24.md).
template <int NL, bool WHOLE>
DQC_DEV void gw_chunk(v4d (&acc)[GW_CT], const double *swr, const double *sbc, int klim) {
    auto step = [&](int k0) {
        const double a = swr[k0];
        double b[NL];
#pragma unroll
        for (int t = 0; t < NL; t++) b[t] = sbc[k0 * GW_BS + 16 * t];
#pragma unroll
        for (int t = 0; t < NL; t++) acc[t] = mfma_f64(a, b[t], acc[t]);
    };
    if constexpr (WHOLE) {
#pragma unroll
        for (int k0 = 0; k0 < GW_KC; k0 += 4) step(k0);
    } else {
        for (int k0 = 0; k0 < klim; k0 += 4) step(k0);
    }
}
#define GW_CASE(NL)                                                  \
    case NL:                                                         \
        if (klim == GW_KC) gw_chunk<NL, true>(acc, swr, sbc, klim);  \
        else gw_chunk<NL, false>(acc, swr, sbc, klim);               \
        break;

__global__ __launch_bounds__(GW_NT, 2) void gw_screened_diag_kernel(GwArgs g) {
    // two buffers each (140 KB of the CU's 160 KB: one block per CU, which the 234 VGPRs of its eight waves allow anyway)
    __shared__ __align__(16) double s_w[2 * GW_PW * GW_WS];     // [P][R] of the chunk, weighted; after the sweep: [wave][row group][column]
    __shared__ __align__(16) double s_b[2 * GW_KC * GW_BS];     // [R][column] of the chunk
    static_assert(8 * 4 * GW_CW <= GW_PW * GW_WS, "the partial sums reuse the Wc block");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
    const long long per = (long long)g.ntarget * g.nct;
    const int k = (int)(blockIdx.x / per);
    const long long rem = blockIdx.x - (long long)k * per;
    const int n = (int)(rem / g.nct), m0 = GW_CW * (int)(rem - (long long)n * g.nct);
    const size_t na = (size_t)g.naux;
    const double *wck = g.wc + (size_t)k * na * na;
    const double *slab = g.bn + (size_t)n * na * g.ldm;
    const int nlive = min(GW_CT, (g.nm - m0 + 15) >> 4);   // column tiles that hold a real column: t < nlive
    v4d acc[GW_CT];
    double part[GW_CT];
#pragma unroll
    for (int t = 0; t < GW_CT; t++) {
        acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
        part[t] = 0.0;
    }

    // the staging map: Wc 128 rows x 32 doubles, eight per thread; Bn 32 rows x 64 double2, four per thread
    double nw[8];
    double2 nb[4];
    auto fetch = [&](int pp, int ch) {
        const int r0 = GW_KC * ch;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = threadIdx.x + GW_NT * u, p = GW_PW * pp + (e >> 5), r = r0 + (e & 31);
            double v = 0.0;
            if (p < g.naux && r <= p) {   // (r <= p < naux: the upper triangle is never read)
                v = wck[(size_t)p * na + r];
                v = r < p ? 2.0 * v : v;
            }
            nw[u] = v;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = threadIdx.x + GW_NT * u, r = r0 + (e >> 6), m = m0 + (e & 63) * 2;
            double2 v{0.0, 0.0};
            if (r < g.naux && m < g.ldm) v = *reinterpret_cast<const double2 *>(slab + (size_t)r * g.ldm + m);   // (m + 1 < ldm: whole 16s)
            nb[u] = double2{m < g.nm ? v.x : 0.0, m + 1 < g.nm ? v.y : 0.0};
        }
    };
    auto store = [&](int buf) {
        double *sw = s_w + buf * (GW_PW * GW_WS), *sb = s_b + buf * (GW_KC * GW_BS);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = threadIdx.x + GW_NT * u;
            sw[(e >> 5) * GW_WS + (e & 31)] = nw[u];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = threadIdx.x + GW_NT * u;
            *reinterpret_cast<double2 *>(&sb[(e >> 6) * GW_BS + (e & 63) * 2]) = nb[u];
        }
    };
    const int dch = wave >> 1, drow = 16 * (wave & 1);       // in a diagonal panel: the chunk that holds this wave's rows, and where
    int pp = 0, ch = 0, buf = 0;
    if (g.np > 0) {
        fetch(0, 0);
        store(0);
    }
    __syncthreads();
    while (pp < g.np) {
        // the chunk after this one: asked for now, stored into the other buffer after the MFMAs (every wave left that buffer before the
        // barrier that ended the previous chunk), one barrier per chunk
        int npp = pp, nch = ch + 1;
        if (nch == min(GW_CPP * (pp + 1), g.nrc)) {          // (chunks run up to the end of the diagonal panel)
            npp = pp + 1;
            nch = 0;
        }
        const bool more = npp < g.np;
        if (more) fetch(npp, nch);
        const double *sw = s_w + buf * (GW_PW * GW_WS), *sb = s_b + buf * (GW_KC * GW_BS);
        const int jd = ch - GW_CPP * pp;                     // >= 0: chunk jd of the diagonal panel
        // (wave-uniform) this wave's tile row holds a real row, and the chunk does not lie wholly above it (staged zeros)
        if (16 * (8 * pp + wave) < g.naux && jd <= dch) {
            const int klim = jd == dch ? drow + 16 : GW_KC;  // (the k-steps past this wave's rows are staged zeros too)
            const double *swr = sw + (16 * wave + l15) * GW_WS + q, *sbc = sb + q * GW_BS + l15;
            switch (nlive) {   // (block-uniform: branch-free bodies, so that the LDS reads of a chunk run ahead of its MFMAs)
                GW_CASE(1) GW_CASE(2) GW_CASE(3) GW_CASE(4) GW_CASE(5) GW_CASE(6) GW_CASE(7) GW_CASE(8)
            }
            if (jd == dch) {   // the staged rows hold this wave's P: lane (l15, q), register r holds row drow + q + 4 r, column 16 t + l15
#pragma unroll
                for (int t = 0; t < GW_CT; t++) {
                    if (t >= nlive) break;
#pragma unroll
                    for (int r = 0; r < 4; r++) part[t] += sb[(drow + q + 4 * r) * GW_BS + 16 * t + l15] * acc[t][r];
                    acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
                }
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
        pp = npp;
        ch = nch;
    }
    // the 32 partial sums of a column in a fixed order (every wave has left both buffers)
    double *s_red = s_w;
#pragma unroll
    for (int t = 0; t < GW_CT; t++) s_red[(wave * 4 + q) * GW_CW + 16 * t + l15] = part[t];
    __syncthreads();
    if (threadIdx.x < GW_CW) {
        double s = 0.0;
#pragma unroll
        for (int x = 0; x < 32; x++) s += s_red[x * GW_CW + threadIdx.x];
        const int m = m0 + threadIdx.x;
        if (m < g.nm) g.w[((size_t)k * g.ntarget + n) * g.nm + m] = s;
    }
}

}  // namespace dqc

extern "C" {

int dqc_gw_screened_diag(double *d_w, const double *d_wc, const double *d_bn, int ntarget, int nm, int ldm, int naux, int nfreq,
                         void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    if (ntarget < 0 || nm < 0 || ldm < 0 || naux < 0 || nfreq < 0) { set_error("dqc_gw_screened_diag: negative count"); return DQC_EINVAL; }
    if (ldm % 16 || ldm < nm) { set_error("dqc_gw_screened_diag: ldm must be a multiple of 16 and at least nm"); return DQC_EINVAL; }
    const size_t out = (size_t)nfreq * (size_t)ntarget * (size_t)nm;
    if (out == 0) return DQC_OK;  // (empty output)
    if (!d_w) { set_error("dqc_gw_screened_diag: null output"); return DQC_EINVAL; }
    if (naux == 0) {              // an empty sum: zeros
        DQC_HIP(hipMemsetAsync(d_w, 0, sizeof(double) * out, st));
        return DQC_OK;
    }
    if (!d_wc || !d_bn) { set_error("dqc_gw_screened_diag: null pointer argument"); return DQC_EINVAL; }
    if ((size_t)d_bn % 16) { set_error("dqc_gw_screened_diag: the tensor must be 16-byte aligned"); return DQC_EINVAL; }
    const int nct = (nm + GW_CW - 1) / GW_CW;
    const long long nblk = (long long)nfreq * ntarget * nct;
    if (nblk > 2147483647LL) { set_error("dqc_gw_screened_diag: more blocks than one launch holds"); return DQC_EINVAL; }
    GwArgs g{d_wc, d_bn, d_w, ntarget, nm, ldm, naux, nfreq, nct, (naux + GW_PW - 1) / GW_PW, (naux + GW_KC - 1) / GW_KC};
    hipLaunchKernelGGL(gw_screened_diag_kernel, dim3((unsigned)nblk), dim3(GW_NT), 0, st, g);
    DQC_CHECK_LAUNCH();
    return DQC_OK;
}

}  // extern "C"
