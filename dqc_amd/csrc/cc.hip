// cc.hip -- the particle-particle ladder of coupled-cluster doubles with density-fitted integrals, integral-driven and fused: every tile
// of the four-index quantity W is summed over the auxiliary index once, in MFMA accumulators, handed to the second product through LDS
// and used by every vector of the block's vector panel.  No element of W reaches global memory.
//
//     out[v, p, q] = sum_{r < nr} sum_{s < ns} W[p, q, r, s] X[v, r, s],      W[p, q, r, s] = sum_P L[p, P, r] R[q, P, s]
//
// LAYOUTS.  L[p, P, r]: one (naux, ldr) slab per p, R[q, P, s]: one (naux, lds) slab per q, ldr and lds the counts nr and ns padded to a
// multiple of 16 (what transform_ov makes); L and R may be one tensor or two.  X is (nr, ns, nvec): THE VECTOR INDEX LAST, so that the
// 16 vectors of an A-operand row are one run of 128 bytes.  out is (nvec, np, nq), plain contiguous.
//
// One block (eight waves) owns one p, one tile of CC_QW = 16 columns q and a panel of vectors: wave w holds up to CC_NVT = 9 vector
// tiles of 16, nine accumulators of v_mfma_f64_16x16x4_f64 (72 registers); a block takes 8 x 9 x 16 = 1152 vectors, a launch of more
// splits them into equal panels (and builds W once per panel).  Two column tiles per block (half the reads of X) spilled: LOG_r33.md.
// A round is one tile of 16 rows r times one tile of 16 columns s:
//   build  wave w sums the two tiles C_q[r, s] = sum_P L[p, P, r] R[q, P, s], q = q0 + 2 w, q0 + 2 w + 1, over ALL P: A[i = r][k = P] and
//          B[k = P][j = s] are runs of 16 doubles of a slab row, loaded straight from global memory (the L fragment serves both
//          tiles), two k-steps ahead of the MFMAs.  The tiles go to LDS as they lie in the registers, [q][reg][lane].
//   use    out[v, q] += sum_r X[v, r, s] C_q[r, s] for each s of the tile: A[i = v][k = r] = X[r, s, v] from global memory, B[k = r][j = q]
//          is register reg = (r >> 2) of the tile of column q at the lane (r & 3, s) -- read from LDS across the 16 tiles of the block.
// LDS: a tile is 256 doubles at stride CC_TS = 257.  Written [reg][lane]: consecutive.  Read at l15 257 + 64 reg + 16 q4 + s:
// the 32 lanes of a half (l15 = 0 ... 15, q4 = 0, 1 or 2, 3) touch 32 different 8-byte banks: conflict-free with ds_read_b64.
// Padding: rows r >= nr, columns s >= ns and q >= nq, auxiliary functions past naux and vectors past nvec are SELECTED to 0.0 without
// being loaded, and nothing past np, nq, nvec is stored: whatever the padding columns of the slabs hold, it changes no bit.
// No atomics, no split sum: every element of out is written once, by one lane, which adds its terms in a fixed order (r tiles, s tiles,
// s, r).  Bit-reproducible as it stands.  The work buffer of the C ABI is empty (dqc_cc_ladder_work_doubles is 0).
//
// Count: 2 np nq nr ns (panels naux + nvec) flops.  Per round and wave 2 ceil(naux / 4) MFMAs build and up to 9 x 64 use; the build
// loads 12 bytes per lane and MFMA, the use 8.  Registers and measurements: docs/LOG_r33.md.
#include <algorithm>

#include "common.hpp"
#include "mfma_tile.hpp"

namespace dqc {

constexpr int CC_NT = 512;   // threads: eight waves
constexpr int CC_NW = CC_NT / 64;
constexpr int CC_QW = 16;    // columns q of a block
constexpr int CC_QT = CC_QW / 16;     // accumulator column tiles per wave and vector tile
constexpr int CC_QB = CC_QW / CC_NW;  // W tiles (columns q) a wave builds per round
constexpr int CC_NVT = 9;    // vector tiles per wave
constexpr int CC_VP = CC_NW * CC_NVT * 16;   // vectors per block at most
constexpr int CC_TS = 257;   // LDS stride of a W tile in doubles

struct CcArgs {
    const double *l, *r, *x;
    double *out;
    int np, nq, nr, ns, ldr, lds, naux, nvec;
    int nqp;             // column panels
    int ntiles, tpp, pw; // vector tiles, vector tiles per panel, vector tiles per wave
};

__global__ __launch_bounds__(CC_NT, 2) void cc_ladder_kernel(CcArgs g) {
    __shared__ double s_w[CC_QW * CC_TS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, q4 = lane >> 4;
    long long b = blockIdx.x;
    const int p = (int)(b % g.np);
    b /= g.np;
    const int qp = (int)(b % g.nqp), vp = (int)(b / g.nqp);
    const int q0 = CC_QW * qp;
    const int tile0 = vp * g.tpp + wave * g.pw;                                                    // this wave's first vector tile
    const int nvt = max(0, min(g.pw, min(g.tpp, g.ntiles - vp * g.tpp) - wave * g.pw));            // its live vector tiles (wave-uniform)
    const int nrt = (g.nr + 15) >> 4, nst = (g.ns + 15) >> 4;
    const double *lp = g.l + (size_t)p * g.naux * g.ldr;
    v4d acc[CC_NVT][CC_QT];
#pragma unroll
    for (int t = 0; t < CC_NVT; t++)
#pragma unroll
        for (int c = 0; c < CC_QT; c++) acc[t][c] = v4d{0.0, 0.0, 0.0, 0.0};

    for (int rt = 0; rt < nrt; rt++) {
        for (int st = 0; st < nst; st++) {
            const int r0 = 16 * rt, s0 = 16 * st;
            const bool rlive = r0 + l15 < g.nr, slive = s0 + l15 < g.ns;
            // ---- build: one k-step (four P) per fetch, two fetches in flight under the MFMAs of a third
            const double *pa = lp + (size_t)q4 * g.ldr + r0 + l15;
            const double *pb = g.r + ((size_t)(q0 + CC_QB * wave) * g.naux + q4) * g.lds + s0 + l15;
            const size_t qstride = (size_t)g.naux * g.lds;
            auto fetch = [&](int P0, double (&f)[1 + CC_QB]) {
                const bool ok = P0 + q4 < g.naux;
                f[0] = (ok && rlive) ? pa[(size_t)P0 * g.ldr] : 0.0;
#pragma unroll
                for (int j = 0; j < CC_QB; j++)
                    f[1 + j] = (ok && slive && q0 + CC_QB * wave + j < g.nq) ? pb[j * qstride + (size_t)P0 * g.lds] : 0.0;
            };
            v4d w[CC_QB];
#pragma unroll
            for (int j = 0; j < CC_QB; j++) w[j] = v4d{0.0, 0.0, 0.0, 0.0};
            auto mm = [&](const double (&f)[1 + CC_QB]) {
#pragma unroll
                for (int j = 0; j < CC_QB; j++) w[j] = mfma_f64(f[0], f[1 + j], w[j]);
            };
            {
                double f0[1 + CC_QB], f1[1 + CC_QB], f2[1 + CC_QB];
                fetch(0, f0);
                fetch(4, f1);
                for (int P0 = 0; P0 < g.naux; P0 += 12) {
                    fetch(P0 + 8, f2);
                    mm(f0);
                    fetch(P0 + 12, f0);
                    if (P0 + 4 < g.naux) mm(f1);
                    fetch(P0 + 16, f1);
                    if (P0 + 8 < g.naux) mm(f2);
                }
            }
            // ---- use: A[i = v][k = r] = X[r0 + 4 reg + q4, s, v]; the step it = 4 (s - s0) + reg
            const int nit = 4 * min(16, g.ns - s0);
            auto xfetch = [&](int it, double (&xv)[CC_NVT]) {
                const int s = s0 + (it >> 2), r = r0 + 4 * (it & 3) + q4;
                const bool ok = it < nit && r < g.nr;
                const double *xp = g.x + ((size_t)r * g.ns + s) * g.nvec;
#pragma unroll
                for (int t = 0; t < CC_NVT; t++) {
                    const int v = 16 * (tile0 + t) + l15;
                    xv[t] = (ok && t < nvt && v < g.nvec) ? xp[v] : 0.0;
                }
            };
            auto xuse = [&](int it, const double (&xv)[CC_NVT]) {
                const int o = 64 * (it & 3) + 16 * q4 + (it >> 2);
                double bw[CC_QT];
#pragma unroll
                for (int c = 0; c < CC_QT; c++) bw[c] = s_w[(16 * c + l15) * CC_TS + o];
#pragma unroll
                for (int t = 0; t < CC_NVT; t++) {
                    if (t >= nvt) continue;
#pragma unroll
                    for (int c = 0; c < CC_QT; c++) acc[t][c] = mfma_f64(xv[t], bw[c], acc[t][c]);
                }
            };
            double xa[CC_NVT], xb[CC_NVT];
            xfetch(0, xa);
            __syncthreads();   // (the tiles of the previous round have been read by every wave)
#pragma unroll
            for (int j = 0; j < CC_QB; j++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) s_w[(CC_QB * wave + j) * CC_TS + 64 * reg + lane] = w[j][reg];
            __syncthreads();
            for (int it = 0; it < nit; it += 2) {
                xfetch(it + 1, xb);
                xuse(it, xa);
                xfetch(it + 2, xa);
                xuse(it + 1, xb);
            }
        }
    }
    // lane (l15, q4), register reg of acc[t][c] holds the vector 16 (tile0 + t) + q4 + 4 reg at the column q0 + 16 c + l15
#pragma unroll
    for (int t = 0; t < CC_NVT; t++) {
        if (t >= nvt) continue;
#pragma unroll
        for (int c = 0; c < CC_QT; c++) {
            const int q = q0 + 16 * c + l15;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int v = 16 * (tile0 + t) + q4 + 4 * reg;
                if (v < g.nvec && q < g.nq) g.out[((size_t)v * g.np + p) * g.nq + q] = acc[t][c][reg];
            }
        }
    }
}

// (column panels, vector panels, vector tiles, vector tiles per panel and per wave) of a launch of non-negative counts; false: the
// output has more elements than a 64-bit count holds
static bool cc_counts(int np, int nq, int nvec, long long &nqp, long long &nvp, int &ntiles, int &tpp, int &pw) {
    if ((double)nvec * (double)np * (double)nq > 4e18) return false;
    nqp = (nq + CC_QW - 1) / CC_QW;
    ntiles = (int)(((long long)nvec + 15) / 16);
    nvp = ((long long)nvec + CC_VP - 1) / CC_VP;
    tpp = nvp ? (int)((ntiles + nvp - 1) / nvp) : 0;   // equal panels: no panel of a few vectors pays for a whole W
    pw = (tpp + CC_NW - 1) / CC_NW;
    return true;
}

}  // namespace dqc

extern "C" {

size_t dqc_cc_ladder_work_doubles(int np, int nq, int nr, int ns, int naux, int nvec) {
    (void)np, (void)nq, (void)nr, (void)ns, (void)naux, (void)nvec;
    return 0;   // no sum is split over blocks: nothing is staged in global memory
}

int dqc_cc_ladder(double *d_out, const double *d_l, const double *d_r, const double *d_x, int np, int nq, int nr, int ns, int ldr, int lds,
                  int naux, int nvec, double *d_work, void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    (void)d_work;
    long long nqp, nvp;
    int ntiles, tpp, pw;
    if (np < 0 || nq < 0 || nr < 0 || ns < 0 || ldr < 0 || lds < 0 || naux < 0 || nvec < 0) { set_error("dqc_cc_ladder: negative count"); return DQC_EINVAL; }
    if (ldr % 16 || ldr < nr) { set_error("dqc_cc_ladder: ldr must be a multiple of 16 and at least nr"); return DQC_EINVAL; }
    if (lds % 16 || lds < ns) { set_error("dqc_cc_ladder: lds must be a multiple of 16 and at least ns"); return DQC_EINVAL; }
    if (!cc_counts(np, nq, nvec, nqp, nvp, ntiles, tpp, pw)) { set_error("dqc_cc_ladder: more blocks than one launch holds"); return DQC_EINVAL; }
    const size_t out = (size_t)nvec * (size_t)np * (size_t)nq;
    if (out == 0) return DQC_OK;  // (empty output)
    if (!d_out) { set_error("dqc_cc_ladder: null output"); return DQC_EINVAL; }
    if (naux == 0 || nr == 0 || ns == 0) {   // an empty sum: zeros
        DQC_HIP(hipMemsetAsync(d_out, 0, sizeof(double) * out, st));
        return DQC_OK;
    }
    if (!d_l || !d_r || !d_x) { set_error("dqc_cc_ladder: null pointer argument"); return DQC_EINVAL; }
    const long long nblk = (long long)np * nqp * nvp;
    if (nblk > 2147483647LL) { set_error("dqc_cc_ladder: more blocks than one launch holds"); return DQC_EINVAL; }
    CcArgs g{d_l, d_r, d_x, d_out, np, nq, nr, ns, ldr, lds, naux, nvec, (int)nqp, ntiles, tpp, pw};
    hipLaunchKernelGGL(cc_ladder_kernel, dim3((unsigned)nblk), dim3(CC_NT), 0, st, g);
    DQC_CHECK_LAUNCH();
    return DQC_OK;
}

}  // extern "C"
