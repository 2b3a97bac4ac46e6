// bse.hip -- the product of a block of trial vectors with a four-index quantity held as two density-fitted factors (the screened
// direct and exchange terms of the Bethe-Salpeter equation), fused: the intermediate Z_P = X_v R_P^T never leaves the registers.
//
//     out[v, p, q] = sum_P sum_{r < nr} sum_{s < ns} L[p, P, r] X[v, r, s] R[q, P, s]
//
// L[p, P, r]: one (naux, ldr) slab per p, R[q, P, s]: one (naux, lds) slab per q, ldr and lds the counts nr and ns padded to a multiple
// of 16 (what transform_ov makes); X (nvec, nr, ns) and out (nvec, np, nq) plain contiguous.  Per auxiliary function P two chained
// products: Z[r, q] = sum_s X[r, s] R[q, P, s], then out[p, q] += sum_r L[p, P, r] Z[r, q].
//
// One block (four waves) owns BSE_NV = 2 trial vectors, one panel of 64 rows p, one panel of 64 columns q and one slot of the sum
// over P; wave w owns the 16 columns q0 + 16 w ... of it: per vector four accumulators of v_mfma_f64_16x16x4_f64 (the four row tiles
// p) and one tile of Z: 80 accumulator VGPRs.  Per P and tile of 16 rows r the sum over s runs in chunks of BSE_SC = 32: the block
// stages the 2 x 16 x 32 block of X [v][r][s] and the 64 x 32 block of R [q][s] in LDS (the next chunk is asked for before the MFMAs
// of this one and stored after the next barrier), and with the first chunk the 64 x 16 block of L [p][r].  A staged row of R serves
// both vectors: three operand reads feed two MFMAs.
// The chaining needs no transpose and no LDS round trip.  By the fragment layout (mfma_tile.hpp) register reg of the C tile Z holds
// the rows r = (lane >> 4) + 4 reg at the column q = lane & 15 -- exactly the element B[k = lane >> 4][j = lane & 15] that the k-step
// reg (k = 4 reg ... 4 reg + 3) of the second product asks of this lane: Z[reg] IS its B operand, with the A operand read as
// L[p = lane & 15][r = 4 reg + (lane >> 4)].
// LDS: X and R rows at stride 34 doubles, L rows at stride 18 (both == 2 mod 32): every operand is read [row = lane & 15][k = lane >> 4]
// (R as B[k][j = row]: the same address pattern), which for a 32-lane half touches 32 different 8-byte banks (the argument in the header
// of rpa.hip) -- conflict-free with ds_read_b64.  X has no alignment to offer (ns is any number): its rows are read as single doubles,
// 32 consecutive per 32 lanes; the slabs as double2.
// Padding: columns r >= nr and s >= ns of the slabs are staged as 0.0 (selected, not multiplied), rows p >= np, q >= nq, r >= nr of X
// and vectors past nvec are staged as 0.0 without being loaded, and none of them is stored.  Whatever the padding holds, it
// contributes exactly zero.
// No atomics.  slots == 1: every element of out is written once, by one lane.  slots > 1 (a launch of few (vector, row, column) panels:
// the sum over P is split over blocks for occupancy): every block writes its partial sums to its slot of the work buffer and
// bse_sum_kernel adds the slots of an element in slot order.  Bit-reproducible as it stands.
//
// Tile: per chunk 24 KB staged for 16 MFMAs per wave -- 5.3 flop per byte, a third of what gw.hip has: the kernel waits on its staging.
// Four vectors per block (8 flop per byte) need 284 registers, one block per CU (docs/LOG_r26.md has the measurements against the
// library route and what is left to try).
#include <algorithm>

#include "common.hpp"
#include "mfma_tile.hpp"

namespace dqc {

constexpr int BSE_NV = 2;    // trial vectors per block
constexpr int BSE_QW = 64;   // column panel q (one tile per wave)
constexpr int BSE_PW = 64;   // row panel p (four accumulator tiles per wave and vector)
constexpr int BSE_SC = 32;   // s per LDS chunk
constexpr int BSE_XS = 34;   // LDS stride of the X and R rows in doubles
constexpr int BSE_LS = 18;   // LDS stride of the L rows in doubles
constexpr int BSE_NT = 256;  // threads
constexpr int BSE_PT = BSE_PW / 16;
constexpr long long BSE_TARGET_BLOCKS = 512;        // the sum over P is split while the launch has fewer blocks than this
constexpr long long BSE_WORK_CAP = 1LL << 24;       // doubles: the work buffer never exceeds this (the host splits less)

struct BseArgs {
    const double *l, *r, *x;
    double *out, *part;   // part: [slot][v][p][q] (slots > 1)
    int np, nq, nr, ns, ldr, lds, naux, nvec;
    int nvb, npp, nqp;    // vector batches, row panels, column panels
    int nrt, nsc;         // tiles of 16 rows r, chunks of 32 columns s
    int slots, pps;       // slots of the sum over P, auxiliary functions per slot
};

__global__ __launch_bounds__(BSE_NT, 2) void bse_exchange_kernel(BseArgs g) {
    __shared__ __align__(16) double s_x[BSE_NV][16][BSE_XS];   // [v][r][s] of the chunk
    __shared__ __align__(16) double s_r[BSE_QW][BSE_XS];       // [q][s] of the chunk
    __shared__ __align__(16) double s_l[BSE_PW][BSE_LS];       // [p][r] of the row tile r
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, q4 = lane >> 4;
    long long b = blockIdx.x;
    const int qp = (int)(b % g.nqp);
    b /= g.nqp;
    const int pp = (int)(b % g.npp);
    b /= g.npp;
    const int vb = (int)(b % g.nvb), slot = (int)(b / g.nvb);
    const int q0 = BSE_QW * qp, p0 = BSE_PW * pp, v0 = BSE_NV * vb;
    const int nv = min(BSE_NV, g.nvec - v0);                  // live vectors (block-uniform)
    const int npt = min(BSE_PT, (g.np - p0 + 15) >> 4);       // row tiles that hold a real row (block-uniform)
    const bool qlive = q0 + 16 * wave < g.nq;                 // this wave's columns hold a real column (wave-uniform)
    const int P_lo = slot * g.pps, P_hi = min(P_lo + g.pps, g.naux);
    v4d acc[BSE_NV][BSE_PT], z[BSE_NV];
#pragma unroll
    for (int v = 0; v < BSE_NV; v++) {
        z[v] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < BSE_PT; t++) acc[v][t] = v4d{0.0, 0.0, 0.0, 0.0};
    }

    // the staging map: X 2 x 16 rows x 32 doubles, four per thread; R 64 rows x 16 double2, four per thread; L 64 rows x 8 double2, two
    // per thread (with the first chunk of a row tile r only)
    double nx[2 * BSE_NV];
    double2 nr_[4], nl[2];
    auto fetch = [&](int P, int rt, int sc) {
        const int r0 = 16 * rt, s0 = BSE_SC * sc;
#pragma unroll
        for (int u = 0; u < 2 * BSE_NV; u++) {
            const int e = threadIdx.x + BSE_NT * u, v = v0 + (e >> 9), r = r0 + ((e >> 5) & 15), s = s0 + (e & 31);
            nx[u] = (v < g.nvec && r < g.nr && s < g.ns) ? g.x[((size_t)v * g.nr + r) * g.ns + s] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = threadIdx.x + BSE_NT * u, q = q0 + (e >> 4), s = s0 + (e & 15) * 2;
            double2 v{0.0, 0.0};
            if (q < g.nq && s < g.lds) v = *reinterpret_cast<const double2 *>(g.r + ((size_t)q * g.naux + P) * g.lds + s);   // (s + 1 < lds: whole 16s)
            nr_[u] = double2{s < g.ns ? v.x : 0.0, s + 1 < g.ns ? v.y : 0.0};
        }
        if (sc == 0) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = threadIdx.x + BSE_NT * u, p = p0 + (e >> 3), r = r0 + (e & 7) * 2;
                double2 v{0.0, 0.0};
                if (p < g.np && r < g.ldr) v = *reinterpret_cast<const double2 *>(g.l + ((size_t)p * g.naux + P) * g.ldr + r);
                nl[u] = double2{r < g.nr ? v.x : 0.0, r + 1 < g.nr ? v.y : 0.0};
            }
        }
    };
    auto store = [&](int sc) {
#pragma unroll
        for (int u = 0; u < 2 * BSE_NV; u++) {
            const int e = threadIdx.x + BSE_NT * u;
            s_x[e >> 9][(e >> 5) & 15][e & 31] = nx[u];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = threadIdx.x + BSE_NT * u;
            *reinterpret_cast<double2 *>(&s_r[e >> 4][(e & 15) * 2]) = nr_[u];
        }
        if (sc == 0) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = threadIdx.x + BSE_NT * u;
                *reinterpret_cast<double2 *>(&s_l[e >> 3][(e & 7) * 2]) = nl[u];
            }
        }
    };
    // one k-step of the first product: Z[v] += X[v][r = l15][s = k0 + q4] R[q = 16 wave + l15][s = k0 + q4]
    auto step = [&](int k0) {
        const double bq = s_r[16 * wave + l15][k0 + q4];
        double a[BSE_NV];
#pragma unroll
        for (int v = 0; v < BSE_NV; v++) a[v] = s_x[v][l15][k0 + q4];
#pragma unroll
        for (int v = 0; v < BSE_NV; v++)
            if (v < nv) z[v] = mfma_f64(a[v], bq, z[v]);
    };

    int P = P_lo, rt = 0, sc = 0;   // the chunk in the registers, then in LDS
    if (P < P_hi) fetch(P, rt, sc);
    while (P < P_hi) {
        __syncthreads();            // (the previous chunk has been read by every wave)
        store(sc);
        __syncthreads();
        int nP = P, nrt = rt, nsc = sc + 1;
        if (nsc == g.nsc) {
            nsc = 0;
            if (++nrt == g.nrt) {
                nrt = 0;
                nP++;
            }
        }
        if (nP < P_hi) fetch(nP, nrt, nsc);
        if (qlive) {
            const int klim = min(BSE_SC, (g.ns - BSE_SC * sc + 3) & ~3);   // (the k-steps past ns are staged zeros)
            if (klim == BSE_SC) {
#pragma unroll
                for (int k0 = 0; k0 < BSE_SC; k0 += 4) step(k0);
            } else {
                for (int k0 = 0; k0 < klim; k0 += 4) step(k0);
            }
            if (sc == g.nsc - 1) {   // Z of this (P, row tile r) is whole: register reg of it is the B operand of k-step reg
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
#pragma unroll
                    for (int t = 0; t < BSE_PT; t++) {
                        if (t >= npt) continue;
                        const double a = s_l[16 * t + l15][4 * reg + q4];
#pragma unroll
                        for (int v = 0; v < BSE_NV; v++)
                            if (v < nv) acc[v][t] = mfma_f64(a, z[v][reg], acc[v][t]);
                    }
                }
#pragma unroll
                for (int v = 0; v < BSE_NV; v++) z[v] = v4d{0.0, 0.0, 0.0, 0.0};
            }
        }
        P = nP;
        rt = nrt;
        sc = nsc;
    }
    // lane (l15, q4), register reg holds row p = p0 + 16 t + q4 + 4 reg, column q = q0 + 16 wave + l15
    const size_t tot = (size_t)g.nvec * g.np * g.nq;
    double *o = g.slots > 1 ? g.part + (size_t)slot * tot : g.out;
    const int q = q0 + 16 * wave + l15;
#pragma unroll
    for (int v = 0; v < BSE_NV; v++) {
        if (v >= nv) continue;
#pragma unroll
        for (int t = 0; t < BSE_PT; t++) {
            if (t >= npt) continue;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int p = p0 + 16 * t + q4 + 4 * reg;
                if (p < g.np && q < g.nq) o[((size_t)(v0 + v) * g.np + p) * g.nq + q] = acc[v][t][reg];
            }
        }
    }
}

// the slots of an element in slot order
__global__ __launch_bounds__(256) void bse_sum_kernel(double *__restrict__ out, const double *__restrict__ part, size_t tot, int slots) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    double s = 0.0;
    for (int sl = 0; sl < slots; sl++) s += part[(size_t)sl * tot + e];
    out[e] = s;
}

// (vector batches, row panels, column panels, slots, auxiliary functions per slot) of a launch of non-negative counts; false: the
// output has more elements than a 64-bit count holds
static bool bse_counts(int np, int nq, int nr, int ns, int naux, int nvec, long long &nvb, long long &npp, long long &nqp, int &slots,
                       int &pps) {
    if ((double)nvec * (double)np * (double)nq > 4e18) return false;
    nvb = (nvec + BSE_NV - 1) / BSE_NV;
    npp = (np + BSE_PW - 1) / BSE_PW;
    nqp = (nq + BSE_QW - 1) / BSE_QW;
    slots = 1;
    pps = naux;
    const long long blocks = nvb * npp * nqp;
    if (blocks == 0 || naux == 0 || nr == 0 || ns == 0) return true;
    long long s = blocks >= BSE_TARGET_BLOCKS ? 1 : (BSE_TARGET_BLOCKS + blocks - 1) / blocks;
    const long long per = (long long)nvec * np * nq;   // doubles per slot
    s = std::min(s, std::max(1LL, BSE_WORK_CAP / per));
    s = std::min(s, (long long)naux);
    pps = (int)((naux + s - 1) / s);
    slots = (naux + pps - 1) / pps;   // (no empty slot)
    return true;
}

}  // namespace dqc

extern "C" {

size_t dqc_bse_work_doubles(int np, int nq, int nr, int ns, int naux, int nvec) {
    long long nvb, npp, nqp;
    int slots, pps;
    if (np < 0 || nq < 0 || nr < 0 || ns < 0 || naux < 0 || nvec < 0) return 0;
    if (!dqc::bse_counts(np, nq, nr, ns, naux, nvec, nvb, npp, nqp, slots, pps)) return 0;
    return slots > 1 ? (size_t)slots * (size_t)nvec * (size_t)np * (size_t)nq : 0;
}

int dqc_bse_exchange(double *d_out, const double *d_l, const double *d_r, const double *d_x, int np, int nq, int nr, int ns, int ldr,
                     int lds, int naux, int nvec, double *d_work, void *stream) {
    using namespace dqc;
    hipStream_t st = (hipStream_t)stream;
    long long nvb, npp, nqp;
    int slots, pps;
    if (np < 0 || nq < 0 || nr < 0 || ns < 0 || ldr < 0 || lds < 0 || naux < 0 || nvec < 0) { set_error("dqc_bse_exchange: negative count"); return DQC_EINVAL; }
    if (ldr % 16 || ldr < nr) { set_error("dqc_bse_exchange: ldr must be a multiple of 16 and at least nr"); return DQC_EINVAL; }
    if (lds % 16 || lds < ns) { set_error("dqc_bse_exchange: lds must be a multiple of 16 and at least ns"); return DQC_EINVAL; }
    if (!bse_counts(np, nq, nr, ns, naux, nvec, nvb, npp, nqp, slots, pps)) { set_error("dqc_bse_exchange: more blocks than one launch holds"); return DQC_EINVAL; }
    const size_t out = (size_t)nvec * (size_t)np * (size_t)nq;
    if (out == 0) return DQC_OK;  // (empty output)
    if (!d_out) { set_error("dqc_bse_exchange: null output"); return DQC_EINVAL; }
    if (naux == 0 || nr == 0 || ns == 0) {   // an empty sum: zeros
        DQC_HIP(hipMemsetAsync(d_out, 0, sizeof(double) * out, st));
        return DQC_OK;
    }
    if (!d_l || !d_r || !d_x || (slots > 1 && !d_work)) { set_error("dqc_bse_exchange: null pointer argument"); return DQC_EINVAL; }
    if ((size_t)d_l % 16 || (size_t)d_r % 16) { set_error("dqc_bse_exchange: the tensors must be 16-byte aligned"); return DQC_EINVAL; }
    const long long nblk = nvb * npp * nqp * slots;
    if (nblk > 2147483647LL) { set_error("dqc_bse_exchange: more blocks than one launch holds"); return DQC_EINVAL; }
    BseArgs g{d_l, d_r, d_x, d_out, d_work, np, nq, nr, ns, ldr, lds, naux, nvec, (int)nvb, (int)npp, (int)nqp, (nr + 15) / 16,
              (ns + BSE_SC - 1) / BSE_SC, slots, pps};
    hipLaunchKernelGGL(bse_exchange_kernel, dim3((unsigned)nblk), dim3(BSE_NT), 0, st, g);
    DQC_CHECK_LAUNCH();
    if (slots > 1) {
        const size_t nsum = (out + 255) / 256;   // (slots > 1: out <= BSE_WORK_CAP / 2)
        hipLaunchKernelGGL(bse_sum_kernel, dim3((unsigned)nsum), dim3(256), 0, st, d_out, (const double *)d_work, out, slots);
        DQC_CHECK_LAUNCH();
    }
    return DQC_OK;
}

}  // extern "C"
